"""GCN at a width read off the weights (flowgnn.h: flowgnn_set_model_emb_dim), the reference side of
tests/test_gcn_wide_cpu.py and tests/test_gcn_wide_gpu.py.  No GPU, and nothing here knows what a GPU returns.

  forward        a float64 GCN forward whose widths come from the weight arrays' shapes: tests/numpy_ref.gcn_forward's equations (which
                 hard-wire 100) with `dense=`, `pooling=` and `num_tasks=`; at width 100 it IS numpy_ref.gcn_forward
                 (tests/test_gcn_wide_cpu.py checks that to 1e-12 before anything relies on it).  `dense` is used for the FOUR products
                 x_1 .. x_4: x_0 = W_0 h0 + b_0 is no matrix-pipe product at this width (W_0 is applied to the node table on the host).
  state_dict     an OGB `GNN(gnn_type='gcn', emb_dim=width)` state_dict, built the way tests/test_export.ogb_state_dict builds its own;
                 ogb_forward: OGB's GNN_node + graph_pred_linear in eval mode, float64, nothing folded, torch's BatchNorm eps.
  table          the separation of tests/split_ref.py at width 300: the split-f16 restatement and its wrong variants through `forward`,
                 and the bound B = sqrt(E_ok * E_bad) that the GPU test uses (committed as tests/golden/gcn_wide_sep.json).
"""
import functools
import json
import os
from collections import namedtuple

import numpy as np

from flowgnn_amd import export, graphpack as gp, weights
from tests import numpy_ref, split_ref
from tests.test_export import _bn, _bn_params

ND_OFF, ED_OFF = numpy_ref.ND_OFF, numpy_ref.ED_OFF
L = 5
WIDE = 300

Out = namedtuple("Out", "logits rows pooled scale")


def forward(batch, w, dense=None, pooling="mean", num_tasks=None, dtype=np.float64):
    """Out(logits [G] or [G][T], pre_4 rows [N][D], pooled rows [G][D], scale); scale = the largest magnitude of any activation (h0,
    every x, m, pre and a, the pooled rows): the `scale` of tests/parity.py."""
    c = lambda a: np.asarray(a, dtype=dtype)
    mm = numpy_ref._matmul if dense is None else (lambda a, W: np.asarray(dense(a, W), dtype=dtype))
    nemb, eemb = c(w["node_embedding_weight"]), c(w["edge_embedding_weight"])
    cw, cb, root = c(w["convs_weight"]), c(w["convs_bias"]), c(w["convs_root_emb_weight"])
    bnw, bnb, bnm, bnv = c(w["bn_weight"]), c(w["bn_bias"]), c(w["bn_mean"]), c(w["bn_var"])
    D = nemb.shape[-1]
    assert cw.shape == (L, D, D) and eemb.shape == (L, 13, D) and root.shape == (L, D), (cw.shape, eemb.shape, root.shape)
    pw, pb = c(w["graph_pred_weights"]).reshape(-1, D), c(w["graph_pred_bias"]).reshape(-1)
    if num_tasks is not None:
        assert pw.shape[0] == num_tasks == pb.shape[0], (pw.shape, pb.shape, num_tasks)
    N = batch.total_nodes
    ge = batch.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    outdeg = np.bincount(u, minlength=N).astype(dtype)
    one = dtype(1.0)
    dinv = np.where(outdeg > 0, one / np.sqrt(outdeg + one), dtype(0.0))
    norm = dinv[u] * dinv[v]
    bn = lambda t, l: (t - bnm[l]) / np.sqrt(bnv[l] + dtype(2.0 ** -10)) * bnw[l] + bnb[l]
    a = nemb[batch.node_feature.astype(np.int64) + ND_OFF[None, :]].sum(axis=1)
    big = [1.0, float(np.abs(a).max())]
    for l in range(L):
        x = (numpy_ref._matmul if l == 0 else mm)(a, cw[l]) + cb[l]
        ee = eemb[l][batch.edge_attr.astype(np.int64) + ED_OFF[None, :]].sum(axis=1)
        m = np.zeros((N, D), dtype)
        np.add.at(m, v, norm[:, None] * np.maximum(x[u] + ee, 0.0))
        pre = bn(m + np.maximum(x + root[l], 0.0) / (outdeg[:, None] + one), l)
        a = np.maximum(pre, 0.0)
        big.extend([float(np.abs(x).max()), float(np.abs(m).max()) if m.size else 0.0, float(np.abs(pre).max())])
    off = batch.node_offsets()
    if pooling == "mean":
        pooled = np.add.reduceat(pre, off[:-1], axis=0) / c(batch.nums_of_nodes)[:, None]
    elif pooling == "sum":
        pooled = np.add.reduceat(pre, off[:-1], axis=0)
    else:
        assert pooling == "max", pooling
        pooled = np.maximum.reduceat(pre, off[:-1], axis=0)
    big.append(float(np.abs(pooled).max()))
    out = pooled @ pw.T + pb
    return Out(out[:, 0] if out.shape[1] == 1 else out, pre, pooled, max(big))


def max_a_per_layer(batch, w):
    """The largest a_{l+1} = relu(pre_l) of the float64 forward for l = 0..3: what the layer kernel's range guard watches."""
    rec = split_ref.Recorder()
    forward(batch, w, dense=rec)
    return [float(np.abs(a).max()) for a in rec.inputs]


def max_a(batch, w):
    return max(max_a_per_layer(batch, w))


def node_logits(w, rows):
    """The per-node terms of the mean readout: rows[v] . W[t] + b[t], [N] or [N][T]."""
    D = rows.shape[1]
    out = rows @ np.asarray(w["graph_pred_weights"], np.float64).reshape(-1, D).T + np.asarray(w["graph_pred_bias"], np.float64).reshape(-1)
    return out[:, 0] if out.shape[1] == 1 else out


# ---------------------------------------------------------------- the OGB side
def state_dict(seed=4, width=WIDE, tasks=1, virtual_node=False):
    """tests.test_export.ogb_state_dict("gcn", ...) at `width`; the conv matrices' scale shrinks with sqrt(100 / width) so that the
    activations keep their size.  virtual_node: gcn-virtual's keys too (the exporter refuses them at 300)."""
    rng = np.random.default_rng(seed)
    D, k = width, float(np.sqrt(100.0 / width))
    sd = {}
    for i, n in enumerate(export.ATOM_DIMS):
        sd[f"gnn_node.atom_encoder.atom_embedding_list.{i}.weight"] = 0.11 * rng.standard_normal((n, D))
    for l in range(L):
        c = f"gnn_node.convs.{l}"
        for i, n in enumerate(export.BOND_DIMS):
            sd[f"{c}.bond_encoder.bond_embedding_list.{i}.weight"] = 0.14 * rng.standard_normal((n, D))
        sd[f"{c}.linear.weight"] = 0.09 * k * rng.standard_normal((D, D))
        sd[f"{c}.linear.bias"] = 0.1 * rng.standard_normal(D)
        sd[f"{c}.root_emb.weight"] = 0.3 * rng.standard_normal((1, D))
        _bn_params(rng, f"gnn_node.batch_norms.{l}", D, sd)
    sd["graph_pred_linear.weight"] = 0.15 * k * rng.standard_normal((tasks, D))
    sd["graph_pred_linear.bias"] = 0.1 * rng.standard_normal(tasks)
    if virtual_node:
        sd[export.VN_KEY] = 0.5 * rng.standard_normal((1, D))
        for l in range(L - 1):
            m = f"gnn_node.mlp_virtualnode_list.{l}"
            sd[f"{m}.0.weight"] = 0.02 * rng.standard_normal((2 * D, D))
            sd[f"{m}.0.bias"] = 0.5 * rng.standard_normal(2 * D)
            sd[f"{m}.2.weight"] = 0.03 * rng.standard_normal((D, 2 * D))
            sd[f"{m}.2.bias"] = 0.3 * rng.standard_normal(D)
    return sd


def ogb_forward(sd, batch):
    """Inference of the OGB example GNN with gnn_type='gcn' (GNN_node: JK='last', no residual; mean pooling; graph_pred_linear), float64,
    nothing folded: GCNConv's linear, deg = out-degree + 1, norm = deg^-1/2[row] deg^-1/2[col], relu(x + root) / deg, the layer's
    BatchNorm with torch's eps, ReLU on all layers but the last.  (On batches whose graphs list both directions of every edge -- every
    batch of these tests that goes through it -- OGB's deg^-1/2 and the reference's dinv, which is 0 at out-degree 0, give the same sums.)"""
    ge = batch.global_edges()
    row, col = ge[:, 0], ge[:, 1]
    N = batch.total_nodes
    h = sum(sd[f"gnn_node.atom_encoder.atom_embedding_list.{k}.weight"][batch.node_feature[:, k]] for k in range(9))
    for l in range(L):
        c = f"gnn_node.convs.{l}"
        e = sum(sd[f"{c}.bond_encoder.bond_embedding_list.{k}.weight"][batch.edge_attr[:, k]] for k in range(3))
        x = h @ sd[f"{c}.linear.weight"].T + sd[f"{c}.linear.bias"]
        deg = np.bincount(row, minlength=N) + 1.0
        norm = deg[row] ** -0.5 * deg[col] ** -0.5
        z = np.zeros((N, h.shape[1]))
        np.add.at(z, col, norm[:, None] * np.maximum(x[row] + e, 0.0))
        z = z + np.maximum(x + sd[f"{c}.root_emb.weight"], 0.0) / deg[:, None]
        z = _bn(sd, f"gnn_node.batch_norms.{l}", z)
        h = z if l == L - 1 else np.maximum(z, 0.0)
    off = batch.node_offsets()
    pooled = np.add.reduceat(h, off[:-1], axis=0) / batch.nums_of_nodes[:, None]
    out = pooled @ sd["graph_pred_linear.weight"].T + sd["graph_pred_linear.bias"]
    return out[:, 0] if out.shape[1] == 1 else out


# ---------------------------------------------------------------- split-f16 separation at width 300
# Batch seeds, chosen on the references alone: the two smallest at which BOTH outputs reach their required ratio E_bad / E_ok,
# split_ref.min_ratio("GCN", output) = 64 for rows and 16 for logits (split_ref.py says why GCN's logits get 16).  Every seed tried, in
# order, with its ratios (rows, logits) -- `python -m tests.gcn_wide_ref` prints this list again:
#   seed 0: rows 137.0 (closest: "a_hi.w_lo dropped in one K-step"), logits 53.2 (closest: "a_hi.w_lo dropped for 16 output columns")
#   seed 1: rows 129.9 (closest: "a_hi.w_lo dropped in one K-step"), logits 49.2 (closest: "a_hi.w_lo dropped for 16 output columns")
# Both reach both ratios, so no further seed was tried.
SEEDS_TRIED = {0: (137.0, 53.2), 1: (129.9, 49.2)}  # seed -> (rows ratio, logits ratio), as printed
SEEDS = (0, 1)
SEP_GRAPHS = 256
SEP_OUTPUTS = ("logits", "rows")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gcn_wide_sep.json")


@functools.lru_cache(maxsize=None)
def sep_batch(seed):
    return gp.synth_molpcba_batch(SEP_GRAPHS, seed=seed)


@functools.lru_cache(maxsize=None)
def sep_weights():
    return weights.synth_gcn_weights(seed=7, emb_dim=WIDE)


def variants():
    """split_ref.VARIANTS as they apply to this width.  "K tail as a single f16 product" cannot show: K = 300 is padded with zero
    weights to whole K-steps, there is no fp32 K tail to get wrong (split_ref.tail_columns is empty at this K); the two "last layer
    before o_3" entries are GAT's (split_ref.applies)."""
    return [s for s in split_ref.VARIANTS if s.tail != "single" and s.where != "last_h"]


def split_dense(spec):
    """split_ref.SplitDense("GCN", spec) for the four products of `forward`.  split_ref numbers GCN's calls by layer (LAST_CALLS: 4),
    and x_0 is no split product here: the count starts at 1, so that a call's number is its layer's."""
    d = split_ref.SplitDense("GCN", spec)
    d.calls = 1
    return d


def misplaced_unscale(w):
    """split_ref.misplaced_unscale("GCN", w) for the products that exist: b_1 .. b_4 (b_0 is added by the encoder, unscaled)."""
    out = split_ref.misplaced_unscale("GCN", w)
    b = np.asarray(out["convs_bias"], np.float32).copy()
    b[0] = np.asarray(w["convs_bias"], np.float32)[0]
    out["convs_bias"] = b
    return out


def unit_of(name, ref):
    """split_ref.unit_of: the activation scale for node rows, max(1, max |f64 output|) for logits."""
    return ref.scale if name == "rows" else max(1.0, float(np.abs(ref.logits).max()))


def err(got, ref, name):
    want = getattr(ref, name)
    return float(np.abs(np.asarray(got, np.float64).reshape(want.shape) - want).max()) / unit_of(name, ref)


Row = namedtuple("Row", "e_ok e_bad bound ok bad")


@functools.lru_cache(maxsize=None)
def reference(seed):
    return forward(sep_batch(seed), sep_weights())


@functools.lru_cache(maxsize=None)
def table(seed):
    """output name -> Row(E_ok, E_bad, B, per-restatement errors, per-variant errors), from the references alone.  The correct
    restatements: every operation in fp32 with an fp32 product, and the three-product split with all of K split (split_ref.OK_SPECS[1]:
    what a kernel without an fp32 K tail computes).  The wrong ones: `variants` and 1 / scale applied before the bias."""
    b, w, ref = sep_batch(seed), sep_weights(), reference(seed)
    ok = {"all fp32": forward(b, w, dense=split_ref.dense_fp32, dtype=np.float32),
          split_ref.OK_SPECS[1].name: forward(b, w, dense=split_dense(split_ref.OK_SPECS[1]))}
    bad = {spec.name: forward(b, w, dense=split_dense(spec)) for spec in variants()}
    bad[split_ref.BIAS_VARIANT] = forward(b, misplaced_unscale(w), dense=split_dense(split_ref.OK_SPECS[1]))
    rows = {}
    for name in SEP_OUTPUTS:
        eo = {k: err(getattr(v, name), ref, name) for k, v in ok.items()}
        eb = {k: err(getattr(v, name), ref, name) for k, v in bad.items()}
        e_ok, e_bad = max(eo.values()), min(eb.values())
        rows[name] = Row(e_ok, e_bad, float(np.sqrt(e_ok * e_bad)), eo, eb)
    return rows


def table_json(seeds=None):
    """The tables of `seeds` as what tests/golden/gcn_wide_sep.json holds: seed -> output -> {e_ok, e_bad, bound, ratio, closest}."""
    out = {}
    for seed in (SEEDS if seeds is None else seeds):
        t = table(seed)
        out[str(seed)] = {name: {"e_ok": r.e_ok, "e_bad": r.e_bad, "bound": r.bound, "ratio": r.e_bad / r.e_ok,
                                 "closest": min(r.bad, key=r.bad.get)} for name, r in t.items()}
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":  # the seed search: every seed from 0 until two reach both ratios (none beyond 39 is tried)
    import sys
    found = []
    for seed in range(40):
        t = table(seed)
        r = {name: t[name].e_bad / t[name].e_ok for name in SEP_OUTPUTS}
        good = all(r[name] >= split_ref.min_ratio("GCN", name) for name in SEP_OUTPUTS)
        print(f"seed {seed}: rows {r['rows']:.1f} (closest: {min(t['rows'].bad, key=t['rows'].bad.get)}), "
              f"logits {r['logits']:.1f} (closest: {min(t['logits'].bad, key=t['logits'].bad.get)}){' <-' if good else ''}", flush=True)
        found += [seed] if good else []
        if len(found) == 2:
            break
    if len(sys.argv) > 1 and sys.argv[1] == "--write" and len(found) == 2:
        with open(GOLDEN, "w") as f:
            json.dump(table_json(found), f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", GOLDEN)
