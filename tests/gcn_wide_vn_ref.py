"""OGB's virtual node for GCN at a width read off the arrays (flowgnn.h: flowgnn_set_gcn_virtual_node_dim), the
reference side of tests/test_gcn_wide_vn_cpu.py, tests/test_gcn_wide_vn_abi.py and tests/test_gcn_wide_vn_gpu.py.  No GPU, and nothing
here knows what a GPU returns.

  forward        a float64 forward of the definition: tests/gcn_wide_ref.forward's GCN with tests/gcn_vn_ref.forward's virtual node, the
                 widths from the arrays' shapes, `dense=` / `vn_dense=` for the four layer products and the update's eight, and the
                 eight wrong forms of gcn_vn_ref.VARIANTS (`variant=`).  At width 100 it IS gcn_vn_ref.forward, and with zero tensors at
                 300 it IS gcn_wide_ref.forward (tests/test_gcn_wide_vn_cpu.py checks both before anything relies on it).
  ogb_forward    OGB's own gcn-virtual forward in eval mode, float64, nothing folded, at the state_dict's width
                 (gcn_vn_ref.ogb_vn_forward without its hard-wired 100).
  fixed_*        the fixed input that tells every wrong form from the definition at width 300.
  table          the split-f16 separation with the virtual node on: split_ref.SplitDense("GCN", ..) on the four layer products and the
                 eight update products (committed as tests/golden/gcn_wide_vn_sep.json).
"""
import functools
import json
import os
from collections import OrderedDict, namedtuple

import numpy as np

from flowgnn_amd import graphpack as gp, weights
from tests import gcn_vn_ref, gcn_wide_ref as R, numpy_ref, split_ref
from tests.test_export import _bn, _bn_params

ND_OFF, ED_OFF = numpy_ref.ND_OFF, numpy_ref.ED_OFF
L = 5
WIDE = 300
VARIANTS = gcn_vn_ref.VARIANTS

Out = namedtuple("Out", "logits rows pooled scale x4 operands")


def zero_virtual_node(emb_dim=WIDE):
    return OrderedDict((k, np.zeros(s, np.float32)) for k, s in weights.gin_virtual_node_shapes(emb_dim).items())


def forward(batch, w, vn, dense=None, vn_dense=None, pooling="mean", num_tasks=None, dtype=np.float64, variant=None):
    """Out(logits [G] or [G][T], pre_4 rows [N][D], pooled rows [G][D], scale, x_4 rows, operands).  scale = the largest magnitude of any
    activation (rows, projected rows, aggregates, pooled rows, t and the update's hidden vector and output): the `scale` of
    tests/parity.py.  operands: the largest |xin_l| (l = 1..4), |t| and pre-scaled hidden value of the update -- what the split-f16
    kernels' range guards watch (6e4).  dense: the products x_1 .. x_4 (x_0 is no matrix-pipe product at this width: W_0 is applied to
    the node table and to E on the host); vn_dense: the update's two products, eight calls."""
    assert variant is None or variant in VARIANTS, variant
    c = lambda a: np.asarray(a, dtype=dtype)
    mm = numpy_ref._matmul if dense is None else (lambda a, M: np.asarray(dense(a, M), dtype=dtype))
    vmm = numpy_ref._matmul if vn_dense is None else (lambda a, M: np.asarray(vn_dense(a, M), dtype=dtype))
    nemb, eemb = c(w["node_embedding_weight"]), c(w["edge_embedding_weight"])
    cw, cb, root = c(w["convs_weight"]), c(w["convs_bias"]), c(w["convs_root_emb_weight"])
    bnw, bnb, bnm, bnv = c(w["bn_weight"]), c(w["bn_bias"]), c(w["bn_mean"]), c(w["bn_var"])
    D = nemb.shape[-1]
    assert cw.shape == (L, D, D) and eemb.shape == (L, 13, D) and root.shape == (L, D), (cw.shape, eemb.shape, root.shape)
    pw, pb = c(w["graph_pred_weights"]).reshape(-1, D), c(w["graph_pred_bias"]).reshape(-1)
    if num_tasks is not None:
        assert pw.shape[0] == num_tasks == pb.shape[0], (pw.shape, pb.shape, num_tasks)
    E = c(vn["vn_embedding"]).reshape(-1)
    v1, c1, v2, c2 = c(vn["w1"]), c(vn["b1"]), c(vn["w2"]), c(vn["b2"])
    assert E.shape == (D,) and v1.shape == (L - 1, 2 * D, D) and v2.shape == (L - 1, D, 2 * D), (E.shape, v1.shape, v2.shape)
    if variant == "embedding_ignored":
        E = np.zeros(D, dtype)
    N, G = batch.total_nodes, batch.num_graphs
    ge = batch.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    nn = c(batch.nums_of_nodes)[:, None]
    seg = lambda rows: np.add.reduceat(rows, off[:-1], axis=0)  # (every graph has a node)
    outdeg = np.bincount(u, minlength=N).astype(dtype)
    one = dtype(1.0)
    dinv = np.where(outdeg > 0, one / np.sqrt(outdeg + one), dtype(0.0))
    norm = dinv[u] * dinv[v]
    bn = lambda t, l: (t - bnm[l]) / np.sqrt(bnv[l] + dtype(2.0 ** -10)) * bnw[l] + bnb[l]
    h = nemb[batch.node_feature.astype(np.int64) + ND_OFF[None, :]].sum(axis=1)
    pre_relu = None
    vec = np.tile(E, (G, 1))
    big = [1.0, float(np.abs(h).max()), float(np.abs(vec).max())]
    ops = [0.0]
    x4 = pre = None
    for l in range(L):
        add = vec[gid]
        if l == L - 1 and variant == "no_add_in_last_layer":
            add = np.zeros_like(add)
        if variant == "added_in_front_of_the_relu" and pre_relu is not None:
            xin = np.maximum(pre_relu + add, 0.0)
        elif variant == "added_behind_the_linear_map":
            xin = h
        else:
            xin = h + add
        x = (numpy_ref._matmul if l == 0 else mm)(xin, cw[l]) + cb[l]
        if variant == "added_behind_the_linear_map":
            x = x + add
        x4 = x
        ee = eemb[l][batch.edge_attr.astype(np.int64) + ED_OFF[None, :]].sum(axis=1)
        m = np.zeros((N, D), dtype)
        np.add.at(m, v, norm[:, None] * np.maximum(x[u] + ee, 0.0))
        pre = bn(m + np.maximum(x + root[l], 0.0) / (outdeg[:, None] + one), l)
        big.extend([float(np.abs(xin).max()), float(np.abs(x).max()), float(np.abs(m).max()) if m.size else 0.0, float(np.abs(pre).max())])
        if l > 0:
            ops.append(float(np.abs(xin).max()))
        if l < L - 1:
            rows = h if variant == "pool_before_add" else h + add
            t = seg(rows) / nn if variant == "mean_instead_of_sum" else seg(rows)
            if variant != "t_without_vn":
                t = t + vec
            k = (l + 1) % 4 if variant == "update_indexed_l_plus_1" else l
            hid = np.maximum(vmm(t, v1[k]) + c1[k], 0.0)
            vec = np.maximum(vmm(hid, v2[k]) + c2[k], 0.0)
            big.extend([float(np.abs(t).max()), float(hid.max()), float(vec.max())])
            ops.extend([float(np.abs(t).max()), split_ref.pow2_scale(np.asarray(vn["w1"], np.float32)[k]) * float(hid.max())])
        pre_relu = pre
        h = np.maximum(pre, 0.0)
    if pooling == "mean":
        pooled = seg(pre) / nn
    elif pooling == "sum":
        pooled = seg(pre)
    else:
        assert pooling == "max", pooling
        pooled = np.maximum.reduceat(pre, off[:-1], axis=0)
    big.append(float(np.abs(pooled).max()))
    out = pooled @ pw.T + pb
    return Out(out[:, 0] if out.shape[1] == 1 else out, pre, pooled, max(big), x4, max(ops))


def node_logits(w, rows):
    return R.node_logits(w, rows)


# ---------------------------------------------------------------- the OGB side
def ogb_forward(sd, batch):
    """Inference of the OGB example GNN with gnn_type='gcn-virtual' (GNN_node_Virtualnode with GCNConv: JK='last', no residual, mean
    pooling), float64, nothing folded, at the state_dict's own width: tests/gcn_vn_ref.ogb_vn_forward without its hard-wired 100."""
    ge = batch.global_edges()
    row, col = ge[:, 0], ge[:, 1]
    N, G = batch.total_nodes, batch.num_graphs
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    h = sum(sd[f"gnn_node.atom_encoder.atom_embedding_list.{k}.weight"][batch.node_feature[:, k]] for k in range(9))
    D = h.shape[1]
    vec = np.tile(np.asarray(sd["gnn_node.virtualnode_embedding.weight"], np.float64).reshape(1, D), (G, 1))  # embedding(zeros(G))
    deg = np.bincount(row, minlength=N) + 1.0
    norm = deg[row] ** -0.5 * deg[col] ** -0.5
    for l in range(L):
        c = f"gnn_node.convs.{l}"
        h = h + vec[gid]
        e = sum(sd[f"{c}.bond_encoder.bond_embedding_list.{k}.weight"][batch.edge_attr[:, k]] for k in range(3))
        x = h @ sd[f"{c}.linear.weight"].T + sd[f"{c}.linear.bias"]
        z = np.zeros((N, D))
        np.add.at(z, col, norm[:, None] * np.maximum(x[row] + e, 0.0))
        z = z + np.maximum(x + sd[f"{c}.root_emb.weight"], 0.0) / deg[:, None]
        z = _bn(sd, f"gnn_node.batch_norms.{l}", z)
        if l < L - 1:
            m = f"gnn_node.mlp_virtualnode_list.{l}"
            t = np.add.reduceat(h, off[:-1], axis=0) + vec  # global_add_pool(h_list[layer], batch) + virtualnode_embedding
            t = t @ sd[f"{m}.0.weight"].T + sd[f"{m}.0.bias"]
            if f"{m}.1.weight" in sd:
                t = np.maximum(_bn(sd, f"{m}.1", t), 0.0) @ sd[f"{m}.3.weight"].T + sd[f"{m}.3.bias"]
                vec = np.maximum(_bn(sd, f"{m}.4", t), 0.0)
            else:
                vec = np.maximum(np.maximum(t, 0.0) @ sd[f"{m}.2.weight"].T + sd[f"{m}.2.bias"], 0.0)
        h = z if l == L - 1 else np.maximum(z, 0.0)
    pooled = np.add.reduceat(h, off[:-1], axis=0) / batch.nums_of_nodes[:, None]
    out = pooled @ sd["graph_pred_linear.weight"].T + sd["graph_pred_linear.bias"]
    return out[:, 0] if out.shape[1] == 1 else out


def vn_state_dict(seed=4, with_bn=True, tasks=1, width=WIDE, vn_w1_scale=1.0):
    """tests/gcn_wide_ref.state_dict(virtual_node=True); with_bn also gives the virtual node's MLP its two BatchNorms (OGB's layout:
    Linear .0, BatchNorm .1, ReLU, Linear .3, BatchNorm .4, ReLU), as tests/gcn_vn_ref.vn_state_dict does at width 100.
    vn_w1_scale: a factor on the first linear layer of every update (tests/gin_wide_vn_ref.vn_state_dict says why)."""
    sd = R.state_dict(seed=seed, width=width, tasks=tasks, virtual_node=True)
    if with_bn:
        rng = np.random.default_rng(seed + 2000)
        for l in range(L - 1):
            m = f"gnn_node.mlp_virtualnode_list.{l}"
            sd[f"{m}.3.weight"], sd[f"{m}.3.bias"] = sd.pop(f"{m}.2.weight"), sd.pop(f"{m}.2.bias")
            _bn_params(rng, f"{m}.1", 2 * width, sd)
            _bn_params(rng, f"{m}.4", width, sd)
    if vn_w1_scale != 1.0:
        for l in range(L - 1):
            sd[f"gnn_node.mlp_virtualnode_list.{l}.0.weight"] = sd[f"gnn_node.mlp_virtualnode_list.{l}.0.weight"] * vn_w1_scale
    return sd


# ---------------------------------------------------------------- the fixed input
def fixed_batch():
    return gcn_vn_ref.fixed_batch()


def fixed_weights(num_tasks=1, emb_dim=WIDE):
    w = weights.synth_gcn_weights(seed=7, num_tasks=num_tasks, emb_dim=emb_dim)
    w["graph_pred_weights"] = (np.asarray(w["graph_pred_weights"], np.float32) * np.float32(8)).astype(np.float32)
    return w


def fixed_virtual_node(emb_dim=WIDE):
    """weights.synth_gcn_virtual_node's random tensors at this width, scaled per tensor in the way of gcn_vn_ref.fixed_virtual_node and
    for the same reasons: t is a SUM over 1 .. 80 nodes, so the first linear layer is scaled down until vn neither dies out nor
    explodes over four updates; the later updates are scaled up until vn outweighs the rows it is added to, so that one part in n + 1
    of t reaches the logits; the biases are scaled down so that they do not drown it; the embedding row is scaled up so that dropping
    E shows.  The factors are the 100-wide ones (synth_gin_virtual_node already shrinks the matrices with sqrt(100 / emb_dim)).  Chosen
    on the references alone (tests/test_gcn_wide_vn_cpu.py prints what each wrong form reaches, and asserts that it is enough)."""
    vn = weights.synth_gcn_virtual_node(seed=13, emb_dim=emb_dim)
    f32 = np.float32
    vn["vn_embedding"] = vn["vn_embedding"] * f32(8)
    vn["w1"] = vn["w1"] * f32(0.03)
    vn["w2"] = vn["w2"] * f32(0.5)
    vn["w2"][2] *= f32(3)
    vn["w2"][3] *= f32(32)
    vn["b1"] = vn["b1"] * f32(0.1)
    vn["b2"] = vn["b2"] * f32(0.1)
    return OrderedDict((k, np.ascontiguousarray(v, dtype=np.float32)) for k, v in vn.items())


def shapes_virtual_node(emb_dim=WIDE, w1_scale=1.0 / 16):
    """The virtual node of the shape and configuration tests: weights.synth_gcn_virtual_node(seed=13) with the first linear layer scaled
    by 1 / 16 (tests/gin_wide_vn_ref.shapes_virtual_node says why: t is a sum over up to 300 nodes, and at the synthetic scales the
    vector passes 6e4 within four updates, where the engine's fp32 re-run would compute every case and the kernels under test none).
    Chosen on the float64 forward alone: every split-path test asserts the range on the reference too."""
    vn = weights.synth_gcn_virtual_node(seed=13, emb_dim=emb_dim)
    vn["w1"] = vn["w1"] * np.float32(w1_scale)
    return vn


def range_virtual_node(emb_dim=WIDE):
    """gcn_vn_ref.range_virtual_node at this width: zero but for one component of update 0's second bias, so vn_1 has a component of
    7e4 in every graph and xin_1 = a_1 + vn_1 leaves the f16 split's range in the registers of the layer kernel's VN instance."""
    vn = zero_virtual_node(emb_dim)
    vn["b2"][0, 17] = np.float32(7.0e4)
    return vn


# ---------------------------------------------------------------- split-f16 separation with the virtual node on
# Batch seeds, chosen on the references alone: the two smallest at which BOTH outputs reach split_ref.min_ratio("GCN", output) (64 for
# rows, 16 for logits) with the virtual node on.  Every seed tried, in order, with its ratios -- `python -m tests.gcn_wide_vn_ref`
# prints this list again:
#   seed 0: rows 108.5, logits 57.2 (closest, both: "a_hi.w_lo dropped for 16 output columns"); largest split operand 5.8e3
#   seed 1: rows 105.4, logits 46.2 (closest, both: "a_hi.w_lo dropped for 16 output columns"); largest split operand 5.06e3
# Both reach both ratios, so no further seed was tried.
SEEDS_TRIED = {0: (108.5, 57.2), 1: (105.4, 46.2)}  # seed -> (rows ratio, logits ratio), as printed
SEEDS = (0, 1)
SEP_GRAPHS = R.SEP_GRAPHS
SEP_OUTPUTS = R.SEP_OUTPUTS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gcn_wide_vn_sep.json")
Row = R.Row


@functools.lru_cache(maxsize=None)
def sep_virtual_node():
    return shapes_virtual_node()


@functools.lru_cache(maxsize=None)
def reference(seed):
    return forward(R.sep_batch(seed), R.sep_weights(), sep_virtual_node())


def split_dense_vn(spec):
    """split_ref.SplitDense("GCN", spec) for the update's eight products, an instance of its own: none of them is "the last layer" of
    split_ref.LAST_CALLS (that is x_4, the layer product), so the count starts behind it."""
    d = split_ref.SplitDense("GCN", spec)
    d.calls = 5
    return d


def misplaced_unscale_vn(vn):
    """split_ref.misplaced_unscale for the update's two matrices: every bias times its matrix's power of two."""
    out = OrderedDict((k, np.asarray(v, np.float32).copy()) for k, v in vn.items())
    for wk, bk in (("w1", "b1"), ("w2", "b2")):
        for l in range(L - 1):
            out[bk][l] = out[bk][l] * np.float32(split_ref.pow2_scale(out[wk][l]))
    return out


def err(got, ref, name):
    return R.err(got, ref, name)


@functools.lru_cache(maxsize=None)
def table(seed):
    """output name -> Row(E_ok, E_bad, B, per-restatement errors, per-variant errors), from the references alone: gcn_wide_ref.table
    with the virtual node on and the same restatement applied to the update's eight products."""
    b, w, vn, ref = R.sep_batch(seed), R.sep_weights(), sep_virtual_node(), reference(seed)
    sd = lambda spec: dict(dense=R.split_dense(spec), vn_dense=split_dense_vn(spec))
    ok = {"all fp32": forward(b, w, vn, dense=split_ref.dense_fp32, vn_dense=split_ref.dense_fp32, dtype=np.float32),
          split_ref.OK_SPECS[1].name: forward(b, w, vn, **sd(split_ref.OK_SPECS[1]))}
    bad = {spec.name: forward(b, w, vn, **sd(spec)) for spec in R.variants()}
    bad[split_ref.BIAS_VARIANT] = forward(b, R.misplaced_unscale(w), misplaced_unscale_vn(vn), **sd(split_ref.OK_SPECS[1]))
    rows = {}
    for name in SEP_OUTPUTS:
        eo = {k: err(getattr(v, name), ref, name) for k, v in ok.items()}
        eb = {k: err(getattr(v, name), ref, name) for k, v in bad.items()}
        e_ok, e_bad = max(eo.values()), min(eb.values())
        rows[name] = Row(e_ok, e_bad, float(np.sqrt(e_ok * e_bad)), eo, eb)
    return rows


def table_json(seeds=None):
    """The tables of `seeds` as what tests/golden/gcn_wide_vn_sep.json holds: seed -> output -> {e_ok, e_bad, bound, ratio, closest}."""
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
              f"logits {r['logits']:.1f} (closest: {min(t['logits'].bad, key=t['logits'].bad.get)}), "
              f"largest split operand {reference(seed).operands:.3g}{' <-' if good else ''}", flush=True)
        found += [seed] if good else []
        if len(found) == 2:
            break
    if len(sys.argv) > 1 and sys.argv[1] == "--write" and len(found) == 2:
        with open(GOLDEN, "w") as f:
            json.dump(table_json(found), f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", GOLDEN)
