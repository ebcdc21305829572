"""OGB's virtual node for GIN at a width read off the arrays (flowgnn.h: flowgnn_set_ogb_virtual_node_dim), the
reference side of tests/test_gin_wide_vn_cpu.py, tests/test_gin_wide_vn_abi.py and tests/test_gin_wide_vn_gpu.py.  No GPU, and nothing
here knows what a GPU returns.

  forward        a float64 forward of the definition: tests/gin_wide_ref.forward's GIN with tests/ogb_vn_ref.forward's virtual node, the
                 widths from the arrays' shapes, `dense=` / `vn_dense=` for the node MLP's and the update's products, and the wrong forms
                 of ogb_vn_ref.VARIANTS (`variant=`).  At width 100 it IS ogb_vn_ref.forward (tests/test_gin_wide_vn_cpu.py checks that to
                 1e-12 before anything relies on it).
  ogb_forward    OGB's own gin-virtual forward in eval mode, float64, nothing folded, at the state_dict's width
                 (tests/gin_wide_ref.state_dict(virtual_node=True) builds such a state_dict).
  fixed_virtual_node / fixed_batch   the fixed input that tells every wrong form from the definition at width 300.
  table          the split-f16 separation with the virtual node on: split_ref.SplitDense on the update's two products as well.
"""
import functools
from collections import OrderedDict, namedtuple

import numpy as np

from flowgnn_amd import graphpack as gp, weights
from tests import gin_wide_ref as W, numpy_ref, ogb_vn_ref, split_ref
from tests.test_export import _bn
from tests.test_gin_eps import self_scale

ND_OFF, ED_OFF = numpy_ref.ND_OFF, numpy_ref.ED_OFF
L = 5
WIDE = 300
VARIANTS = ogb_vn_ref.VARIANTS
NOOP_VARIANT = ogb_vn_ref.NOOP_VARIANT

Out = namedtuple("Out", "logits rows pooled scale")


def zero_virtual_node(emb_dim=WIDE):
    return OrderedDict((k, np.zeros(s, np.float32)) for k, s in weights.gin_virtual_node_shapes(emb_dim).items())


def forward(batch, w, vn, dense=None, vn_dense=None, eps=None, pooling="mean", num_tasks=None, dtype=np.float64, variant=None, eps_f64=False):
    """Out(logits [G] or [G][T], h_5 rows [N][D], pooled rows [G][D], scale); scale = the largest magnitude of any activation (rows,
    aggregates, hidden values, pooled rows, t and the virtual node's hidden vector and output): the `scale` of tests/parity.py.
    dense: the node MLP's two products per layer (ten calls, as tests/gin_wide_ref.forward makes them); vn_dense: the update's (eight)."""
    assert variant is None or variant in VARIANTS or variant == NOOP_VARIANT, variant
    c = lambda a: np.asarray(a, dtype=dtype)
    mm = numpy_ref._matmul if dense is None else (lambda a, M: np.asarray(dense(a, M), dtype=dtype))
    vmm = numpy_ref._matmul if vn_dense is None else (lambda a, M: np.asarray(vn_dense(a, M), dtype=dtype))
    nemb, eemb = c(w["node_embedding_weight"]), c(w["edge_embedding_weight"])
    w1, b1 = c(w["node_mlp_1_weights"]), c(w["node_mlp_1_bias"])
    w2, b2 = c(w["node_mlp_2_weights"]), c(w["node_mlp_2_bias"])
    D = nemb.shape[-1]
    assert w1.shape == (L, 2 * D, D) and w2.shape == (L, D, 2 * D) and eemb.shape == (L, 13, D), (w1.shape, w2.shape, eemb.shape)
    pw, pb = c(w["graph_pred_weights"]).reshape(-1, D), c(w["graph_pred_bias"]).reshape(-1)
    if num_tasks is not None:
        assert pw.shape[0] == num_tasks == pb.shape[0], (pw.shape, pb.shape, num_tasks)
    E = c(vn["vn_embedding"]).reshape(-1)
    v1, c1, v2, c2 = c(vn["w1"]), c(vn["b1"]), c(vn["w2"]), c(vn["b2"])
    assert E.shape == (D,) and v1.shape == (L - 1, 2 * D, D) and v2.shape == (L - 1, D, 2 * D), (E.shape, v1.shape, v2.shape)
    if variant == "embedding_ignored":
        E = np.zeros(D, dtype)
    # (eps: s_l = (float)(1.0f + eps[l]) as the engine forms it; eps_f64: 1 + eps[l] in float64, as OGB's own forward has it)
    s = np.ones(L, dtype) if eps is None else (1.0 + np.asarray(eps, np.float64) if eps_f64 else c(self_scale(eps)))
    N, G = batch.total_nodes, batch.num_graphs
    ge = batch.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    nn = c(batch.nums_of_nodes)[:, None]
    seg = lambda rows: np.add.reduceat(rows, off[:-1], axis=0)  # (every graph has a node)
    h = nemb[batch.node_feature.astype(np.int64) + ND_OFF[None, :]].sum(axis=1)
    vec = np.tile(E, (G, 1))
    big = [1.0, float(np.abs(h).max()), float(np.abs(vec).max())]

    def update(l, x, h_in, vec):
        rows = h_in if variant == "pool_before_add" else x
        t = seg(rows) / nn if variant == "mean_instead_of_sum" else seg(rows)
        if variant != "t_without_vn":
            t = t + vec
        k = (l + 1) % 4 if variant == "update_indexed_l_plus_1" else l
        hid = np.maximum(vmm(t, v1[k]) + c1[k], 0.0)
        out = np.maximum(vmm(hid, v2[k]) + c2[k], 0.0)
        big.extend([float(np.abs(t).max()), float(hid.max()), float(out.max())])
        return out

    for l in range(L):
        x = h if (l == L - 1 and variant == "no_add_in_last_layer") else h + vec[gid]
        ee = eemb[l][batch.edge_attr.astype(np.int64) + ED_OFF[None, :]].sum(axis=1)
        m = np.zeros((N, D), dtype)
        np.add.at(m, v, np.maximum(x[u] + ee, 0.0))
        a = m + s[l] * x
        hid = np.maximum(mm(a, w1[l]) + b1[l], 0.0)
        h_next = mm(hid, w2[l]) + b2[l]
        if l != L - 1:
            h_next = np.maximum(h_next, 0.0)
        big.extend([float(np.abs(x).max()), float(np.abs(a).max()), float(hid.max()), float(np.abs(h_next).max())])
        if l < L - 1:
            vec = update(l, x, h, vec)
        elif variant == NOOP_VARIANT:
            update(L - 2, x, h, vec)  # computed and dropped
        h = h_next
    if pooling == "mean":
        pooled = seg(h) / nn
    elif pooling == "sum":
        pooled = seg(h)
    else:
        assert pooling == "max", pooling
        pooled = np.maximum.reduceat(h, off[:-1], axis=0)
    big.append(float(np.abs(pooled).max()))
    out = pooled @ pw.T + pb
    return Out(out[:, 0] if out.shape[1] == 1 else out, h, pooled, max(big))


def split_operands(batch, w, vn, **kw):
    """The largest operand each split-f16 kernel sees, from the float64 forward alone: the raw input of a first product (|a|, |t|), and
    the hidden values times the first matrix's power-of-two pre-scale (the kernels keep the hidden layer pre-scaled).  -> (node MLP's,
    update's); the kernels raise the range flag at 6e4."""
    node, upd = split_ref.Recorder(), split_ref.Recorder()
    forward(batch, w, vn, dense=node, vn_dense=upd, **kw)

    def worst(rec, w1):
        m = 0.0
        for l, M in enumerate(np.asarray(w1, np.float32)):
            m = max(m, float(np.abs(rec.inputs[2 * l]).max()), split_ref.pow2_scale(M) * float(np.abs(rec.inputs[2 * l + 1]).max()))
        return m

    return worst(node, w["node_mlp_1_weights"]), worst(upd, vn["w1"])


def node_logits(w, rows):
    return W.node_logits(w, rows)


# ---------------------------------------------------------------- the OGB side
def ogb_forward(sd, batch):
    """Inference of the OGB example GNN with gnn_type='gin-virtual' (GNN_node_Virtualnode: JK='last', no residual; mean pooling), float64,
    nothing folded, at the state_dict's own width: tests/ogb_vn_ref.ogb_vn_forward without its hard-wired 100."""
    ge = batch.global_edges()
    row, col = ge[:, 0], ge[:, 1]
    N, G = batch.total_nodes, batch.num_graphs
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    h = sum(sd[f"gnn_node.atom_encoder.atom_embedding_list.{k}.weight"][batch.node_feature[:, k]] for k in range(9))
    D = h.shape[1]
    vec = np.tile(np.asarray(sd["gnn_node.virtualnode_embedding.weight"], np.float64).reshape(1, D), (G, 1))  # embedding(zeros(G))
    for l in range(L):
        c = f"gnn_node.convs.{l}"
        h = h + vec[gid]
        e = sum(sd[f"{c}.bond_encoder.bond_embedding_list.{k}.weight"][batch.edge_attr[:, k]] for k in range(3))
        agg = np.zeros((N, D))
        np.add.at(agg, col, np.maximum(h[row] + e, 0.0))
        z = ((1.0 + sd[f"{c}.eps"][0]) * h + agg) @ sd[f"{c}.mlp.0.weight"].T + sd[f"{c}.mlp.0.bias"]
        if f"{c}.mlp.1.weight" in sd:
            z = np.maximum(_bn(sd, f"{c}.mlp.1", z), 0.0) @ sd[f"{c}.mlp.3.weight"].T + sd[f"{c}.mlp.3.bias"]
        else:
            z = np.maximum(z, 0.0) @ sd[f"{c}.mlp.2.weight"].T + sd[f"{c}.mlp.2.bias"]
        if f"gnn_node.batch_norms.{l}.weight" in sd:
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


def vn_state_dict(seed=3, with_bn=True, tasks=1, width=WIDE, vn_w1_scale=1.0):
    """tests/gin_wide_ref.state_dict(virtual_node=True); with_bn also gives the virtual node's MLP its two BatchNorms (OGB's layout:
    Linear .0, BatchNorm .1, ReLU, Linear .3, BatchNorm .4, ReLU), as tests/ogb_vn_ref.vn_state_dict does at width 100.
    vn_w1_scale: a factor on the first linear layer of every update.  As generated (1.0) the vector explodes over four updates -- the
    logits of 40 molhiv-shaped graphs reach 2.3e5 -- and an engine runs such a checkpoint on its fp32 re-run; at 1 / 16 the exported
    model stays inside the split-f16 kernels' range (the largest operand they see is 4.3e3 on that batch), on the references alone."""
    from tests.test_export import _bn_params
    sd = W.state_dict(seed=seed, width=width, tasks=tasks, with_bn=with_bn, virtual_node=True)
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
def fixed_virtual_node(emb_dim=WIDE):
    """The virtual node of the fixed input: weights.synth_gin_virtual_node's random tensors, scaled per tensor in the way of
    tests/ogb_vn_ref.fixed_virtual_node and for the same reasons -- t is a SUM over the graph's nodes, so the first linear layer is
    scaled down until vn neither dies out nor explodes over four updates; the last two updates are scaled up until vn_3 and vn_4
    outweigh the rows they are added to, so that one part in n + 1 of t reaches the logits; the biases are scaled down so that they do
    not drown it; the embedding row is scaled up so that dropping E shows.  The factors differ from the 100-wide ones: with those,
    "pool_before_add" moves 38 % and "t_without_vn" none of the logits of 48 molhiv-shaped graphs by 10 x the bound at this width, so
    the first layer is scaled down less (0.1), the biases more (0.02), and the batch is one of small graphs (fixed_batch).  Chosen on
    the references alone (tests/test_gin_wide_vn_cpu.py prints what each wrong form reaches)."""
    vn = weights.synth_gin_virtual_node(seed=11, emb_dim=emb_dim)
    f32 = np.float32
    vn["vn_embedding"] = vn["vn_embedding"] * f32(16)
    vn["w1"] = vn["w1"] * f32(0.1)
    vn["w2"][2] *= f32(3)
    vn["w2"][3] *= f32(32)
    vn["b1"] = vn["b1"] * f32(0.02)
    vn["b2"] = vn["b2"] * f32(0.02)
    return OrderedDict((k, np.ascontiguousarray(v, dtype=np.float32)) for k, v in vn.items())


def shapes_virtual_node(emb_dim=WIDE, w1_scale=1.0 / 16):
    """The virtual node of the shape and configuration tests: weights.synth_gin_virtual_node(seed=11) with the first linear layer scaled
    by 1 / 16.  t is a sum over a graph's nodes (up to 300 of them in these tests), and at the synthetic scales, which are a node MLP's,
    every update multiplies the vector by about ten: after four of them the float64 forward itself passes 6e4, where the engine's
    fp32 re-run would compute every case and the kernels under test none.  A trained model's BatchNorm keeps the vector in range; this
    factor stands in for it.  Chosen on the float64 forward alone (tests/test_gin_wide_vn_cpu.py prints the scales)."""
    vn = weights.synth_gin_virtual_node(seed=11, emb_dim=emb_dim)
    vn["w1"] = vn["w1"] * np.float32(w1_scale)
    return vn


@functools.lru_cache(maxsize=None)
def fixed_batch():
    """The graphs of at most 12 nodes among 400 molhiv-shaped ones (33 of them, 8 .. 12 nodes): leaving `+ vn_l` out of t changes t by
    one part in n + 1, which shows in the logits only where n is small."""
    big = gp.synth_molhiv_batch(400, seed=29)
    return gp.concat_batches([big.slice(i, i + 1) for i in range(big.num_graphs) if big.nums_of_nodes[i] <= 12])


# ---------------------------------------------------------------- split-f16 separation with the virtual node on
# Batch seeds: 27 and 29, the two smallest seeds that leave both outputs at split_ref.MIN_RATIO (64) with the virtual node on.  The ROWS have
# E_bad / E_ok = 144 .. 231 at every seed tried; the LOGITS are short of 64 at most of them -- 3: 31.5, 5: 58.4, 7: 41.3, 10: 28.9, 11: 25.6,
# 12: 28.7, 13: 41.1, 14: 51.3, 15: 43.8, 16: 43.9, 17: 45.2, 18: 49.7, 19: 31.4, 20: 53.6, 21: 48.9, 22: 48.6, 24: 20.3, 25: 19.5, 26: 26.3,
# 28: 37.8 -- and reach it at 27: 78.2, 29: 69.8, 30: 64.1, 35: 77.1, 36: 73.1.  The closest wrong variant is "a_hi.w_lo dropped" in one
# K-step or for 16 output columns, as in section 4.16; the logit is a mean over rows that all carry the same vn, which dilutes a defect of
# that kind further, so fewer batches separate it by 64.  Chosen on the references alone, as tests/gin_wide_ref.SEEDS was.
SEP_GRAPHS = W.SEP_GRAPHS
SEP_OUTPUTS = W.SEP_OUTPUTS
SEEDS = (27, 29)
MIN_RATIO = split_ref.MIN_RATIO
Row = W.Row


@functools.lru_cache(maxsize=None)
def sep_virtual_node():
    return shapes_virtual_node()


@functools.lru_cache(maxsize=None)
def reference(seed):
    return forward(W.sep_batch(seed), W.sep_weights(), sep_virtual_node())


def misplaced_unscale_vn(vn):
    """split_ref.misplaced_unscale for the update's two matrices: every bias times its matrix's power of two."""
    out = OrderedDict((k, np.asarray(v, np.float32).copy()) for k, v in vn.items())
    for wk, bk in (("w1", "b1"), ("w2", "b2")):
        for l in range(L - 1):
            out[bk][l] = out[bk][l] * np.float32(split_ref.pow2_scale(out[wk][l]))
    return out


def err(got, ref, name):
    return W.err(got, ref, name)


@functools.lru_cache(maxsize=None)
def table(seed):
    """output name -> Row(E_ok, E_bad, B, per-restatement errors, per-variant errors), from the references alone: tests/gin_wide_ref.table
    with the virtual node on and the same restatement applied to the update's two products (an instance of its own, so that "the last
    layer" stays the node MLP's calls 8 and 9)."""
    b, w, vn, ref = W.sep_batch(seed), W.sep_weights(), sep_virtual_node(), reference(seed)
    sd = lambda spec: dict(dense=split_ref.SplitDense("GIN", spec), vn_dense=split_ref.SplitDense("GIN", spec))
    ok = {"all fp32": forward(b, w, vn, dense=split_ref.dense_fp32, vn_dense=split_ref.dense_fp32, dtype=np.float32)}
    for spec in split_ref.OK_SPECS:
        ok[spec.name] = forward(b, w, vn, **sd(spec))
    bad = {spec.name: forward(b, w, vn, **sd(spec)) for spec in W.variants()}
    bad[split_ref.BIAS_VARIANT] = forward(b, split_ref.misplaced_unscale("GIN", w), misplaced_unscale_vn(vn), **sd(split_ref.OK_SPECS[0]))
    rows = {}
    for name in SEP_OUTPUTS:
        eo = {k: err(getattr(v, name), ref, name) for k, v in ok.items()}
        eb = {k: err(getattr(v, name), ref, name) for k, v in bad.items()}
        e_ok, e_bad = max(eo.values()), min(eb.values())
        rows[name] = Row(e_ok, e_bad, float(np.sqrt(e_ok * e_bad)), eo, eb)
    return rows


# ---------------------------------------------------------------- the table as a fixture
GOLDEN = "gin_wide_vn_sep.json"  # tests/golden: `table` of the seeds in use, so that the GPU test does not spend 25 s per seed on it


def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)


def write_golden(seeds=None):
    """python -c "from tests import gin_wide_vn_ref as V; V.write_golden()": recompute `table` for SEEDS and write the fixture."""
    import json
    out = {"graphs": SEP_GRAPHS, "seeds": {}}
    for seed in (SEEDS if seeds is None else seeds):
        t = table(seed)
        out["seeds"][str(seed)] = {n: {"e_ok": t[n].e_ok, "e_bad": t[n].e_bad, "ok": t[n].ok, "bad": t[n].bad} for n in SEP_OUTPUTS}
    json.dump(out, open(golden_path(), "w"), indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def golden_table(seed):
    """`table(seed)` as the fixture recorded it (tests/test_gin_wide_vn_cpu.py checks the fixture against a recomputation)."""
    import json
    rec = json.load(open(golden_path()))
    assert rec["graphs"] == SEP_GRAPHS
    t = rec["seeds"][str(seed)]
    return {n: Row(t[n]["e_ok"], t[n]["e_bad"], float(np.sqrt(t[n]["e_ok"] * t[n]["e_bad"])), t[n]["ok"], t[n]["bad"]) for n in SEP_OUTPUTS}
