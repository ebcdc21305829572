"""Attention coefficients (flowgnn.h: flowgnn_set_attention): for layer l, head h and destination v, with the implicit self edge,
    e(u->v) = exp(leaky_0.2(ssrc_l[v][h] + stgt_l[u][h])),  den[v] = e(v->v) + sum over v's in-edges,  alpha = e / den,
stored per edge of the batch AS THE CALLER PASSED IT and per node (the self term) -- by gat_resident_attn_kernel (gat_attn.hip) on the
graph-resident path and by gat_attention_kernel beside every selected layer on every other path.

Expected values: a float64 restatement in this file, built from the oracle's dump (oracle.gat_forward(dump_h=True): the ELU outputs
o_0..o_3).  o_{-1} = the raw features in dims 0..8 of head 0, proj_l = o_{l-1} . mat(lin, l)^T as tests/numpy_ref.py::gat_forward has
it, then scores, e, den and alpha as above.

Bound: the project's row rule (tests/parity.py: |row error| <= REL * (scale + |row|) per element) carried through the softmax.  A
score is a dot product of a projection row with a scoring vector, so a score s = ssrc[v][h] + stgt[u][h] is off by at most
    ds = REL * (max(1, max |proj_l|) * (||a_src[l][h]||_1 + ||a_tgt[l][h]||_1) + |s|).
alpha_i = e_i / sum_j e_j: with every s_j of the destination's row off by at most D = max_j ds_j (the self term included), e_i moves
by a factor within exp(+-D) and so does the sum, alpha_i by a factor within exp(+-2 D).  So
    |got - want| <= want * expm1(2 D) + 2^-22                 (the constant: two fp32 roundings of a value <= 1)
with D taken per destination, layer and head.  Every comparison prints its ratio to that bound; DESIGN.md section 4.10 is where
the measured figures belong (none recorded yet: these tests have not run on a GPU, see there)."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, graphpack as gp, weights
from tests.golden.make_ref_weights import load as load_trained
from tests.parity import REL
from tests.test_embeddings_gpu import PER_LAYER, launched
from tests.test_resident_limits_gpu import LIMITS, random_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
f64 = lambda a: np.asarray(a, dtype=np.float64)
PER_LAYER_KERNELS = {"gat_layer", "gat_scores0", "gat_attention", "mean_pool_linear", "node_logits", "mean_pool_rows"}
OTHERS = ["GIN", "GIN-VN", "GCN", "PNA", "DGN"]


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """As tests/test_embeddings_gpu.py: torch's HIP context before the first engine exists."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


# ---------------------------------------------------------------- expected values and the bound
def expected(b, w, oracle, quirk=False):
    """-> (edge [5][E][4], self [5][N][4], D [5][N][4]): float64 coefficients and the bound's per-destination score error"""
    _, hd = oracle.gat_forward(b, [w], dump_h=True, nthreads=8, feature_offset_quirk=quirk)
    tgt, srcw, lin = f64(w["scoring_fn_target"]), f64(w["scoring_fn_source"]), f64(w["linear_proj_weights"])
    N = b.total_nodes
    ge = b.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    mat = lambda t, l: t[l].transpose(1, 0, 3, 2).reshape(64, 64)  # rows do*4+ho, cols di*4+hi (tests/numpy_ref.py)
    rows = np.arange(N)
    if quirk:  # gat_reference_quirk: every graph reads the first rows of the batch's feature array (GAT_compute.cc:72)
        rows = rows - np.repeat(b.node_offsets()[:-1], b.nums_of_nodes)
    o = np.zeros((N, 16, 4))
    o[:, :9, 0] = f64(b.node_feature)[rows]
    o = o.reshape(N, 64)
    edge, own, D = [], [], []
    for l in range(5):
        if l > 0:
            o = f64(hd[l - 1])
        p3 = (o @ mat(lin, l).T).reshape(N, 16, 4)
        ssrc, stgt = np.einsum("ndh,hd->nh", p3, srcw[l]), np.einsum("ndh,hd->nh", p3, tgt[l])
        leaky = lambda s: np.where(s < 0, 0.2 * s, s)
        s_e, s_s = ssrc[v] + stgt[u], ssrc + stgt
        e_e, e_s = np.exp(leaky(s_e)), np.exp(leaky(s_s))
        den = e_s.copy()
        np.add.at(den, v, e_e)
        edge.append(e_e / den[v])
        own.append(e_s / den)
        fixed = max(1.0, float(np.abs(p3).max())) * (np.abs(srcw[l]).sum(axis=1) + np.abs(tgt[l]).sum(axis=1))  # [4 heads]
        smax = np.abs(s_s)
        np.maximum.at(smax, v, np.abs(s_e))
        D.append(REL * (fixed[None, :] + smax))
    return np.stack(edge), np.stack(own), np.stack(D)


def ratio(got, want, D):
    """max of |got - want| / (want * expm1(2 D) + 2^-22); <= 1 passes"""
    got, want = f64(got), f64(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - want) / (want * np.expm1(2.0 * D) + 2.0 ** -22)).max())


def assert_attention(got, exp, b, mask, what):
    """got = (edge, self) of the layers in `mask`; exp = expected(...)"""
    sel = [l for l in range(5) if (mask >> l) & 1]
    edge, own = got
    v = b.global_edges()[:, 1]
    assert edge.dtype == np.float32 and own.dtype == np.float32
    assert edge.shape == (len(sel), b.total_edges, 4) and own.shape == (len(sel), b.total_nodes, 4), (what, edge.shape, own.shape)
    assert np.isfinite(edge).all() and np.isfinite(own).all(), what
    r_e = ratio(edge, exp[0][sel], exp[2][sel][:, v])
    r_s = ratio(own, exp[1][sel], exp[2][sel])
    print(what, "ratio to the bound: edges", round(r_e, 5), "self", round(r_s, 5), "| D from", float(exp[2][sel].min()), "to", float(exp[2][sel].max()))
    assert r_e <= 1.0 and r_s <= 1.0, (what, r_e, r_s)


def assert_normalised(got, b, what):
    """per node, head and layer: float64 sum of the self term and the in-edges' terms within (in_deg + 8) 2^-23 of 1; values in (0, 1]"""
    edge, own = got
    v = b.global_edges()[:, 1]
    indeg = np.bincount(v, minlength=b.total_nodes).astype(np.float64)
    assert (edge > 0).all() and (edge <= 1).all() and (own > 0).all() and (own <= 1).all(), what
    worst = 0.0
    for k in range(edge.shape[0]):
        tot = f64(own[k]).copy()
        np.add.at(tot, v, f64(edge[k]))
        worst = max(worst, float((np.abs(tot - 1.0) / ((indeg[:, None] + 8.0) * 2.0 ** -23)).max()))
    print(what, "normalisation: ratio to (in_deg + 8) 2^-23:", round(worst, 4))
    assert worst <= 1.0, (what, worst)


def run_on(w, b, mask=31, options=None, names=None, embeddings=False, node_embeddings=False, node_logits=False, engine_out=None):
    """-> (logits, (edge, self)) [+ the other outputs between them]; mask 0: logits alone"""
    e = Engine("GAT", device=0, options=options or {})
    try:
        e.set_weights(w)
        if names is not None:
            e.profile_enable(True)
        res = {}
        layers = [l for l in range(5) if (mask >> l) & 1] or None
        go = lambda: res.update(r=e.forward(b, return_embeddings=embeddings, return_node_embeddings=node_embeddings,
                                            return_node_logits=node_logits, return_attention=layers))
        if names is not None:
            names |= launched(e, go)
        else:
            go()
        if engine_out is not None:
            engine_out["exact_reruns"] = e.exact_reruns()
        return res["r"]
    finally:
        e.close()


def sharpened(w, factor=16.0):
    w2 = dict(w)
    for k in ("scoring_fn_target", "scoring_fn_source"):
        w2[k] = np.asarray(w[k], np.float32) * np.float32(factor)
    return w2


WEIGHTS = {"synthetic": lambda: weights.synth_gat_weights(seed=7),
           "sharpened x16": lambda: sharpened(weights.synth_gat_weights(seed=7)),
           "trained": lambda: load_trained("GAT")}


@pytest.fixture(scope="module")
def mol():
    return gp.synth_molhiv_batch(300, seed=13)


@pytest.fixture(scope="module")
def cases(oracle, mol):
    """weight set -> (weights, expected(...)) on the 300-graph batch: computed once, shared, left unchanged"""
    out = {}

    def get(name):
        if name not in out:
            w = WEIGHTS[name]()
            out[name] = (w, expected(mol, w, oracle))
        return out[name]
    return get


@pytest.fixture(scope="module")
def full(cases, mol):
    """the mask-31 run of the synthetic set on the resident path: (logits, (edge, self))"""
    return run_on(cases("synthetic")[0], mol)


# ---------------------------------------------------------------- 1. parity on the resident path
@pytest.mark.parametrize("wset", list(WEIGHTS))
def test_resident_path_parity(wset, cases, mol):
    w, exp = cases(wset)
    ge = mol.global_edges()
    assert not np.array_equal(np.lexsort((ge[:, 0], ge[:, 1])), np.arange(len(ge))), "the caller's edge order must not be CSR order"
    tiles_probe = Engine("GAT", device=0)
    tiles_probe.set_weights(w)
    tiles_probe.set_batch(mol)
    assert tiles_probe.batch_tiles()[0] >= 3, tiles_probe.batch_tiles()  # later tiles: e0 != 0, t0 != 0
    tiles_probe.close()
    names = set()
    logits, attn = run_on(w, mol, names=names)
    off = run_on(w, mol, mask=0)
    assert "gat_resident" in names and not names & PER_LAYER_KERNELS, names
    assert np.array_equal(logits, off)
    assert_attention(attn, exp, mol, 31, ("resident", wset))
    assert_normalised(attn, mol, ("resident", wset))


# ---------------------------------------------------------------- 3. the order of the caller's edge list
def test_edge_order_invariance(cases, mol, full):
    w, _ = cases("synthetic")
    rng = np.random.default_rng(5)
    eo = mol.edge_offsets()
    perm = np.concatenate([eo[g] + rng.permutation(eo[g + 1] - eo[g]) for g in range(mol.num_graphs)]).astype(np.int64)
    shuffled = gp.GraphBatch(mol.nums_of_nodes, mol.nums_of_edges, mol.node_feature, mol.edge_list[perm], mol.edge_attr[perm])
    logits, (edge, own) = run_on(w, shuffled)
    back = np.empty_like(edge)
    back[:, perm] = edge  # edge i of the shuffled batch is edge perm[i] of the original
    assert np.array_equal(back, full[1][0]) and np.array_equal(own, full[1][1]) and np.array_equal(logits, full[0])


# ---------------------------------------------------------------- 4. the layer mask
@pytest.mark.parametrize("mask", [16, 1, 0b10001])
def test_layer_mask(mask, cases, mol, full):
    w, _ = cases("synthetic")
    sel = [l for l in range(5) if (mask >> l) & 1]
    for opts in ({}, {"gat_resident": 0}):
        logits, (edge, own) = run_on(w, mol, mask=mask, options=opts)
        assert edge.shape == (len(sel), mol.total_edges, 4) and own.shape == (len(sel), mol.total_nodes, 4)
        if not opts:
            assert np.array_equal(edge, full[1][0][sel]) and np.array_equal(own, full[1][1][sel]) and np.array_equal(logits, full[0])
        else:
            _, (e31, o31) = run_on(w, mol, mask=31, options=opts)
            assert np.array_equal(edge, e31[sel]) and np.array_equal(own, o31[sel])


# ---------------------------------------------------------------- 5. edges of the shapes
def shape_edges_batch():
    m = gp.synth_molhiv_batch(30, seed=4)
    rng = np.random.default_rng(5)

    def graph(n, edges):
        nf = np.stack([rng.integers(0, c, n) for c in (119, 4, 12, 12, 10, 6, 6, 2, 2)], 1).astype(np.int32)
        el = np.asarray(edges, np.int32).reshape(-1, 2)
        ea = np.stack([rng.integers(0, 5, len(el)), rng.integers(0, 6, len(el)), rng.integers(0, 2, len(el))], 1).astype(np.int32)
        return gp.GraphBatch(np.array([n], np.int32), np.array([len(el)], np.int32), nf, el, ea.reshape(-1, 3))
    star = [[i, 0] for i in range(1, 41)] + [[0, i] for i in range(1, 41, 3)]  # the hub (node 0) has in-degree 40
    dup = [[0, 1], [1, 2], [0, 1], [2, 0], [1, 0], [0, 1]]
    parts = [m.slice(0, 7), graph(1, []), graph(1, [[0, 0]]), graph(5, []), m.slice(7, 19), graph(17, []), graph(2, [[0, 1], [1, 0]]),
             graph(3, dup), graph(41, star), m.slice(19, 30), random_graph(*[LIMITS["GAT"][0], LIMITS["GAT"][0] + 40], seed=1)]
    first = np.cumsum([0] + [p.num_graphs for p in parts])
    return gp.concat_batches(parts), {"lone": first[1], "loop": first[2], "dup": first[7], "star": first[8]}


def test_shape_edges(oracle):
    b, at = shape_edges_batch()
    w = weights.synth_gat_weights(seed=11)
    exp = expected(b, w, oracle)
    names = set()
    logits, attn = run_on(w, b, names=names)
    assert "gat_resident" in names and not names & PER_LAYER_KERNELS, names
    assert_attention(attn, exp, b, 31, "shape edges")
    assert_normalised(attn, b, "shape edges")
    edge, own = attn
    no, eo = b.node_offsets(), b.edge_offsets()
    assert (own[:, no[at["lone"]]] == 1.0).all()                      # a node without any edge: the self term is everything
    lo_n, lo_e = no[at["loop"]], eo[at["loop"]]
    assert np.abs(own[:, lo_n] - 0.5).max() <= 2.0 ** -23 and np.abs(edge[:, lo_e] - 0.5).max() <= 2.0 ** -23
    d = eo[at["dup"]]
    assert np.array_equal(edge[:, d], edge[:, d + 2]) and np.array_equal(edge[:, d], edge[:, d + 5])  # the three [0, 1] entries
    hub_in = eo[at["star"]] + np.arange(40)
    assert (b.global_edges()[hub_in, 1] == no[at["star"]]).all()
    # ... and the same batch on the per-layer path
    names = set()
    _, attn2 = run_on(w, b, options={"gat_resident": 0}, names=names)
    assert "gat_attention" in names and "gat_resident" not in names, names
    assert_attention(attn2, exp, b, 31, "shape edges, per-layer path")
    assert_normalised(attn2, b, "shape edges, per-layer path")
    assert (attn2[1][:, no[at["lone"]]] == 1.0).all()


# ---------------------------------------------------------------- 6. every other path
@pytest.mark.parametrize("opts", PER_LAYER["GAT"] + [{"gat_resident": 0, "gat_mfma": 32}])
def test_per_layer_paths(opts, cases, mol):
    w, exp = cases("synthetic")
    names = set()
    logits, attn = run_on(w, mol, options=opts, names=names)
    assert "gat_attention" in names and "gat_resident" not in names, names
    assert_attention(attn, exp, mol, 31, opts)
    assert_normalised(attn, mol, opts)


def test_batch_below_the_fill_threshold(oracle):
    """Graphs of 100 nodes and 700 edges: one per tile by the edge limit, 39 % full -- the per-layer kernels take the batch."""
    b = gp.concat_batches([random_graph(100, 700, seed=s) for s in range(12)])
    w = weights.synth_gat_weights(seed=11)
    names = set()
    _, attn = run_on(w, b, names=names)
    assert "gat_attention" in names and "gat_resident" not in names, names
    assert_attention(attn, expected(b, w, oracle), b, 31, "below the fill threshold")
    assert_normalised(attn, b, "below the fill threshold")


def test_a_graph_beyond_the_tile_limit(oracle):
    m = gp.synth_molhiv_batch(30, seed=8)
    b = gp.concat_batches([m.slice(0, 20), random_graph(300, 330, seed=5), m.slice(20, 30)])
    w = weights.synth_gat_weights(seed=11)
    names = set()
    _, attn = run_on(w, b, names=names)
    assert "gat_attention" in names and "gat_resident" not in names, names
    assert_attention(attn, expected(b, w, oracle), b, 31, "beyond the tile limit")


@pytest.mark.parametrize("other", ["embeddings", "node_embeddings", "node_logits"])
def test_together_with_the_other_outputs(other, cases, mol, full):
    w, exp = cases("synthetic")
    names = set()
    res = run_on(w, mol, names=names, **{other: True})
    assert len(res) == 3
    assert_attention(res[2], exp, mol, 31, other)
    if other == "node_logits":  # the attention instance stores them too: the resident launch and everyone's bits are kept
        assert "gat_resident" in names and not names & PER_LAYER_KERNELS, names
        assert np.array_equal(res[0], full[0]) and np.array_equal(res[2][0], full[1][0]) and np.array_equal(res[2][1], full[1][1])
        alone = run_on(w, mol, mask=0, node_logits=True)
        assert np.array_equal(res[1], alone[1])
    else:  # GAT leaves the resident kernel for the rows: attention comes from the per-layer path
        assert "gat_attention" in names and "gat_resident" not in names, names
        alone = run_on(w, mol, mask=0, **{other: True})
        assert np.array_equal(res[0], alone[0]) and np.array_equal(res[1], alone[1])


def test_exact_rerun_refills(oracle, mol):
    """o_0 of the order 1e5 (W_skip_0 scaled up, layer 1's two matrices scaled down by as much) leaves the split's range: the pass is
    repeated on the fp32 kernels, and the attention coefficients are refilled with the logits."""
    w = dict(weights.synth_gat_weights(seed=7))
    skip, lin = np.array(w["skip_proj_weights"], np.float32), np.array(w["linear_proj_weights"], np.float32)
    skip[0] *= np.float32(2.0 ** 20)
    skip[1] *= np.float32(2.0 ** -20)
    lin[1] *= np.float32(2.0 ** -20)
    w["skip_proj_weights"], w["linear_proj_weights"] = skip, lin
    info, names = {}, set()
    _, attn = run_on(w, mol, engine_out=info, names=names)
    assert info["exact_reruns"] == 1
    assert "gat_resident" in names and "gat_attention" in names, names  # the first pass, then the refill
    assert_attention(attn, expected(mol, w, oracle), mol, 31, "exact re-run")
    _, again = run_on(w, mol, options={"gat_resident": 0, "gat_mfma": 32})
    assert np.array_equal(attn[0], again[0]) and np.array_equal(attn[1], again[1])  # the refill is the fp32 path's values


@pytest.mark.parametrize("opts", [{}, {"gat_resident": 0}])
def test_reference_quirk(opts, oracle, mol):
    w = weights.synth_gat_weights(seed=7)
    exp = expected(mol, w, oracle, quirk=True)
    assert np.abs(exp[0] - expected(mol, w, oracle)[0]).max() > 1e-3  # the quirk changes the coefficients
    names = set()
    _, attn = run_on(w, mol, options=dict(opts, gat_reference_quirk=1), names=names)
    assert ("gat_resident" in names) == (not opts), names
    assert_attention(attn, exp, mol, 31, ("quirk", opts))


# ---------------------------------------------------------------- 7. bit identity, state
def test_bit_identity_and_state():
    torch = pytest.importorskip("torch")
    b, w = gp.synth_molhiv_batch(1200, seed=13), weights.synth_gat_weights(seed=7)
    G, no, eo = b.num_graphs, b.node_offsets(), b.edge_offsets()
    e = Engine("GAT", device=0)
    e.set_weights(w)
    logits, (edge, own) = e.forward(b, return_attention="all")
    # a slice computed as a shard of the whole job
    e.set_job_totals(b.total_nodes, b.total_edges)
    e.set_job_tile_fill(e.graph_tile_fill(b.nums_of_nodes, b.nums_of_edges))
    plog, (pe, ps) = e.forward(b.slice(G // 4, 3 * G // 4), return_attention="all")
    e.set_job_totals()
    e.set_job_tile_fill()
    assert np.array_equal(pe, edge[:, eo[G // 4]: eo[3 * G // 4]]) and np.array_equal(ps, own[:, no[G // 4]: no[3 * G // 4]])
    assert np.array_equal(plog, logits[G // 4: 3 * G // 4])
    # on -> off -> on reproduces itself (and survives set_batch); off, the values are not to be had
    e.set_batch(b)
    e.set_attention(None)
    e.run()
    assert np.array_equal(e.results(), logits)
    for fn in (e.attention, e.attention_device_ptrs):
        with pytest.raises(FlowGNNError) as ei:
            fn()
        assert ei.value.code == 6
    e.set_attention("all")
    with pytest.raises(FlowGNNError) as ei:  # switched on, but no run since
        e.attention()
    assert ei.value.code == 6
    e.set_batch(b)
    e.run()
    a2 = e.attention()
    assert np.array_equal(a2[0], edge) and np.array_equal(a2[1], own) and np.array_equal(e.results(), logits)
    # caller-owned buffers (stream-ordered: no host sync in the call), then back to the engine's own
    n_e, n_n = 5 * b.total_edges * 4, 5 * b.total_nodes * 4
    te = torch.full((n_e,), -1.0, dtype=torch.float32, device="cuda:0")
    ts = torch.full((n_n,), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    own_ptrs = e.attention_device_ptrs()
    e.set_attention_buffers(te.data_ptr(), ts.data_ptr())
    e.run()
    e.sync()
    assert e.attention_device_ptrs() == (te.data_ptr(), ts.data_ptr())
    assert np.array_equal(te.cpu().numpy().reshape(edge.shape), edge) and np.array_equal(ts.cpu().numpy().reshape(own.shape), own)
    e.set_attention_buffers(None, None)
    e.run()
    e.sync()
    assert e.attention_device_ptrs() == own_ptrs
    # an empty batch
    _, (ee, es) = e.forward(b.slice(0, 0), return_attention=[0, 4])
    assert ee.shape == (2, 0, 4) and es.shape == (2, 0, 4)
    e.close()
    # a two-member group on one device = one engine
    g = EngineGroup("GAT", [0, 0])
    g.set_weights(w)
    g.set_attention("all")
    assert np.array_equal(g.forward(b), logits)
    ge_, gs_ = g.attention()
    assert np.array_equal(ge_, edge) and np.array_equal(gs_, own)
    g.close()
    # launch-sequence replay = direct launches
    h = Engine("GAT", device=0, options={"hipgraph": 1})
    h.set_weights(w)
    h.set_batch(b)
    h.run()
    h.run()
    h.set_attention("all")  # drops the recording made with attention off
    replays0 = h.graph_replays()
    outs = []
    for _ in range(4):
        h.run()
        outs.append((h.results().copy(), h.attention()))
    assert replays0 >= 1 and h.graph_replays() - replays0 >= 1
    assert all(np.array_equal(o[0], logits) and np.array_equal(o[1][0], edge) and np.array_equal(o[1][1], own) for o in outs)
    h.close()


# ---------------------------------------------------------------- 8. refusals
@pytest.mark.parametrize("model", OTHERS)
def test_other_models_refuse(model):
    e = Engine(model, device=0)
    with pytest.raises(FlowGNNError) as ei:
        e.set_attention("last")
    assert ei.value.code == 8 and "only GAT" in str(ei.value)
    e.close()
    g = EngineGroup(model, [0, 0])
    with pytest.raises(FlowGNNError) as ei:
        g.set_attention("last")
    assert ei.value.code == 8
    g.close()


def test_fixed_point_refuses_both_ways_round_and_bad_masks():
    e = Engine("GAT", device=0)
    e.set_weights(weights.synth_gat_weights(seed=7))
    e.set_numeric_mode("q6.10")
    with pytest.raises(FlowGNNError) as ei:
        e.set_attention("last")
    assert ei.value.code == 8 and "fixed-point" in str(ei.value)
    e.set_numeric_mode("f32")
    e.set_attention("last")
    with pytest.raises(FlowGNNError) as ei:
        e.set_numeric_mode("q6.10")
    assert ei.value.code == 8 and "attention" in str(ei.value)
    for bad in (32, -1, 1 << 10):
        assert e.lib.flowgnn_set_attention(e._h, bad) == 1  # FLOWGNN_ERR_ARG
    e.close()


# ---------------------------------------------------------------- 9. device path
def test_forward_device_returns_device_tensors():
    torch = pytest.importorskip("torch")
    b, w = gp.synth_molhiv_batch(700, seed=9), weights.synth_gat_weights(seed=7)
    e = Engine("GAT", device=0)
    try:
        e.set_weights(w)
        want_logits, (want_e, want_s) = e.forward(b, return_attention="last")
        d = b.to_pyg("cuda:0")
        logits, (te, ts) = e.forward_device(d["x"], d["edge_index"], None, None, ptr=d["ptr"], return_attention="last")
        e.sync()
        for t, shape in ((te, (1, b.total_edges, 4)), (ts, (1, b.total_nodes, 4))):
            assert isinstance(t, torch.Tensor) and t.device == torch.device("cuda:0") and tuple(t.shape) == shape
        torch.cuda.synchronize()
        assert np.array_equal(te.cpu().numpy(), want_e) and np.array_equal(ts.cpu().numpy(), want_s)
        assert np.array_equal(logits.cpu().numpy(), want_logits)
        assert e.attention_device_ptrs() == (te.data_ptr(), ts.data_ptr())
    finally:
        e.close()


# ---------------------------------------------------------------- 10. host CLI
def test_host_cli(tmp_path):
    w = weights.synth_gat_weights(seed=7)
    b = gp.synth_molhiv_batch(40, seed=3)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    weights.SAVERS["GAT"](w, str(wdir))
    outs = []
    for extra in ([], ["--attention", str(tmp_path / "attn.txt")], ["--attention", str(tmp_path / "attn2.txt"), "--attention-layers", "17"]):
        out = tmp_path / f"HLS_output_{len(extra)}.txt"
        r = subprocess.run([HOST, "GAT", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--out", str(out)] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(open(out).read())
    assert outs[0] == outs[1] == outs[2]  # the flags leave HLS_output.txt as it was
    _, (edge, _own) = run_on(w, b, mask=17)
    for name, sel in (("attn.txt", [1]), ("attn2.txt", [0, 1])):
        rows = np.array([[float(x) for x in ln.split()] for ln in open(tmp_path / name).read().strip().splitlines()])
        want = edge[sel]
        assert rows.shape == (len(sel) * b.total_edges, 6)
        layers = [4] if name == "attn.txt" else [0, 4]
        assert np.array_equal(rows[:, 0], np.repeat(layers, b.total_edges)) and np.array_equal(rows[:, 1], np.tile(np.arange(b.total_edges), len(sel)))
        assert np.abs(rows[:, 2:] - f64(want).reshape(-1, 4)).max() <= 1e-8  # the file's 8 decimals (values <= 1)


# ---------------------------------------------------------------- 11. speed
def test_speed_guard():
    """The last layer's attention (mask 16) out of the graph-resident kernel against the same out of the per-layer path (gat_resident
    0) -- the only other way to these values -- same process, same batch of 2^16 graphs, the two engines alternating; device-event
    time of all kernels of a step (profile_read), best of three medians of ten.  No margin, no absolute figure."""
    b = gp.synth_molhiv_batch(1 << 16, seed=3)
    w = weights.synth_gat_weights(seed=7)
    eng = {}
    for key, opts in (("resident", {}), ("per_layer", {"gat_resident": 0})):
        e = Engine("GAT", device=0, options=opts)
        e.set_weights(w)
        e.set_attention("last")
        e.set_batch(b)
        e.profile_enable(True)
        e.run()
        e.results()
        eng[key] = e
    assert "gat_resident" in eng["resident"].profile_read() and "gat_attention" in eng["per_layer"].profile_read()

    def median_ms(e, runs=10):
        total = lambda: sum(v["total_ms"] for v in e.profile_read().values())
        ms = []
        for _ in range(runs):
            t0 = total()
            e.run()
            e.sync()
            ms.append(total() - t0)
        return float(np.median(ms))

    m = {"resident": [], "per_layer": []}
    for _ in range(3):
        for key in ("per_layer", "resident"):
            m[key].append(median_ms(eng[key]))
    for e in eng.values():
        e.close()
    print("GAT step with the last layer's attention, resident:", m["resident"], "per-layer:", m["per_layer"])
    assert min(m["resident"]) <= min(m["per_layer"]), m
