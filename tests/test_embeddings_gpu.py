"""Graph embeddings (flowgnn.h: flowgnn_set_embeddings): emb[g] = the mean over the graph's nodes of the rows the model's readout head
is applied to, produced beside the logits -- on chip by the graph-resident kernels of GIN / GIN-VN / PNA / DGN, by the per-layer path
plus mean_pool_rows_kernel for GCN / GAT.

Expected values: the float64 per-graph mean of the oracle's last dumped layer (GIN h_5, PNA / DGN h_4).  The GCN and GAT dumps stop one
stage short of the rows the readout pools (GCN: x_4, GAT: the ELU output of layer 3), so `gcn_last_stage` / `gat_last_stage` below
restate that one stage in float64 (tests/numpy_ref.py's equations) on the oracle's last dumped rows; each first reproduces the
oracle's logits through the linear head before it serves as an expected value.  Tolerance: tests/parity.py, REL = 1e-4, scale = the
oracle's largest activation."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, embedding_dim, graphpack as gp, weights
from tests import f16_ref
from tests.parity import assert_close, oracle_scale
from tests.test_resident_limits_gpu import random_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
MODELS = ["GIN", "GIN-VN", "GCN", "GAT", "PNA", "DGN"]
ND_OFF = np.array([0, 119, 123, 135, 147, 157, 163, 169, 171])
ED_OFF = np.array([0, 5, 11])
PER_LAYER = {
    "GIN": [{"gin_resident": 0}, {"gin_resident": 0, "gin_fold_readout": 0}],
    "GIN-VN": [{"gin_resident": 0}],
    "GCN": [{"gcn_resident": 0}, {"gcn_resident": 0, "gcn_unfused": 1}],
    "GAT": [{"gat_resident": 0}, {"gat_resident": 0, "gat_fold_readout": 0}],
    "PNA": [{"pna_resident": 0}, {"pna_resident": 0, "pna_fused": 0}],
    "DGN": [{"dgn_resident": 0}, {"dgn_resident": 0, "dgn_fold_readout": 0}, {"dgn_resident": 0, "dgn_fused": 0}],
}
f64 = lambda a: np.asarray(a, dtype=np.float64)


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """The tests below that hand torch tensors to the engine need torch's HIP context, and torch finds no device when it initialises
    after the process has destroyed an engine (so it does on the parent commit): initialise it before the first engine exists, as
    tests/test_device_batch_gpu.py does by running early in the suite."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def base(model):
    return model.replace("-VN", "").lower()


def model_weights(model, seed=7, num_tasks=1):
    fn = getattr(weights, f"synth_{base(model)}_weights")
    return fn(seed=seed, num_tasks=num_tasks) if num_tasks != 1 else fn(seed=seed)


def model_batch(model, num_graphs, seed):
    if model in ("PNA", "DGN"):
        return gp.synth_hep10k_batch(num_graphs, seed=seed, with_eigen=model == "DGN")
    b = gp.synth_molhiv_batch(num_graphs, seed=seed)
    return gp.add_virtual_nodes(b) if model == "GIN-VN" else b


def pooled(rows, b):
    return np.add.reduceat(f64(rows), b.node_offsets()[:-1], axis=0) / f64(b.nums_of_nodes)[:, None]


def gcn_last_stage(b, w, x4):
    """numpy_ref.gcn_forward at l = 4 on the oracle's x_4: edge term, normalised sum, root term, BatchNorm, no ReLU."""
    eemb, root = f64(w["edge_embedding_weight"]), f64(w["convs_root_emb_weight"])
    bnw, bnb, bnm, bnv = f64(w["bn_weight"]), f64(w["bn_bias"]), f64(w["bn_mean"]), f64(w["bn_var"])
    N, x = b.total_nodes, f64(x4)
    ge = b.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    outdeg = np.bincount(u, minlength=N).astype(np.float64)
    dinv = np.where(outdeg > 0, 1.0 / np.sqrt(outdeg + 1.0), 0.0)
    norm = dinv[u] * dinv[v]
    ee = eemb[4][b.edge_attr.astype(np.int64) + ED_OFF[None, :]].sum(axis=1)
    m = np.zeros((N, 100))
    np.add.at(m, v, norm[:, None] * np.maximum(x[u] + ee, 0.0))
    t = m + np.maximum(x + root[4], 0.0) / (outdeg[:, None] + 1.0)
    return (t - bnm[4]) / np.sqrt(bnv[4] + 2.0 ** -10) * bnw[4] + bnb[4]


def gat_last_stage(b, w, o3):
    """numpy_ref.gat_forward's l == 4 branch on the oracle's ELU output of layer 3: projection, attention, skip, mean over the heads."""
    tgt, srcw = f64(w["scoring_fn_target"]), f64(w["scoring_fn_source"])
    lin, skip = f64(w["linear_proj_weights"]), f64(w["skip_proj_weights"])
    mat = lambda t, l: t[l].transpose(1, 0, 3, 2).reshape(64, 64)
    N, o = b.total_nodes, f64(o3)
    ge = b.global_edges()
    u = np.concatenate([np.arange(N), ge[:, 0]])
    v = np.concatenate([np.arange(N), ge[:, 1]])
    p3 = (o @ mat(lin, 4).T).reshape(N, 16, 4)
    ssrc = np.einsum("ndh,hd->nh", p3, srcw[4])
    stgt = np.einsum("ndh,hd->nh", p3, tgt[4])
    s = ssrc[v] + stgt[u]
    e = np.exp(np.where(s < 0, 0.2 * s, s))
    den = np.zeros((N, 4))
    np.add.at(den, v, e)
    num = np.zeros((N, 16, 4))
    np.add.at(num, v, e[:, None, :] * p3[u])
    out = (num / den[:, None, :]).reshape(N, 64) + o @ mat(skip, 4).T
    return out.reshape(N, 16, 4).mean(axis=2)


def head(model, w, emb):
    """The model's readout head on pooled rows, float64."""
    emb = f64(emb)
    if model in ("GIN", "GIN-VN", "GCN", "GAT"):
        D = emb.shape[1]
        out = emb @ f64(w["graph_pred_weights"]).reshape(-1, D).T + f64(w["graph_pred_bias"]).reshape(-1)
        return out[:, 0] if out.shape[1] == 1 else out
    k = (("graph_mlp_1", "graph_mlp_2", "graph_mlp_3") if model == "PNA"
         else ("MLP_layer_FC_layers_0", "MLP_layer_FC_layers_1", "MLP_layer_FC_layers_2"))
    wk = (lambda n: n + "_weights") if model == "PNA" else (lambda n: n + "_weight")
    o1 = np.maximum(emb @ f64(w[wk(k[0])]).T + f64(w[k[0] + "_bias"]), 0.0)
    o2 = np.maximum(o1 @ f64(w[wk(k[1])]).T + f64(w[k[1] + "_bias"]), 0.0)
    return o2 @ f64(w[wk(k[2])]).reshape(-1) + float(np.asarray(w[k[2] + "_bias"]).reshape(-1)[0])


def expected(model, b, w, oracle):
    """(oracle logits, expected embeddings float64, activation scale)"""
    want, hd = getattr(oracle, f"{base(model)}_forward")(b, [w], dump_h=True, nthreads=8)
    scale = oracle_scale(hd)
    if model == "GCN":
        rows = gcn_last_stage(b, w, hd[4])
    elif model == "GAT":
        rows = gat_last_stage(b, w, hd[3])
    else:
        rows = hd[-1]
    emb = pooled(rows, b)
    if model in ("GCN", "GAT"):  # the restatement proves itself on the oracle's logits first
        assert_close(head(model, w, emb), want, scale=scale, what=(model, "restated last stage vs the oracle's logits"))
    return want, emb, scale


def assert_logits(model, got, want, scale, what):
    if model in ("GIN", "GIN-VN", "GCN"):  # the rule of tests/test_gin_gpu.py / test_gcn_gpu.py
        assert np.isfinite(got).all() and np.allclose(got, want, rtol=1e-4, atol=1e-4), (what, float(np.abs(got - want).max()))
    else:
        assert_close(got, want, scale=scale, what=what)


def run_on(model, w, b, options=None, num_tasks=1, numeric=None):
    e = Engine(model, device=0, options=options or {})
    try:
        if num_tasks != 1:
            e.set_num_tasks(num_tasks)
        e.set_weights(w)
        if numeric:
            e.set_numeric_mode(numeric)
        return e.forward(b, return_embeddings=True)
    finally:
        e.close()


def launched(e, fn):
    """Names of the profile slots that gain launches while fn() runs (and is synchronised)."""
    before = {k: v["launches"] for k, v in e.profile_read().items()}
    fn()
    e.sync()
    after = e.profile_read()
    return {k for k, v in after.items() if v["launches"] > before.get(k, 0)}


# ---------------------------------------------------------------- 1. parity at dataset-shaped batches
@pytest.fixture(scope="module")
def cases(oracle):
    """model -> (batch, weights, oracle logits, expected embeddings, scale), computed once"""
    out = {}

    def get(model):
        if model not in out:
            b = model_batch(model, 512 if model in ("PNA", "DGN") else 4113, seed=13)
            w = model_weights(model)
            out[model] = (b, w) + expected(model, b, w, oracle)
        return out[model]
    return get


@pytest.mark.parametrize("model", MODELS)
def test_parity(model, cases):
    b, w, want, want_emb, scale = cases(model)
    logits, emb = run_on(model, w, b)
    assert emb.shape == (b.num_graphs, embedding_dim(model)) and emb.dtype == np.float32
    print(model, "max |emb - want| =", float(np.abs(emb - want_emb).max()), "scale", scale)
    assert_close(emb, want_emb, scale=scale, what=(model, "embeddings"))
    assert_logits(model, logits, want, scale, (model, "logits"))


# ---------------------------------------------------------------- 2. every path
@pytest.mark.parametrize("model", MODELS)
def test_per_layer_paths(model, cases):
    b, w, want, want_emb, scale = cases(model)
    for opts in PER_LAYER[model]:
        logits, emb = run_on(model, w, b, options=opts)
        assert_close(emb, want_emb, scale=scale, what=(model, opts, "embeddings"))
        assert_logits(model, logits, want, scale, (model, opts, "logits"))


def test_gin_multi_task(oracle):
    b = gp.synth_molhiv_batch(1500, seed=17)
    w = weights.synth_gin_weights(seed=7, num_tasks=2)
    want, hd = oracle.gin_forward(b, [w], dump_h=True, nthreads=8, num_tasks=2)
    for opts in ({}, {"gin_resident": 0}):
        logits, emb = run_on("GIN", w, b, options=opts, num_tasks=2)
        assert_close(emb, pooled(hd[5], b), scale=oracle_scale(hd), what=("NUM_TASK 2", opts))
        assert np.allclose(logits, np.asarray(want).reshape(logits.shape), rtol=1e-4, atol=1e-4)
        assert_close(head("GIN", w, emb), logits, scale=oracle_scale(hd), what="head(emb), NUM_TASK 2")


def test_gin_batch_below_the_fill_threshold(oracle, gin_weights):
    """Graphs of 100 nodes and 700 edges: one per tile by the edge limit, 39 % full -- the per-layer kernels take the batch."""
    b = gp.concat_batches([random_graph(100, 700, seed=s) for s in range(12)])
    e = Engine("GIN", device=0)
    e.set_weights(gin_weights)
    assert e.graph_tile_fill(b.nums_of_nodes, b.nums_of_edges) < 0.5
    e.profile_enable(True)
    res = {}
    names = launched(e, lambda: res.update(r=e.forward(b, return_embeddings=True)))
    e.close()
    assert "gin_resident" not in names and "mean_pool_rows" in names, names
    want, hd = oracle.gin_forward(b, [gin_weights], dump_h=True, nthreads=8)
    assert_close(res["r"][1], pooled(hd[5], b), scale=oracle_scale(hd), what="below the fill threshold")
    assert np.allclose(res["r"][0], want, rtol=1e-4, atol=1e-4)


def f16_unfolded(batch, w):
    """tests/f16_ref.gin_forward(fold=False, rnd="rne"): the logits and the pooled h_5 (single task)."""
    o = f16_ref.gin_forward(batch, w, fold=False, rnd="rne", outputs=("logits", "pooled"))
    return o["logits"], o["pooled"]


def test_gin_f16_mode(oracle, gin_weights):
    b = gp.synth_molhiv_batch(1200, seed=13)
    want, want_emb = f16_unfolded(b, gin_weights)
    assert np.allclose(want, f16_ref.gin_forward(b, gin_weights, fold=False), rtol=1e-12, atol=1e-12)  # the restatement is f16_ref's
    _, hd = oracle.gin_forward(b, [gin_weights], dump_h=True, nthreads=8)
    scale = oracle_scale(hd)
    for opts in ({}, {"gin_resident": 0}):
        logits, emb = run_on("GIN", gin_weights, b, options=opts, numeric="f16")
        assert_close(emb, want_emb, scale=scale, what=("f16", opts, "embeddings"))
        assert_close(logits, want, scale=scale, what=("f16", opts, "logits"))
    _, emb32 = run_on("GIN", gin_weights, b)
    assert float(np.abs(emb.astype(np.float64) - emb32).max()) > 1e-6  # the mode did change the arithmetic


# ---------------------------------------------------------------- 3. head consistency
@pytest.mark.parametrize("model", MODELS)
def test_head_of_the_embeddings_is_the_logit(model, cases):
    b, w, want, want_emb, scale = cases(model)
    logits, emb = run_on(model, w, b)
    assert_close(head(model, w, emb), logits, scale=scale, what=(model, "head(emb) vs the run's logits"))


# ---------------------------------------------------------------- 4. off means off
@pytest.mark.parametrize("model", MODELS)
def test_off_means_off(model):
    b, w = model_batch(model, 300 if model in ("PNA", "DGN") else 2000, seed=5), model_weights(model)
    e = Engine(model, device=0)
    e.set_weights(w)
    e.profile_enable(True)
    e.set_batch(b)
    res = {}
    names0 = launched(e, lambda: (e.run(), res.update(first=e.results().copy())))
    e.set_embeddings(True)
    names_on = launched(e, lambda: (e.run(), res.update(on=e.results().copy(), emb=e.embeddings())))
    e.set_embeddings(False)
    names2 = launched(e, lambda: (e.run(), res.update(last=e.results().copy())))
    e.close()
    assert np.array_equal(res["last"], res["first"]) and names2 == names0, (names0, names2)
    assert np.isfinite(res["emb"]).all()
    if model in ("PNA", "DGN"):
        assert np.array_equal(res["on"], res["first"]) and names_on == names0, (names0, names_on)


# ---------------------------------------------------------------- 5. on chip, structurally
@pytest.mark.parametrize("model", MODELS)
def test_kernels_by_name(model):
    b, w = model_batch(model, 300 if model in ("PNA", "DGN") else 2000, seed=5), model_weights(model)
    e = Engine(model, device=0)
    e.set_weights(w)
    e.profile_enable(True)
    e.set_batch(b)
    off = launched(e, lambda: (e.run(), e.results()))
    e.set_embeddings(True)
    on = launched(e, lambda: (e.run(), e.embeddings()))
    e.close()
    resident = f"{base(model)}_resident"
    assert resident in off, (model, off)  # the batch packs well: the default path is the graph-resident one
    if model in ("PNA", "DGN"):
        assert on == off, (on, off)
    elif model in ("GIN", "GIN-VN"):
        assert "gin_resident" in on, on
        assert not on & {"mean_pool_linear", "mean_pool_rows", "gin_layer_fused", "gin_aggregate", "gin_mlp"}, on
    else:
        assert "mean_pool_rows" in on and resident not in on, on


# ---------------------------------------------------------------- 6. bit identity
@pytest.mark.parametrize("model,opts", [("GIN", {}), ("GIN-VN", {}), ("GCN", {}), ("GAT", {}), ("PNA", {}), ("DGN", {"dgn_mfma_agg": 0})])
def test_bit_identity(model, opts):
    """(DGN: with the in-edge walk -- its default matrix-pipe aggregation sums in tile order, tests/test_dgn_gpu.py)"""
    torch = pytest.importorskip("torch")
    b, w = model_batch(model, 240 if model in ("PNA", "DGN") else 1200, seed=13), model_weights(model)
    G = b.num_graphs
    e = Engine(model, device=0, options=opts)
    e.set_weights(w)
    logits, full = e.forward(b, return_embeddings=True)
    # a slice computed as a shard of the whole job
    e.set_job_totals(b.total_nodes, b.total_edges)
    e.set_job_tile_fill(e.graph_tile_fill(b.nums_of_nodes, b.nums_of_edges))
    _, part = e.forward(b.slice(G // 4, 3 * G // 4), return_embeddings=True)
    e.set_job_totals()
    e.set_job_tile_fill()
    assert np.array_equal(part, full[G // 4: 3 * G // 4])
    # a caller-owned buffer receives the same bits; NULL restores the engine's own
    e.set_batch(b)
    mine = torch.zeros((G, embedding_dim(model)), dtype=torch.float32, device="cuda:0")
    e.set_embeddings_buffer(mine.data_ptr())
    e.run()
    assert np.array_equal(e.embeddings(), full) and e.embeddings_device_ptr() == mine.data_ptr()
    assert np.array_equal(mine.cpu().numpy(), full)
    mine.zero_()
    e.set_embeddings_buffer(None)
    e.run()
    assert np.array_equal(e.embeddings(), full) and e.embeddings_device_ptr() != mine.data_ptr()
    assert not mine.cpu().numpy().any()
    e.close()
    # a two-member group on one device = one engine
    g = EngineGroup(model, [0, 0], options=opts)
    g.set_weights(w)
    g.set_embeddings(True)
    assert np.array_equal(g.forward(b), logits) and np.array_equal(g.embeddings(), full)
    g.close()
    # launch-sequence replay = direct launches
    h = Engine(model, device=0, options=dict(opts, hipgraph=1))
    h.set_weights(w)
    h.set_batch(b)
    h.run()
    h.run()
    h.set_embeddings(True)  # drops the recording made with embeddings off
    replays0 = h.graph_replays()
    outs = []
    for _ in range(4):
        h.run()
        outs.append((h.results().copy(), h.embeddings()))
    assert replays0 >= 1 and h.graph_replays() - replays0 >= 1
    assert all(np.array_equal(o[0], logits) and np.array_equal(o[1], full) for o in outs)
    h.close()


# ---------------------------------------------------------------- 7. device round trip
@pytest.mark.parametrize("model", MODELS)
def test_forward_device_returns_a_device_tensor(model):
    torch = pytest.importorskip("torch")
    b, w = model_batch(model, 200 if model in ("PNA", "DGN") else 700, seed=9), model_weights(model)
    e = Engine(model, device=0)
    try:
        e.set_weights(w)
        want_logits, want = e.forward(b, return_embeddings=True)
        d = b.to_pyg("cuda:0")
        attr = d["edge_attr"] if model in ("GIN", "GIN-VN", "GCN") else None
        logits, emb = e.forward_device(d["x"], d["edge_index"], attr, d.get("node_eigen") if model == "DGN" else None, ptr=d["ptr"],
                                       return_embeddings=True)
        e.sync()
        assert isinstance(emb, torch.Tensor) and emb.device == torch.device("cuda:0") and tuple(emb.shape) == want.shape
        torch.cuda.synchronize()
        assert np.array_equal(emb.cpu().numpy(), want) and np.array_equal(logits.cpu().numpy(), want_logits)
    finally:
        e.close()


# ---------------------------------------------------------------- 8. refusals and state
@pytest.mark.parametrize("model", ["GIN", "PNA"])
def test_fixed_point_refuses(model):
    e = Engine(model, device=0)
    e.set_weights(model_weights(model))
    e.set_numeric_mode("q6.10")
    with pytest.raises(FlowGNNError) as ei:
        e.set_embeddings(True)
    assert ei.value.code == 8
    e.set_numeric_mode("f32")
    e.set_embeddings(True)
    with pytest.raises(FlowGNNError) as ei:
        e.set_numeric_mode("q6.10")
    assert ei.value.code == 8
    e.close()


def test_embeddings_before_an_embeddings_run_is_a_state_error(gin_weights):
    e = Engine("GIN", device=0)
    e.set_weights(gin_weights)
    e.forward(gp.synth_molhiv_batch(20, seed=2))
    for fn in (e.embeddings, e.embeddings_device_ptr):
        with pytest.raises(FlowGNNError) as ei:
            fn()
        assert ei.value.code == 6
    e.set_embeddings(True)
    with pytest.raises(FlowGNNError) as ei:  # switched on, but no run since
        e.embeddings()
    assert ei.value.code == 6
    e.run()
    assert e.embeddings().shape == (20, 100)
    e.close()


@pytest.mark.parametrize("numeric", ["f32", "f16"])
def test_range_fallback_refills_the_embeddings(numeric, oracle, gin_weights):
    b = gp.synth_molhiv_batch(200, seed=21)
    big = dict(gin_weights)
    big["node_embedding_weight"] = gin_weights["node_embedding_weight"] * np.float32(1e5)
    e = Engine("GIN", device=0)
    e.set_weights(big)
    e.set_numeric_mode(numeric)
    logits, emb = e.forward(b, return_embeddings=True)
    assert e.exact_reruns() == 1
    e.close()
    want, hd = oracle.gin_forward(b, [big], dump_h=True, nthreads=8)
    assert np.isfinite(emb).all()
    assert_close(emb, pooled(hd[5], b), scale=oracle_scale(hd), what="embeddings after the exact re-run")
    assert np.allclose(logits, want, rtol=1e-4, atol=1e-4 * np.abs(want).max())


# ---------------------------------------------------------------- 9. host CLI
def test_host_cli(tmp_path):
    w = weights.synth_gin_weights(seed=7)
    b = gp.synth_molhiv_batch(40, seed=3)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    weights.SAVERS["GIN"](w, str(wdir))
    outs = []
    for extra in ([], ["--embeddings", str(tmp_path / "emb.txt")]):
        out = tmp_path / f"HLS_output_{len(extra)}.txt"
        r = subprocess.run([HOST, "GIN", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--out", str(out)] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(open(out).read())
    assert outs[0] == outs[1]  # the flag leaves HLS_output.txt as it was
    got = np.array([[float(x) for x in ln.split()] for ln in open(tmp_path / "emb.txt").read().strip().splitlines()])
    _, want = run_on("GIN", w, b)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-8 * (1.0 + np.abs(want).max())  # the file's 8 decimals


# ---------------------------------------------------------------- speed
def test_speed_guard():
    """GIN with embeddings on against NUM_TASK = 2 of the same commit, same process, same batch.  NUM_TASK = 2 runs the same
    un-folded resident instance, writes every h_5 row to HBM and reads it back in mean_pool_linear_mt_kernel; the pooling instance
    does strictly less, so it may be slower only by the noise of the comparison: t_on <= t_T2 * (1 + s), s = (max - min) / median of
    the three NUM_TASK = 2 medians of this session.  Device-event time of all kernels of a step (profile_read)."""
    b = gp.synth_molhiv_batch(1 << 16, seed=3)
    on = Engine("GIN", device=0)
    on.set_weights(weights.synth_gin_weights(seed=7))
    on.set_embeddings(True)
    t2 = Engine("GIN", device=0)
    t2.set_num_tasks(2)
    t2.set_weights(weights.synth_gin_weights(seed=7, num_tasks=2))
    for e in (on, t2):
        e.set_batch(b)
        e.profile_enable(True)
        e.run()
        e.results()

    def median_ms(e, runs=10):
        total = lambda: sum(v["total_ms"] for v in e.profile_read().values())
        ms = []
        for _ in range(runs):
            t0 = total()
            e.run()
            e.sync()
            ms.append(total() - t0)
        return float(np.median(ms))

    m_on, m_t2 = [], []
    for _ in range(3):
        m_t2.append(median_ms(t2))
        m_on.append(median_ms(on))
    on.close()
    t2.close()
    s = (max(m_t2) - min(m_t2)) / float(np.median(m_t2))
    print("embeddings on:", m_on, "NUM_TASK 2:", m_t2, "spread", s)
    assert min(m_on) <= min(m_t2) * (1.0 + s), (m_on, m_t2, s)
