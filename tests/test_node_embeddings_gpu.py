"""Node embeddings (flowgnn.h: flowgnn_set_node_embeddings): node_emb[v] = the row the readout pools, per node and in the caller's
node order -- stored by the graph-resident kernels of GCN / PNA / DGN out of the registers / the LDS tile they hold at the end of the
last layer (gcn_rows.hip, pna_rows.hip, dgn_rows.hip), by GIN's un-folded resident instance, and by the per-layer path for GAT.

Expected rows: the rows tests/test_embeddings_gpu.py's expected() forms before it pools them -- the oracle's last dumped layer
(GIN h_5, PNA / DGN h_4), restated one stage for GCN / GAT (gcn_last_stage / gat_last_stage, which first reproduce the oracle's
logits through the head).  Tolerance: tests/parity.py, REL = 1e-4, scale = the oracle's largest activation: the project's rule for
per-layer rows."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, embedding_dim, graphpack as gp, weights
from tests.parity import assert_close, err_ratio, oracle_scale
from tests.test_embeddings_gpu import (PER_LAYER, assert_logits, base, gat_last_stage, gcn_last_stage, head, launched, model_batch,
                                       model_weights, pooled)
from tests.test_resident_limits_gpu import random_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
MODELS = ["GIN", "GIN-VN", "GCN", "GAT", "PNA", "DGN"]
ON_CHIP = ["GCN", "PNA", "DGN"]  # the resident kernel keeps its readout and additionally stores the rows: logits bit-identical to off
BIN_PACKED = ["GCN", "PNA", "DGN"]  # with node embeddings on these walk bin-packed tile lists (GIN's un-folded instance: batch order)
f64 = lambda a: np.asarray(a, dtype=np.float64)


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """As tests/test_embeddings_gpu.py: torch's HIP context before the first engine exists."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def expected_rows(model, b, w, oracle):
    """(oracle logits, expected rows float64 [N][dim], activation scale)"""
    want, hd = getattr(oracle, f"{base(model)}_forward")(b, [w], dump_h=True, nthreads=8)
    scale = oracle_scale(hd)
    if model == "GCN":
        rows = gcn_last_stage(b, w, hd[4])
    elif model == "GAT":
        rows = gat_last_stage(b, w, hd[3])
    else:
        rows = f64(hd[-1])
    if model in ("GCN", "GAT"):  # the restatement proves itself on the oracle's logits first
        assert_close(head(model, w, pooled(rows, b)), want, scale=scale, what=(model, "restated last stage vs the oracle's logits"))
    return want, rows, scale


@pytest.fixture(scope="module")
def cases(oracle):
    """model -> (batch, weights, oracle logits, expected rows, scale), computed once"""
    out = {}

    def get(model):
        if model not in out:
            b = model_batch(model, 512 if model in ("PNA", "DGN") else 4113, seed=13)
            w = model_weights(model)
            out[model] = (b, w) + expected_rows(model, b, w, oracle)
        return out[model]
    return get


def run_on(model, w, b, options=None, embeddings=False, num_tasks=1, numeric=None, check_packed=False):
    e = Engine(model, device=0, options=options or {})
    try:
        if num_tasks != 1:
            e.set_num_tasks(num_tasks)
        e.set_weights(w)
        if numeric:
            e.set_numeric_mode(numeric)
        r = e.forward(b, return_embeddings=embeddings, return_node_embeddings=True)
        if check_packed:  # the caller-order mapping is really exercised: the kernel walks a tile-ordered row space
            assert e.batch_tiles()[1] > 0, (model, e.batch_tiles())
        return r
    finally:
        e.close()


# ---------------------------------------------------------------- 1. parity at dataset-shaped batches
@pytest.mark.parametrize("model", MODELS)
def test_parity(model, cases):
    b, w, want, want_rows, scale = cases(model)
    logits, rows = run_on(model, w, b, check_packed=model in BIN_PACKED)
    assert rows.shape == (b.total_nodes, embedding_dim(model)) and rows.dtype == np.float32
    print(model, "max |rows - want| =", float(np.abs(rows - want_rows).max()), "scale", scale, "ratio to the bound",
          err_ratio(rows, want_rows, scale))
    assert_close(rows, want_rows, scale=scale, what=(model, "node embeddings"))
    assert_logits(model, logits, want, scale, (model, "logits"))


# ---------------------------------------------------------------- 2. every per-layer path
@pytest.mark.parametrize("model", MODELS)
def test_per_layer_paths(model, cases):
    b, w, want, want_rows, scale = cases(model)
    for opts in PER_LAYER[model]:
        logits, rows = run_on(model, w, b, options=opts)
        print(model, opts, "ratio to the bound", err_ratio(rows, want_rows, scale))
        assert_close(rows, want_rows, scale=scale, what=(model, opts, "node embeddings"))
        assert_logits(model, logits, want, scale, (model, opts, "logits"))


def test_gin_batch_below_the_fill_threshold(oracle, gin_weights):
    """Graphs of 100 nodes and 700 edges: one per tile by the edge limit, 39 % full -- the per-layer kernels take the batch."""
    b = gp.concat_batches([random_graph(100, 700, seed=s) for s in range(12)])
    e = Engine("GIN", device=0)
    e.set_weights(gin_weights)
    assert e.graph_tile_fill(b.nums_of_nodes, b.nums_of_edges) < 0.5
    e.profile_enable(True)
    res = {}
    names = launched(e, lambda: res.update(r=e.forward(b, return_node_embeddings=True)))
    e.close()
    assert "gin_resident" not in names, names
    want, hd = oracle.gin_forward(b, [gin_weights], dump_h=True, nthreads=8)
    assert_close(res["r"][1], f64(hd[5]), scale=oracle_scale(hd), what="below the fill threshold")
    assert np.allclose(res["r"][0], want, rtol=1e-4, atol=1e-4)


def test_gin_multi_task_and_f16(oracle, gin_weights):
    """NUM_TASK > 1: the rows are the oracle's h_5.  FLOWGNN_NUMERIC_F16: the rows are h_5 of that mode's "every other path" rule, whose
    values tests/test_embeddings_gpu.py::test_gin_f16_mode pins through the embeddings -- here: the mean of the rows is the run's
    embedding and its head the run's logit."""
    b = gp.synth_molhiv_batch(1500, seed=17)
    w2 = weights.synth_gin_weights(seed=7, num_tasks=2)
    want, hd = oracle.gin_forward(b, [w2], dump_h=True, nthreads=8, num_tasks=2)
    for opts in ({}, {"gin_resident": 0}):
        logits, rows = run_on("GIN", w2, b, options=opts, num_tasks=2)
        assert_close(rows, f64(hd[5]), scale=oracle_scale(hd), what=("NUM_TASK 2", opts))
        assert np.allclose(logits, np.asarray(want).reshape(logits.shape), rtol=1e-4, atol=1e-4)
    _, hd1 = oracle.gin_forward(b, [gin_weights], dump_h=True, nthreads=8)
    for opts in ({}, {"gin_resident": 0}):
        logits, emb, rows = run_on("GIN", gin_weights, b, options=opts, embeddings=True, numeric="f16")
        assert np.isfinite(rows).all() and rows.shape == (b.total_nodes, 100)
        assert_close(pooled(rows, b), f64(emb), scale=oracle_scale(hd1), what=("f16", opts, "mean of the rows vs the embeddings"))
        assert_close(head("GIN", gin_weights, pooled(rows, b)), logits, scale=oracle_scale(hd1), what=("f16", opts, "head"))


# ---------------------------------------------------------------- 3. consistency with the graph embeddings and the logits
@pytest.mark.parametrize("model", MODELS)
def test_mean_of_the_rows_is_the_embedding_and_its_head_the_logit(model, cases):
    b, w, want, want_rows, scale = cases(model)
    logits, emb, rows = run_on(model, w, b, embeddings=True)
    mean = pooled(rows, b)
    assert_close(emb, mean, scale=scale, what=(model, "embeddings vs the mean of the rows"))
    assert_close(head(model, w, mean), logits, scale=scale, what=(model, "head(mean of the rows) vs the run's logits"))
    assert_close(rows, want_rows, scale=scale, what=(model, "node embeddings, both on"))


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
    e.set_node_embeddings(True)
    names_on = launched(e, lambda: (e.run(), res.update(on=e.results().copy(), rows=e.node_embeddings())))
    e.set_node_embeddings(False)
    names2 = launched(e, lambda: (e.run(), res.update(last=e.results().copy())))
    e.close()
    assert np.array_equal(res["last"], res["first"]) and names2 == names0, (names0, names2)
    assert np.isfinite(res["rows"]).all()
    if model in ON_CHIP:
        assert np.array_equal(res["on"], res["first"]) and names_on == names0, (names0, names_on)


# ---------------------------------------------------------------- 5. on chip, by name
@pytest.mark.parametrize("model", MODELS)
def test_kernels_by_name(model):
    b, w = model_batch(model, 300 if model in ("PNA", "DGN") else 2000, seed=5), model_weights(model)
    resident = f"{base(model)}_resident"

    def names(options, on):
        e = Engine(model, device=0, options=options)
        e.set_weights(w)
        e.profile_enable(True)
        e.set_batch(b)
        e.set_node_embeddings(on)
        got = launched(e, lambda: (e.run(), e.node_embeddings() if on else e.results()))
        e.close()
        return got

    off, on, per_layer = names({}, False), names({}, True), names({resident: 0}, True)
    assert resident in off, (model, off)  # the batch packs well: the default path is the graph-resident one
    if model == "GAT":  # the documented per-layer path (the open item)
        assert resident not in on and "gat_layer" in on and on == per_layer, (on, per_layer)
        return
    assert resident in on, (model, on)
    # what the engine launches only under <model>_resident 0.  (The index build and the atom encoder are no such kernels: they are
    # the front end of GIN's un-folded resident instance too, as with flowgnn_set_embeddings.)
    only_per_layer = per_layer - off - {"build_csr", "atom_encoder"}
    assert only_per_layer and resident not in per_layer, (model, per_layer)
    assert not on & only_per_layer, (model, on, only_per_layer)


# ---------------------------------------------------------------- 6. bit identity
def test_bit_identity():
    """DGN with the in-edge walk (its default matrix-pipe aggregation sums in tile order, tests/test_dgn_gpu.py)."""
    torch = pytest.importorskip("torch")
    model, opts = "DGN", {"dgn_mfma_agg": 0}
    b, w = model_batch(model, 240, seed=13), model_weights(model)
    G, off = b.num_graphs, b.node_offsets()
    e = Engine(model, device=0, options=opts)
    e.set_weights(w)
    logits, full = e.forward(b, return_node_embeddings=True)
    # a slice computed as a shard of the whole job
    e.set_job_totals(b.total_nodes, b.total_edges)
    e.set_job_tile_fill(e.graph_tile_fill(b.nums_of_nodes, b.nums_of_edges))
    plog, part = e.forward(b.slice(G // 4, 3 * G // 4), return_node_embeddings=True)
    e.set_job_totals()
    e.set_job_tile_fill()
    assert np.array_equal(part, full[off[G // 4]: off[3 * G // 4]]) and np.array_equal(plog, logits[G // 4: 3 * G // 4])
    # a caller-owned buffer receives the same bits; NULL restores the engine's own
    e.set_batch(b)
    mine = torch.zeros((b.total_nodes, embedding_dim(model)), dtype=torch.float32, device="cuda:0")
    e.set_node_embeddings_buffer(mine.data_ptr())
    e.run()
    assert np.array_equal(e.node_embeddings(), full) and e.node_embeddings_device_ptr() == mine.data_ptr()
    assert np.array_equal(mine.cpu().numpy(), full) and np.array_equal(e.results(), logits)
    mine.zero_()
    e.set_node_embeddings_buffer(None)
    e.run()
    assert np.array_equal(e.node_embeddings(), full) and e.node_embeddings_device_ptr() != mine.data_ptr()
    assert not mine.cpu().numpy().any()
    # forward_device against forward
    d = b.to_pyg("cuda:0")
    dlog, drows = e.forward_device(d["x"], d["edge_index"], None, d.get("node_eigen"), ptr=d["ptr"], return_node_embeddings=True)
    e.sync()
    assert isinstance(drows, torch.Tensor) and drows.device == torch.device("cuda:0") and tuple(drows.shape) == full.shape
    torch.cuda.synchronize()
    assert np.array_equal(drows.cpu().numpy(), full) and np.array_equal(dlog.cpu().numpy(), logits)
    e.close()
    # a two-member group on one device = one engine
    g = EngineGroup(model, [0, 0], options=opts)
    g.set_weights(w)
    g.set_node_embeddings(True)
    assert np.array_equal(g.forward(b), logits) and np.array_equal(g.node_embeddings(), full)
    g.close()
    # launch-sequence replay = direct launches
    h = Engine(model, device=0, options=dict(opts, hipgraph=1))
    h.set_weights(w)
    h.set_batch(b)
    h.run()
    h.run()
    h.set_node_embeddings(True)  # drops the recording made with node embeddings off
    replays0 = h.graph_replays()
    outs = []
    for _ in range(4):
        h.run()
        outs.append((h.results().copy(), h.node_embeddings()))
    assert replays0 >= 1 and h.graph_replays() - replays0 >= 1
    assert all(np.array_equal(o[0], logits) and np.array_equal(o[1], full) for o in outs)
    h.close()


# ---------------------------------------------------------------- 7. refusals and fallback
@pytest.mark.parametrize("model", ["GIN", "PNA"])
def test_fixed_point_refuses(model):
    e = Engine(model, device=0)
    e.set_weights(model_weights(model))
    e.set_numeric_mode("q6.10")
    with pytest.raises(FlowGNNError) as ei:
        e.set_node_embeddings(True)
    assert ei.value.code == 8
    e.set_numeric_mode("f32")
    e.set_node_embeddings(True)
    with pytest.raises(FlowGNNError) as ei:
        e.set_numeric_mode("q6.10")
    assert ei.value.code == 8
    e.close()


def test_rows_before_a_run_with_the_feature_on_is_a_state_error(gin_weights):
    e = Engine("GIN", device=0)
    e.set_weights(gin_weights)
    b = gp.synth_molhiv_batch(20, seed=2)
    e.forward(b)
    for fn in (e.node_embeddings, e.node_embeddings_device_ptr):
        with pytest.raises(FlowGNNError) as ei:
            fn()
        assert ei.value.code == 6
    e.set_node_embeddings(True)
    with pytest.raises(FlowGNNError) as ei:  # switched on, but no run since
        e.node_embeddings()
    assert ei.value.code == 6
    e.run()
    assert e.node_embeddings().shape == (b.total_nodes, 100)
    e.close()


def test_range_fallback_refills_the_rows(oracle, gin_weights):
    b = gp.synth_molhiv_batch(200, seed=21)
    big = dict(gin_weights)
    big["node_embedding_weight"] = gin_weights["node_embedding_weight"] * np.float32(1e5)
    e = Engine("GIN", device=0)
    e.set_weights(big)
    logits, rows = e.forward(b, return_node_embeddings=True)
    assert e.exact_reruns() == 1
    e.close()
    want, hd = oracle.gin_forward(b, [big], dump_h=True, nthreads=8)
    assert np.isfinite(rows).all()
    assert_close(rows, f64(hd[5]), scale=oracle_scale(hd), what="node embeddings after the exact re-run")
    assert np.allclose(logits, want, rtol=1e-4, atol=1e-4 * np.abs(want).max())


# ---------------------------------------------------------------- 8. host CLI
def test_host_cli(tmp_path):
    w = weights.synth_gin_weights(seed=7)
    b = gp.synth_molhiv_batch(40, seed=3)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    weights.SAVERS["GIN"](w, str(wdir))
    outs = []
    for extra in ([], ["--node-embeddings", str(tmp_path / "rows.txt")]):
        out = tmp_path / f"HLS_output_{len(extra)}.txt"
        r = subprocess.run([HOST, "GIN", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--out", str(out)] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(open(out).read())
    assert outs[0] == outs[1]  # the flag leaves HLS_output.txt as it was
    got = np.array([[float(x) for x in ln.split()] for ln in open(tmp_path / "rows.txt").read().strip().splitlines()])
    _, want = run_on("GIN", w, b)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-8 * (1.0 + np.abs(want).max())  # the file's 8 decimals


# ---------------------------------------------------------------- 9. speed
@pytest.mark.parametrize("model", ON_CHIP)
def test_speed_guard(model):
    """Node embeddings on: the graph-resident kernel's storing instance against the per-layer path of <model>_resident 0 (the parent's
    kernels, which leave the rows in HBM anyway), same process, same batch of 2^16 graphs, the two alternating; device-event time of
    all kernels of a step (profile_read), best of three medians of ten.  Storing the rows on the way out of the chip must not be
    slower than a path that moves every layer's rows through HBM: no margin."""
    b = model_batch(model, 1 << 16, seed=3)
    w = model_weights(model)
    eng = {}
    for key, opts in (("resident", {}), ("per_layer", {f"{base(model)}_resident": 0})):
        e = Engine(model, device=0, options=opts)
        e.set_weights(w)
        e.set_node_embeddings(True)
        e.set_batch(b)
        e.profile_enable(True)
        e.run()
        e.results()
        eng[key] = e

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
    print(model, "node embeddings on, resident:", m["resident"], "per-layer:", m["per_layer"])
    assert min(m["resident"]) <= min(m["per_layer"]), (model, m)
