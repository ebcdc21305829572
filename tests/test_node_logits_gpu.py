"""Node logits (flowgnn.h: flowgnn_set_node_logits): node_logits[v][t] = r[v] . W[t] + b[t], the per-node terms whose mean over a
graph's nodes is the graph's logit -- stored by the graph-resident kernels of GIN / GIN-VN / GCN / GAT out of the LDS array the readout
sums (gin_split_nlogit.hip, gcn_nlogit.hip, gat_nlogit.hip), and by two small kernels on every other path.

Expected values: rows64 . w + b in float64, rows64 as tests/test_node_embeddings_gpu.py::expected_rows takes them (the oracle's last
dumped layer, restated one stage for GCN / GAT).  Bound: the project's row rule (tests/parity.py: |row error| <= REL * (scale + |row|)
per element) carried through the dot product: |got - want| <= REL * (scale * ||w||_1 + |b| + |want|), scale = oracle_scale(hd).
Measured ratios to that bound: DESIGN.md section 4.9."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, graphpack as gp, weights
from tests.parity import REL
from tests.test_embeddings_gpu import PER_LAYER, base, launched, model_batch, model_weights
from tests.test_node_embeddings_gpu import expected_rows
from tests.test_resident_limits_gpu import LIMITS, random_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
MODELS = ["GIN", "GIN-VN", "GCN", "GAT"]
BIN_PACKED = ["GIN", "GCN"]  # (asserted: the batch walks bin-packed tile lists, so the caller-order map is really used)
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


def head_of(w):
    pw = f64(w["graph_pred_weights"])
    return pw.reshape(-1, pw.shape[-1]), f64(w["graph_pred_bias"]).reshape(-1)


def terms(rows, w):
    """rows64 . W[t] + b[t], float64: [N] for one task, [N][T] otherwise."""
    pw, pb = head_of(w)
    out = f64(rows) @ pw.T + pb
    return out[:, 0] if out.shape[1] == 1 else out


def ratio(got, want, w, scale, rel=REL):
    """max over elements of |got - want| / (rel * (scale * ||w_t||_1 + |b_t| + |want|)): <= 1 passes."""
    pw, pb = head_of(w)
    got, want = f64(got), f64(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    fixed = max(1.0, float(scale)) * np.abs(pw).sum(axis=1) + np.abs(pb)
    bound = rel * ((fixed if want.ndim == 2 else fixed[0]) + np.abs(want))
    return float((np.abs(got - want) / bound).max())


def assert_terms(got, want, w, scale, what, rel=REL):
    assert got.dtype == np.float32 and np.isfinite(got).all(), what
    r = ratio(got, want, w, scale, rel)
    print(what, "ratio to the bound", round(r, 4))
    assert r <= 1.0, (what, f"{r:.3f} x the bound (rel {rel:g}, scale {scale:.3g})")


def two_task(w, seed=3):
    """The same model with a second task: the rows do not depend on the head, so the single-task case's expected rows serve."""
    rng = np.random.default_rng(seed)
    pw1 = np.asarray(w["graph_pred_weights"], np.float32).reshape(1, -1)
    w2 = dict(w)
    w2["graph_pred_weights"] = np.concatenate([pw1, (rng.standard_normal(pw1.shape) * 0.15).astype(np.float32)])
    w2["graph_pred_bias"] = np.array([np.asarray(w["graph_pred_bias"]).reshape(-1)[0], 0.07], np.float32)
    return w2


@pytest.fixture(scope="module")
def cases(oracle):
    """model -> (batch, weights, oracle logits, expected rows float64, scale): computed once, shared, left unchanged"""
    out = {}

    def get(model):
        if model not in out:
            b = model_batch(model, 4113, seed=13)
            w = model_weights(model)
            out[model] = (b, w) + expected_rows(model, b, w, oracle)
        return out[model]
    return get


def run_on(model, w, b, options=None, num_tasks=1, numeric=None, embeddings=False, node_embeddings=False, node_logits=True,
           check_packed=False, names=None):
    e = Engine(model, device=0, options=options or {})
    try:
        if num_tasks != 1:
            e.set_num_tasks(num_tasks)
        e.set_weights(w)
        if numeric:
            e.set_numeric_mode(numeric)
        if names is not None:
            e.profile_enable(True)
        res = {}
        go = lambda: res.update(r=e.forward(b, return_embeddings=embeddings, return_node_embeddings=node_embeddings,
                                            return_node_logits=node_logits))
        if names is not None:
            names |= launched(e, go)
        else:
            go()
        if check_packed:
            assert e.batch_tiles()[1] > 0, (model, e.batch_tiles())
        return res["r"]
    finally:
        e.close()


def decomposition_ratio(b, logits, nl, w, unfolded_scale=None):
    """For every graph: |float64 mean of its node logits - the engine's logit| over the fp32 bound of an in-order sum, one division
    and the additions: (n_g + 4) 2^-24 (mean_v |node_logit[v]| + 2 |b| + |logit[g]|).  That is the bound where the engine's logit IS
    the mean of the terms (every folded readout: the graph-resident kernels and the default per-layer paths).
    unfolded_scale: the paths that pool the rows first and apply the head to the pooled row (un-folded by option, NUM_TASK > 1, the
    exact re-run, embeddings on as well) round D more products of magnitude up to scale * |w_d| that cancel in the logit, and the
    node logits' own dot products likewise: (n_g + 2 D + 4) 2^-24 (scale ||w||_1 + 2 |b| + |logit[g]|), D = the row's width."""
    pw, pb = head_of(w)
    off, n = b.node_offsets()[:-1], f64(b.nums_of_nodes)
    nl2, lg2 = f64(nl).reshape(b.total_nodes, -1), f64(logits).reshape(b.num_graphs, -1)
    mean = np.add.reduceat(nl2, off, axis=0) / n[:, None]
    if unfolded_scale is None:
        mabs = np.add.reduceat(np.abs(nl2), off, axis=0) / n[:, None]
        bound = (n[:, None] + 4.0) * 2.0 ** -24 * (mabs + 2.0 * np.abs(pb)[None, :] + np.abs(lg2))
    else:
        size = max(1.0, float(unfolded_scale)) * np.abs(pw).sum(axis=1)[None, :]
        bound = (n[:, None] + 2.0 * pw.shape[1] + 4.0) * 2.0 ** -24 * (size + 2.0 * np.abs(pb)[None, :] + np.abs(lg2))
    return float((np.abs(mean - lg2) / bound).max())


def assert_decomposition(b, logits, nl, w, what, unfolded_scale=None):
    r = decomposition_ratio(b, logits, nl, w, unfolded_scale)
    print(what, "decomposition: ratio to the fp32 bound", round(r, 4), "(un-folded readout)" if unfolded_scale is not None else "")
    assert r <= 1.0, (what, r)


# ---------------------------------------------------------------- 1. parity, decomposition and kernel choice on the resident path
@pytest.mark.parametrize("model", MODELS)
def test_parity_on_the_resident_path(model, cases):
    b, w, want, want_rows, scale = cases(model)
    resident = f"{base(model)}_resident"
    names_on, names_off, names_pl = set(), set(), set()
    logits, nl = run_on(model, w, b, check_packed=model in BIN_PACKED, names=names_on)
    off = run_on(model, w, b, node_logits=False, names=names_off)
    run_on(model, w, b, options={resident: 0}, node_logits=False, names=names_pl)
    assert nl.shape == (b.total_nodes,)
    assert_terms(nl, terms(want_rows, w), w, scale, (model, "node logits"))
    # node logits alone: the graph-resident launch, none of the kernels that only <model>_resident 0 launches, the logits' bits kept
    assert resident in names_on and names_on == names_off, (names_on, names_off)
    assert not names_on & (names_pl - names_off), (names_on, names_pl)
    assert np.array_equal(logits, off)
    assert_decomposition(b, logits, nl, w, model)


# ---------------------------------------------------------------- 2. every other path
@pytest.mark.parametrize("model", MODELS)
def test_per_layer_paths(model, cases):
    b, w, want, want_rows, scale = cases(model)
    want_nl = terms(want_rows, w)
    for opts in PER_LAYER[model]:
        logits, nl = run_on(model, w, b, options=opts)
        assert_terms(nl, want_nl, w, scale, (model, opts))
        folded = len(opts) == 1  # <model>_resident 0 alone keeps the folded readout; the second option of a set un-folds it
        assert_decomposition(b, logits, nl, w, (model, opts), None if folded else scale)


@pytest.mark.parametrize("model", ["GIN", "GCN"])
def test_two_tasks(model, cases):
    b, w, want, want_rows, scale = cases(model)
    w2 = two_task(w)
    want_nl = terms(want_rows, w2)
    for opts in [{}] + PER_LAYER[model]:
        logits, nl = run_on(model, w2, b, options=opts, num_tasks=2)
        assert nl.shape == (b.total_nodes, 2) and logits.shape == (b.num_graphs, 2)
        assert_terms(nl, want_nl, w2, scale, (model, "NUM_TASK 2", opts))
        assert_decomposition(b, logits, nl, w2, (model, "NUM_TASK 2", opts), scale)


@pytest.mark.parametrize("model", ["GIN", "GIN-VN"])
def test_f16_mode(model, cases):
    """FLOWGNN_NUMERIC_F16 against the fp32 oracle at rel = 2e-4, as tests/test_f16_mode_gpu.py compares that mode's logits."""
    b, w, want, want_rows, scale = cases(model)
    want_nl = terms(want_rows, w)
    for opts in [{}] + PER_LAYER[model]:
        names = set()
        logits, nl = run_on(model, w, b, options=opts, numeric="f16", names=names)
        assert ("gin_resident" in names) == (not opts), (opts, names)
        assert_terms(nl, want_nl, w, scale, (model, "f16", opts), rel=2e-4)
        assert_decomposition(b, logits, nl, w, (model, "f16", opts), None if len(opts) <= 1 else scale)


@pytest.mark.parametrize("model", MODELS)
def test_against_the_engines_own_rows(model, cases):
    """A second run with node embeddings on as well (and a third with graph embeddings): rows . w + b in float64 agrees with the
    first run's node logits under the parity bound, and both runs' own node logits meet the oracle's."""
    b, w, want, want_rows, scale = cases(model)
    _, alone = run_on(model, w, b)
    _, rows, both = run_on(model, w, b, node_embeddings=True)
    assert_terms(alone, terms(rows, w), w, scale, (model, "node logits vs node embeddings . w + b"))
    assert_terms(both, terms(want_rows, w), w, scale, (model, "node logits with node embeddings on"))
    lg, emb, with_emb = run_on(model, w, b, embeddings=True)
    assert_terms(with_emb, terms(want_rows, w), w, scale, (model, "node logits with graph embeddings on"))
    assert_decomposition(b, lg, with_emb, w, (model, "graph embeddings on"), scale)


# ---------------------------------------------------------------- 3. edges of the shapes
def check_against_oracle(model, b, oracle, options=None, names=None, w=None):
    w = w or model_weights(model, seed=11)
    want, rows, scale = expected_rows(model, b, w, oracle)
    logits, nl = run_on(model, w, b, options=options, names=names)
    assert_terms(nl, terms(rows, w), w, scale, (model, options, "edge shapes"))
    assert_decomposition(b, logits, nl, w, (model, options, "edge shapes"))
    return logits, nl


def test_gin_batch_below_the_fill_threshold(oracle):
    """Graphs of 100 nodes and 700 edges: one per tile by the edge limit, 39 % full -- the per-layer kernels take the batch."""
    b = gp.concat_batches([random_graph(100, 700, seed=s) for s in range(12)])
    names = set()
    check_against_oracle("GIN", b, oracle, names=names)
    assert "gin_resident" not in names and "node_logits" in names, names


def tiny_graphs_batch():
    """One-node graphs (with and without a self loop), edgeless graphs of several sizes, between ordinary molecules."""
    mol = gp.synth_molhiv_batch(30, seed=4)
    rng = np.random.default_rng(5)

    def graph(n, edges):
        nf = np.stack([rng.integers(0, c, n) for c in (119, 4, 12, 12, 10, 6, 6, 2, 2)], 1).astype(np.int32)
        el = np.asarray(edges, np.int32).reshape(-1, 2)
        ea = np.stack([rng.integers(0, 5, len(el)), rng.integers(0, 6, len(el)), rng.integers(0, 2, len(el))], 1).astype(np.int32)
        return gp.GraphBatch(np.array([n], np.int32), np.array([len(el)], np.int32), nf, el, ea.reshape(-1, 3))
    parts = [mol.slice(0, 7), graph(1, []), graph(1, [[0, 0]]), graph(5, []), mol.slice(7, 19), graph(1, []), graph(17, []),
             graph(2, [[0, 1]]), mol.slice(19, 30), graph(1, [])]
    return gp.concat_batches(parts)


@pytest.mark.parametrize("model", MODELS)
def test_one_node_and_edgeless_graphs(model, oracle):
    b = tiny_graphs_batch()
    if model == "GIN-VN":
        b = gp.add_virtual_nodes(b)
    check_against_oracle(model, b, oracle)


@pytest.mark.parametrize("model", MODELS)
def test_a_graph_at_the_tile_limit(model, oracle):
    rows, edges = LIMITS[model]
    mol = gp.synth_molhiv_batch(40, seed=3)
    b = gp.concat_batches([mol.slice(0, 13), random_graph(rows, rows + 40, seed=1), mol.slice(13, 40)])
    names = set()
    check_against_oracle(model, b, oracle, names=names)
    assert f"{base(model)}_resident" in names, names


@pytest.mark.parametrize("model", MODELS)
def test_empty_batch(model):
    b = model_batch(model, 5, seed=1).slice(0, 0)
    e = Engine(model, device=0)
    e.set_weights(model_weights(model))
    logits, nl = e.forward(b, return_node_logits=True)
    e.close()
    assert logits.shape == (0,) and nl.shape == (0,)


def test_range_fallback_refills_the_node_logits(oracle, gin_weights):
    b = gp.synth_molhiv_batch(200, seed=21)
    big = dict(gin_weights)
    big["node_embedding_weight"] = gin_weights["node_embedding_weight"] * np.float32(1e5)
    e = Engine("GIN", device=0)
    e.set_weights(big)
    logits, nl = e.forward(b, return_node_logits=True)
    assert e.exact_reruns() == 1
    e.close()
    want, rows, scale = expected_rows("GIN", b, big, oracle)
    assert_terms(nl, terms(rows, big), big, scale, "node logits after the exact re-run")
    assert_decomposition(b, logits, nl, big, "exact re-run", scale)


# ---------------------------------------------------------------- 4. bit identity, state
@pytest.mark.parametrize("model", MODELS)
def test_bit_identity(model):
    b, w = model_batch(model, 1200, seed=13), model_weights(model)
    G, off = b.num_graphs, b.node_offsets()
    e = Engine(model, device=0)
    e.set_weights(w)
    logits, full = e.forward(b, return_node_logits=True)
    # a slice computed as a shard of the whole job
    e.set_job_totals(b.total_nodes, b.total_edges)
    e.set_job_tile_fill(e.graph_tile_fill(b.nums_of_nodes, b.nums_of_edges))
    plog, part = e.forward(b.slice(G // 4, 3 * G // 4), return_node_logits=True)
    e.set_job_totals()
    e.set_job_tile_fill()
    assert np.array_equal(part, full[off[G // 4]: off[3 * G // 4]]) and np.array_equal(plog, logits[G // 4: 3 * G // 4])
    # on -> off -> on reproduces itself; off, the values are not to be had
    e.set_batch(b)
    e.set_node_logits(False)
    e.run()
    assert np.array_equal(e.results(), logits)
    for fn in (e.node_logits, e.node_logits_device_ptr):
        with pytest.raises(FlowGNNError) as ei:
            fn()
        assert ei.value.code == 6
    e.set_node_logits(True)
    with pytest.raises(FlowGNNError) as ei:  # switched on, but no run since
        e.node_logits()
    assert ei.value.code == 6
    e.run()
    assert np.array_equal(e.node_logits(), full) and np.array_equal(e.results(), logits)
    e.close()
    # a two-member group on one device = one engine
    g = EngineGroup(model, [0, 0])
    g.set_weights(w)
    g.set_node_logits(True)
    assert np.array_equal(g.forward(b), logits) and np.array_equal(g.node_logits(), full)
    g.close()
    # launch-sequence replay = direct launches
    h = Engine(model, device=0, options={"hipgraph": 1})
    h.set_weights(w)
    h.set_batch(b)
    h.run()
    h.run()
    h.set_node_logits(True)  # drops the recording made with node logits off
    replays0 = h.graph_replays()
    outs = []
    for _ in range(4):
        h.run()
        outs.append((h.results().copy(), h.node_logits()))
    assert replays0 >= 1 and h.graph_replays() - replays0 >= 1
    assert all(np.array_equal(o[0], logits) and np.array_equal(o[1], full) for o in outs)
    h.close()


# ---------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("model", ["PNA", "DGN"])
def test_mlp_heads_refuse(model):
    e = Engine(model, device=0)
    with pytest.raises(FlowGNNError) as ei:
        e.set_node_logits(True)
    assert ei.value.code == 8 and "MLP head" in str(ei.value)
    e.set_node_logits(False)
    e.close()
    g = EngineGroup(model, [0, 0])
    with pytest.raises(FlowGNNError) as ei:
        g.set_node_logits(True)
    assert ei.value.code == 8
    g.close()


def test_fixed_point_refuses_both_ways_round():
    e = Engine("GIN", device=0)
    e.set_weights(model_weights("GIN"))
    e.set_numeric_mode("q6.10")
    with pytest.raises(FlowGNNError) as ei:
        e.set_node_logits(True)
    assert ei.value.code == 8
    e.set_numeric_mode("f32")
    e.set_node_logits(True)
    with pytest.raises(FlowGNNError) as ei:
        e.set_numeric_mode("q6.10")
    assert ei.value.code == 8
    e.close()


# ---------------------------------------------------------------- 6. device path
@pytest.mark.parametrize("model", MODELS)
def test_forward_device_returns_a_device_tensor(model):
    torch = pytest.importorskip("torch")
    b, w = model_batch(model, 700, seed=9), model_weights(model)
    e = Engine(model, device=0)
    try:
        e.set_weights(w)
        want_logits, want = e.forward(b, return_node_logits=True)
        d = b.to_pyg("cuda:0")
        attr = d["edge_attr"] if model in ("GIN", "GIN-VN", "GCN") else None
        logits, nl = e.forward_device(d["x"], d["edge_index"], attr, None, ptr=d["ptr"], return_node_logits=True)
        e.sync()
        assert isinstance(nl, torch.Tensor) and nl.device == torch.device("cuda:0") and tuple(nl.shape) == (d["x"].shape[0],)
        torch.cuda.synchronize()
        assert np.array_equal(nl.cpu().numpy(), want) and np.array_equal(logits.cpu().numpy(), want_logits)
        assert e.node_logits_device_ptr() == nl.data_ptr()
        # with the node embeddings as well: the rows' path, in the order of the rows of x too
        _, want_rows, want_both = e.forward(b, return_node_embeddings=True, return_node_logits=True)
        logits2, rows, nl2 = e.forward_device(d["x"], d["edge_index"], attr, None, ptr=d["ptr"], return_node_embeddings=True,
                                              return_node_logits=True)
        e.sync()
        torch.cuda.synchronize()
        assert np.array_equal(nl2.cpu().numpy(), want_both) and np.array_equal(rows.cpu().numpy(), want_rows)
    finally:
        e.close()


# ---------------------------------------------------------------- 7. host CLI
def test_host_cli(tmp_path):
    w = weights.synth_gat_weights(seed=7)
    b = gp.synth_molhiv_batch(40, seed=3)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    weights.SAVERS["GAT"](w, str(wdir))
    outs = []
    for extra in ([], ["--node-logits", str(tmp_path / "terms.txt")]):
        out = tmp_path / f"HLS_output_{len(extra)}.txt"
        r = subprocess.run([HOST, "GAT", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--out", str(out)] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(open(out).read())
    assert outs[0] == outs[1]  # the flag leaves HLS_output.txt as it was
    got = np.array([float(ln) for ln in open(tmp_path / "terms.txt").read().strip().splitlines()])
    _, want = run_on("GAT", w, b)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-8 * (1.0 + np.abs(want).max())  # the file's 8 decimals


# ---------------------------------------------------------------- 8. speed
@pytest.mark.parametrize("model", MODELS)
def test_speed_guard(model):
    """Node logits on against node embeddings on -- the only way to these values before (rows, then a dot product on the caller's
    side) -- same process, same batch of 2^16 graphs, the two settings alternating; device-event time of all kernels of a step
    (profile_read), best of three medians of ten.  Four bytes per node out of the kernel that holds them must not cost more than
    the rows: no margin, no absolute figure."""
    b = model_batch(model, 1 << 16, seed=3)
    w = model_weights(model)
    eng = {}
    for key in ("node_logits", "node_embeddings"):
        e = Engine(model, device=0)
        e.set_weights(w)
        getattr(e, "set_" + key)(True)
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

    m = {"node_logits": [], "node_embeddings": []}
    for _ in range(3):
        for key in ("node_embeddings", "node_logits"):
            m[key].append(median_ms(eng[key]))
    for e in eng.values():
        e.close()
    print(model, "step, node logits on:", m["node_logits"], "node embeddings on:", m["node_embeddings"])
    assert min(m["node_logits"]) <= min(m["node_embeddings"]), (model, m)
