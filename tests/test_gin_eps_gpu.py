"""A trained eps for GIN / GIN-VN on the GPU (flowgnn.h: flowgnn_set_gin_eps): a[v] = s_l h[v] + sum of messages, s_l = 1 + eps[l].

Expected values: the float64 forward of tests/test_gin_eps.py (numpy_ref.gin_forward with the s_l term; it reproduces numpy_ref exactly
at s = 1 and the oracle within the parity rule there -- the oracle itself has no eps).  Tolerance: the project's rule and nothing else,
|gpu - want| <= rel (scale + |want|), rel = 1e-4 in f32 mode and 2e-4 in f16 mode (tests/test_f16_mode_gpu.py), scale = max(1, max |hs|)
of the float64 eps forward; node-embedding rows by the same rule on rows.  Every comparison prints its worst ratio to the bound.

The fixed input B, its weights (head x 8) and EPS are tests/test_gin_eps.py's, where a CPU test shows that every wrong variant of EPS
(all zero, one layer zeroed, two adjacent layers swapped) moves more than a quarter of the logits by more than 10 x the bound."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, compute_graphs, entry_set_gin_eps, export, graphpack as gp, weights
from tests.parity import REL, assert_close, err_ratio, oracle_scale
from tests.test_embeddings_gpu import PER_LAYER, head, launched
from tests.test_gin_eps import EPS, REL_F16, fixed_batch, fixed_weights, gin_eps_forward, trained_state_dict
from tests.test_resident_limits_gpu import LIMITS, random_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
MODELS = ["GIN", "GIN-VN"]
PER_SLOTS = {"gin_layer_fused", "gin_aggregate", "gin_mlp"}
ZERO = [0.0] * 5
f64 = lambda a: np.asarray(a, dtype=np.float64)
rel_of = lambda numeric: REL_F16 if numeric == "f16" else REL


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


class Ref:
    def __init__(self, b, w, eps=EPS):
        self.b, self.w = b, w
        self.want, self.hs, self.amax, self.hmax = gin_eps_forward(b, w, eps)
        self.scale = oracle_scale(self.hs)
        self.rows = self.hs[5]
        self.starts = b.node_offsets()[:-1]


@pytest.fixture(scope="module")
def ref():
    """model -> Ref on the fixed input, computed once and left unchanged"""
    out = {}

    def get(model):
        if model not in out:
            out[model] = Ref(fixed_batch(model), fixed_weights())
        return out[model]
    return get


def close(got, want, scale, rel, what):
    print(what, f"worst ratio to the bound {err_ratio(got, want, scale, rel):.3f}")
    assert_close(got, want, scale=scale, rel=rel, what=what)


def make(model, w, eps=EPS, options=None, numeric=None, num_tasks=1, pooling=None):
    e = Engine(model, device=0, options=options or {})
    if num_tasks != 1:
        e.set_num_tasks(num_tasks)
    e.set_weights(w)
    if numeric:
        e.set_numeric_mode(numeric)
    if pooling:
        e.set_pooling(pooling)
    if eps is not None:
        e.set_gin_eps(eps)
    e.profile_enable(True)
    return e


def run_on(model, w, b, eps=EPS, **kw):
    e = make(model, w, eps, **kw)
    try:
        return e.forward(b)
    finally:
        e.close()


def tile_limit_batch(model):
    """tests/test_resident_limits_gpu.py::test_graphs_at_the_tile_limits' batch; GIN-VN: sized so that each graph is AT the limits once
    its virtual node (one row, two edges per real node) is in -- 255 rows, and the edge counts less 2 n."""
    rows, edges = LIMITS[model]
    mol = gp.synth_molhiv_batch(40, seed=3)
    if model == "GIN-VN":
        at_rows = random_graph(rows - 1, rows + 39, seed=1)
        at_edges = random_graph(edges // 8, edges - 2 * (edges // 8), seed=2)
        both = random_graph(rows - 1, edges - 2 * (rows - 1), seed=4)
    else:
        at_rows = random_graph(rows, rows + 40, seed=1)
        at_edges = random_graph(edges // 8, edges, seed=2)
        both = random_graph(rows, edges, seed=4)
    b = gp.concat_batches([mol.slice(0, 13), at_rows, mol.slice(13, 14), at_edges, both, mol.slice(14, 40)])
    return gp.add_virtual_nodes(b) if model == "GIN-VN" else b


# ---------------------------------------------------------------- 1. parity on the intended path
@pytest.mark.parametrize("binpack", [1, 0])
@pytest.mark.parametrize("tile_build", [1, 0])
@pytest.mark.parametrize("numeric", ["f32", "f16"])
@pytest.mark.parametrize("model", MODELS)
def test_parity_on_the_resident_eps_kernel(model, numeric, tile_build, binpack, ref):
    r = ref(model)
    e = make(model, r.w, numeric=numeric, options={"gin_tile_build": tile_build, "gin_binpack": binpack})
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(r.b)))
    reruns = e.exact_reruns()
    e.close()
    assert "gin_resident" in names and not (names & PER_SLOTS), names
    assert ("gin_tile_build" in names) == bool(tile_build), names
    assert reruns == 0
    close(res["got"], r.want, r.scale, rel_of(numeric), (model, numeric, "tile_build", tile_build, "binpack", binpack))


# ---------------------------------------------------------------- 2. zero is the identity, bit for bit
IDENTITY_PATHS = [("GIN", None, {"gin_tile_build": 1}), ("GIN", None, {"gin_tile_build": 0}), ("GIN", None, {"gin_resident": 0}),
                  ("GIN", None, {"gin_mfma": 32}), ("GIN", "f16", {}), ("GIN", "f16", {"gin_resident": 0}),
                  ("GIN-VN", None, {}), ("GIN-VN", None, {"gin_resident": 0})]


@pytest.mark.parametrize("model,numeric,options", IDENTITY_PATHS)
def test_zero_eps_is_the_identity_bit_for_bit(model, numeric, options):
    """x * 1.0f == x: the eps instances with five zeros against an engine that never set it -- the instance plumbing apart from the
    arithmetic.  The fixed input plus the three graphs at the tile limits."""
    b = gp.concat_batches([fixed_batch(model), tile_limit_batch(model)])
    w = fixed_weights()
    never = make(model, w, None, options=options, numeric=numeric)
    names_never = launched(never, lambda: never.forward(b))
    base = never.results().copy()
    never.close()
    e = make(model, w, ZERO, options=options, numeric=numeric)
    names = launched(e, lambda: e.forward(b))
    got = e.results().copy()
    on = e.gin_eps()
    e.close()
    assert on is not None and np.array_equal(on, np.zeros(5, np.float32))  # on is a state, not a value
    assert names == names_never, (names, names_never)
    assert ("gin_resident" in names) == ("gin_resident" not in options and "gin_mfma" not in options), names
    assert np.array_equal(got, base), (model, numeric, options, float(np.abs(got - base).max()))


# ---------------------------------------------------------------- 3. tile shapes
@pytest.mark.parametrize("model", MODELS)
def test_graphs_at_the_tile_limits(model):
    # (the batch of tests/test_resident_limits_gpu.py as it is there: GIN-VN gets the same graphs, without virtual nodes of their own)
    b, w = tile_limit_batch("GIN"), fixed_weights()
    r = Ref(b, w)
    assert max(r.amax, r.hmax) < 6.0e4
    e = make(model, w)
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(b)))
    assert "gin_resident" in names and not (names & PER_SLOTS), names
    assert e.exact_reruns() == 0
    e.close()
    close(res["got"], r.want, r.scale, REL, (model, "graphs at the tile limits"))
    # any split of the batch gives the same bits (tiles are re-packed, rows change lanes)
    part = run_on(model, w, b.slice(10, 20))
    assert np.array_equal(part, res["got"][10:20])


@pytest.mark.parametrize("model", MODELS)
def test_many_ragged_tiles(model):
    """2 000 molpcba-shaped graphs: ~200 tiles of different fill."""
    b = gp.synth_molpcba_batch(2000, seed=21)
    if model == "GIN-VN":
        b = gp.add_virtual_nodes(b)
    w = fixed_weights()
    r = Ref(b, w)
    e = make(model, w)
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(b)))
    assert "gin_resident" in names and not (names & PER_SLOTS), names
    assert e.exact_reruns() == 0
    e.close()
    close(res["got"], r.want, r.scale, REL, (model, "2 000 graphs"))


# ---------------------------------------------------------------- 4. every other configuration computes with eps
def below_fill_batch():
    return gp.concat_batches([random_graph(100, 700, seed=s) for s in range(12)])  # tests/test_embeddings_gpu.py: one graph per tile, 39 % full


def beyond_limit_batch():
    mol = gp.synth_molhiv_batch(30, seed=8)
    return gp.concat_batches([mol.slice(0, 20), random_graph(LIMITS["GIN"][0] + 1, LIMITS["GIN"][0] + 30, seed=5), mol.slice(20, 30)])


OTHER = [("graph embeddings", dict(fwd={"return_embeddings": True})),
         ("node embeddings", dict(fwd={"return_node_embeddings": True})),
         ("node logits", dict(fwd={"return_node_logits": True})),
         ("pooling sum", dict(pooling="sum")),
         ("pooling max", dict(pooling="max")),
         ("NUM_TASK 2", dict(num_tasks=2)),
         ("below the fill threshold", dict(batch=below_fill_batch)),
         ("one graph beyond a tile limit", dict(batch=beyond_limit_batch))]
OTHER += [(f"options {o}", dict(options=o)) for o in PER_LAYER["GIN"]]
OTHER += [(f"options {o}, node embeddings", dict(options=o, fwd={"return_node_embeddings": True})) for o in PER_LAYER["GIN"]]
OTHER += [("gin_head_fold 0", dict(options={"gin_head_fold": 0})), ("gin_mfma 32, node embeddings", dict(options={"gin_mfma": 32}, fwd={"return_node_embeddings": True}))]


# GIN: every configuration in f32 mode.  In f16 mode: the option sets, whose only output is the mean logit of the fixed input through
# the single-task head -- what the rule's f16 factor (2e-4, tests/test_f16_mode_gpu.py) is stated for and what test 1 checks on the
# resident path.  An f16 run's ROWS carry 2^-11 per rounded MLP operand, more than 2e-4 of the scale, so this rule cannot hold them:
# the f16 arithmetic of the eps instances -- rows, sum / max / NUM_TASK 2 / per-node readouts, resident and per-layer -- is pinned by
# tests/test_f16_probe_gpu.py against tests/f16_ref.py's rounded forward with eps, exactly.  Here those cases run in f32 mode.
# GIN-VN (the same per-layer kernels, hub rows in their walk): the configurations on the fixed input, f32 mode.
OTHER_CASES = [("GIN", n, c, "f32") for n, c in OTHER]
OTHER_CASES += [("GIN", n, c, "f16") for n, c in OTHER if set(c) == {"options"}]
OTHER_CASES += [("GIN-VN", n, c, "f32") for n, c in OTHER if "batch" not in c and c.get("options", {}).get("gin_fold_readout", 1)]


@pytest.mark.parametrize("model,name,cfg,numeric", OTHER_CASES, ids=[f"{m}-{n}-{q}" for m, n, _, q in OTHER_CASES])
def test_other_configurations_compute_with_eps(model, name, cfg, numeric, ref):
    tasks, pooling, fwd = cfg.get("num_tasks", 1), cfg.get("pooling"), cfg.get("fwd", {})
    if "batch" in cfg or tasks != 1:
        r = Ref(cfg["batch"]() if "batch" in cfg else fixed_batch(model), fixed_weights(tasks))
    else:
        r = ref(model)
    rel = rel_of(numeric)
    e = make(model, r.w, options=cfg.get("options"), numeric=numeric, num_tasks=tasks, pooling=pooling)
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(r.b, **fwd)))
    reruns = e.exact_reruns()
    e.close()
    assert names & PER_SLOTS and "gin_resident" not in names, (name, names)
    assert reruns == 0
    got = res["got"] if isinstance(res["got"], tuple) else (res["got"],)
    logits = got[0]
    W = f64(r.w["graph_pred_weights"]).reshape(-1, 100)
    if pooling == "sum":
        want = head("GIN", r.w, np.add.reduceat(r.rows, r.starts, axis=0))
    elif pooling == "max":
        want = head("GIN", r.w, np.maximum.reduceat(r.rows, r.starts, axis=0))
    else:
        want = r.want
    close(logits, want, r.scale, rel, (model, numeric, name, "logits"))
    if fwd.get("return_embeddings"):
        close(got[1], np.add.reduceat(r.rows, r.starts, axis=0) / f64(r.b.nums_of_nodes)[:, None], r.scale, rel, (model, numeric, name, "embeddings"))
    if fwd.get("return_node_embeddings"):
        close(got[1], r.rows, r.scale, rel, (model, numeric, name, "node-embedding rows"))
    if fwd.get("return_node_logits"):
        terms = got[1]
        close(terms, (r.rows @ W.T + f64(r.w["graph_pred_bias"]).reshape(-1))[:, 0], r.scale, rel, (model, numeric, name, "node logits"))
        mean = np.add.reduceat(f64(terms), r.starts) / f64(r.b.nums_of_nodes)
        close(logits, mean, r.scale, rel, (model, numeric, name, "the mean of the node logits is the logit"))


# ---------------------------------------------------------------- 5. range fallback
@pytest.mark.parametrize("numeric", ["f32", "f16"])
def test_range_fallback_honours_eps(numeric, gin_weights):
    b = gp.synth_molhiv_batch(200, seed=21)
    big = dict(gin_weights)
    big["node_embedding_weight"] = gin_weights["node_embedding_weight"] * np.float32(1e5)
    r = Ref(b, big)
    e = make("GIN", big, numeric=numeric)
    logits, rows = e.forward(b, return_node_embeddings=True)
    assert e.exact_reruns() == 1
    e.close()
    close(rows, r.rows, r.scale, rel_of(numeric), (numeric, "range fallback, node-embedding rows"))
    close(logits, r.want, r.scale, rel_of(numeric), (numeric, "range fallback, logits"))
    e = make("GIN", big, numeric=numeric)  # ... and on the path the plain run takes (resident first, then the exact re-run)
    got = e.forward(b)
    assert e.exact_reruns() == 1
    e.close()
    close(got, r.want, r.scale, rel_of(numeric), (numeric, "range fallback behind the resident kernel, logits"))
    zero, unset = make("GIN", big, ZERO, numeric=numeric), make("GIN", big, None, numeric=numeric)
    a, c = zero.forward(b), unset.forward(b)
    assert zero.exact_reruns() == 1 and unset.exact_reruns() == 1
    zero.close(); unset.close()
    assert np.array_equal(a, c)


# ---------------------------------------------------------------- 6. off means off
@pytest.mark.parametrize("model", MODELS)
def test_off_means_off(model, ref):
    r = ref(model)
    fresh = make(model, r.w, None)
    names_fresh = launched(fresh, lambda: fresh.forward(r.b))
    want = fresh.results().copy()
    assert fresh.gin_eps() is None
    fresh.close()
    e = make(model, r.w, None)
    e.set_batch(r.b)
    res = {}
    n0 = launched(e, lambda: (e.run(), res.update(first=e.results().copy())))
    e.set_gin_eps(EPS)  # changed between runs on a resident batch
    n1 = launched(e, lambda: (e.run(), res.update(on=e.results().copy())))
    e.set_gin_eps(None)
    assert e.gin_eps() is None
    n2 = launched(e, lambda: (e.run(), res.update(off=e.results().copy())))
    e.close()
    assert np.array_equal(res["first"], want) and np.array_equal(res["off"], want)
    assert n0 == names_fresh and n2 == names_fresh, (n0, n2, names_fresh)
    assert "gin_resident" in n1
    close(res["on"], r.want, r.scale, REL, (model, "eps set on a resident batch"))
    assert not np.array_equal(res["on"], want)


# ---------------------------------------------------------------- 7. refusals
def refused(fn, code=8):
    with pytest.raises(FlowGNNError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_refusals(ref):
    g = Engine("GCN", device=0)
    assert "GIN" in refused(lambda: g.set_gin_eps(EPS))
    assert "GIN" in refused(lambda: g.set_gin_eps(None))
    assert g.lib.flowgnn_gin_eps(g._h, None) == 0
    g.close()
    r = ref("GIN")
    e = make("GIN", r.w, None)
    assert "finite" in refused(lambda: e.set_gin_eps([0.0, float("nan"), 0.0, 0.0, 0.0]), code=1)
    assert "finite" in refused(lambda: e.set_gin_eps([0.0, 0.0, 0.0, 0.0, float("-inf")]), code=1)
    assert e.gin_eps() is None
    # the fixed-point mode, in both orders
    e.set_numeric_mode("q6.10")
    assert "eps" in refused(lambda: e.set_gin_eps(EPS))
    e.set_gin_eps(None)  # off is always accepted
    e.set_numeric_mode("f32")
    e.set_gin_eps(EPS)
    assert "eps" in refused(lambda: e.set_numeric_mode("q6.10"))
    e.set_numeric_mode("f16")
    e.set_numeric_mode("f32")
    # the stand-alone aggregation kernel has no eps instance
    e.forward(r.b)
    assert "eps" in refused(lambda: e.aggregation_only_ms(0, 1))
    assert "eps" in refused(lambda: e.aggregate(0))
    e.set_gin_eps(None)
    assert e.aggregation_only_ms(0, 1) > 0.0
    e.close()
    u = make("GIN", r.w, EPS, options={"gin_unfused": 1})
    u.set_batch(r.b)
    assert "gin_unfused" in refused(u.run)
    u.set_gin_eps(None)
    u.run()
    assert np.isfinite(u.results()).all()
    u.close()
    v = EngineGroup("GCN", [0, 0])
    refused(lambda: v.set_gin_eps(EPS))
    v.close()


# ---------------------------------------------------------------- 8. the same bits through the other doors
@pytest.mark.parametrize("model", MODELS)
def test_group_entry_points_and_device_batches(model, ref):
    r = ref(model)
    e = make(model, r.w)
    want = e.forward(r.b)
    back = e.gin_eps()
    assert back is not None and np.array_equal(back, np.asarray(EPS, np.float32))
    close(want, r.want, r.scale, REL, (model, "one engine"))
    try:
        import torch  # noqa: F401
        d = r.b.to_pyg("cuda:0")
        got = e.forward_device(d["x"], d["edge_index"], d["edge_attr"], None, ptr=d["ptr"])
        e.sync()
        assert np.array_equal(got.cpu().numpy(), want)
    except ImportError:
        pass
    finally:
        e.close()
    g = EngineGroup(model, [0, 0])
    g.set_weights(r.w)
    g.set_gin_eps(EPS)
    assert np.array_equal(g.forward(r.b), want)
    g.close()
    if model != "GIN":
        return
    plain = run_on(model, r.w, r.b, None)
    try:
        entry_set_gin_eps(model, EPS)
        assert np.array_equal(compute_graphs(model, r.b, [r.w]), want)
    finally:
        entry_set_gin_eps(model, None)  # the entry engines outlive the test
    assert np.array_equal(compute_graphs(model, r.b, [r.w]), plain)


# ---------------------------------------------------------------- 9. a recorded launch sequence is dropped
def test_hipgraph_replay_is_dropped(ref):
    r = ref("GIN")
    want = run_on("GIN", r.w, r.b)
    h = Engine("GIN", device=0, options={"hipgraph": 1})
    h.set_weights(r.w)
    h.set_batch(r.b)
    h.run()
    h.run()
    h.run()
    plain = h.results().copy()
    assert h.graph_replays() >= 1
    h.set_gin_eps(EPS)
    h.run()
    first = h.results().copy()
    outs = []
    for _ in range(3):
        h.run()
        outs.append(h.results().copy())
    h.close()
    assert np.array_equal(first, want) and not np.array_equal(first, plain)
    assert all(np.array_equal(o, want) for o in outs)
    close(first, r.want, r.scale, REL, "hipgraph, the run after set_gin_eps")


# ---------------------------------------------------------------- 10. host CLI
def test_host_cli(tmp_path):
    sd = trained_state_dict()
    b = gp.synth_molhiv_batch(40, seed=3)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    export.export_weights("GIN", sd, str(wdir), keep_eps=True)
    w, eps = weights.load_gin_weights(str(wdir)), weights.load_gin_eps(str(wdir))
    outs = {}
    for flag in ("--eps", None):
        out = tmp_path / f"HLS_output_{flag}.txt"
        r = subprocess.run([HOST, "GIN", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--out", str(out)] + ([flag] if flag else []),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[flag] = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    with_eps, without = Ref(b, w, eps), Ref(b, w, None)
    close(outs["--eps"], with_eps.want, with_eps.scale, REL, "host --eps")
    close(outs[None], without.want, without.scale, REL, "host without --eps")
    assert err_ratio(outs[None], with_eps.want, with_eps.scale, REL) > 10.0  # the two are different models at this tolerance


# ---------------------------------------------------------------- 11. speed
def test_speed_guard():
    """GIN at 2^16 molhiv-shaped graphs: the eps instance of gin_resident against the default one (the parent commit's kernel, unchanged)
    in the same process, on one engine whose eps state alternates; device-event time of the `gin_resident` slot (profile_read), three
    medians of seven behind one unmeasured round per state.  No ratio fixed in advance: the eps instance may cost the larger of 5 % and
    three times the spread of the default's own three medians."""
    b = gp.synth_molhiv_batch(1 << 16, seed=3)
    e = Engine("GIN", device=0)
    e.set_weights(weights.synth_gin_weights(seed=7))
    e.set_batch(b)
    e.profile_enable(True)

    def median_ms(eps, runs=7):
        e.set_gin_eps(eps)
        e.run()
        e.sync()
        slot = lambda: e.profile_read()["gin_resident"]["total_ms"]
        ms = []
        for _ in range(runs):
            t0 = slot()
            e.run()
            e.sync()
            ms.append(slot() - t0)
        return float(np.median(ms))

    states = {"off": None, "on": EPS}
    for k in states:  # one unmeasured round per state: the first one is cold, and its median would widen the default's own spread
        median_ms(states[k])
    m = {"off": [], "on": []}
    for _ in range(3):
        for k in states:
            m[k].append(median_ms(states[k]))
    e.close()
    spread = (max(m["off"]) - min(m["off"])) / float(np.median(m["off"]))
    allow = max(0.05, 3.0 * spread)
    print("gin_resident ms, eps off:", m["off"], "eps on:", m["on"], "spread of the default's medians", spread, "allowed", allow)
    assert min(m["on"]) <= min(m["off"]) * (1.0 + allow), (m, spread)
