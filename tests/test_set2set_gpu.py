"""OGB's set2set readout at width 300 on the GPU (flowgnn.h: flowgnn_set_set2set_pooling; kernels: flowgnn_amd/csrc/wide_s2s.hip, DESIGN.md
section 4.23), for gin, gin-virtual, gcn and gcn-virtual.

Expected values: tests/set2set_ref.py -- the torch.nn model (a real torch.nn.LSTM driven as PyG's Set2Set drives it) through the exporter
and the files, or the float64 restatement on the wide references' rows (or on the rows the engine itself returned, where the test says
so).  Tolerance: the project's rule and nothing else, |gpu - want| <= REL (scale + |want|), REL = 1e-4, scale = the reference's
activation scale (tests/parity.py).  tests/test_set2set_cpu.py shows that every named wrong form of the readout is at least 16 x the rule
away.  Every comparison prints its worst ratio to the bound.  Every test here fails on a library without flowgnn_set_set2set_pooling."""
import functools
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, export, graphpack as gp, weights
from tests import gcn_wide_ref as C, gin_wide_ref as W, ogb_torch as T, set2set_ref as S
from tests.parity import REL, assert_close, err_ratio
from tests.test_embeddings_gpu import launched
from tests.test_ogb_torch_cpu import export_kwargs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
LSTM, DOT, POOL, HEAD, MEAN = "s2s_lstm", "s2s_dot_rows", "s2s_pool_rows", "s2s_head", "mean_pool_rows"
SLOTS = {LSTM, DOT, POOL, HEAD}
EPS = np.asarray(W.TRAINED_EPS, np.float32)
KINDS = [("gin", False), ("gin", True), ("gcn", False), ("gcn", True)]
name_of = lambda kind, vn: f"{kind}{'-virtual' if vn else ''}"


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def close(got, want, scale, what, rel=REL):
    print(what, f"worst ratio to the bound {err_ratio(got, want, scale, rel):.4f}")
    assert_close(got, want, scale=scale, rel=rel, what=what)


@functools.lru_cache(maxsize=None)
def s2s_of(tasks=1):
    return weights.synth_set2set(num_tasks=tasks)


@functools.lru_cache(maxsize=None)
def model_weights(kind, tasks=1):
    return (weights.synth_gin_weights if kind == "gin" else weights.synth_gcn_weights)(seed=7, num_tasks=tasks, emb_dim=300)


@functools.lru_cache(maxsize=None)
def shapes_batch():
    """Graph sizes 1, 2, 64, 65 and 130 nodes (a wave's 64 nodes per trip and its boundary), a graph without an edge, a one-node graph
    twice (the same graph at two positions), 17 graphs in all: one past a 16-row wave tile, no multiple of 4."""
    path = lambda n: T._both([(i, i + 1) for i in range(n - 1)])
    one = T._graph(1, [], 11)
    gs = [T._graph(2, path(2), 12), one, T._graph(64, path(64), 13), T._graph(65, path(65), 14), gp.synth_molhiv_batch(9, seed=4),
          T._graph(130, path(130), 15), T._graph(5, [], 16), one, T._graph(3, path(3), 17)]
    b = gp.concat_batches(gs)
    assert b.num_graphs == 17 and {1, 2, 64, 65, 130} <= set(b.nums_of_nodes.tolist())
    return b


def reference(kind, b, s2s, steps, w=None, tasks=1):
    """(rows, q*, logits, scale) in float64: the wide reference's forward for the rows, then the restatement on them."""
    w = model_weights(kind, tasks) if w is None else w
    ref = W.forward(b, w, eps=EPS, num_tasks=tasks) if kind == "gin" else C.forward(b, w, num_tasks=tasks)
    stats = {}
    q, logits, _ = S.readout(ref.rows, b, s2s, steps=steps, stats=stats)
    return ref.rows, q, logits, max(ref.scale, stats["q_max"], stats["e_max"], float(np.abs(logits).max()))


def make(kind, s2s=None, steps=2, tasks=1, w=None, options=None, cls=Engine, devices=0, profile=True):
    e = cls(kind.upper(), devices, options=options or {}) if cls is Engine else cls(kind.upper(), devices)
    (e.set_emb_dim if kind == "gin" else e.set_model_emb_dim)(300)
    if tasks != 1:
        e.set_num_tasks(tasks)
    e.set_weights(model_weights(kind, tasks) if w is None else w)
    if kind == "gin":
        e.set_gin_eps(EPS)
    if s2s is not None:
        e.set_set2set_pooling(s2s, steps=steps)
    if cls is Engine and profile:
        e.profile_enable(True)
    return e


def run(e, b, expect_reruns=0, **fwd):
    """One forward with the readout on: its four slots ran, the mean's and the model's own head did not."""
    res = {}
    before = e.exact_reruns()
    names = launched(e, lambda: res.update(got=e.forward(b, **fwd)))
    assert SLOTS <= names and MEAN not in names and "pooled_head" not in names, names
    assert e.exact_reruns() - before == expect_reruns, (e.exact_reruns(), before)
    return res["got"]


# ---------------------------------------------------------------- 1. parity against the torch model, through the exporter and the files
@pytest.mark.parametrize("steps", [2, 3])
@pytest.mark.parametrize("tasks", [1, 3])
@pytest.mark.parametrize("kind,vn", KINDS, ids=[name_of(k, v) for k, v in KINDS])
def test_parity_with_the_torch_model(kind, vn, tasks, steps, tmp_path):
    pytest.importorskip("torch")
    model = S.set2set_model(kind, vn, num_tasks=tasks, steps=steps)
    b = T.batch_of(kind)
    assert b.num_graphs % 4 != 0 and 1 in b.nums_of_nodes and 17 in b.nums_of_nodes and 129 in b.nums_of_nodes
    want, scale, _ = T.run(model, b)
    export.export_weights(kind.upper(), model.state_dict(), str(tmp_path), set2set=True, **export_kwargs(kind, vn, 300, tasks=tasks))
    e = Engine(kind.upper(), device=0)
    try:
        (e.set_emb_dim if kind == "gin" else e.set_model_emb_dim)(300)
        if tasks != 1:
            e.set_num_tasks(tasks)
        e.load_weights_dir(str(tmp_path), eps=kind == "gin", virtual_node=vn, set2set=True, set2set_steps=steps)
        assert e.set2set_pooling() == steps
        e.profile_enable(True)
        got, rows = run(e, b, return_node_embeddings=True)
        assert e.exact_reruns() == 0
        h = e.final_h()
        e.set_set2set_pooling(None)  # the flag forgotten: the model's own set carries a zero head
        zeros = e.forward(b)
    finally:
        e.close()
    what = (name_of(kind, vn), f"NUM_TASK {tasks}", f"steps {steps}")
    assert got.shape == ((b.num_graphs, tasks) if tasks > 1 else (b.num_graphs,))
    close(rows, want.rows, scale, what + ("node embeddings",))
    close(got, want.logits, scale, what + ("logits",))
    assert np.isfinite(h).all() and (kind != "gin" or np.array_equal(h, rows))
    assert not zeros.any()


# ---------------------------------------------------------------- 2. graph counts and sizes
@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_graph_sizes_and_an_edgeless_graph(kind):
    b = shapes_batch()
    s2s = s2s_of()
    rows, q, logits, scale = reference(kind, b, s2s, 3)
    e = make(kind, s2s, steps=3)
    try:
        got, nemb = run(e, b, return_node_embeddings=True)
    finally:
        e.close()
    close(nemb, rows, scale, (kind, "sizes, node embeddings"))
    close(got, logits, scale, (kind, "sizes, logits"))
    # one-node graphs: r_t = r[v] exactly, so the logit is head_b + head_W [h_T, r[v]] with h_T from the returned row alone
    one = np.nonzero(b.nums_of_nodes == 1)[0]
    assert len(one) == 2
    off = b.node_offsets()
    for g in one:
        sub = b.slice(int(g), int(g) + 1)
        r = nemb[off[g]:off[g] + 1]
        qg, lg, _ = S.readout(r, sub, s2s, steps=3)
        assert np.array_equal(qg[0, 300:], r[0].astype(np.float64))  # the restatement's r_T is the row itself
        close(got[g:g + 1], np.atleast_1d(lg), max(1.0, float(np.abs(r).max()), float(np.abs(lg).max())), (kind, "one-node graph", int(g)))
    assert got[one[0]] == got[one[1]]  # the same graph at two positions: the same bits


@pytest.mark.parametrize("count", [1, 17, 129])
def test_graph_counts(count):
    """One row; one past a 16-row wave tile; one past 128 rows (two workgroups of the LSTM kernel and a second wave tile in the last)."""
    b = gp.synth_molhiv_batch(count, seed=20 + count)
    s2s = s2s_of()
    rows, q, logits, scale = reference("gin", b, s2s, 3)
    e = make("gin", s2s, steps=3)
    try:
        got = run(e, b)
    finally:
        e.close()
    close(got, logits, scale, ("graph count", count))


# ---------------------------------------------------------------- 3. one engine's bits at other placements
@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_placements_give_the_same_bits(kind):
    pytest.importorskip("torch")
    from tests.test_device_batch_gpu import device_args
    b = T.batch_of(kind)
    s2s = s2s_of()
    e = make(kind, s2s, steps=3)
    try:
        want = run(e, b).copy()
        for layout in ("pyg", "reference"):
            args, kw = device_args(b, layout, kind.upper())
            got = e.forward_device(*args, **kw)
            e.sync()
            assert np.array_equal(got.cpu().numpy(), want), layout
        e.set_job_totals(b.total_nodes, b.total_edges)
        part = run(e, b.slice(5, 27)).copy()
        e.set_job_totals(-1, -1)
        assert e.exact_reruns() == 0
    finally:
        e.close()
    assert np.array_equal(part, want[5:27])  # a slice run as a shard
    g = make(kind, s2s, steps=3, cls=EngineGroup, devices=[0, 0])
    try:
        got = g.forward(b).copy()
        g.set_set2set_pooling(None)
        off = g.forward(b).copy()
    finally:
        g.close()
    assert np.array_equal(got, want) and not np.array_equal(off, want)


def test_off_on_off_returns_the_bytes_of_an_engine_that_never_had_it():
    b = T.gin_batch()
    never = make("gin")
    try:
        base = never.forward(b).copy()
    finally:
        never.close()
    e = make("gin")
    try:
        off = e.forward(b).copy()
        e.set_set2set_pooling(s2s_of(), steps=2)
        on = run(e, b).copy()
        e.set_set2set_pooling(s2s_of(), steps=3)  # may change between runs on a resident batch
        e.run()
        on3 = e.results().copy()
        e.set_set2set_pooling(None)
        names = launched(e, lambda: e.run())
        off2 = e.results().copy()
    finally:
        e.close()
    assert MEAN in names and "pooled_head" in names and not names & SLOTS, names
    assert off.tobytes() == base.tobytes() == off2.tobytes()
    assert not np.array_equal(on, off) and not np.array_equal(on3, on)


def test_hipgraph_replay_equals_direct_launches():
    b = T.gin_batch()
    plain = make("gin", s2s_of(), steps=3)
    try:
        expected = run(plain, b).copy()
    finally:
        plain.close()
    h = make("gin", options={"hipgraph": 2}, profile=False)  # (a profiled run is launched directly)
    try:
        h.set_batch(b)
        for _ in range(3):
            h.run()
        mean = h.results().copy()
        assert h.graph_replays() >= 1
        h.set_set2set_pooling(s2s_of(), steps=3)  # drops the recorded sequence
        h.run()
        first = h.results().copy()
        before = h.graph_replays()
        outs = []
        for _ in range(3):
            h.run()
            outs.append(h.results().copy())
        assert h.graph_replays() > before  # the new sequence is recorded and replayed in its turn
        h.set_set2set_pooling(None)
        h.run()
        off = h.results().copy()
    finally:
        h.close()
    assert np.array_equal(first, expected) and all(np.array_equal(o, expected) for o in outs)
    assert np.array_equal(off, mean) and not np.array_equal(first, mean)


# ---------------------------------------------------------------- 4. saturation, the range fallback, the f16 mode
def test_saturation():
    """The LSTM's four tensors x 64: every gate and the softmax saturated; the logits are finite and within the rule."""
    b = gp.synth_molhiv_batch(64, seed=5)
    s = {k: v * np.float32(64) if k in ("w_ih", "w_hh", "b_ih", "b_hh") else v for k, v in s2s_of().items()}
    rows, q, logits, scale = reference("gin", b, s, 2)
    e = make("gin", s, steps=2)
    try:
        got = run(e, b)
    finally:
        e.close()
    assert np.isfinite(got).all()
    close(got, logits, scale, "saturated, logits")


def test_range_fallback():
    """The last layer's b2 = 1e5 on eight columns: the rows, and with them r_t and q*, leave the f16 range where no layer kernel reads
    them as an operand -- one exact re-run, raised by the LSTM kernel, and the results within the rule of the same reference."""
    b = gp.synth_molhiv_batch(64, seed=7)
    w = {k: v.copy() for k, v in model_weights("gin").items()}
    cols = np.array([3, 64, 130, 255, 256, 271, 290, 299])
    w["node_mlp_2_bias"].reshape(5, 300)[4, cols] = np.float32(1e5)
    s2s = s2s_of()
    rows, q, logits, scale = reference("gin", b, s2s, 3, w=w)
    assert np.abs(q).max() > 6.6e4 and np.abs(W.forward(b, model_weights("gin"), eps=EPS).rows).max() < 3e4
    e = make("gin", s2s, steps=3, w=w)
    try:
        res = {}
        names = launched(e, lambda: res.update(got=e.forward(b)))
        assert e.exact_reruns() == 1 and SLOTS | {"gin_wide_layer_f32"} <= names, (e.exact_reruns(), names)
    finally:
        e.close()
    close(res["got"], logits, scale, "range fallback, logits")
    e = make("gin", s2s, steps=3)
    try:
        run(e, b, expect_reruns=0)
        assert e.exact_reruns() == 0
    finally:
        e.close()


def test_f16_mode_keeps_the_readout_fp32_accurate():
    """GIN's f16 numeric mode at 300: the rows are the f16 kernels', the readout on them is the restatement's within the rule."""
    b = gp.synth_molhiv_batch(64, seed=5)
    s2s = s2s_of()
    e = make("gin", s2s, steps=3)
    try:
        e.set_numeric_mode("f16", emb_dim=300)
        res = {}
        names = launched(e, lambda: res.update(got=e.forward(b, return_node_embeddings=True)))
        assert SLOTS | {"gin_wide_layer_f16"} <= names and e.exact_reruns() == 0, names
        got, rows = res["got"]
    finally:
        e.close()
    q, logits, _ = S.readout(rows, b, s2s, steps=3)
    close(got, logits, max(1.0, float(np.abs(rows).max()), float(np.abs(q).max()), float(np.abs(logits).max())), "f16 mode, logits on the returned rows")


@pytest.mark.parametrize("seed", [5, 7])
def test_readout_error_on_the_returned_rows(seed):
    """The readout alone: the restatement on the rows the engine itself returned (float32 values in float64), as a fraction of the rule
    with scale = the largest magnitude among rows, q* and logits."""
    b = gp.synth_molhiv_batch(64, seed=seed)
    s2s = s2s_of()
    for steps in (2, 3):
        e = make("gin", s2s, steps=steps)
        try:
            got, rows = run(e, b, return_node_embeddings=True)
        finally:
            e.close()
        q, logits, _ = S.readout(rows, b, s2s, steps=steps)
        scale = max(1.0, float(np.abs(rows).max()), float(np.abs(q).max()), float(np.abs(logits).max()))
        print(f"| {seed} | {steps} | {float(np.abs(got - logits).max()):.2e} | {err_ratio(got, logits, scale):.4f} |")
        close(got, logits, scale, ("readout alone", seed, steps))


# ---------------------------------------------------------------- 5. end to end: torch model -> files -> host CLI
@pytest.mark.parametrize("kind,vn", [("gin", False), ("gcn", True)], ids=["gin", "gcn-virtual"])
def test_end_to_end(kind, vn, tmp_path):
    pytest.importorskip("torch")
    model = S.set2set_model(kind, vn)
    b = T.batch_of(kind)
    want, scale, _ = T.run(model, b)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    export.export_weights(kind.upper(), model.state_dict(), str(wdir), set2set=True, **export_kwargs(kind, vn, 300))
    out = tmp_path / "HLS_output.txt"
    flags = ["--eps"] if kind == "gin" else []
    flags += ["--ogb-vn"] if vn else []
    base = [HOST, kind.upper(), "--emb-dim", "300"] + flags + ["--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--out", str(out)]
    p = subprocess.run(base + ["--set2set"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    cli = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    close(cli, want.logits, scale, (name_of(kind, vn), "host --set2set"))
    p = subprocess.run(base + ["--set2set", "--attn-pool"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--attn-pool" in p.stderr, p.stdout + p.stderr
    p = subprocess.run(base + ["--set2set", "--set2set-steps", "9"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "steps" in p.stderr, p.stdout + p.stderr


# ---------------------------------------------------------------- 6. speed guard
def _best(e, slots, runs=7):
    """Per slot, the best of three medians of `runs` device-event totals of one run (tests/test_attn_pool_gpu.test_speed_guard)."""
    best = {k: np.inf for k in slots}
    for _ in range(3):
        ms = {k: [] for k in slots}
        for _ in range(runs):
            t0 = e.profile_read()
            e.run()
            e.results()
            t1 = e.profile_read()
            for k in slots:
                ms[k].append(t1[k]["total_ms"] - t0.get(k, {"total_ms": 0.0})["total_ms"])
        for k in slots:
            best[k] = min(best[k], float(np.median(ms[k])))
    return best


def test_speed_guard():
    """2^14 molhiv-shaped graphs, GIN at 300, one process, device events.  Bounds from kernels that exist without the readout: each of
    s2s_dot_rows and s2s_pool_rows, per step, <= 1.5 x mean_pool_rows of a mean-readout run of the same batch (the same single read of
    the rows; the margin covers the dot's cross-lane sums); s2s_lstm per step <= 3 x one gin_wide_vn_update launch of a gin-virtual run
    (720 000 against 360 000 MACs per graph, times 1.5) -- here all three s2s_lstm launches of steps = 3, the cell-only first one
    included, are charged to the two that run the product, which asks more."""
    from tests import gin_wide_vn_ref as V
    b = gp.synth_molhiv_batch(1 << 14, seed=3)
    steps = 3
    e = make("gin")
    try:
        e.set_batch(b)
        e.run()
        e.results()
        mean = _best(e, (MEAN,))[MEAN]
        e.set_ogb_virtual_node(V.shapes_virtual_node(w1_scale=1.0 / 64))
        e.run()
        e.results()
        update = _best(e, ("gin_wide_vn_update",))["gin_wide_vn_update"] / 4
        e.set_ogb_virtual_node(None)
        e.set_set2set_pooling(s2s_of(), steps=steps)
        e.run()
        e.results()
        assert e.exact_reruns() == 0
        s = _best(e, (LSTM, DOT, POOL, HEAD))
    finally:
        e.close()
    dot, pool, lstm = s[DOT] / steps, s[POOL] / steps, s[LSTM] / (steps - 1)
    print(f"per step: s2s_dot_rows {dot:.4f} ms, s2s_pool_rows {pool:.4f} ms against mean_pool_rows {mean:.4f} ms; "
          f"s2s_lstm {lstm:.4f} ms against one gin_wide_vn_update launch {update:.4f} ms; s2s_head {s[HEAD]:.4f} ms")
    assert dot <= 1.5 * mean and pool <= 1.5 * mean, (dot, pool, mean)
    assert lstm <= 3.0 * update, (lstm, update)
