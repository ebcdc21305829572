"""PNA in the f16 numeric mode on the GPU (flowgnn.h: flowgnn_set_model_numeric_mode_dim at FLOWGNN_EMB_DIM_PNA; kernels:
flowgnn_amd/csrc/pna_f16.hip, pna_emb_f16.hip, pna_rows_f16.hip).

(a) The probe pins the arithmetic itself: on dyadic weights and a bipartite batch of in-degrees 0, 1, 2, 4 and 32 the fp32 sums of
    the mode are exact (tests/test_pna_f16_cpu.py proves which rows), so the kernels must reproduce the float64 restatement with one
    f16 rounding, to nearest even, of each of the 320 operands -- proven rows bit for bit, everything else within 1e-6 (1 + |x|) --
    and must stay apart, by more than 100 x that bound on more than half of the compared values, from the restatements without the
    rounding, with the rounding toward zero, with one aggregator left unrounded, and from the engine's own f32 result.
(b) The smallest shapes at which the kernels can go wrong (tests/pna_f16_ref.shape_cases), logits under TOL, rows printed.
(c) At a realistic shape |gpu - f64| <= tol (scale + |f64|), tol from the ladder (tests/pna_f16_ref.TOL).
(d) An operand beyond 6e4: one exact re-run, the f32 mode's bytes.
(e) The refusals, which launch nothing; the mode across weights, batches and outputs; flowgnn_get_h; device batches; groups; hipGraph;
    the host CLI.
Every test here fails on a library where width 80 is FLOWGNN_ERR_ARG."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, graphpack as gp, weights
from tests import pna_f16_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 8
F32, Q, F16 = 0, 1, 2
PNA_DIM = 80
f64 = lambda a: np.asarray(a, dtype=np.float64)


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def _rc(fn):
    try:
        fn()
    except FlowGNNError as ex:
        return ex.code, str(ex)
    return OK, ""


def counts(e, fn):
    """slot -> launches gained while fn() runs (and is synchronised)"""
    before = {k: v["launches"] for k, v in e.profile_read().items()}
    fn()
    e.sync()
    after = e.profile_read()
    return {k: v["launches"] - before.get(k, 0) for k, v in after.items() if v["launches"] > before.get(k, 0)}


def make(w, mode="f16", options=None):
    e = Engine("PNA", device=0, options=options or {})
    e.set_weights(w)
    if mode is not None:
        e.set_numeric_mode(mode, emb_dim=PNA_DIM)
    e.profile_enable(True)
    return e


def run(w, b, mode="f16", options=None, **fwd):
    """one engine of its own -> (the forward's tuple as float arrays, launches per slot, exact re-runs)"""
    e = make(w, mode, options)
    try:
        res = {}
        n = counts(e, lambda: res.update(got=e.forward(b, **fwd)))
        got = res["got"] if isinstance(res["got"], tuple) else (res["got"],)
        return [np.asarray(x).copy() for x in got], n, e.exact_reruns()
    finally:
        e.close()


def f16_only(n, slot, launches):
    assert n.get(slot) == launches, n
    for s in R.SPLIT_SLOTS + tuple(x for x in (R.RESIDENT_SLOT, R.FUSED_SLOT, R.DENSE_SLOT) if x != slot):
        assert s not in n, (s, n)


# ---------------------------------------------------------------- (a) the probe
PROBE_INSTANCES = [  # name, options, forward's outputs, the f16 slot and its launches
    ("resident-default", {}, {}, R.RESIDENT_SLOT, 1),
    ("resident-rows", {}, {"return_node_embeddings": True, "return_embeddings": True}, R.RESIDENT_SLOT, 1),
    ("per-layer-fused", {"pna_resident": 0}, {"return_node_embeddings": True, "return_embeddings": True}, R.FUSED_SLOT, 4),
    ("two-kernel", {"pna_fused": 0}, {"return_node_embeddings": True, "return_embeddings": True}, R.DENSE_SLOT, 4),
]


@pytest.fixture(scope="module")
def probe():
    b, w = R.probe_batch(), R.probe_weights()
    res, exact, worst, margin = R.probe_check(b, w)
    assert worst <= 24.0 and margin < -100.0
    others = {v: R.forward(b, w, *v) for v in R.VARIANTS}
    return b, w, res, exact, others


def _rows_of(got, fwd):
    """(logits, embeddings or None, rows or None) of a forward's tuple"""
    it = iter(got)
    logits = next(it)
    emb = next(it) if fwd.get("return_embeddings") else None
    rows = next(it) if fwd.get("return_node_embeddings") else None
    return logits, emb, rows


@pytest.mark.parametrize("name,options,fwd,slot,launches", PROBE_INSTANCES, ids=[i[0] for i in PROBE_INSTANCES])
def test_probe(name, options, fwd, slot, launches, probe):
    """Whether v_rcp_f32 of a power of two and v_sqrt_f32 of a perfect square are exact on this device is supposed, not known; a value
    one ulp off the f16 grid rounds back onto it, but a std of in-degree 2 is a tie between two f16 values and would not."""
    b, w, want, exact, others = probe
    got, n, reruns = run(w, b, "f16", options, **fwd)
    assert reruns == 0
    f16_only(n, slot, launches)
    logits, emb, rows = _rows_of(got, fwd)
    worst = float((np.abs(f64(logits) - want.logits) / R.bound(want.logits)).max())
    print(f"{name}: logits: max |gpu - rne| / bound = {worst:.3g}")
    assert worst <= 1.0, worst
    if rows is None:
        return
    rows = f64(rows).reshape(want.rows.shape)
    miss = np.argwhere(rows[exact] != want.rows[exact])
    rest = float((np.abs(rows - want.rows) / R.bound(want.rows))[~exact].max())
    print(f"{name}: rows: {len(miss)} of {int(exact.sum()) * R.D} proven values differ (asserted bit for bit); the other rows at {rest:.3g} of the bound")
    assert len(miss) == 0, miss[:8]
    assert rest <= 1.0, rest
    # apart from every restatement the references tell apart, and from the engine's own f32 result
    f32, n32, _ = run(w, b, None, options, **fwd)
    assert not any(s in n32 for s in (R.RESIDENT_SLOT, R.FUSED_SLOT, R.DENSE_SLOT)), n32
    f32rows = f64(_rows_of(f32, fwd)[2]).reshape(want.rows.shape)
    for v, o in list(others.items()) + [(("f32 mode", None), None)]:
        x = f32rows if o is None else o.rows
        for cname, mask in R.compared(b, v if o is not None else ("none", None)).items():
            ok, frac = R.separated(rows, x, want.rows, mask)
            print(f"{name}: apart from {v[0] if o is None else R.variant_name(v)} ({cname}): {frac:.3f} of {int(mask.sum())} values")
            assert ok, (v, cname, frac)


def test_probe_resident_and_per_layer_agree_in_every_byte(probe):
    b, w, _, _, _ = probe
    fwd = {"return_node_embeddings": True, "return_embeddings": True}
    res, n_res, _ = run(w, b, "f16", {}, **fwd)
    per, n_per, _ = run(w, b, "f16", {"pna_resident": 0}, **fwd)
    dflt, _, _ = run(w, b, "f16", {})
    emb_only, _, _ = run(w, b, "f16", {}, return_embeddings=True)  # the _emb instance
    f16_only(n_res, R.RESIDENT_SLOT, 1)
    f16_only(n_per, R.FUSED_SLOT, 4)
    for a, p in zip(res, per):
        assert a.tobytes() == p.tobytes()
    assert dflt[0].tobytes() == res[0].tobytes() and emb_only[0].tobytes() == res[0].tobytes() and emb_only[1].tobytes() == res[1].tobytes()


# ---------------------------------------------------------------- (b) the shape families
CASES = R.shape_cases()


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_shape_families(c):
    """logits under TOL against the float64 forward; the rows are printed (tests/test_gcn_wide_f16_gpu.py says why: where fp32 and
    float64 fall on either side of an f16 rounding boundary the operands differ by a whole f16 spacing; the probe holds rows to bits)"""
    w = weights.synth_pna_weights(7)
    ref = R.forward(c.batch, w, "none")
    tol = R.TOL[("synth", "logits")]
    e = make(w, "f16", c.options)
    try:
        if c.slot == R.DENSE_SLOT and c.name == "graphs-of-70-nodes":
            assert e.graph_tile_fill(c.batch.nums_of_nodes, c.batch.nums_of_edges) < 0.4
        res = {}
        n = counts(e, lambda: res.update(plain=e.forward(c.batch).copy()))  # the default instance first (outputs stay on once asked for)
        f16_only(n, c.slot, 1 if c.slot == R.RESIDENT_SLOT else 4)
        n = counts(e, lambda: res.update(got=e.forward(c.batch, return_node_embeddings=True)))
        f16_only(n, c.slot, 1 if c.slot == R.RESIDENT_SLOT else 4)
        if c.name == "tile-build-off":
            assert "pna_tile_desc" in n and "pna_tile_build" not in n, n
        logits, rows = res["got"]
        assert res["plain"].tobytes() == np.asarray(logits).tobytes()  # the row-storing instance: the same logits
        assert np.isfinite(rows).all()
        r_l, r_r = R.rule(f64(logits), ref, tol), R.rule(f64(rows), ref, tol)
        print(f"{c.name}: logits at {r_l:.3f} of tol {tol:g}, rows at {r_r:.3f} (scale {ref.scale:.3g})")
        assert r_l <= 1.0, (c.name, r_l)
        assert e.exact_reruns() == 0
    finally:
        e.close()


# ---------------------------------------------------------------- (c) accuracy at a realistic shape
@pytest.mark.parametrize("seed", R.ACCURACY_SEEDS)
def test_accuracy_at_a_realistic_shape(seed):
    b = R.accuracy_batch(seed)
    assert b.num_graphs == 24
    w = R.accuracy_weights("synth")
    ref, rne = R.forward(b, w, "none"), R.forward(b, w, "rne")
    tol = R.TOL[("synth", "logits")]
    assert R.rule(rne.logits, ref, tol) <= 0.5  # (tests/test_pna_f16_cpu.py: the ladder's rung)
    out = {}
    for mode in ("f16", None):
        got, n, reruns = run(w, b, mode, {}, return_node_embeddings=True)
        assert reruns == 0
        if mode:
            f16_only(n, R.RESIDENT_SLOT, 1)
        else:
            assert n.get("pna_resident") == 1 and R.RESIDENT_SLOT not in n, n
        out[mode] = [f64(x) for x in got]
    r16, r32 = R.rule(out["f16"][0], ref, tol), R.rule(out[None][0], ref, tol)
    print(f"seed {seed}: logits: f16 mode at {r16:.3f} of tol {tol:g} (restatement {R.rule(rne.logits, ref, tol):.3f}, f32 mode {r32:.4f})")
    rt = R.TOL[("synth", "rows")]
    print(f"seed {seed}: rows: f16 mode at {R.rule(out['f16'][1], ref, rt):.3f} of tol {rt:g} (restatement {R.rule(rne.rows, ref, rt):.3f})")
    assert r16 <= 1.0, r16
    assert np.mean(out["f16"][0] != out[None][0]) > 0.5  # the mode is engaged
    assert R.rule(out["f16"][1], ref, rt) <= 1.0


@pytest.mark.parametrize("seed", R.ACCURACY_SEEDS)
def test_rows_with_the_trained_weights_are_under_their_rung(seed):
    b, w = R.accuracy_batch(seed), R.accuracy_weights("trained")
    ref = R.forward(b, w, "none")
    tol = R.TOL[("trained", "rows")]
    got, n, reruns = run(w, b, "f16", {}, return_node_embeddings=True)
    f16_only(n, R.RESIDENT_SLOT, 1)
    r = R.rule(f64(got[1]), ref, tol)
    print(f"trained weights, seed {seed}: rows at {r:.3f} of tol {tol:g} (scale {ref.scale:.3g})")
    assert reruns == 0 and r <= 1.0, r


# ---------------------------------------------------------------- (d) range
def test_range_flag_reruns_on_the_exact_path():
    """the encoder table scaled until an aggregate passes 6e4: the kernel raises the flag, the engine repeats the pass on the fp32
    path, and that is what the f32 mode does on this input"""
    b, w = R.accuracy_batch(3), weights.synth_pna_weights(7)
    h0 = R.forward(b, w, "none").hs[0]
    src = np.unique(b.global_edges()[:, 0])
    above = dict(w)
    above["node_embedding_weight"] = (np.asarray(w["node_embedding_weight"], np.float32) * np.float32(8.0e4 / np.abs(h0[src]).max())).astype(np.float32)
    assert np.abs(R.forward(b, above, "none").hs[0][src]).max() > 6.6e4
    out = {}
    for mode in ("f16", None):
        got, n, reruns = run(above, b, mode, {}, return_node_embeddings=True)
        assert reruns == 1, (mode, reruns, n)
        assert (n.get(R.RESIDENT_SLOT), n.get("pna_resident")) == ((1, None) if mode else (None, 1)), n
        assert R.FUSED_SLOT not in n and R.DENSE_SLOT not in n and n.get("pna_dense") == 4, n  # the re-run: the fp32 pipe
        out[mode] = got
    for a, f in zip(out["f16"], out[None]):
        assert a.tobytes() == f.tobytes()


# ---------------------------------------------------------------- (e) plumbing
def _err(e):
    return (e.lib.flowgnn_last_error(e._h) or b"").decode()


def _model(e, d, mode):
    return e.lib.flowgnn_set_model_numeric_mode_dim(e._h, d, mode), _err(e)


def _dim(e, d, mode):
    return e.lib.flowgnn_set_numeric_mode_dim(e._h, d, mode), _err(e)


def test_refusals_in_both_orders_launch_nothing():
    b, w = gp.synth_hep10k_batch(4, seed=5, with_eigen=False), weights.synth_pna_weights(7)
    e = Engine("PNA")
    try:
        e.set_weights(w)
        e.profile_enable(True)

        def refusals():
            assert e.lib.flowgnn_set_numeric_mode(e._h, F16) == ERR_UNSUPPORTED and "flowgnn_set_model_numeric_mode_dim" in _err(e)
            assert _dim(e, 100, F16)[0] == ERR_UNSUPPORTED
            assert _model(e, 100, F16)[0] == ERR_UNSUPPORTED
            rc, text = _dim(e, PNA_DIM, F16)
            assert rc == ERR_ARG and "flowgnn_set_model_numeric_mode_dim" in text, (rc, text)
            for bad in (0, 79, 81, 300, -80):
                assert _model(e, bad, F16)[0] == ERR_ARG, bad
            for bad in (-1, 3, 16):
                assert _model(e, PNA_DIM, bad)[0] == ERR_ARG, bad
            for pooling in ("sum", "max"):
                assert _rc(lambda: e.set_pooling(pooling))[0] == ERR_UNSUPPORTED

        n = counts(e, refusals)  # ---- in f32 mode
        assert n == {}, n
        f32 = e.forward(b).copy()
        assert _model(e, PNA_DIM, F16)[0] == OK
        n = counts(e, refusals)  # ---- and with the mode on: it stays on
        assert n == {}, n
        n = counts(e, lambda: e.forward(b))
        f16_only(n, R.RESIDENT_SLOT, 1)
        f16 = e.results().copy()
        assert not np.array_equal(f16, f32)
        # width 80 takes the plain call's modes too
        assert _model(e, PNA_DIM, Q)[0] == OK
        q = e.forward(b).copy()
        assert _model(e, PNA_DIM, F32)[0] == OK
        assert np.array_equal(e.forward(b), f32)
        e.set_numeric_mode("q6.10")
        assert np.array_equal(e.forward(b), q)
        e.set_numeric_mode("f16", emb_dim=PNA_DIM)
        assert np.array_equal(e.forward(b), f16)
        e.set_numeric_mode("f32")  # the plain call always goes back
        assert np.array_equal(e.forward(b), f32)
    finally:
        e.close()


@pytest.mark.parametrize("model", ["GIN", "GIN-VN", "GCN", "GAT", "DGN"])
def test_width_80_stays_an_argument_error_on_every_other_engine(model):
    e = Engine(model)
    try:
        for mode in (F32, Q, F16):
            assert _model(e, PNA_DIM, mode)[0] == ERR_ARG and _dim(e, PNA_DIM, mode)[0] == ERR_ARG, mode
    finally:
        e.close()


def test_the_mode_survives_weights_batches_and_outputs():
    b, b2 = gp.synth_hep10k_batch(6, seed=5, with_eigen=False), gp.synth_hep10k_batch(4, seed=6, with_eigen=False)
    w, w2 = weights.synth_pna_weights(7), weights.synth_pna_weights(8)
    e = Engine("PNA")
    try:
        e.set_numeric_mode("f16", emb_dim=PNA_DIM)  # before the weights
        e.set_weights(w)
        e.profile_enable(True)
        f16_only(counts(e, lambda: e.forward(b)), R.RESIDENT_SLOT, 1)
        first = e.results().copy()
        e.set_weights(w2)
        f16_only(counts(e, lambda: e.forward(b2)), R.RESIDENT_SLOT, 1)
        ref2 = R.forward(b2, w2, "none")
        assert R.rule(f64(e.results()), ref2, R.TOL[("synth", "logits")]) <= 1.0
        e.set_weights(w)
        res = {}
        n = counts(e, lambda: res.update(got=e.forward(b, return_embeddings=True, return_node_embeddings=True)))
        f16_only(n, R.RESIDENT_SLOT, 1)
        logits, emb, rows = res["got"]
        assert np.array_equal(logits, first)
        rne = R.forward(b, w, "rne")
        off = b.node_offsets()
        pooled = np.add.reduceat(f64(rows), off[:-1], axis=0) / f64(b.nums_of_nodes)[:, None]
        assert np.abs(f64(emb) - pooled).max() <= 1e-5 * (1 + np.abs(pooled).max())  # the embeddings are the mean of the rows
        assert R.rule(f64(rows), rne, 1e-4) <= 1.0  # ... and the rows are the mode's
        # flowgnn_get_h: h_4 of the f16 per-layer path -- the resident rows, byte for byte
        n = counts(e, lambda: res.update(h=e.final_h()))
        assert n.get(R.FUSED_SLOT) == 4 and "pna_layer_fused" not in n, n
        assert res["h"].tobytes() == np.asarray(rows).tobytes()
        assert e.exact_reruns() == 0
    finally:
        e.close()


def test_device_batch_form():
    pytest.importorskip("torch")
    from tests.test_device_batch_gpu import device_args
    b, w = gp.synth_hep10k_batch(6, seed=5, with_eigen=False), weights.synth_pna_weights(7)
    e = make(w)
    try:
        want = e.forward(b).copy()
        for layout in ("pyg", "reference"):
            args, kw = device_args(b, layout, "PNA")
            res = {}
            n = counts(e, lambda: res.update(got=e.forward_device(*args, **kw)))
            f16_only(n, R.RESIDENT_SLOT, 1)
            got = res["got"]
            got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
            assert np.array_equal(got.reshape(want.shape), want), layout
    finally:
        e.close()


def test_group_form():
    b, w = gp.synth_hep10k_batch(9, seed=5, with_eigen=False), weights.synth_pna_weights(7)
    single, _, _ = run(w, b, "f16", {})
    g = EngineGroup("PNA", [0, 0])
    try:
        g.set_weights(w)
        assert _rc(lambda: g.set_numeric_mode("f16"))[0] == ERR_UNSUPPORTED
        assert g.lib.flowgnn_group_set_numeric_mode_dim(g._h, PNA_DIM, F16) == ERR_ARG
        assert g.lib.flowgnn_group_set_model_numeric_mode_dim(g._h, 100, F16) == ERR_UNSUPPORTED
        g.set_numeric_mode("f16", emb_dim=PNA_DIM)
        members = [C.c_void_p(g.lib.flowgnn_group_engine(g._h, i)) for i in range(2)]
        for h in members:
            assert g.lib.flowgnn_profile_enable(h, 1) == OK
        got = g.forward(b).copy()
        assert np.array_equal(got, single[0])
        for h in members:
            n = C.c_int()
            names, ms, cnt = (C.c_char_p * 32)(), (C.c_double * 32)(), (C.c_longlong * 32)()
            assert g.lib.flowgnn_profile_read(h, C.byref(n), names, ms, cnt) == OK
            ran = {names[i].decode(): int(cnt[i]) for i in range(n.value) if cnt[i] > 0}
            assert ran.get(R.RESIDENT_SLOT, 0) >= 1 and "pna_resident" not in ran, ran
    finally:
        g.close()


def test_one_hipgraph_replay_equals_the_eager_bytes(monkeypatch):
    b, w = gp.synth_hep10k_batch(6, seed=5, with_eigen=False), weights.synth_pna_weights(7)
    monkeypatch.setenv("FLOWGNN_HIPGRAPH", "0")
    eager, _, _ = run(w, b, "f16", {})
    monkeypatch.setenv("FLOWGNN_HIPGRAPH", "1")
    e = Engine("PNA", device=0)  # (no profiler: its events keep the engine from capturing)
    try:
        e.set_weights(w)
        e.set_numeric_mode("f16", emb_dim=PNA_DIM)
        e.set_batch(b)
        outs = []
        for _ in range(3):  # plain, captured + launched, replay
            e.run()
            outs.append(e.results().copy())
        assert e.graph_replays() == 2
        for o in outs:
            assert o.tobytes() == eager[0].tobytes()
        assert e.exact_reruns() == 0
    finally:
        e.close()


def test_host_cli_runs_pna_in_f16_mode(tmp_path):
    """`host PNA --numeric f16` on a written pack: the engine's bytes (as the eight decimals the host prints), not the f32 mode's"""
    b, w = gp.synth_hep10k_batch(5, seed=3, with_eigen=False), weights.synth_pna_weights(7)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    weights.SAVERS["PNA"](w, str(wdir))
    got = {}
    for mode in ("f16", "f32"):
        out = tmp_path / f"out_{mode}.txt"
        p = subprocess.run([HOST, "PNA", "--numeric", mode, "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--out", str(out)],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        got[mode] = [ln.split(":")[1].strip() for ln in open(out).read().strip().splitlines()]
    engine, _, _ = run(w, b, "f16", {})
    assert got["f16"] == ["%.8f" % x for x in engine[0]]
    assert np.mean(np.array(got["f16"]) != np.array(got["f32"])) > 0.5
