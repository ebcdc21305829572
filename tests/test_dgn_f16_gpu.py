"""DGN in the f16 numeric mode on the GPU (flowgnn.h: flowgnn_set_model_numeric_mode on a FLOWGNN_MODEL_DGN engine; kernels:
flowgnn_amd/csrc/dgn_f16.hip, dgn_emb_f16.hip, dgn_rows_f16.hip).

(a) The probe pins the arithmetic itself: on dyadic weights and eigenvectors and graphs of sources -> sinks -> drains every fp32 sum of
    the mode is exact (tests/test_dgn_f16_cpu.py proves it for every row), so the kernels must reproduce the float64 restatement with
    one f16 rounding, to nearest even, of each operand of the matrix-pipe products -- every value of h_4 bit for bit, the logits within
    1e-6 (1 + |x|) -- and must stay apart, by more than 100 x that bound on more than half of the compared values, from the
    restatements without the rounding, with the rounding toward zero, with one operand left unrounded, and from the engine's own f32
    result.  The resident and the per-layer matrix-pipe kernels agree in every byte where the default pair does.
(b) The smallest shapes at which the kernels can go wrong (tests/dgn_f16_ref.shape_cases), logits under TOL, rows printed.
(c) At a realistic shape |gpu - f64| <= tol (scale + |f64|), tol from the ladder (tests/dgn_f16_ref.TOL).
(d) A source row or an a2 beyond 6e4: one exact re-run, the f32 mode's bytes.
(e) Jobs whose plan has no matrix-pipe kernel return the f32 mode's bytes; the refusals, which launch nothing; the call on the other
    engines; the mode across weights, batches and outputs; flowgnn_get_h; device batches; groups; hipGraph; the host CLI; speed.
Every test marked (*) fails on a library without flowgnn_set_model_numeric_mode -- there the call does not exist."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, graphpack as gp, weights, _lib
from tests import dgn_f16_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 8
F32, Q, F16 = 0, 1, 2
DGN = _lib.MODEL_IDS["DGN"]
f64 = lambda a: np.asarray(a, dtype=np.float64)
ROWS = {"return_node_embeddings": True, "return_embeddings": True}
PER_LAYER = {"dgn_resident": 0, "dgn_mfma_agg": 1}


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
    e = Engine("DGN", device=0, options=options or {})
    e.set_weights(w)
    if mode is not None:
        e.set_numeric_mode(mode, emb_dim=100)
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
    for s in R.DEFAULT_SLOTS + tuple(x for x in (R.RESIDENT_SLOT, R.LAYER_SLOT) if x != slot):
        assert s not in n, (s, n)


def no_f16(n):
    assert R.RESIDENT_SLOT not in n and R.LAYER_SLOT not in n, n


def _rows_of(got, fwd):
    """(logits, embeddings or None, rows or None) of a forward's tuple"""
    it = iter(got)
    logits = next(it)
    emb = next(it) if fwd.get("return_embeddings") else None
    rows = next(it) if fwd.get("return_node_embeddings") else None
    return logits, emb, rows


# ---------------------------------------------------------------- (a) the probe
PROBE_INSTANCES = [  # name, options, the f16 slot and its launches
    ("resident-rows", R.PROBE_OPTIONS, R.RESIDENT_SLOT, 1),
    ("per-layer-matrix-pipe", PER_LAYER, R.LAYER_SLOT, 4),
]


@pytest.fixture(scope="module")
def probe():
    (b, roles), w = R.probe_batch(), R.probe_weights()
    res, worst = R.probe_check(b, w)
    assert (worst <= 24.0).all()
    others = {v: R.forward(b, w, *v) for v in R.VARIANTS}
    return b, roles, w, res, others


@pytest.mark.parametrize("name,options,slot,launches", PROBE_INSTANCES, ids=[i[0] for i in PROBE_INSTANCES])
def test_probe(name, options, slot, launches, probe):
    """(*) Supposed, not known: that the MFMA adds products whose every partial sum is representable without losing a bit, and that
    v_rcp_f32 of a power of two is exact on this device."""
    b, roles, w, want, others = probe
    got, n, reruns = run(w, b, "f16", options, **ROWS)
    assert reruns == 0
    f16_only(n, slot, launches)
    logits, emb, rows = _rows_of(got, ROWS)
    worst = float((np.abs(f64(logits) - want.logits) / R.bound(want.logits)).max())
    print(f"{name}: logits: max |gpu - rne| / bound = {worst:.3g}")
    rows = f64(rows).reshape(want.rows.shape)
    miss = np.argwhere(rows != want.rows)
    print(f"{name}: rows: {len(miss)} of {rows.size} proven values differ (asserted bit for bit)")
    assert len(miss) == 0, miss[:8]
    assert worst <= 1.0, worst
    off = b.node_offsets()
    pooled = np.add.reduceat(want.rows, off[:-1], axis=0) / f64(b.nums_of_nodes)[:, None]
    assert (np.abs(f64(emb) - pooled) <= R.bound(pooled)).all()
    # apart from every restatement the references tell apart, and from the engine's own f32 result
    f32, n32, _ = run(w, b, None, options, **ROWS)
    no_f16(n32)
    f32rows = f64(_rows_of(f32, ROWS)[2]).reshape(want.rows.shape)
    for v, o in list(others.items()) + [(("f32 mode", None), None)]:
        x = f32rows if o is None else o.rows
        mask = R.compared(b, roles, v if o is not None else ("none", None))
        ok, frac = R.separated(rows, x, want.rows, mask)
        print(f"{name}: apart from {v[0] if o is None else R.variant_name(v)}: {frac:.3f} of {int(mask.sum())} values")
        assert ok, (v, frac)


def test_resident_and_per_layer_agree_in_every_byte():
    """(*) The default pair's relation carries over (tests/test_dgn_gpu.py: test_resident_kernel_is_the_per_layer_path_bit_for_bit, whose
    options these are): full kNN tiles, ragged molecule tiles forced onto the matrix pipe, a batch that ends inside a tile -- rows,
    embeddings and logits; flowgnn_get_h after a resident run repeats the pass per layer, in the mode."""
    from tests.test_dgn_gpu import _without_duplicates
    from tests.ref_pin import with_eigen
    w = weights.synth_dgn_weights(7)
    per_layer = make(w, "f16", {"dgn_resident": 0, "dgn_fold_readout": 0, "dgn_mfma_agg": 1})
    forced = make(w, "f16", {"dgn_resident": 2, "dgn_mfma_agg": 1, "dgn_binpack": 0})  # (the per-layer path's tiles: graphs in batch order)
    try:
        mol = _without_duplicates(with_eigen(gp.synth_molhiv_batch(300, seed=78), 1))
        for b in (gp.synth_hep10k_batch(70, seed=77), mol, gp.synth_hep10k_batch(3, seed=79)):
            res = {}
            n = counts(per_layer, lambda: res.update(want=[np.asarray(x).copy() for x in per_layer.forward(b, **ROWS)]))
            f16_only(n, R.LAYER_SLOT, 4)
            n = counts(forced, lambda: res.update(got=[np.asarray(x).copy() for x in forced.forward(b, **ROWS)]))
            f16_only(n, R.RESIDENT_SLOT, 1)
            assert all(np.isfinite(x).all() for x in res["want"])
            for a, p in zip(res["got"], res["want"]):
                assert a.tobytes() == p.tobytes()
            n = counts(forced, lambda: res.update(h=forced.final_h()))
            assert n.get(R.LAYER_SLOT) == 4 and "dgn_layer_fused" not in n, n
            assert np.asarray(res["h"]).tobytes() == res["got"][2].tobytes()  # the taps of a forward in the mode are the mode's values
        # the default and the _emb instance: the same logits and pooled rows as the row-storing one
        b = gp.synth_hep10k_batch(70, seed=77)
        rows_inst = [np.asarray(x).copy() for x in forced.forward(b, **ROWS)]
        dflt, _, _ = run(w, b, "f16", {"dgn_resident": 2, "dgn_mfma_agg": 1, "dgn_binpack": 0})
        emb_only, _, _ = run(w, b, "f16", {"dgn_resident": 2, "dgn_mfma_agg": 1, "dgn_binpack": 0}, return_embeddings=True)
        assert dflt[0].tobytes() == rows_inst[0].tobytes() and emb_only[0].tobytes() == rows_inst[0].tobytes()
        assert emb_only[1].tobytes() == rows_inst[1].tobytes()
        assert per_layer.exact_reruns() == 0 and forced.exact_reruns() == 0
    finally:
        per_layer.close()
        forced.close()


# ---------------------------------------------------------------- (b) the shape families
CASES = R.shape_cases()


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_shape_families(c):
    """logits under TOL against the float64 forward; the rows are printed (where fp32 and float64 fall on either side of an f16
    rounding boundary the operands differ by a whole f16 spacing; the probe holds rows to bits)"""
    w = weights.synth_dgn_weights(7)
    ref = R.forward(c.batch, w, "none")
    tol = R.TOL[("synth", "logits")]
    e = make(w, "f16", c.options)
    try:
        res = {}
        n = counts(e, lambda: res.update(plain=e.forward(c.batch).copy()))  # the default instance first (outputs stay on once asked for)
        f16_only(n, R.RESIDENT_SLOT, 1)
        n = counts(e, lambda: res.update(got=e.forward(c.batch, return_node_embeddings=True)))
        f16_only(n, R.RESIDENT_SLOT, 1)
        logits, rows = res["got"]
        assert res["plain"].tobytes() == np.asarray(logits).tobytes()  # the row-storing instance: the same logits
        assert np.isfinite(rows).all()
        r_l, r_r = R.rule(f64(logits), ref, tol), R.rule(f64(rows), ref, tol)
        print(f"{c.name}: logits at {r_l:.3f} of tol {tol:g}, rows at {r_r:.3f} (scale {ref.scale:.3g})")
        assert r_l <= 1.0, (c.name, r_l)
        assert e.exact_reruns() == 0
    finally:
        e.close()


def test_out_of_range_edges_are_refused_as_in_the_default_mode():
    """an out-of-range edge becomes the self-loop on its graph's node 0 in the tile build and raises the batch's error flag: the forward
    is refused in the mode as it is without it (tests/test_dgn_gpu.py), and the engine goes on"""
    w = weights.synth_dgn_weights(7)
    good, bad = gp.synth_hep10k_batch(4, seed=83), gp.synth_hep10k_batch(4, seed=83)
    bad.edge_list[3] = [0, 1000]
    e = make(w, "f16", {"dgn_resident": 2})
    try:
        want = e.forward(good).copy()
        with pytest.raises(FlowGNNError):
            e.forward(bad)
        n = counts(e, lambda: e.forward(good))
        f16_only(n, R.RESIDENT_SLOT, 1)
        assert e.results().tobytes() == want.tobytes()
    finally:
        e.close()


def test_more_tiles_than_the_persistent_grid():
    """about 800 hep10k-shaped graphs are more than 256 tiles: a workgroup walks a second tile (slot parity, the next tile's records)"""
    b, w = gp.synth_hep10k_batch(800, seed=21), weights.synth_dgn_weights(7)
    ref = R.forward(b, w, "none")
    tol = R.TOL[("synth", "logits")]
    e = make(w, "f16")
    try:
        assert e.graph_tile_fill(b.nums_of_nodes, b.nums_of_edges) >= 0.4 and b.total_nodes > 256 * R.TILE_ROWS
        res = {}
        n = counts(e, lambda: res.update(got=e.forward(b, return_node_embeddings=True)))
        f16_only(n, R.RESIDENT_SLOT, 1)
        logits, rows = res["got"]
        r_l, r_r = R.rule(f64(logits), ref, tol), R.rule(f64(rows), ref, R.TOL[("synth", "rows")])
        print(f"800 graphs: logits at {r_l:.3f} of tol {tol:g}, rows at {r_r:.3f} of their rung")
        assert r_l <= 1.0 and r_r <= 1.0 and e.exact_reruns() == 0
    finally:
        e.close()


# ---------------------------------------------------------------- (c) accuracy at a realistic shape
@pytest.mark.parametrize("wname", ["synth", "trained"])
@pytest.mark.parametrize("seed", R.ACCURACY_SEEDS)
def test_accuracy_at_a_realistic_shape(seed, wname):
    """(*)"""
    b = R.accuracy_batch(seed)
    assert b.num_graphs == 24
    w = R.accuracy_weights(wname)
    ref, rne = R.forward(b, w, "none"), R.forward(b, w, "rne")
    tl, tr = R.TOL[(wname, "logits")], R.TOL[(wname, "rows")]
    assert R.rule(rne.logits, ref, tl) <= 0.5 and R.rule(rne.rows, ref, tr) <= 0.5  # (tests/test_dgn_f16_cpu.py: the ladder's rungs)
    out = {}
    for mode in ("f16", None):
        got, n, reruns = run(w, b, mode, {}, return_node_embeddings=True)
        assert reruns == 0
        if mode:
            f16_only(n, R.RESIDENT_SLOT, 1)
        else:
            assert n.get("dgn_resident") == 1, n
            no_f16(n)
        out[mode] = [f64(x) for x in got]
    r16, r32 = R.rule(out["f16"][0], ref, tl), R.rule(out[None][0], ref, tl)
    print(f"{wname}, seed {seed}: logits: f16 mode at {r16:.3f} of tol {tl:g} (restatement {R.rule(rne.logits, ref, tl):.3f}, f32 mode {r32:.4f})")
    rr = R.rule(out["f16"][1], ref, tr)
    print(f"{wname}, seed {seed}: rows: f16 mode at {rr:.3f} of tol {tr:g} (restatement {R.rule(rne.rows, ref, tr):.3f}, f32 mode {R.rule(out[None][1], ref, tr):.4f})")
    assert r16 <= 1.0, r16
    assert rr <= 1.0, rr
    assert np.mean(out["f16"][1] != out[None][1]) > 0.5  # the mode is engaged


# ---------------------------------------------------------------- (d) range
def test_range_flag_reruns_on_the_exact_path():
    """the encoder table scaled until |h_0| passes 6e4: the kernel raises the flag, the engine repeats the pass on the fp32 path, and
    that is what the f32 mode does on this input"""
    b, w = R.accuracy_batch(3), weights.synth_dgn_weights(7)
    h0 = R.forward(b, w, "none").hs[0]
    above = dict(w)
    above[R.K_EMB] = (np.asarray(w[R.K_EMB], np.float32) * np.float32(8.0e4 / np.abs(h0).max())).astype(np.float32)
    assert np.abs(R.forward(b, above, "none").hs[0]).max() > 6.6e4
    out = {}
    for mode in ("f16", None):
        got, n, reruns = run(above, b, mode, {}, return_node_embeddings=True)
        assert reruns == 1, (mode, reruns, n)
        assert (n.get(R.RESIDENT_SLOT), n.get("dgn_resident")) == ((1, None) if mode else (None, 1)), n
        assert R.LAYER_SLOT not in n and n.get("dgn_dense") == 4, n  # the re-run: the fp32 pipe
        out[mode] = got
    for a, f in zip(out["f16"], out[None]):
        assert a.tobytes() == f.tobytes()


def _two_kinds(h_a, h_b, cross, copies=6):
    """`copies` graphs (96 of a tile's 128 rows) of eight nodes of kind A (every feature of h_0 is h_a) and eight of kind B (h_b), eig1
    +1/4 and -1/4.  cross: every node has in-edges from the eight nodes of the OTHER kind (and as many out-edges); else sources A ->
    sinks B, one in-edge each"""
    n = 16
    f = np.zeros((n, 9), np.int32)
    f[8:, 0] = 1
    if cross:
        el = [(u, v) for v in range(n) for u in (range(8, 16) if v < 8 else range(8))]
    else:
        el = [(v - 8, v) for v in range(8, 16)]
    el = np.array(el, np.int32)
    eig = np.zeros((n, 4), np.float32)
    eig[:8, 1], eig[8:, 1] = 0.25, -0.25
    b = gp.GraphBatch(np.full(copies, n, np.int32), np.full(copies, len(el), np.int32), np.tile(f, (copies, 1)), np.tile(el, (copies, 1)),
                      np.zeros((copies * len(el), 3), np.int32), np.tile(eig, (copies, 1)))
    w = weights.synth_dgn_weights(7)
    T = np.zeros_like(np.asarray(w[R.K_EMB], np.float32))
    T[0, 0, :], T[0, 1, :] = h_a, h_b
    w[R.K_EMB] = T
    return b, w


def test_range_flag_through_a2_alone():
    """|h| = 4e4 everywhere and a1 = +-4e4 (eight in-edges, eight out-edges), but the two kinds have opposite signs: a2 = |h_A - h_B| = 8e4"""
    b, w = _two_kinds(4.0e4, -4.0e4, cross=True)
    ref = R.forward(b, w, "none")
    assert np.abs(ref.hs[0]).max() < 6.0e4
    opts = {"dgn_mfma_agg": 1, "dgn_resident": 2}
    out = {}
    for mode in ("f16", None):
        got, n, reruns = run(w, b, mode, opts, return_node_embeddings=True)
        assert reruns == 1, (mode, reruns, n)
        assert (n.get(R.RESIDENT_SLOT), n.get("dgn_resident")) == ((1, None) if mode else (None, 1)), n
        out[mode] = got
    for a, f in zip(out["f16"], out[None]):
        assert a.tobytes() == f.tobytes()


def test_range_flag_through_a_source_row_alone():
    """h_0 = 7e4 on every node, sources -> sinks: a1 = 0 (a sink has no out-edge) and a2 = |h_u - h_v| = 0, so the default kernels see
    nothing beyond 6e4 and do not re-run; in the mode the source rows are rounded to f16, where 7e4 is an infinity: the flag trips on h
    itself, and the result is the fp32 path's (option dgn_mfma=32), byte for byte"""
    b, w = _two_kinds(7.0e4, 7.0e4, cross=False)
    opts = {"dgn_mfma_agg": 1, "dgn_resident": 2}
    got, n, reruns = run(w, b, "f16", opts, return_node_embeddings=True)
    assert reruns == 1 and n.get(R.RESIDENT_SLOT) == 1 and n.get("dgn_dense") == 4, (reruns, n)
    f32, n32, reruns32 = run(w, b, None, opts, return_node_embeddings=True)
    assert reruns32 == 0 and n32.get("dgn_resident") == 1, (reruns32, n32)
    exact, _, _ = run(w, b, None, dict(opts, dgn_mfma=32), return_node_embeddings=True)
    for a, f in zip(got, exact):
        assert np.isfinite(a).all() and a.tobytes() == f.tobytes()


# ---------------------------------------------------------------- (e) fallback paths, plumbing
def test_jobs_without_a_matrix_pipe_kernel_return_the_f32_modes_bytes():
    """a sparse molecule-shaped job (E < 8 N: the in-edge walk) and a job under dgn_mfma=32 (the fp32 pipe) have no single-product
    instance: the default kernels run, in the mode"""
    from tests.ref_pin import with_eigen
    w = weights.synth_dgn_weights(7)
    mol, hep = with_eigen(gp.synth_molhiv_batch(40, seed=5), 1), gp.synth_hep10k_batch(8, seed=5)
    for b, options, ran in ((mol, {}, "dgn_layer_fused"), (hep, {"dgn_mfma": 32}, "dgn_dense")):
        f16, n16, _ = run(w, b, "f16", options, **ROWS)
        f32, n32, _ = run(w, b, None, options, **ROWS)
        no_f16(n16)
        assert n16 == n32 and ran in n16, (n16, n32)
        for a, f in zip(f16, f32):
            assert a.tobytes() == f.tobytes()


def _err(e):
    return (e.lib.flowgnn_last_error(e._h) or b"").decode()


def _new(e, model, mode):
    return e.lib.flowgnn_set_model_numeric_mode(e._h, model, mode), _err(e)


def _model(e, d, mode):
    return e.lib.flowgnn_set_model_numeric_mode_dim(e._h, d, mode), _err(e)


def _dim(e, d, mode):
    return e.lib.flowgnn_set_numeric_mode_dim(e._h, d, mode), _err(e)


def test_refusals_in_both_orders_launch_nothing():
    """(*)"""
    b, w = gp.synth_hep10k_batch(4, seed=5), weights.synth_dgn_weights(7)
    e = Engine("DGN")
    try:
        e.set_weights(w)
        e.profile_enable(True)

        def refusals():
            # F16 sticks to the three old calls' UNSUPPORTED, and each text names the new call
            assert e.lib.flowgnn_set_numeric_mode(e._h, F16) == ERR_UNSUPPORTED and "flowgnn_set_model_numeric_mode(" in _err(e)
            for rc, text in (_dim(e, 100, F16), _model(e, 100, F16)):
                assert rc == ERR_UNSUPPORTED and "flowgnn_set_model_numeric_mode(" in text, (rc, text)
            assert _rc(lambda: e.set_numeric_mode("f16"))[0] == ERR_UNSUPPORTED
            for wrong in (0, 1, 2, 3, 4, 6, -1):  # a model that is not the engine's: both are named
                rc, text = _new(e, wrong, F16)
                assert rc == ERR_ARG and "FLOWGNN_MODEL_DGN" in text and str(wrong) in text, (wrong, rc, text)
            assert "FLOWGNN_MODEL_PNA" in _new(e, 4, F16)[1]
            for bad in (-1, 3, 16):
                assert _new(e, DGN, bad)[0] == ERR_ARG, bad
            for pooling in ("sum", "max"):
                assert _rc(lambda: e.set_pooling(pooling))[0] == ERR_UNSUPPORTED

        n = counts(e, refusals)  # ---- in f32 mode
        assert n == {}, n
        f32 = e.forward(b).copy()
        assert _new(e, DGN, F16)[0] == OK
        n = counts(e, refusals)  # ---- and with the mode on: it stays on
        assert n == {}, n
        n = counts(e, lambda: e.forward(b))
        f16_only(n, R.RESIDENT_SLOT, 1)
        f16 = e.results().copy()
        assert not np.array_equal(f16, f32)
        # the new call takes the plain call's modes too
        assert _new(e, DGN, Q)[0] == OK
        q = e.forward(b).copy()
        assert _new(e, DGN, F32)[0] == OK
        assert np.array_equal(e.forward(b), f32)
        e.set_numeric_mode("q6.10")
        assert np.array_equal(e.forward(b), q)
        # Q6_10 beside embeddings is refused on the new call as on the old ones; F16 beside them is not
        e.set_numeric_mode("f32")
        e.forward(b, return_embeddings=True)
        n = counts(e, lambda: None)
        rc, text = _new(e, DGN, Q)
        assert rc == ERR_UNSUPPORTED and text, (rc, text)
        assert e.lib.flowgnn_set_numeric_mode(e._h, Q) == ERR_UNSUPPORTED
        assert _new(e, DGN, F16)[0] == OK
        res = {}
        n = counts(e, lambda: res.update(got=e.forward(b, return_embeddings=True)))
        f16_only(n, R.RESIDENT_SLOT, 1)
        assert np.array_equal(res["got"][0], f16)
        e.set_numeric_mode("f32")  # the plain call always goes back
        assert np.array_equal(e.forward(b, return_embeddings=True)[0], f32)
    finally:
        e.close()


@pytest.mark.parametrize("model", ["GIN", "GIN-VN", "GCN", "GAT", "PNA"])
def test_on_every_other_engine_the_call_is_the_dim_form_at_the_engines_width(model):
    """(*) return code for return code, in every mode, at every width the engine can have; a wrong model is an argument error"""
    mid = _lib.MODEL_IDS[model]
    widths = {"GIN": (100, 300), "GCN": (100, 300), "PNA": (80,)}.get(model, (100,))
    for width in widths:
        a, b = Engine(model), Engine(model)
        try:
            if width == 300:
                for e in (a, b):
                    (e.set_emb_dim if model == "GIN" else e.set_model_emb_dim)(300)
            for mode in (F32, Q, F16, F32, F16, Q, 3, -1):
                got, want = _new(a, mid, mode)[0], _model(b, width, mode)[0]
                assert got == want, (model, width, mode, got, want)
                a.lib.flowgnn_set_numeric_mode(a._h, F32)
                b.lib.flowgnn_set_numeric_mode(b._h, F32)
            rc, text = _new(a, DGN, F16)
            assert rc == ERR_ARG and "FLOWGNN_MODEL_DGN" in text, (rc, text)
        finally:
            a.close()
            b.close()


def test_the_mode_survives_weights_batches_and_outputs():
    b, b2 = gp.synth_hep10k_batch(6, seed=5), gp.synth_hep10k_batch(4, seed=6)
    w, w2 = weights.synth_dgn_weights(7), weights.synth_dgn_weights(8)
    e = Engine("DGN")
    try:
        e.set_numeric_mode("f16", emb_dim=100)  # before the weights
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
        n = counts(e, lambda: res.update(got=e.forward(b, **ROWS)))
        f16_only(n, R.RESIDENT_SLOT, 1)
        logits, emb, rows = res["got"]
        assert np.array_equal(logits, first)
        rne = R.forward(b, w, "rne")
        off = b.node_offsets()
        pooled = np.add.reduceat(f64(rows), off[:-1], axis=0) / f64(b.nums_of_nodes)[:, None]
        assert np.abs(f64(emb) - pooled).max() <= 1e-5 * (1 + np.abs(pooled).max())  # the embeddings are the mean of the rows
        assert R.rule(f64(rows), rne, R.TOL[("synth", "rows")]) <= 1.0  # ... and the rows are the mode's
        # flowgnn_get_h: h_4 of the f16 per-layer path (its own tiles: toleranced against the bin-packed resident rows)
        n = counts(e, lambda: res.update(h=e.final_h()))
        assert n.get(R.LAYER_SLOT) == 4 and "dgn_layer_fused" not in n, n
        assert np.allclose(f64(res["h"]).reshape(f64(rows).shape), f64(rows), rtol=1e-5, atol=1e-5 * rne.scale)
        assert e.exact_reruns() == 0
    finally:
        e.close()


def test_device_batch_form():
    pytest.importorskip("torch")
    from tests.test_device_batch_gpu import device_args
    b, w = gp.synth_hep10k_batch(6, seed=5), weights.synth_dgn_weights(7)
    e = make(w)
    try:
        want = e.forward(b).copy()
        for layout in ("pyg", "reference"):
            args, kw = device_args(b, layout, "DGN")
            res = {}
            n = counts(e, lambda: res.update(got=e.forward_device(*args, **kw)))
            f16_only(n, R.RESIDENT_SLOT, 1)
            got = res["got"]
            got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
            assert np.array_equal(got.reshape(want.shape), want), layout
    finally:
        e.close()


def test_group_form():
    b, w = gp.synth_hep10k_batch(9, seed=5), weights.synth_dgn_weights(7)
    g = EngineGroup("DGN", [0, 0])
    try:
        g.set_weights(w)
        f32 = g.forward(b).copy()
        assert _rc(lambda: g.set_numeric_mode("f16"))[0] == ERR_UNSUPPORTED
        assert g.lib.flowgnn_group_set_numeric_mode_dim(g._h, 100, F16) == ERR_UNSUPPORTED
        assert g.lib.flowgnn_group_set_model_numeric_mode_dim(g._h, 100, F16) == ERR_UNSUPPORTED
        assert g.lib.flowgnn_group_set_model_numeric_mode(g._h, _lib.MODEL_IDS["PNA"], F16) == ERR_ARG
        g.set_numeric_mode("f16", emb_dim=100)
        members = [C.c_void_p(g.lib.flowgnn_group_engine(g._h, i)) for i in range(2)]
        for h in members:
            assert g.lib.flowgnn_profile_enable(h, 1) == OK
        got = g.forward(b).copy()
        ref = R.forward(b, w, "none")
        assert R.rule(f64(got), ref, R.TOL[("synth", "logits")]) <= 1.0 and not np.array_equal(got, f32)
        for h in members:
            n = C.c_int()
            names, ms, cnt = (C.c_char_p * 32)(), (C.c_double * 32)(), (C.c_longlong * 32)()
            assert g.lib.flowgnn_profile_read(h, C.byref(n), names, ms, cnt) == OK
            ran = {names[i].decode(): int(cnt[i]) for i in range(n.value) if cnt[i] > 0}
            assert ran.get(R.RESIDENT_SLOT, 0) >= 1 and "dgn_resident" not in ran, ran
        g.set_numeric_mode("f32")
        assert np.array_equal(g.forward(b), f32)
    finally:
        g.close()


def test_one_hipgraph_replay_equals_the_eager_bytes(monkeypatch):
    b, w = gp.synth_hep10k_batch(6, seed=5), weights.synth_dgn_weights(7)
    monkeypatch.setenv("FLOWGNN_HIPGRAPH", "0")
    eager, _, _ = run(w, b, "f16", {})
    monkeypatch.setenv("FLOWGNN_HIPGRAPH", "1")
    e = Engine("DGN", device=0)  # (no profiler: its events keep the engine from capturing)
    try:
        e.set_weights(w)
        e.set_batch(b)
        e.run()
        e.run()
        f32 = e.results().copy()
        e.set_numeric_mode("f16", emb_dim=100)  # the recorded launch sequence is dropped on the switch
        outs = []
        for _ in range(3):  # plain, captured + launched, replay
            e.run()
            outs.append(e.results().copy())
        for o in outs:
            assert o.tobytes() == eager[0].tobytes()
        assert not np.array_equal(outs[0], f32)
        assert e.graph_replays() >= 2 and e.exact_reruns() == 0
    finally:
        e.close()


def test_host_cli_runs_dgn_in_f16_mode(tmp_path):
    """`host DGN --numeric f16` on a written pack: the engine's bytes (as the eight decimals the host prints), not the f32 mode's"""
    b, w = gp.synth_hep10k_batch(5, seed=3), weights.synth_dgn_weights(7)
    gdir, wdir, edir = tmp_path / "graphs", tmp_path / "weights", tmp_path / "eig"
    gp.write_pack(b, str(gdir), eig_dir=str(edir))
    seen = gp.read_pack(str(gdir), eig_dir=str(edir))  # the eigenvectors as the text files carry them
    weights.SAVERS["DGN"](w, str(wdir))
    got = {}
    for mode in ("f16", "f32"):
        out = tmp_path / f"out_{mode}.txt"
        p = subprocess.run([HOST, "DGN", "--numeric", mode, "--graphs", str(gdir), "--weights", str(wdir), "--eig", str(edir), "--trials", "1",
                            "--out", str(out)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        got[mode] = [ln.split(":")[1].strip() for ln in open(out).read().strip().splitlines()]
    engine, n, _ = run(w, seen, "f16", {})
    f16_only(n, R.RESIDENT_SLOT, 1)
    assert got["f16"] == ["%.8f" % x for x in engine[0]]
    assert np.mean(np.array(got["f16"]) != np.array(got["f32"])) > 0.5


def test_speed_guard():
    """(*) in one process, on one batch of 2^14 hep10k-shaped graphs: the device-event median of dgn_resident_f16 is below that of
    dgn_resident (the condition is only "faster"; the measured ratio is DESIGN.md's)"""
    b = gp.synth_hep10k_batch(1 << 14, seed=3)
    e = Engine("DGN", device=0)
    try:
        e.set_weights(weights.synth_dgn_weights(7))
        e.set_batch(b)
        e.profile_enable(True)

        def median_ms(mode, slot, runs=7):
            e.set_numeric_mode(mode, emb_dim=100)
            e.run()
            e.results()
            ms = []
            for _ in range(runs):
                t0 = e.profile_read()[slot]["total_ms"]
                e.run()
                e.results()
                ms.append(e.profile_read()[slot]["total_ms"] - t0)
            return float(np.median(ms))

        best = {"f32": np.inf, "f16": np.inf}
        for _ in range(3):
            for mode, slot in (("f32", "dgn_resident"), ("f16", R.RESIDENT_SLOT)):
                best[mode] = min(best[mode], median_ms(mode, slot))
        print(f"dgn_resident {best['f32']:.3f} ms, dgn_resident_f16 {best['f16']:.3f} ms: ratio {best['f16'] / best['f32']:.3f}")
        assert best["f16"] < best["f32"], best
        assert e.exact_reruns() == 0
    finally:
        e.close()
