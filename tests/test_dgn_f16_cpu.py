"""DGN's f16 numeric mode on the CPU (tests/dgn_f16_ref.py): what the GPU test takes for granted.

1. The ladder: dgn_f16_ref.TOL is the smallest rung at which the "rne" restatement alone lies at <= 0.5 of the rule, per accuracy input.
2. The probe's premises: dyadic weights and eigenvectors, out-degrees that are powers of two, encoder values with bits beyond f16's
   eleven, that EVERY fp32 sum of every row is exact in any order (the bookkeeping of tests/f16_ref._Exact, per row), and that the
   probe tells "rne" apart from "none", "rtz" and each skipped operand by more than 100 x its bound on more than half of the values
   it compares.
3. The shape cases are what they claim.
4. The plan (flowgnn_amd/csrc/dgn_plan.h) on every combination of its inputs: single_product is the stated expression and nothing
   else moves with f16.
5. The ABI where it needs no device: declarations, null handles, the Python and CLI routes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import f16_ref as F, dgn_f16_ref as R, numpy_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. the ladder
def test_ladder_is_the_issues():
    assert np.allclose(R.LADDER[:6], [1e-4, 2e-4, 5e-4, 1e-3, 2e-3, 5e-3], rtol=1e-12)
    assert R.ACCURACY_SEEDS == (3, 11)


def test_the_unrounded_restatement_is_the_plain_model():
    b, w = R.accuracy_batch(3), R.accuracy_weights("synth")
    out, hs = N.dgn_forward(b, w, return_h=True)
    ref = R.forward(b, w, "none")
    assert np.abs(ref.logits - out).max() <= 1e-12 * (1 + np.abs(out).max()) and np.abs(ref.hs - hs).max() <= 1e-12 * ref.scale


@pytest.mark.parametrize("wname,out", R.ACCURACY)
def test_tol_is_the_smallest_rung_at_which_the_restatement_lies_at_half(wname, out):
    assert os.path.exists(os.path.join(ROOT, "tests", "golden", "ref_weights_dgn.npz"))  # the trained DGN set
    w = R.accuracy_weights(wname)
    ratios = []
    for seed in R.ACCURACY_SEEDS:
        b = R.accuracy_batch(seed)
        assert b.num_graphs == 24
        ref, rne, rtz = R.forward(b, w, "none"), R.forward(b, w, "rne"), R.forward(b, w, "rtz")
        pick = lambda r: r.logits if out == "logits" else r.rows
        ratios.append(R.rule(pick(rne), ref, 1e-4))
        print(f"{wname} {out} seed {seed}: rne at {ratios[-1]:.3f} of the 1e-4 rule, rtz at {R.rule(pick(rtz), ref, 1e-4):.3f} (scale {ref.scale:.3g})")
    assert R.TOL[(wname, out)] == R.rung(max(ratios)), (ratios, R.rung(max(ratios)))
    assert max(ratios) * 1e-4 / R.TOL[(wname, out)] <= 0.5


# ---------------------------------------------------------------- 2. the probe's premises
@pytest.fixture(scope="module")
def probe():
    (b, roles), w = R.probe_batch(), R.probe_weights()
    return b, roles, w, R.probe_check(b, w)


def test_probe_is_built_as_it_says(probe):
    b, roles, w, _ = probe
    lw = np.asarray(w[R.K_W], np.float64)
    for l in range(4):
        s = F.pow2_scale(lw[l])
        ws = lw[l] * s
        assert np.array_equal(ws * 4, np.rint(ws * 4)) and np.abs(ws).max() < 2  # two bits behind the point after the layer's scale
    lb = np.asarray(w[R.K_B], np.float64)
    assert (lb <= 0).all() and np.array_equal(lb * 2 ** 12, np.rint(lb * 2 ** 12))  # non-positive and dyadic
    T = np.asarray(w[R.K_EMB], np.float64)
    assert np.array_equal(T * 2 ** 12, np.rint(T * 2 ** 12))
    h0 = R.forward(b, w, "none").hs[0]
    r16, z16 = F.rounder("rne")(h0), F.rounder("rtz")(h0)
    differ = (r16 != h0) & (z16 != h0) & (r16 != z16)  # "rne", "rtz" and "none" are three values
    print(f"encoder values on which the three roundings differ: {differ.mean():.3f}")
    assert differ.mean() > 0.5 and (r16 != h0).mean() > 0.8  # a majority
    eig = np.asarray(b.node_eigen, np.float64)[:, 1]
    assert np.array_equal(eig * 2 ** 24, np.rint(eig * 2 ** 24)) and np.abs(eig).max() <= R.P_EIG
    indeg, outdeg = R.probe_classes(b)
    src, sink, drain = roles == 0, roles == 1, roles == 2
    assert (indeg[src] == 0).all() and (outdeg[src] >= 1).all()
    assert sorted(set(indeg[sink])) == [1, 2, 4, 32, 64] and set(outdeg[sink]) == {1, 2, 4}  # every sink feeds a drain: a1 != 0
    assert (outdeg[drain] == 0).all() and (eig[sink] == 0).all() and (eig[drain] == 0).all()
    # a sink of in-degree 64 reads sources of more than one 32-source block of its tile (one graph per tile: the row in the tile is the node's)
    ge, off = b.global_edges(), b.node_offsets()
    for v in np.nonzero(sink & (indeg == 64))[0]:
        rows = ge[ge[:, 1] == v, 0] - off[np.searchsorted(off, v, side="right") - 1]
        assert len(set(rows // 32)) >= 2
    assert (b.nums_of_nodes == R.N_PER).all() and R.N_PER / R.TILE_ROWS >= 0.4 and 2 * R.N_PER > R.TILE_ROWS


def test_probe_sums_are_exact_in_fp32_on_every_row(probe):
    b, roles, w, (res, worst) = probe
    print(f"worst log2(sum |terms| / quantum) per role: sources {worst[roles == 0].max():.2f}, sinks {worst[roles == 1].max():.2f}, "
          f"drains {worst[roles == 2].max():.2f}; by sum: {R.probe_check.kinds}")
    assert (worst <= 24.0).all()  # every row is proven: the GPU test holds all of h_4 to the restatement bit for bit
    assert np.array_equal(res.rows.astype(np.float32).astype(np.float64), res.rows)  # ... and the results are fp32 values
    assert np.array_equal(res.hs[4][roles != 1], res.hs[0][roles != 1])  # sources and drains keep h_0
    assert (res.hs[4][roles == 1] != res.hs[0][roles == 1]).mean() > 0.5  # ... the sinks do not
    assert np.abs(res.hs).max() < 6.0e4
    ref = R.forward(b, w, "rne")
    assert np.array_equal(ref.hs, res.hs) and np.array_equal(ref.logits, res.logits)


@pytest.mark.parametrize("v", R.VARIANTS, ids=[R.variant_name(v) for v in R.VARIANTS])
def test_probe_separates_the_mode_from(v, probe):
    b, roles, w, (res, _) = probe
    other = R.forward(b, w, *v)
    mask = R.compared(b, roles, v)
    ok, frac = R.separated(other.rows, res.rows, res.rows, mask)
    print(f"{R.variant_name(v)}: {frac:.3f} of {int(mask.sum())} values apart by more than {R.SEPARATION:g} x the bound")
    assert ok, frac


# ---------------------------------------------------------------- 3. the shape cases
def test_shape_cases_are_what_they_claim():
    cases = R.shape_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for want in ("one-node-without-edges", "graph-of-31-nodes", "graph-of-32-nodes", "graph-of-33-nodes", "graph-of-128-nodes",
                 "tile-of-100-tiny-graphs", "rows-without-in-edges", "rows-whose-weights-are-all-zero", "duplicate-edges-x2",
                 "duplicate-edges-x3", "six-graphs-binpack-1", "six-graphs-binpack-0"):
        assert want in names, want
    for c in cases:
        b = c.batch
        assert bool(c.claim(b)), c.name
        n_of_edge = np.repeat(b.nums_of_nodes, b.nums_of_edges)
        assert ((b.edge_list >= 0) & (b.edge_list < n_of_edge[:, None])).all(), c.name
        assert b.nums_of_nodes.max() <= R.TILE_ROWS and b.nums_of_edges.max() <= R.TILE_EDGES, c.name  # every graph fits a tile
        assert c.options["dgn_mfma_agg"] == 1 and c.options["dgn_resident"] == 2


# ---------------------------------------------------------------- 4. the plan
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dgn_f16_plan") / "dgn_f16_plan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "flowgnn_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "dgn_f16_plan_shim.cpp")])
    lib = C.CDLL(so)
    p32, pi, pd = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lib.dgn_f16_plan_many.restype = None
    lib.dgn_f16_plan_many.argtypes = [C.c_int, p32, pi, pi, pi, pd, p32]
    lib.dgn_f16_wants_packed.restype = C.c_int
    lib.dgn_f16_wants_packed.argtypes = [C.c_uint32, C.c_int]
    return lib


NBITS = 17  # tests/dgn_f16_plan_shim.cpp: f16, qmode, exact, split, fused, tiles, keep_h, emb, node_emb, ... eigen
FILLS = (0.0, 0.39, 0.4, 1.0)


def _plans(lib, word, mfma, res, dense, fill):
    n = len(word)
    out = np.empty(n, np.uint32)
    a = lambda x, t: np.ascontiguousarray(x, t)
    word, mfma, res, dense, fill = a(word, np.uint32), a(mfma, np.int32), a(res, np.int32), a(dense, np.int32), a(fill, np.float64)
    p32, pi, pd = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lib.dgn_f16_plan_many(n, word.ctypes.data_as(p32), mfma.ctypes.data_as(pi), res.ctypes.data_as(pi), dense.ctypes.data_as(pi),
                          fill.ctypes.data_as(pd), out.ctypes.data_as(p32))
    return out


def test_plan_runs_the_f16_kernels_exactly_where_it_should_and_on_the_path_it_had(plan_lib):
    word = np.arange(1 << NBITS, dtype=np.uint32)
    total = 0
    for mfma in (-1, 0, 1):
        for res in (0, 1, 2):
            for dense in (0, 1):
                for fill in FILLS:
                    k = lambda x: np.full(len(word), x)
                    p = _plans(plan_lib, word, k(mfma), k(res), k(dense), k(fill))
                    off = _plans(plan_lib, word & ~np.uint32(1), k(mfma), k(res), k(dense), k(fill))
                    f16, qmode, exact, split = (word & 1).astype(bool), (word >> 1 & 1).astype(bool), (word >> 2 & 1).astype(bool), (word >> 3 & 1).astype(bool)
                    path, fused_layers, mfma_aggregation = (p >> 1) & 3, (p >> 7 & 1).astype(bool), (p >> 8 & 1).astype(bool)
                    want = f16 & ((path == 1) | (fused_layers & mfma_aggregation))  # DgnPath::Resident is 1
                    assert np.array_equal((p & 1).astype(bool), want)
                    assert not (p & 1)[qmode | exact | ~split].any()  # behind qmode's early return; off under exact and !split
                    assert not (off & 1).any() and np.array_equal(p >> 1, off >> 1)  # nothing else moves with f16
                    total += len(word)
                    if mfma == 1 and res == 2 and fill == 1.0:
                        assert (p & 1).any() and ((p & 1).astype(bool) & (path == 1)).any() and ((p & 1).astype(bool) & (path == 2)).any()
    assert total == (1 << NBITS) * 3 * 3 * 2 * len(FILLS)
    for bits in range(16):  # dgn_wants_packed_tile_lists, on the four bits it reads (f16, qmode, fused, binpack)
        w = (bits & 1) | (bits >> 1 & 1) << 1 | (bits >> 2 & 1) << 4 | (bits >> 3 & 1) << 11
        for res in (0, 1, 2):
            assert plan_lib.dgn_f16_wants_packed(w, res) == plan_lib.dgn_f16_wants_packed(w & ~1, res)


def test_the_resident_plan_shim_never_sets_the_field():
    src = open(os.path.join(ROOT, "tests", "resident_plan_shim.cpp")).read()
    assert "f16" not in src


# ---------------------------------------------------------------- 5. the ABI without a device
def test_header_declares_the_call_that_names_the_model():
    h = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    assert re.search(r"int\s+flowgnn_set_model_numeric_mode\(flowgnn_engine\*\s*e,\s*int\s+model_id,\s*int\s+mode\);", h)
    assert re.search(r"int\s+flowgnn_group_set_model_numeric_mode\(flowgnn_group\*\s*g,\s*int\s+model_id,\s*int\s+mode\);", h)
    assert h.index("int flowgnn_set_model_numeric_mode_dim(flowgnn_engine") < h.index("int flowgnn_set_model_numeric_mode(flowgnn_engine")
    assert "DGN is the one model left without" not in h


def test_null_handles_are_argument_errors_and_the_bindings_declare_the_calls():
    from flowgnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the library is not built")
    lib = _lib.load()
    for model in range(6):
        for mode in (0, 1, 2):
            assert lib.flowgnn_set_model_numeric_mode(None, model, mode) == 1
            assert lib.flowgnn_group_set_model_numeric_mode(None, model, mode) == 1
    assert lib.flowgnn_set_model_numeric_mode.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert lib.flowgnn_group_set_model_numeric_mode.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert lib.flowgnn_set_model_numeric_mode.restype == C.c_int and lib.flowgnn_group_set_model_numeric_mode.restype == C.c_int


def test_engine_source_keeps_the_three_old_refusals_and_names_the_new_call():
    src = open(os.path.join(ROOT, "flowgnn_amd", "csrc", "engine_config.hip")).read()
    # on a DGN engine only the route of the call that names the model reaches f16 ...
    assert re.search(r"case FLOWGNN_MODEL_DGN: return route == ModeRoute::ModelNumericMode;", src)
    # ... and every other route is refused, FLOWGNN_ERR_UNSUPPORTED, with a text that names that call
    m = re.search(r"if \(mode == FLOWGNN_NUMERIC_F16 && !route_reaches_f16\(e, route\)\)\n\s*return refuse\(e, FLOWGNN_ERR_UNSUPPORTED,\s*e->model_id == FLOWGNN_MODEL_DGN \?(.*?)\n\s*: e->model_id", src, re.S)
    assert m and "flowgnn_set_model_numeric_mode(e, FLOWGNN_MODEL_DGN, FLOWGNN_NUMERIC_F16)" in m.group(1)
    body = src[src.index("int flowgnn_set_model_numeric_mode(flowgnn_engine* e, int model_id, int mode)"):]
    body = body[:body.index("\n}\n")]
    assert "model_id != e->model_id" in body and "FLOWGNN_ERR_ARG" in body and "return flowgnn_set_model_numeric_mode_dim(e, width, mode);" in body
    assert re.search(r"if \(model_id != e->model_id\)\s*return refuse\(e, FLOWGNN_ERR_ARG,", body)
    assert body.index("model_id != e->model_id") < body.index("ModeRoute::ModelNumericMode")
    # the three old calls never pass that route: its one call site is in the call that names the model
    assert len(re.findall(r"set_numeric_mode\(e, mode, ModeRoute::ModelNumericMode\)", src)) == 1 and "set_numeric_mode(e, mode, ModeRoute::ModelNumericMode)" in body
    assert len(re.findall(r"ModeRoute::ModelNumericMode\b", src)) == 2  # (the rule above and that call site)


def test_python_and_cli_route_dgn_to_the_new_call():
    py = open(os.path.join(ROOT, "flowgnn_amd", "engine.py")).read()
    assert re.search(r'elif self\.model == "DGN":.*?self\.lib\.flowgnn_set_model_numeric_mode\(self\._h, _lib\.MODEL_IDS\["DGN"\], code\)', py, re.S)
    assert re.search(r'elif self\.model == "DGN":.*?self\.lib\.flowgnn_group_set_model_numeric_mode\(self\._h, _lib\.MODEL_IDS\["DGN"\]', py, re.S)
    cli = open(os.path.join(ROOT, "flowgnn_amd", "csrc", "host_main.cpp")).read()
    assert "if (mid == FLOWGNN_MODEL_DGN && numeric == FLOWGNN_NUMERIC_F16) rc = flowgnn_group_set_model_numeric_mode(eng, FLOWGNN_MODEL_DGN, numeric);" in cli
