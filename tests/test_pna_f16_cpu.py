"""PNA's f16 numeric mode on the CPU (tests/pna_f16_ref.py): what the GPU test takes for granted.

1. The ladder: pna_f16_ref.TOL is the smallest rung at which the "rne" restatement alone lies at <= 0.5 of the rule, per accuracy input.
2. The probe's premises: dyadic weights, in-degrees whose reciprocal is a power of two, which fp32 sums are exact (per row), and that
   the probe tells "rne" apart from "none", "rtz" and each skipped aggregator by more than 100 x its bound on more than half of the
   values it compares.
3. The shape cases are what they claim.
4. The plan (flowgnn_amd/csrc/pna_plan.h) on every combination of its inputs that bear on the mode."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import f16_ref as F, pna_f16_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. the ladder
def test_ladder_is_the_issues():
    assert np.allclose(R.LADDER[:6], [1e-4, 2e-4, 5e-4, 1e-3, 2e-3, 5e-3], rtol=1e-12)


@pytest.mark.parametrize("wname,out", [("synth", "logits"), ("synth", "rows"), ("trained", "rows")])
def test_tol_is_the_smallest_rung_at_which_the_restatement_lies_at_half(wname, out):
    w = R.accuracy_weights(wname)
    ratios = []
    for seed in R.ACCURACY_SEEDS:
        b = R.accuracy_batch(seed)
        ref, rne, rtz = R.forward(b, w, "none"), R.forward(b, w, "rne"), R.forward(b, w, "rtz")
        x = rne.logits if out == "logits" else rne.rows
        ratios.append(R.rule(x, ref, 1e-4))
        print(f"{wname} {out} seed {seed}: rne at {ratios[-1]:.3f} of the 1e-4 rule, rtz at {R.rule(rtz.logits if out == 'logits' else rtz.rows, ref, 1e-4):.3f}")
        if wname == "trained":  # the head saturates: the same logit in every mode, so this set tests rows only
            assert np.ptp(ref.logits) < 1e-9 and np.array_equal(np.round(rne.logits, 9), np.round(ref.logits, 9))
    assert R.TOL[(wname, out)] == R.rung(max(ratios)), (ratios, R.rung(max(ratios)))
    assert max(ratios) * 1e-4 / R.TOL[(wname, out)] <= 0.5


# ---------------------------------------------------------------- 2. the probe's premises
@pytest.fixture(scope="module")
def probe():
    b, w = R.probe_batch(), R.probe_weights()
    return b, w, R.probe_check(b, w)


def test_probe_weights_are_dyadic_with_few_bits_and_degrees_are_powers_of_two(probe):
    b, w, _ = probe
    cw = np.asarray(w["node_conv_weights"], np.float64)
    for l in range(4):
        s = F.pow2_scale(cw[l])
        ws = cw[l] * s
        assert np.array_equal(ws * 4, np.rint(ws * 4)) and np.abs(ws).max() < 2  # two bits behind the point after the layer's scale
    for k in ("node_embedding_weight", "node_conv_bias"):
        x = np.asarray(w[k], np.float64)
        assert np.array_equal(x * 2 ** 13, np.rint(x * 2 ** 13))
    indeg, outdeg = R.probe_classes(b)
    assert set(np.unique(indeg)) == {0, 1, 2, 4, 32}
    assert ((indeg == 0) | (outdeg == 0)).all() and (indeg[outdeg > 0] == 0).all()  # bipartite: a sink's t is 0 and its scale 1
    assert b.num_graphs <= 64


def test_probe_sums_are_exact_in_fp32_on_the_rows_it_claims(probe):
    b, w, (res, exact, worst, margin) = probe
    indeg, outdeg = R.probe_classes(b)
    print(f"worst log2(sum |terms| / quantum) = {worst:.2f}; largest acc of a closed update = {margin:.1f}; {exact.sum()} of {len(exact)} rows exact")
    assert worst <= 24.0
    assert margin < -100.0  # a closed update stays closed whatever fp32 makes of its irrational scalers
    assert np.array_equal(exact, (indeg <= 2))  # every row but the sinks of in-degree 4 and 32, whose std is no perfect square
    assert exact.sum() > 0.9 * len(exact)
    rows32 = res.rows[exact].astype(np.float32).astype(np.float64)
    assert np.array_equal(rows32, res.rows[exact])  # ... and the results are fp32 values
    ref = R.forward(b, w, "rne")  # the bookkeeping forward IS numpy_ref's through the dense hook
    assert np.array_equal(ref.hs, res.hs) and np.array_equal(ref.logits, res.logits)


@pytest.mark.parametrize("v", R.VARIANTS, ids=[R.variant_name(v) for v in R.VARIANTS])
def test_probe_separates_the_mode_from(v, probe):
    b, w, (res, _, _, _) = probe
    other = R.forward(b, w, *v)
    for name, mask in R.compared(b, v).items():
        ok, frac = R.separated(other.rows, res.rows, res.rows, mask)
        print(f"{R.variant_name(v)}: {name}: {frac:.3f} of {int(mask.sum())} values apart by more than {R.SEPARATION:g} x the bound")
        assert ok, (name, frac)


# ---------------------------------------------------------------- 3. the shape cases
def test_shape_cases_are_what_they_claim():
    cases = R.shape_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for want in ("one-node-first-and-last", "edgeless-four-nodes", "tile-of-15-rows", "tile-of-16-rows", "tile-of-17-rows", "tile-of-255-rows",
                 "tile-of-256-rows", "graph-across-the-wave-halves", "hub-of-16-in-edges", "hub-of-17-in-edges", "hub-of-40-in-edges",
                 "graph-of-300-nodes", "graphs-of-70-nodes", "33-graphs-binpack-1", "33-graphs-binpack-0", "tile-build-off"):
        assert want in names, want
    for c in cases:
        b = c.batch
        assert b.num_graphs <= 64 and bool(c.claim(b)), c.name
        ge = b.edge_list
        n_of_edge = np.repeat(b.nums_of_nodes, b.nums_of_edges)
        assert ((ge >= 0) & (ge < n_of_edge[:, None])).all(), c.name
        if c.slot == R.RESIDENT_SLOT:  # every graph fits a tile
            assert b.nums_of_nodes.max() <= R.TILE_ROWS and b.nums_of_edges.max() <= R.TILE_EDGES, c.name


# ---------------------------------------------------------------- 4. the plan
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pna_f16_plan") / "pna_f16_plan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "flowgnn_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "pna_f16_plan_shim.cpp")])
    lib = C.CDLL(so)
    lib.pna_f16_plan.restype = C.c_uint32
    lib.pna_f16_plan.argtypes = [C.c_uint32, C.c_double]
    return lib


def test_plan_runs_the_f16_kernels_exactly_where_it_should_and_on_the_path_it_had(plan_lib):
    n = 0
    for bits in itertools.product((0, 1), repeat=10):
        f16, qmode, exact, split, resident, fused, tiles, keep_h, emb, node_emb = bits
        word = sum(v << i for i, v in enumerate(bits))
        for fill in (0.0, 0.39, 0.4, 1.0):
            p = plan_lib.pna_f16_plan(word, fill)
            assert (p & 1) == int(f16 and not qmode and not exact and split), (bits, fill)
            off = plan_lib.pna_f16_plan(word & ~1, fill)
            assert (off & 1) == 0 and (p >> 1) == (off >> 1), (bits, fill)  # the path is the one the same input takes with f16 off
            if p & 1:  # a split kernel runs: resident, fused layers or the split dense kernel
                path, fused_layers, split_dense = (p >> 1) & 3, (p >> 8) & 1, (p >> 9) & 1
                assert path == 1 or fused_layers or split_dense, (bits, fill)
            n += 1
    assert n == 4096
