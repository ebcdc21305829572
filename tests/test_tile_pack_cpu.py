"""The graph-tile planner of flowgnn_set_batch (flowgnn_amd/csrc/tile_pack.cpp) on the CPU: plain C++, built here with g++ and called
through ctypes (tests/tile_pack_shim.cpp).

tests/golden/tile_plans.npz holds the tile lists the engine uploaded BEFORE the planner was split out of engine.hip (recorded on an
MI355X from commit 65d2c62, the half-tile lists from its `make DEV=1` build with gin_pingpong = 1): the planner must reproduce every
array exactly, whatever the thread count.  Arrays of batches of more than 1 025 graphs are stored as length + SHA-256.
The invariants below hold for any plan and are checked on the same inputs and on random count arrays."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import graphpack as gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flowgnn_amd", "csrc")
ARRAYS = ["row_start", "graph_start", "bp_list", "bp_lrow", "bp_graph", "bp_row", "sub", "big_row", "big_graph"]
LIMITS = {"GIN": (256, 1280), "GAT": (256, 1280), "GCN": (192, 960), "PNA": (256, 4608), "DGN": (128, 2560)}
BINPACK = {"GIN", "GCN", "PNA", "DGN"}  # the models whose resident kernels read bin-packed tile lists
INPUTS = {
    "molhiv4113": lambda: gp.synth_molhiv_batch(4113, seed=1234),
    "molhiv300": lambda: gp.synth_molhiv_batch(300, seed=1),
    "molhiv1025": lambda: gp.synth_molhiv_batch(1025, seed=5),
    "hep2500": lambda: gp.synth_hep10k_batch(2500, seed=3, with_eigen=False),
    "molhiv24000": lambda: gp.synth_molhiv_batch(24000, seed=7),
    "molhiv1": lambda: gp.synth_molhiv_batch(1, seed=1),
    "molhiv2": lambda: gp.synth_molhiv_batch(2, seed=1),
}
_counts = {}


def counts(name):
    if name not in _counts:
        b = INPUTS[name]()
        _counts[name] = (np.ascontiguousarray(b.nums_of_nodes, np.int32), np.ascontiguousarray(b.nums_of_edges, np.int32))
    return _counts[name]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tile_pack") / "libtile_pack_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so, os.path.join(ROOT, "tests", "tile_pack_shim.cpp"),
                           os.path.join(CSRC, "tile_pack.cpp"), os.path.join(CSRC, "h2d_pack.cpp"), "-lpthread"])
    lib = C.CDLL(so)
    pi = C.POINTER(C.c_int)
    lib.tp_plan.argtypes = [C.c_int] * 8 + [pi, pi]
    lib.tp_plan.restype = C.c_void_p
    lib.tp_len.argtypes = [C.c_void_p, C.c_int]
    lib.tp_data.argtypes = [C.c_void_p, C.c_int]
    lib.tp_data.restype = pi
    for f in (lib.tp_ok, lib.tp_sub_ok, lib.tp_fill, lib.tp_sub_fill, lib.tp_free):
        f.argtypes = [C.c_void_p]
    lib.tp_fill.restype = lib.tp_sub_fill.restype = lib.tp_greedy_fill.restype = C.c_double
    lib.tp_free.restype = None
    lib.tp_greedy_fill.argtypes = [C.c_int, C.c_int, C.c_int, pi, pi]
    return lib


def plan(lib, nn, ne, rows, edges, sub_rows=0, sub_edges=0, balance=1, binpack=1, threads=1):
    pi = C.POINTER(C.c_int)
    p = lib.tp_plan(rows, edges, sub_rows, sub_edges, balance, binpack, threads, len(nn), nn.ctypes.data_as(pi), ne.ctypes.data_as(pi))
    try:
        out = {k: np.ctypeslib.as_array(lib.tp_data(p, i), (lib.tp_len(p, i),)).copy() if lib.tp_len(p, i) else np.zeros(0, np.int32)
               for i, k in enumerate(ARRAYS)}
        out.update(ok=bool(lib.tp_ok(p)), sub_ok=bool(lib.tp_sub_ok(p)), fill=lib.tp_fill(p), sub_fill=lib.tp_sub_fill(p))
        return out
    finally:
        lib.tp_free(p)


def greedy_fill(lib, nn, ne, rows, edges):
    pi = C.POINTER(C.c_int)
    return lib.tp_greedy_fill(rows, edges, len(nn), nn.ctypes.data_as(pi), ne.ctypes.data_as(pi))


def py_greedy_fill(nn, ne, rows, edges):
    tiles, cr, ce, total, before_last = 1, 0, 0, 0, 0
    for n, m in zip(nn.tolist(), ne.tolist()):
        if n > rows or m > edges:
            return 0.0
        if cr + n > rows or ce + m > edges:
            tiles, before_last, cr, ce = tiles + 1, total, 0, 0
        cr, ce, total = cr + n, ce + m, total + n
    return before_last / ((tiles - 1) * rows) if tiles > 1 else 1.0


@pytest.mark.parametrize("threads", [1, 16])
def test_plans_equal_the_parents(lib, threads):
    z = np.load(os.path.join(ROOT, "tests", "golden", "tile_plans.npz"))
    cases = json.loads(str(z["cases"]))
    assert len(cases) >= 40
    for c in cases:
        nn, ne = counts(c["input"])
        assert hashlib.sha256(nn.tobytes() + ne.tobytes()).hexdigest() == c["input_sha"], (c["name"], "the generator's counts changed")
        got = plan(lib, nn, ne, c["rows"], c["edges"], c["sub_rows"], c["sub_edges"], c["balance"], c["binpack_asked"], threads)
        assert got["ok"] == bool(c["ok"]) and got["sub_ok"] == bool(c["sub_ok"]), c["name"]
        assert got["fill"] == c["fill"] and got["sub_fill"] == c["sub_fill"], (c["name"], got["fill"], c["fill"], got["sub_fill"], c["sub_fill"])
        for k in ARRAYS:
            want = c["arrays"].get(k)
            if want is None:
                assert got[k].size == 0, (c["name"], k, "built, the parent built none")
            elif want["stored"]:
                assert np.array_equal(got[k], z[f"{c['name']}/{k}"]), (c["name"], k)
            else:
                assert got[k].size == want["len"], (c["name"], k, got[k].size, want["len"])
                assert hashlib.sha256(got[k].astype(np.int32).tobytes()).hexdigest() == want["sha256"], (c["name"], k)


def check_invariants(lib, nn, ne, rows, edges, sub_rows, sub_edges, balance, binpack, what):
    G = len(nn)
    noff = np.concatenate([[0], np.cumsum(nn)]).astype(np.int64)
    eoff = np.concatenate([[0], np.cumsum(ne)]).astype(np.int64)
    p = plan(lib, nn, ne, rows, edges, sub_rows, sub_edges, balance, binpack, threads=3)
    fill = greedy_fill(lib, nn, ne, rows, edges)
    assert fill == p["fill"] == py_greedy_fill(nn, ne, rows, edges), what
    fits = bool((nn <= rows).all() and (ne <= edges).all())
    assert p["ok"] == fits, what
    if not fits:
        assert all(p[k].size == 0 for k in ARRAYS) and p["fill"] == 0.0 and not p["sub_ok"], what
        return
    # tiles in batch order: consecutive graph ranges that cover 0 .. G once, rows the running sums, within the limits
    gs, rs = p["graph_start"], p["row_start"]
    assert gs[0] == 0 and gs[-1] == G and (np.diff(gs) > 0).all(), what
    assert np.array_equal(rs, noff[gs]), what
    assert (np.diff(rs) <= rows).all() and (np.diff(eoff[gs]) <= edges).all(), what
    if not balance:
        assert p["fill"] == (rs[-2] / ((len(rs) - 2) * rows) if len(rs) > 2 else 1.0), what
    # bin-packed tile lists
    assert (p["bp_list"].size > 0) == bool(binpack and G > 1), what
    if p["bp_list"].size:
        bl, bg = p["bp_list"], p["bp_graph"]
        assert np.array_equal(np.sort(bl), np.arange(G)), what
        assert bg[0] == 0 and bg[-1] == G and (np.diff(bg) > 0).all(), what
        t_rows = np.add.reduceat(nn[bl].astype(np.int64), bg[:-1])
        t_edges = np.add.reduceat(ne[bl].astype(np.int64), bg[:-1])
        assert (t_rows <= rows).all() and (t_edges <= edges).all(), what
        assert np.array_equal(p["bp_row"], np.concatenate([[0], np.cumsum(t_rows)])), what
        run = np.cumsum(nn[bl].astype(np.int64)) - nn[bl]  # rows before this list position ...
        assert np.array_equal(p["bp_lrow"], run - np.repeat(run[bg[:-1]], np.diff(bg))), what  # ... minus those before its tile
    # half-tile runs and the graphs beyond the half-tile limits
    assert p["sub_ok"] == (sub_rows > 0), what
    if p["sub_ok"]:
        sub, br, bgr = p["sub"].reshape(-1, 4), p["big_row"].reshape(-1, 2), p["big_graph"].reshape(-1, 2)
        seen = np.zeros(G, np.int64)
        for row, n_rows, g0, g1 in sub:
            seen[g0:g1] += 1
            assert row == noff[g0] and n_rows == noff[g1] - noff[g0] and n_rows <= sub_rows and eoff[g1] - eoff[g0] <= sub_edges, what
        for (r0, r1), (g0, g1) in zip(br, bgr):
            seen[g0] += 1
            assert g1 == g0 + 1 and r0 == noff[g0] and r1 == noff[g1] and (nn[g0] > sub_rows or ne[g0] > sub_edges), what
        assert (seen == 1).all(), what
        assert p["sub_fill"] == (noff[-1] - int(nn[bgr[:, 0]].sum())) / (len(sub) * sub_rows) if len(sub) else p["sub_fill"] == 0.0, what


def test_plan_invariants_on_the_fixture_inputs(lib):
    for name in INPUTS:
        nn, ne = counts(name)
        for model, (rows, edges) in LIMITS.items():
            if name == "molhiv24000" and model != "GIN":
                continue
            for balance, binpack, sub in ((1, 1, 0), (0, 1, 0), (1, 0, 0), (1, 0, 1)):
                check_invariants(lib, nn, ne, rows, edges, rows // 2 * sub, edges // 2 * sub, balance, binpack and model in BINPACK,
                                 (name, model, balance, binpack, sub))


def test_plan_invariants_on_random_counts(lib):
    rng = np.random.default_rng(2024)
    for i in range(20):
        rows, edges = list(LIMITS.values())[i % len(LIMITS)]
        G = int(rng.integers(1, 6000))
        top = int(rng.choice([rows // 8, rows // 2, rows, rows + 1]))  # (rows + 1: some batches do not fit)
        nn = rng.integers(1, top + 1, G).astype(np.int32)
        ne = np.minimum(nn.astype(np.int64) * rng.integers(0, 12, G), edges + (i % 7 == 0)).astype(np.int32)
        check_invariants(lib, nn, ne, rows, edges, rows // 2 * (i % 2), edges // 2 * (i % 2), i % 3 != 0, i % 4 != 0, ("random", i))
