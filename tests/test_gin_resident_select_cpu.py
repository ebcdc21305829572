"""Which compiled instance of GIN's graph-resident kernel a launch_gin_resident call runs (flowgnn_amd/csrc/gin_resident_launch.h,
gin_resident_pick) on the CPU: plain C++, built here with g++ and called through ctypes (tests/gin_resident_select_shim.cpp).

Up to and including commit f5365e0 the choice was an if-chain of early returns inside launch_gin_resident, with the two refusals as separate conditions
in front of it.  `parent_pick` below transcribes that function (gin_split.hip lines 2375-2434 at f5365e0) statement by statement; the
header's function must agree with it on the full product of the inputs either of them reads."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flowgnn_amd", "csrc")
INSTANCES = ["default", "eps", "pool_mean", "pool_max", "pool_sum", "node_logits", "refused"]  # enum class GinResidentInstance, in order
REFUSAL_POOLING = ("launch_gin_resident: pooling 1 (sum) runs the folded instances only (head_u, out, no hout / emb / node_logits), pooling 2 (max) "
                   "the pooling instance only (emb)")
REFUSAL_EPS = "launch_gin_resident: a trained eps runs the folded mean-pooling instances only (head_u, out, no hout / emb / node_logits)"
FIELDS = ["hout", "out", "head_u", "emb", "node_logits", "self_scale", "tb", "pooling", "tstride", "prof"]
CASES = list(itertools.product(*([(0, 1)] * 7), (0, 1, 2), (1, 2), (0, 1)))


def parent_pick(hout, out, head_u, emb, node_logits, self_scale, tb, pooling, tstride, prof):
    """gin_split.hip at f5365e0, launch_gin_resident past `if (n_tiles <= 0) return 0;` -> (instance, fold, enc, refusal text or None).
    fold / enc of a refused call: as the header reports them, from the lines that compute them (2378, 2390)."""
    if emb:  # 2377: if (emb != nullptr) { head_u = nullptr; hout = nullptr; prof = false; }
        head_u = hout = prof = 0
    fold = bool(head_u and out and not hout)  # 2378
    enc = bool(tb and fold)  # 2390
    # 2380-2384
    if pooling != 0 and not (pooling == 1 and fold and not node_logits and not emb) and not (pooling == 2 and emb):
        return "refused", fold, enc, REFUSAL_POOLING
    # 2386-2389
    if self_scale and not (fold and pooling == 0 and not emb and not node_logits and tstride == 1):
        return "refused", fold, enc, REFUSAL_EPS
    if self_scale:  # 2401-2408
        return "eps", fold, enc, None
    if emb and pooling == 2:  # 2409-2413
        return "pool_max", fold, enc, None
    if pooling == 1 and fold and not node_logits:  # 2414-2419
        return "pool_sum", fold, enc, None
    if emb:  # 2420-2424
        return "pool_mean", fold, enc, None
    if node_logits and fold:  # 2425-2431
        return "node_logits", fold, enc, None
    return "default", fold, enc, None  # 2432-2434


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gin_resident_select") / "libgin_resident_select_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, "-o", so,
                           os.path.join(ROOT, "tests", "gin_resident_select_shim.cpp")])
    lib = C.CDLL(so)
    lib.grs_pick.argtypes = [C.c_int] * 10 + [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
    return lib


def pick(lib, case):
    fold, enc, why = C.c_int(-1), C.c_int(-1), C.c_char_p()
    inst = lib.grs_pick(*case, C.byref(fold), C.byref(enc), C.byref(why))
    return INSTANCES[inst], bool(fold.value), bool(enc.value), None if why.value is None else why.value.decode()


def test_pick_agrees_with_the_parents_if_chain(lib):
    assert len(CASES) == 2 ** 7 * 3 * 2 * 2
    wrong = [(dict(zip(FIELDS, c)), pick(lib, c), parent_pick(*c)) for c in CASES if pick(lib, c) != parent_pick(*c)]
    assert not wrong, f"{len(wrong)} of {len(CASES)} cases differ, the first: {wrong[0]}"


def test_every_instance_and_both_refusals_are_reached(lib):
    picks = [pick(lib, c) for c in CASES]
    assert {p[0] for p in picks} == set(INSTANCES)
    assert {p[3] for p in picks if p[0] == "refused"} == {REFUSAL_POOLING, REFUSAL_EPS}
    # no refused case picks an instance, and nothing else carries a refusal
    assert all((p[0] == "refused") == (p[3] is not None) for p in picks)
    # the in-kernel encoder rides on the folded last layer
    assert not any(enc and not fold for _, fold, enc, _ in picks)
