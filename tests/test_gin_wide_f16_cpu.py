"""GIN at width 300 in the f16 numeric mode (flowgnn.h: flowgnn_set_numeric_mode_dim), what can be shown
without a GPU: that the probe of tests/test_gin_wide_f16_gpu.py can prove what it claims (every fp32 sum exact on its inputs, the
references apart from one another), that the restatement is tests/f16_ref.py's at width 100, and that the call exists in every layer
-- header, library, ctypes prototypes, wrappers, host CLI, build lists.  The last group fails on a tree without the call."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, _lib, graphpack as gp
from tests import f16_ref, gin_wide_f16_ref as R
from tests.test_f16_mode_gpu import probe_weights as probe_weights_100

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flowgnn_amd", "csrc")
ERR_ARG = 1


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---------------------------------------------------------------- the probe's inputs
def test_probe_batch_shape():
    b = R.probe_batch()
    assert (b.num_graphs, b.total_nodes) == (65, 934)
    assert int(b.nums_of_nodes[0]) == 1 and int(b.nums_of_nodes[-1]) == 1 and (np.asarray(b.nums_of_edges) == 0).sum() >= 3
    assert b.total_nodes > 7 * 128 and b.total_nodes % 16 != 0  # eight workgroups, the last one ending inside a 16-row tile


@pytest.mark.parametrize("c", R.CASES, ids=R.IDS)
def test_every_fp32_sum_of_the_mode_is_exact_on_the_probe(c):
    refs = R.references(c)
    for v in R.CHECKED:
        print(c.name, v, f"2^{refs[v][1]:.2f}")
        assert refs[v][1] <= 24.0, f"fp32 would round on this input (2^{refs[v][1]:.1f} > 2^24): the probe proves nothing"


def test_matmul_figure():
    """the node MLP's two products alone, on the plain case (2^18.6 with these weights): two non-zeros per row keep them below the
    walk, the pool and the head, which decide the figure of the whole forward (2^21.2)"""
    _, mm = R.forward(R.probe_batch(), R.weights_of(1), check="products")
    _, whole = R.forward(R.probe_batch(), R.weights_of(1), check=True)
    print(f"both products of the five layers: 2^{mm:.1f}; the whole forward: 2^{whole:.1f}")
    assert mm <= whole <= 24.0


@pytest.mark.parametrize("c", [c for c in R.CASES if c.name in ("plain", "eps", "sum", "max")], ids=lambda c: c.name)
def test_all_fp32_evaluation_equals_the_float64_one_bit_for_bit(c):
    kw = dict(eps=R.EPS if c.eps else None, pooling=c.pooling)
    a = R.forward(R.probe_batch(), R.weights_of(c.tasks), **kw)
    b = R.forward(R.probe_batch(), R.weights_of(c.tasks), dtype=np.float32, **kw)
    for name in ("logits", "rows", "pooled"):
        got = getattr(b, name)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), getattr(a, name)), name


def test_separation_table_and_the_named_exceptions():
    """NOT_SEPARATED is the computed table's complement, in both directions; logits, rows and pooled rows against rtz, the unrounded
    forward and both weight variants must separate in every case."""
    found = {}
    spread = {}
    for c in R.CASES:
        for (o, v), (ok, frac, med) in R.separation(c, R.TABLE_OUTPUTS).items():
            spread.setdefault((v, o), []).append(frac)
            if not ok:
                found[(c.name, o, v)] = frac
    for (v, o), f in sorted(spread.items()):
        print(f"{v:30s} {o:7s} {100 * min(f):.0f} .. {100 * max(f):.0f} %")
    assert set(found) == set(R.NOT_SEPARATED), (set(found) ^ set(R.NOT_SEPARATED))
    for k, frac in found.items():
        assert abs(frac - R.NOT_SEPARATED[k]) < 0.01, (k, frac)
        assert k[2] == "activations not rounded" and k[1] == "pooled", k  # nothing else may be listed


@pytest.mark.parametrize("cfg", [dict(), dict(eps=R.EPS), dict(pooling="sum"), dict(pooling="max"), dict(rnd="rtz"), dict(rnd={"w": "none"})],
                         ids=["plain", "eps", "sum", "max", "rtz", "weights not rounded"])
def test_at_width_100_it_is_f16_ref(cfg):
    b = gp.synth_molhiv_batch(12, seed=3)
    w = probe_weights_100(num_tasks=2, tight=True)
    got = R.forward(b, w, **cfg)
    want = f16_ref.gin_forward(b, w, fold=False, outputs=f16_ref.OUTPUTS, **cfg)
    for name in f16_ref.OUTPUTS:
        assert np.abs(getattr(got, name) - want[name]).max() <= 1e-12, name


def test_virtual_node_with_zero_tensors_is_the_plain_forward():
    from tests import gin_wide_vn_ref as V
    b, w = R.probe_batch(), R.weights_of(1)
    zero = V.zero_virtual_node()
    a, z = R.forward(b, w), R.forward(b, w, vn=zero)
    assert np.array_equal(a.rows, z.rows) and np.array_equal(a.logits, z.logits)
    # ... and unrounded it is tests/gin_wide_vn_ref.forward
    vn = R.virtual_node_of()
    got, want = R.forward(b, w, vn=vn, rnd="none"), V.forward(b, w, vn)
    assert np.abs(got.rows - want.rows).max() <= 1e-9 * want.scale and np.abs(got.logits - want.logits).max() <= 1e-9 * want.scale


# ---------------------------------------------------------------- the call, layer by layer
def test_header_declares_and_defines_the_call():
    h = _read("include", "flowgnn.h")
    assert re.search(r"int\s+flowgnn_set_numeric_mode_dim\(flowgnn_engine\*\s*e,\s*int\s+emb_dim,\s*int\s+mode\);", h)
    assert re.search(r"int\s+flowgnn_group_set_numeric_mode_dim\(flowgnn_group\*\s*g,\s*int\s+emb_dim,\s*int\s+mode\);", h)
    at = h.index("#define FLOWGNN_NUMERIC_F16")
    assert at < h.index("flowgnn_set_numeric_mode_dim(flowgnn_engine") < at + 4000  # next to the mode's definition
    assert "r(hid s1) / s1" in h and "FLOWGNN_ERR_ARG" in h[at:at + 4000]


def test_library_exports_prototypes_and_null_handles():
    lib = _lib.load()
    null = C.c_void_p()
    assert lib.flowgnn_set_numeric_mode_dim(null, 300, 2) == ERR_ARG
    assert lib.flowgnn_group_set_numeric_mode_dim(null, 300, 2) == ERR_ARG
    assert lib.flowgnn_set_numeric_mode_dim.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert lib.flowgnn_group_set_numeric_mode_dim.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert lib.flowgnn_set_numeric_mode_dim.restype == C.c_int and lib.flowgnn_group_set_numeric_mode_dim.restype == C.c_int


@pytest.mark.parametrize("cls", [Engine, EngineGroup])
def test_wrappers_take_the_width_as_a_keyword(cls):
    p = inspect.signature(cls.set_numeric_mode).parameters
    assert list(p)[1:] == ["mode", "emb_dim"] and p["emb_dim"].default is None and p["mode"].default == "f32"
    src = inspect.getsource(cls.set_numeric_mode)
    assert "_set_numeric_mode_dim" in src and "if emb_dim is None" in src  # the new call only when the width is given


def test_host_cli_routes_the_mode_through_the_group_form():
    src = _read("flowgnn_amd", "csrc", "host_main.cpp")
    assert re.search(r"emb_dim != FLOWGNN_EMB_DIM_REFERENCE \? flowgnn_group_set_numeric_mode_dim\(eng, emb_dim, numeric\) : "
                     r"flowgnn_group_set_numeric_mode\(eng, numeric\)", src)


def test_build_lists_and_the_width_written_once():
    mk = _read("flowgnn_amd", "csrc", "Makefile")
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "gin_wide_f16.hip" in srcs and "gin_wide_f16.h" in mk
    dev = _read("scripts", "dev", "devlib.sh")
    assert re.search(r"^for f in .*\bgin_wide_f16\b.*; do", dev, re.M)
    # templates on D: no literal width in the new translation unit or its header
    for name in ("gin_wide_f16.hip", "gin_wide_f16.h"):
        code = "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, name)).read().splitlines())
        for lit in ("300", "600", "320", "608"):
            assert not re.search(rf"\b{lit}\b", code), (name, lit)
    hip = open(os.path.join(CSRC, "gin_wide_f16.hip")).read()
    assert "gw_layer_f16_kernel" in hip and "gw_layer_vn_f16_kernel" in hip
    assert '"gin_wide_layer_f16"' in open(os.path.join(CSRC, "gin_wide.hip")).read()
