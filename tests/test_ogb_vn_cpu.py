"""OGB's virtual node for GIN (flowgnn.h: flowgnn_set_ogb_virtual_node), the part that needs no GPU: the exporter and the weight file
against an un-folded float64 restatement of OGB's gin-virtual, the header and the library's exports, and the proof that the fixed
input of tests/test_ogb_vn_gpu.py tells the definition from every wrong form of it."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, _lib, export, graphpack as gp, weights
from tests import ogb_vn_ref as R
from tests.parity import REL
from tests.test_export import ogb_state_dict
from tests.test_gin_eps import EPS, fixed_batch, fixed_weights, gin_eps_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_set_ogb_virtual_node", "flowgnn_ogb_virtual_node", "flowgnn_group_set_ogb_virtual_node"]


# ---------------------------------------------------------------- exporter and weight file
@pytest.mark.parametrize("with_bn", [True, False])
def test_exported_files_reproduce_the_unfolded_state_dict_forward(tmp_path, with_bn):
    """BatchNorm folding, key mapping and tensor order: the float64 forward of the exported tensors (before the files round them to
    float32) against OGB's semantics with nothing folded, within 1e-9 relative; then the files themselves at float32's precision."""
    sd = R.vn_state_dict(seed=3, with_bn=with_bn)
    batch = gp.synth_molhiv_batch(24, seed=9)
    want = R.ogb_vn_forward(sd, batch)
    # the exporter's arithmetic is float64: what it hands to the float32 cast reproduces the source to rounding (1e-9 relative)
    w32 = export.gin_weights_from_ogb_state_dict(sd, keep_eps=True, virtual_node=True)
    vn32 = export.gin_virtual_node_from_ogb_state_dict(sd)
    eps = export.gin_eps_from_ogb_state_dict(sd)
    exact = _forward_unrounded(sd, batch)
    assert np.abs(exact - want).max() <= 1e-9 * np.abs(want).max(), np.abs(exact - want).max()
    export.export_weights("GIN", sd, str(tmp_path), keep_eps=True, virtual_node=True)
    assert sorted(os.listdir(tmp_path)) == sorted([f for f, _ in weights.GIN_FILES.values()] + ["gin_ep1_eps_dim100.bin", weights.GIN_VIRTUAL_NODE_FILE])
    assert os.path.getsize(tmp_path / weights.GIN_VIRTUAL_NODE_FILE) == 161300 * 4
    w, vn = weights.load_gin_weights(str(tmp_path)), weights.load_gin_virtual_node(str(tmp_path))
    assert all(np.array_equal(vn[k], vn32[k]) for k in vn32) and all(np.array_equal(w[k], w32[k]) for k in w32)
    got = R.forward(batch, w, vn, eps=weights.load_gin_eps(str(tmp_path)))[0]
    assert np.array_equal(weights.load_gin_eps(str(tmp_path)), eps)
    assert np.allclose(got, want, rtol=1e-4, atol=2e-5), np.abs(got - want).max()  # float32 files vs float64 source
    without = gin_eps_forward(batch, w, eps)[0]
    assert np.abs(without - want).max() > 100 * np.abs(got - want).max()  # ... and the model without its virtual node is another model


def _forward_unrounded(sd, batch):
    """R.forward on the exporter's folded tensors in float64 (the exporter's own functions, with the float32 cast taken out)."""
    real = export._checked
    try:
        export._checked = lambda w, spec, shape_of: {k: np.asarray(w[k], np.float64).reshape(tuple(shape_of(k, v))) for k, v in spec.items()}
        w = export.gin_weights_from_ogb_state_dict(sd, keep_eps=True, virtual_node=True)
        vn = export.gin_virtual_node_from_ogb_state_dict(sd)
    finally:
        export._checked = real
    eps64 = np.array([float(np.asarray(sd[f"gnn_node.convs.{l}.eps"]).ravel()[0]) for l in range(5)])
    return _forward_eps64(batch, w, vn, eps64)


def _forward_eps64(batch, w, vn, eps64):
    """R.forward with s_l = 1 + eps[l] in float64 (R.forward forms it in float32, as the engine does)."""
    real = R.self_scale
    try:
        R.self_scale = lambda eps: 1.0 + np.asarray(eps, np.float64)
        return R.forward(batch, w, vn, eps=eps64)[0]
    finally:
        R.self_scale = real


def test_file_round_trip_and_short_file(tmp_path):
    vn = R.fixed_virtual_node()
    weights.save_gin_virtual_node(vn, str(tmp_path))
    path = tmp_path / weights.GIN_VIRTUAL_NODE_FILE
    assert os.path.getsize(path) == 161300 * 4 == weights.GIN_VIRTUAL_NODE_FLOATS * 4
    back = weights.load_gin_virtual_node(str(tmp_path))
    assert list(back) == ["vn_embedding", "w1", "b1", "w2", "b2"]
    assert [back[k].shape for k in back] == [(100,), (4, 200, 100), (4, 200), (4, 100, 200), (4, 100)]
    assert all(back[k].dtype == np.float32 and np.array_equal(back[k], vn[k]) for k in vn)
    flat = np.fromfile(path, dtype="<f4")  # the five tensors in the C call's order, end to end
    assert np.array_equal(flat[:100], vn["vn_embedding"]) and np.array_equal(flat[100:80100], vn["w1"].ravel())
    assert np.array_equal(flat[-400:], vn["b2"].ravel())
    with open(path, "r+b") as f:
        f.truncate(161299 * 4)
    with pytest.raises(IOError):
        weights.load_gin_virtual_node(str(tmp_path))
    with pytest.raises(ValueError):
        weights.save_gin_virtual_node({k: v for k, v in vn.items() if k != "b2"}, str(tmp_path))
    with pytest.raises(ValueError):
        weights.save_gin_virtual_node(dict(vn, w1=vn["w1"][:3]), str(tmp_path))


def test_a_gin_virtual_state_dict_is_refused_without_the_new_argument(tmp_path):
    sd = R.vn_state_dict()
    with pytest.raises(export.ExportError, match="virtual_node=True"):
        export.gin_weights_from_ogb_state_dict(sd, keep_eps=True)
    with pytest.raises(export.ExportError, match="virtual_node=True"):
        export.export_weights("GIN", sd, str(tmp_path), keep_eps=True)
    assert not os.path.exists(tmp_path / weights.GIN_VIRTUAL_NODE_FILE)
    export.gin_weights_from_ogb_state_dict(sd, keep_eps=True, virtual_node=True)
    with pytest.raises(export.ExportError, match="GIN"):
        export.export_weights("GIN-VN", sd, str(tmp_path), keep_eps=True, virtual_node=True)
    plain = ogb_state_dict("gin", 3)  # a gin state_dict has no such keys: the exporter says which one is missing
    with pytest.raises(export.ExportError, match="virtualnode_embedding"):
        export.gin_virtual_node_from_ogb_state_dict(plain)
    bad = R.vn_state_dict()
    bad["gnn_node.mlp_virtualnode_list.2.3.weight"] = np.full((100, 200), np.nan)
    with pytest.raises(export.ExportError, match="non-finite"):
        export.gin_virtual_node_from_ogb_state_dict(bad)
    assert inspect.signature(export.gin_weights_from_ogb_state_dict).parameters["virtual_node"].default is False
    assert inspect.signature(export.export_weights).parameters["virtual_node"].default is False
    assert inspect.signature(Engine.load_weights_dir).parameters["virtual_node"].default is False


# ---------------------------------------------------------------- C ABI
def test_header_declares_the_three_functions_and_two_constants():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    five = r"const float\* vn_embedding, const float\* w1, const float\* b1, const float\* w2, const float\* b2\);"
    assert re.search(r"^int flowgnn_set_ogb_virtual_node\(flowgnn_engine\* e, " + five, text, re.M)
    assert re.search(r"^int flowgnn_ogb_virtual_node\(const flowgnn_engine\* e\);", text, re.M)
    assert re.search(r"^int flowgnn_group_set_ogb_virtual_node\(flowgnn_group\* g, " + five, text, re.M)
    assert re.search(r"^#define FLOWGNN_OGB_VN_LAYERS 4$", text, re.M) and re.search(r"^#define FLOWGNN_OGB_VN_HIDDEN 200$", text, re.M)


def test_library_exports_them_and_null_handles_answer():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f) and getattr(lib, f).restype == C.c_int, f
    assert lib.flowgnn_set_ogb_virtual_node.argtypes == [C.c_void_p] + [_lib.p_float] * 5
    assert lib.flowgnn_group_set_ogb_virtual_node.argtypes == [C.c_void_p] + [_lib.p_float] * 5
    null = C.c_void_p()
    vn = R.fixed_virtual_node()
    p = [vn[k].ctypes.data_as(_lib.p_float) for k in vn]
    assert lib.flowgnn_set_ogb_virtual_node(null, *p) == 1          # FLOWGNN_ERR_ARG
    assert lib.flowgnn_set_ogb_virtual_node(null, *[None] * 5) == 1
    assert lib.flowgnn_set_ogb_virtual_node(null, p[0], None, p[2], p[3], p[4]) == 1  # some but not all
    assert lib.flowgnn_ogb_virtual_node(null) == -1
    assert lib.flowgnn_group_set_ogb_virtual_node(null, *p) == 1
    assert lib.flowgnn_group_set_ogb_virtual_node(null, p[0], p[1], p[2], p[3], None) == 1
    for name in ("set_ogb_virtual_node", "ogb_virtual_node"):
        assert callable(getattr(Engine, name)), name
    assert callable(EngineGroup.set_ogb_virtual_node)


def test_host_cli_and_build_lists_know_it():
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    text = open(os.path.join(src, "host_main.cpp")).read()
    assert '"--ogb-vn"' in text and "[--ogb-vn]" in text and "gin_ep1_virtualnode_dim100.bin" in text and "flowgnn_group_set_ogb_virtual_node" in text
    units = re.search(r"^SRCS := (.*)$", open(os.path.join(src, "Makefile")).read(), re.M).group(1).split()
    assert "gin_ogbvn.hip" in units and os.path.exists(os.path.join(src, "gin_ogbvn.hip"))


# ---------------------------------------------------------------- the reference is the project's own with the vector at zero
def test_forward_with_zero_tensors_is_the_eps_forward():
    b, w = fixed_batch("GIN"), fixed_weights()
    for eps in (None, EPS):
        out, rows, scale = R.forward(b, w, R.zero_virtual_node(), eps=eps)
        want, hs, amax, hmax = gin_eps_forward(b, w, eps)
        assert np.array_equal(out, want) and np.array_equal(rows, hs[5])
        assert scale >= max(amax, hmax, float(np.abs(hs).max()))


# ---------------------------------------------------------------- the input proves something
@pytest.fixture(scope="module")
def fixed():
    b, w, vn = fixed_batch("GIN"), fixed_weights(), R.fixed_virtual_node()
    return b, w, vn, {on: R.forward(b, w, vn, eps=EPS if on else None) for on in (False, True)}


@pytest.mark.parametrize("eps_on", [False, True])
@pytest.mark.parametrize("variant", R.VARIANTS)
def test_the_fixed_input_separates_every_wrong_form(variant, eps_on, fixed):
    """No add in the last layer, the pool taken before the add, t without + vn_l, a mean instead of the sum, an update indexed l + 1
    and E ignored must each move more than a quarter of the graphs' logits by more than 10 x the f32 bound (that is 5 x the f16
    mode's): otherwise the GPU tests' comparisons on this input would pass with the virtual node computed wrongly."""
    b, w, vn, refs = fixed
    want, _, scale = refs[eps_on]
    assert scale < 6.0e4  # far from the range threshold: the GPU runs assert exact_reruns() == 0
    got = R.forward(b, w, vn, eps=EPS if eps_on else None, variant=variant)[0]
    share = float((np.abs(got - want) > 10.0 * REL * (scale + np.abs(want))).mean())
    print(variant, "eps", eps_on, "share of graphs moved:", share, "scale", scale)
    assert share > 0.25, (variant, eps_on, share)


@pytest.mark.parametrize("eps_on", [False, True])
def test_an_update_behind_the_last_layer_is_a_no_op(eps_on, fixed):
    """The launch of layer 4 only adds: a fifth update would feed nothing, so the four weight sets are indexed by the layer they
    follow (l), and `update_indexed_l_plus_1` above is the wrong reading."""
    b, w, vn, refs = fixed
    got = R.forward(b, w, vn, eps=EPS if eps_on else None, variant=R.NOOP_VARIANT)
    assert np.array_equal(got[0], refs[eps_on][0]) and np.array_equal(got[1], refs[eps_on][1])
