"""OGB's virtual node for GCN (flowgnn.h: flowgnn_set_gcn_virtual_node), the part that needs no GPU: the exporter and the weight file
against an un-folded float64 restatement of OGB's gcn-virtual, the header and the library's exports, the plan (gcn_plan.h) on every
input, and the proof that the fixed input of tests/test_gcn_vn_gpu.py tells the definition from every wrong form of it."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, _lib, export, graphpack as gp, weights
from tests import gcn_vn_ref as R
from tests import numpy_ref
from tests import resident_plan as rp
from tests.parity import REL
from tests.test_export import ogb_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_set_gcn_virtual_node", "flowgnn_gcn_virtual_node", "flowgnn_group_set_gcn_virtual_node"]


# ---------------------------------------------------------------- exporter and weight file
@pytest.mark.parametrize("with_bn", [True, False])
def test_exported_files_reproduce_the_unfolded_state_dict_forward(tmp_path, with_bn):
    """BatchNorm folding, the variance shift, key mapping and tensor order: the float64 forward of the exported tensors (before the
    files round them to float32) against OGB's semantics with nothing folded, within 1e-9 relative; then the files themselves at
    float32's precision."""
    sd = R.vn_state_dict(seed=4, with_bn=with_bn)
    batch = gp.synth_molpcba_batch(24, seed=10)
    want = R.ogb_vn_forward(sd, batch)
    real = export._checked
    try:  # the exporter's own functions with the float32 cast taken out
        export._checked = lambda w, spec, shape_of: {k: np.asarray(w[k], np.float64).reshape(tuple(shape_of(k, v))) for k, v in spec.items()}
        w64 = export.gcn_weights_from_ogb_state_dict(sd, virtual_node=True)
        vn64 = export.gcn_virtual_node_from_ogb_state_dict(sd)
    finally:
        export._checked = real
    exact = R.forward(batch, w64, vn64)[0]
    assert np.abs(exact - want).max() <= 1e-9 * np.abs(want).max(), np.abs(exact - want).max()
    w32 = export.gcn_weights_from_ogb_state_dict(sd, virtual_node=True)
    vn32 = export.gcn_virtual_node_from_ogb_state_dict(sd)
    gin32 = export.gin_virtual_node_from_ogb_state_dict(sd)  # the shared folding: the GIN function gives the same five tensors
    assert list(vn32) == list(gin32) and all(np.array_equal(vn32[k], gin32[k]) for k in vn32)
    export.export_weights("GCN", sd, str(tmp_path), virtual_node=True)
    assert sorted(os.listdir(tmp_path)) == sorted([weights.GCN_FILE, weights.GCN_VIRTUAL_NODE_FILE])
    assert weights.GCN_VIRTUAL_NODE_FILE == "gcn_ep1_virtualnode_dim100.bin"
    assert os.path.getsize(tmp_path / weights.GCN_VIRTUAL_NODE_FILE) == 161300 * 4
    w, vn = weights.load_gcn_weights(str(tmp_path)), weights.load_gcn_virtual_node(str(tmp_path))
    assert all(np.array_equal(vn[k], vn32[k]) for k in vn32) and all(np.array_equal(w[k], w32[k]) for k in w32)
    got = R.forward(batch, w, vn)[0]
    assert np.allclose(got, want, rtol=1e-4, atol=2e-5), np.abs(got - want).max()  # float32 files vs float64 source
    without = numpy_ref.gcn_forward(batch, w)
    assert np.abs(without - want).max() > 100 * np.abs(got - want).max()  # ... and the model without its virtual node is another model


def test_file_round_trip_and_short_file(tmp_path):
    vn = R.fixed_virtual_node()
    weights.save_gcn_virtual_node(vn, str(tmp_path))
    path = tmp_path / weights.GCN_VIRTUAL_NODE_FILE
    assert os.path.getsize(path) == 161300 * 4 == weights.GIN_VIRTUAL_NODE_FLOATS * 4
    back = weights.load_gcn_virtual_node(str(tmp_path))
    assert list(back) == ["vn_embedding", "w1", "b1", "w2", "b2"]
    assert [back[k].shape for k in back] == [(100,), (4, 200, 100), (4, 200), (4, 100, 200), (4, 100)]
    assert all(back[k].dtype == np.float32 and np.array_equal(back[k], vn[k]) for k in vn)
    flat = np.fromfile(path, dtype="<f4")  # the five tensors in the C call's order, end to end: GIN's file
    assert np.array_equal(flat[:100], vn["vn_embedding"]) and np.array_equal(flat[100:80100], vn["w1"].ravel())
    assert np.array_equal(flat[-400:], vn["b2"].ravel())
    weights.save_gin_virtual_node(vn, str(tmp_path))
    assert np.array_equal(np.fromfile(tmp_path / weights.GIN_VIRTUAL_NODE_FILE, dtype="<f4"), flat)
    with open(path, "r+b") as f:
        f.truncate(161299 * 4)
    with pytest.raises(IOError):
        weights.load_gcn_virtual_node(str(tmp_path))
    with pytest.raises(ValueError):
        weights.save_gcn_virtual_node({k: v for k, v in vn.items() if k != "b2"}, str(tmp_path))
    with pytest.raises(ValueError):
        weights.save_gcn_virtual_node(dict(vn, w1=vn["w1"][:3]), str(tmp_path))
    s = weights.synth_gcn_virtual_node()
    assert [s[k].shape for k in s] == [back[k].shape for k in back] and all(v.dtype == np.float32 and np.isfinite(v).all() for v in s.values())


def test_exporter_refusals_and_defaults(tmp_path):
    sd = R.vn_state_dict()
    with pytest.raises(export.ExportError, match="virtual_node=True"):
        export.gcn_weights_from_ogb_state_dict(sd)
    with pytest.raises(export.ExportError, match="virtual_node=True"):
        export.export_weights("GCN", sd, str(tmp_path))
    assert not os.path.exists(tmp_path / weights.GCN_VIRTUAL_NODE_FILE) and not os.path.exists(tmp_path / weights.GCN_FILE)
    export.gcn_weights_from_ogb_state_dict(sd, virtual_node=True)
    for model in ("GIN-VN", "PNA", "DGN", "GAT"):  # every model other than GIN and GCN: refused as ever, "GIN" in the message
        with pytest.raises(export.ExportError, match="GIN"):
            export.export_weights(model, sd, str(tmp_path), virtual_node=True)
    plain = ogb_state_dict("gcn", 4)  # a gcn state_dict has no such keys: it exports as before, and the VN exporter says what is missing
    a = export.export_weights("GCN", plain, str(tmp_path / "plain"))
    b = export.gcn_weights_from_ogb_state_dict(plain, virtual_node=True)  # (the argument permits, it does not demand)
    assert sorted(os.listdir(tmp_path / "plain")) == [weights.GCN_FILE]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    with pytest.raises(export.ExportError, match="virtualnode_embedding"):
        export.gcn_virtual_node_from_ogb_state_dict(plain)
    bad = R.vn_state_dict()
    bad["gnn_node.mlp_virtualnode_list.2.3.weight"] = np.full((100, 200), np.nan)
    with pytest.raises(export.ExportError, match="non-finite"):
        export.gcn_virtual_node_from_ogb_state_dict(bad)
    assert inspect.signature(export.gcn_weights_from_ogb_state_dict).parameters["virtual_node"].default is False
    assert inspect.signature(export.export_weights).parameters["virtual_node"].default is False
    assert inspect.signature(Engine.load_weights_dir).parameters["virtual_node"].default is False


# ---------------------------------------------------------------- C ABI
def test_header_declares_the_three_functions():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    five = r"const float\* vn_embedding, const float\* w1, const float\* b1, const float\* w2, const float\* b2\);"
    assert re.search(r"^int flowgnn_set_gcn_virtual_node\(flowgnn_engine\* e, " + five, text, re.M)
    assert re.search(r"^int flowgnn_gcn_virtual_node\(const flowgnn_engine\* e\);", text, re.M)
    assert re.search(r"^int flowgnn_group_set_gcn_virtual_node\(flowgnn_group\* g, " + five, text, re.M)


def test_library_exports_them_and_null_handles_answer():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f) and getattr(lib, f).restype == C.c_int, f
    assert lib.flowgnn_set_gcn_virtual_node.argtypes == [C.c_void_p] + [_lib.p_float] * 5
    assert lib.flowgnn_group_set_gcn_virtual_node.argtypes == [C.c_void_p] + [_lib.p_float] * 5
    null = C.c_void_p()
    vn = R.fixed_virtual_node()
    p = [vn[k].ctypes.data_as(_lib.p_float) for k in vn]
    assert lib.flowgnn_set_gcn_virtual_node(null, *p) == 1          # FLOWGNN_ERR_ARG
    assert lib.flowgnn_set_gcn_virtual_node(null, *[None] * 5) == 1
    assert lib.flowgnn_set_gcn_virtual_node(null, p[0], None, p[2], p[3], p[4]) == 1  # some but not all
    assert lib.flowgnn_gcn_virtual_node(null) == -1
    assert lib.flowgnn_group_set_gcn_virtual_node(null, *p) == 1
    assert lib.flowgnn_group_set_gcn_virtual_node(null, p[0], p[1], p[2], p[3], None) == 1
    for name in ("set_gcn_virtual_node", "gcn_virtual_node"):
        assert callable(getattr(Engine, name)), name
    assert callable(EngineGroup.set_gcn_virtual_node)


def test_host_cli_and_build_lists_know_it():
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    text = open(os.path.join(src, "host_main.cpp")).read()
    assert '"--ogb-vn"' in text and "gcn_ep1_virtualnode_dim100.bin" in text and "flowgnn_group_set_gcn_virtual_node" in text
    make = open(os.path.join(src, "Makefile")).read()
    units = re.search(r"^SRCS := (.*)$", make, re.M).group(1).split()
    assert "gcn_ogbvn.hip" in units and os.path.exists(os.path.join(src, "gcn_ogbvn.hip"))
    assert "gcn_ogbvn.h" in make and "ogbvn_dense.h" in make  # the object files follow the new headers


# ---------------------------------------------------------------- the reference is the project's own with the vector at zero
def test_forward_with_zero_tensors_is_the_gcn_forward():
    b, w = R.fixed_batch(), R.fixed_weights()
    out, rows, scale, x4 = R.forward(b, w, R.zero_virtual_node(), return_x4=True)
    want, xs = numpy_ref.gcn_forward(b, w, return_x=True)
    assert np.array_equal(out, want) and np.array_equal(x4, xs[4])
    assert scale >= float(np.abs(xs).max()) and rows.shape == (b.total_nodes, 100)


# ---------------------------------------------------------------- the plan, on every input
@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """every case of tests/resident_plan.py's full product: the plan with ogb_vn set, clear, and left alone (a shim of this test's
    own), and the plan of the existing shim, which never names the field"""
    d = tmp_path_factory.mktemp("gcn_vn_plan")
    so = os.path.join(str(d), "libgcn_vn_plan_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", rp.CSRC, "-o", so,
                           os.path.join(ROOT, "tests", "gcn_vn_plan_shim.cpp")])
    lib = C.CDLL(so)
    lib.gvp_gcn_bulk.argtypes = [C.POINTER(C.c_uint32), C.c_longlong, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_uint32)]
    lib.gvp_gcn_bulk.restype = None
    cases = rp.full_product("GCN")
    n = len(cases["pooling"])
    words, at = np.zeros(n, np.uint32), 0
    for k, bits in rp.INPUTS["GCN"]:
        words |= np.asarray(cases[k]).astype(np.uint32) << np.uint32(at)
        at += bits
    fields = rp.RESULTS["GCN"] + [("vn_fused", 1)]

    def run(ogb_vn):
        out = np.zeros(n, np.uint32)
        lib.gvp_gcn_bulk(words.ctypes.data_as(C.POINTER(C.c_uint32)), n, rp.FILLS["GCN"].ctypes.data_as(C.POINTER(C.c_double)), ogb_vn,
                         out.ctypes.data_as(C.POINTER(C.c_uint32)))
        res, at = {}, 0
        for k, bits in fields:
            res[k] = (out >> np.uint32(at)) & np.uint32((1 << bits) - 1)
            at += bits
        return res
    return cases, {"on": run(1), "off": run(0), "default": run(-1), "old": rp.plan(rp.build_shim(d), "GCN", cases)}


def test_plan_with_the_virtual_node(plans):
    cases, p = plans
    on = p["on"]
    assert len(cases["pooling"]) == 2 ** 17 * 3 * 3
    resident = rp.PATHS.index("resident")
    assert not (on["path"] == resident).any()
    assert (p["off"]["path"] == resident).any()  # (the inputs do reach that path without it)
    assert not on["wants_packed_tile_lists"].any()
    assert np.array_equal(on["vn_fused"], on["fused_encoder"] & on["fused_layers"])
    float_path = cases["qmode"] == 0
    assert on["vn_fused"][float_path].any() and (on["vn_fused"] == 0)[float_path].any()  # both forms are reached
    assert not on["vn_fused"][~float_path].any()
    # the in-place form adds to rows in HBM in front of every dense launch, the first included: no fused encoder without fused layers
    assert not (on["fused_encoder"] & (on["fused_layers"] == 0)).any()
    # where the plan fuses, it fuses what the plan without the virtual node's per-layer path fuses
    fast = (cases["split"] == 1) & (cases["exact"] == 0) & (cases["fused"] == 1) & (cases["edges"] == 1) & float_path
    assert np.array_equal(on["vn_fused"].astype(bool), fast)
    # and everything behind the layer loop is the per-layer path's
    per = (p["off"]["path"] == rp.PATHS.index("per_layer")) & float_path
    for k in ("folded_last", "multi_task", "node_logits_from_scores", "pool_rows", "node_logits_from_rows", "fused_layers"):
        assert np.array_equal(on[k][per], p["off"][k][per]), k


def test_plan_without_it_is_the_plan_it_was(plans):
    cases, p = plans
    assert not p["off"]["vn_fused"].any() and not p["default"]["vn_fused"].any()
    for k, _ in rp.RESULTS["GCN"]:
        assert np.array_equal(p["off"][k], p["old"][k].astype(np.uint32)), k
        assert np.array_equal(p["default"][k], p["old"][k].astype(np.uint32)), k


# ---------------------------------------------------------------- the input proves something
@pytest.fixture(scope="module")
def fixed():
    b, w, vn = R.fixed_batch(), R.fixed_weights(), R.fixed_virtual_node()
    return b, w, vn, R.forward(b, w, vn)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_the_fixed_input_separates_every_wrong_form(variant, fixed):
    """Each wrong form must move at least half of the logits by more than 10 x the f32 bound REL (scale + |want|): otherwise the GPU
    tests' comparisons on this input would pass with the virtual node computed wrongly.  A condition on the fixture."""
    b, w, vn, (want, _, scale) = fixed
    assert scale < 6.0e4  # far from the range threshold: the GPU runs assert exact_reruns() == 0
    got = R.forward(b, w, vn, variant=variant)[0]
    share = float((np.abs(got - want) > 10.0 * REL * (scale + np.abs(want))).mean())
    print(variant, "share of graphs moved:", share, "scale", scale)
    assert share >= 0.5, (variant, share)


def test_range_tensors_keep_the_reference_finite():
    """tests/test_gcn_vn_gpu.py's range re-run (R.range_virtual_node says what the tensors are and why): the float64 reference stays
    finite, the rows the vector is added to stay small, and the sum leaves the f16 split's range."""
    b, w = R.fixed_batch(), R.fixed_weights()
    out, rows, scale = R.forward(b, w, R.range_virtual_node())
    small = R.forward(b, w, R.zero_virtual_node())[2]
    assert np.isfinite(out).all() and np.isfinite(rows).all() and scale > 6.0e4 and small < 1000.0
