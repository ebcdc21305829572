"""GCN's width as a run-time choice (flowgnn.h: flowgnn_set_model_emb_dim).  Without a GPU: the header, the library's exports, the
null-handle answers, the ctypes prototypes, the Python wrappers, the host CLI's call and the build lists.  With one (marked gpu:
flowgnn_create needs the device, nothing here launches a kernel except where a test says so): the getters, every refusal in both orders
of two calls, the argument errors, the no-op, and the state after a change of width."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, _lib, embedding_dim, export, graphpack as gp, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_set_model_emb_dim", "flowgnn_group_set_model_emb_dim"]
OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 0, 1, 6, 8


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why).  Without a GPU this does nothing."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def test_header_declares_the_two_functions():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    assert re.search(r"^int flowgnn_set_model_emb_dim\(flowgnn_engine\* e, int emb_dim\);", text, re.M)
    assert re.search(r"^int flowgnn_group_set_model_emb_dim\(flowgnn_group\* g, int emb_dim\);", text, re.M)
    assert text.index("int flowgnn_emb_dim(") < text.index("int flowgnn_set_model_emb_dim(")  # placed behind flowgnn_emb_dim
    assert "have no effect at 300" in text  # the options that choose among the 100-wide GCN paths


def test_library_exports_them_and_null_handles_answer():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f), f
    null = C.c_void_p()
    assert lib.flowgnn_set_model_emb_dim(null, 300) == ERR_ARG
    assert lib.flowgnn_group_set_model_emb_dim(null, 300) == ERR_ARG


def test_prototypes():
    lib = _lib.load()
    assert lib.flowgnn_set_model_emb_dim.argtypes == [C.c_void_p, C.c_int]
    assert lib.flowgnn_group_set_model_emb_dim.argtypes == [C.c_void_p, C.c_int]
    for f in FUNCS:
        assert getattr(lib, f).restype == C.c_int, f


def test_python_wrappers_exist():
    assert callable(Engine.set_model_emb_dim) and callable(EngineGroup.set_model_emb_dim)
    for fn in (weights.synth_gcn_weights, weights.load_gcn_weights, export.gcn_weights_from_ogb_state_dict, export.export_weights):
        assert inspect.signature(fn).parameters["emb_dim"].default == 100, fn
    assert inspect.signature(weights.save_gcn_weights).parameters["emb_dim"].default is None
    assert embedding_dim("GCN") == 100


def test_host_cli_names_the_new_group_call():
    text = open(os.path.join(ROOT, "flowgnn_amd", "csrc", "host_main.cpp")).read()
    assert "flowgnn_group_set_model_emb_dim" in text and "flowgnn_group_set_emb_dim" in text and "[--emb-dim 100|300]" in text


def test_the_build_lists_contain_the_new_file():
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    make = open(os.path.join(src, "Makefile")).read()
    units = re.search(r"^SRCS := (.*)$", make, re.M).group(1).split()
    loop = re.search(r"^for f in (.*); do$", open(os.path.join(ROOT, "scripts", "dev", "devlib.sh")).read(), re.M).group(1).split()
    assert "gcn_wide.hip" in units and "gcn_wide" in loop and os.path.exists(os.path.join(src, "gcn_wide.hip"))
    assert "wide_common.h" in make and os.path.exists(os.path.join(src, "wide_common.h"))  # the shared device code is a dependency of every object


def test_the_width_is_written_once():
    """gcn_wide.hip's kernels are templates on D: the literal width appears in the one instantiation only, and wide_common.h has none."""
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    code = lambda name: "\n".join(line.split("//")[0] for line in open(os.path.join(src, name)).read().splitlines())
    text = code("gcn_wide.hip")
    assert len(re.findall(r"\b300\b", text)) == 2, re.findall(r".*\b300\b.*", text)  # `emb_dim == 300` and `GcnWideModel<300>`
    for n in ("320", "304", "600"):
        assert not re.search(r"\b" + n + r"\b", text), n
    assert not re.search(r"\b(300|600)\b", code("wide_common.h"))


# ---------------------------------------------------------------- with a device
def _rc(call):
    try:
        call()
    except FlowGNNError as e:
        return e.code, str(e)
    return OK, ""


def _vn():
    return weights.synth_gin_virtual_node(seed=11)


@pytest.mark.gpu
def test_getters_and_argument_errors():
    e = Engine("GCN")
    try:
        assert e.emb_dim == 100
        for bad in (0, 200, -1):
            rc, text = _rc(lambda: e.set_model_emb_dim(bad))
            assert rc == ERR_ARG and "100" in text and "300" in text, (bad, rc, text)
            assert e.emb_dim == 100
        e.set_model_emb_dim(300)
        assert e.emb_dim == 300 and embedding_dim("GCN") == 100
        e.set_model_emb_dim(100)
        assert e.emb_dim == 100
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["GIN-VN", "GAT", "PNA", "DGN"])
def test_other_models_refuse(model):
    e = Engine(model)
    try:
        rc, text = _rc(lambda: e.set_model_emb_dim(300))
        assert rc == ERR_UNSUPPORTED and "GIN" in text and "GCN" in text, (rc, text)
        assert e.emb_dim == embedding_dim(model)
        rc, _ = _rc(lambda: e.set_model_emb_dim(200))
        assert rc == ERR_ARG
    finally:
        e.close()


@pytest.mark.gpu
def test_the_old_call_on_gcn_is_still_refused_and_names_the_new_one():
    e = Engine("GCN")
    try:
        for width in (300, 100):
            rc, text = _rc(lambda: e.set_emb_dim(width))
            assert rc == ERR_UNSUPPORTED and "GIN" in text and "flowgnn_set_model_emb_dim" in text, (rc, text)
        assert e.emb_dim == 100
        e.set_model_emb_dim(300)
        rc, text = _rc(lambda: e.set_emb_dim(100))
        assert rc == ERR_UNSUPPORTED and e.emb_dim == 300, (rc, text)
    finally:
        e.close()


@pytest.mark.gpu
def test_on_gin_it_is_set_emb_dim():
    """The same state after the call: emb_dim 300, weights dropped, the refusals of the width in force; and back."""
    b = gp.synth_molhiv_batch(4, seed=1)
    e = Engine("GIN")
    try:
        e.set_weights(weights.synth_gin_weights(seed=7))
        e.set_model_emb_dim(300)
        assert e.emb_dim == 300
        e.set_batch(b)
        assert e.lib.flowgnn_run(e._h) == ERR_STATE  # the weights went with the width
        rc, text = _rc(lambda: e.set_numeric_mode("f16"))
        assert rc == ERR_UNSUPPORTED and "300" in text
        e.set_emb_dim(300)  # the width it has, through the other call: a no-op
        e.set_emb_dim(100)
        assert e.emb_dim == 100
        e.set_ogb_virtual_node(_vn())
        rc, text = _rc(lambda: e.set_model_emb_dim(300))
        assert rc == ERR_UNSUPPORTED and "virtual node" in text, (rc, text)
    finally:
        e.close()


@pytest.mark.gpu
def test_fixed_point_refuses_in_both_orders():
    e = Engine("GCN")
    try:
        e.set_model_emb_dim(300)
        rc, text = _rc(lambda: e.set_numeric_mode("q6.10"))
        assert rc == ERR_UNSUPPORTED and "300" in text, (rc, text)
        e.set_numeric_mode("f32")
        e.set_model_emb_dim(100)
        e.set_numeric_mode("q6.10")
        rc, text = _rc(lambda: e.set_model_emb_dim(300))
        assert rc == ERR_UNSUPPORTED and "300" in text and "numeric" in text, (rc, text)
        assert e.emb_dim == 100
        e.set_model_emb_dim(100)  # the width it has: a no-op in any mode
    finally:
        e.close()


@pytest.mark.gpu
def test_gcn_virtual_node_refuses_in_both_orders():
    e = Engine("GCN")
    try:
        e.set_model_emb_dim(300)
        rc, text = _rc(lambda: e.set_gcn_virtual_node(_vn()))
        assert rc == ERR_UNSUPPORTED and "300" in text and "100 wide" in text, (rc, text)
        e.set_gcn_virtual_node(None)  # all five NULL stays accepted
        e.set_model_emb_dim(100)
        e.set_gcn_virtual_node(_vn())
        rc, text = _rc(lambda: e.set_model_emb_dim(300))
        assert rc == ERR_UNSUPPORTED and "300" in text and "virtual node" in text, (rc, text)
        assert e.emb_dim == 100
        e.set_model_emb_dim(100)  # the width it has: a no-op while the virtual node is on
        e.set_gcn_virtual_node(None)
        e.set_model_emb_dim(300)
        assert e.emb_dim == 300
    finally:
        e.close()


@pytest.mark.gpu
def test_aggregation_probes_refuse():
    e = Engine("GCN")
    try:
        e.set_model_emb_dim(300)
        lib, ms = e.lib, C.c_float()
        assert lib.flowgnn_run_aggregation_only(e._h, 0, 1, C.byref(ms)) == ERR_UNSUPPORTED
        assert b"300" in lib.flowgnn_last_error(e._h)
        d0, d1 = C.c_int(), C.c_int()
        assert lib.flowgnn_get_aggregate(e._h, 0, None, C.byref(d0), None, C.byref(d1)) == ERR_UNSUPPORTED
        assert b"300" in lib.flowgnn_last_error(e._h)
    finally:
        e.close()


@pytest.mark.gpu
def test_options_of_the_100_wide_paths_are_accepted_at_300():
    e = Engine("GCN")
    try:
        e.set_model_emb_dim(300)
        for key in ("gcn_resident", "gcn_binpack", "gcn_tile_build", "gcn_unfused", "gcn_mfma"):
            assert e.lib.flowgnn_set_option(e._h, key.encode(), 0.0) == OK, key
        assert e.emb_dim == 300
    finally:
        e.close()


@pytest.mark.gpu
def test_the_same_width_twice_keeps_weights_and_batch():
    """A no-op returns FLOWGNN_OK and drops nothing; a change drops the weights and the batch: FLOWGNN_ERR_STATE on flowgnn_run until
    both are set again.  (This one launches kernels: flowgnn_run is how the state shows.)"""
    b = gp.synth_molpcba_batch(4, seed=1)
    e = Engine("GCN")
    try:
        e.set_weights(weights.synth_gcn_weights(seed=7))
        e.set_batch(b)
        e.set_model_emb_dim(100)
        assert e.lib.flowgnn_run(e._h) == OK
        e.sync()
        e.set_model_emb_dim(300)
        assert e.lib.flowgnn_run(e._h) == ERR_STATE
        e.set_batch(b)
        assert e.lib.flowgnn_run(e._h) == ERR_STATE  # the weights went with the width
        e.set_weights(weights.synth_gcn_weights(seed=7, emb_dim=300))
        assert e.lib.flowgnn_run(e._h) == OK
        e.sync()
        e.set_model_emb_dim(300)
        assert e.lib.flowgnn_run(e._h) == OK
        e.sync()
        e.set_model_emb_dim(100)
        assert e.lib.flowgnn_run(e._h) == ERR_STATE
        e.set_weights(weights.synth_gcn_weights(seed=7))
        assert e.lib.flowgnn_run(e._h) == ERR_STATE  # ... and the batch
        e.set_batch(b)
        assert e.lib.flowgnn_run(e._h) == OK
        e.sync()
    finally:
        e.close()


@pytest.mark.gpu
def test_group_form():
    g = EngineGroup("GCN", [0, 0])
    try:
        assert g.emb_dim == 100
        g.set_model_emb_dim(300)
        assert g.emb_dim == 300
        rc, _ = _rc(lambda: g.set_model_emb_dim(200))
        assert rc == ERR_ARG
        rc, _ = _rc(lambda: g.set_emb_dim(100))
        assert rc == ERR_UNSUPPORTED and g.emb_dim == 300
        g.set_model_emb_dim(100)
        assert g.emb_dim == 100
    finally:
        g.close()
    g = EngineGroup("GIN", [0])
    try:
        g.set_model_emb_dim(300)
        assert g.emb_dim == 300
    finally:
        g.close()
    g = EngineGroup("GAT", [0])
    try:
        rc, _ = _rc(lambda: g.set_model_emb_dim(300))
        assert rc == ERR_UNSUPPORTED
    finally:
        g.close()
