"""GIN's width as a run-time choice (flowgnn.h: flowgnn_set_emb_dim).  Without a GPU: the header, the library's exports, the null-handle
answers, the ctypes prototypes, the Python wrappers, the host CLI's flag and the build lists.  With one (marked gpu: flowgnn_create
needs the device, nothing here launches a kernel): the getters, every refusal in both orders of the two calls, the argument errors,
the no-op, and the state after a change of width."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, _lib, embedding_dim, export, graphpack as gp, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_set_emb_dim", "flowgnn_emb_dim", "flowgnn_group_set_emb_dim"]
OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 0, 1, 6, 8


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why): the tests below destroy engines, and
    tests/test_gin_wide_gpu.py, which runs next, hands torch tensors to one.  Without a GPU this does nothing."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def test_status_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    for name, value in (("FLOWGNN_OK", OK), ("FLOWGNN_ERR_ARG", ERR_ARG), ("FLOWGNN_ERR_STATE", ERR_STATE), ("FLOWGNN_ERR_UNSUPPORTED", ERR_UNSUPPORTED)):
        assert re.search(r"^#define " + name + r"\s+" + str(value) + r"\b", text, re.M), name


def test_header_declares_the_three_functions_and_two_constants():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    assert re.search(r"^#define FLOWGNN_EMB_DIM_REFERENCE\s+100\b", text, re.M)
    assert re.search(r"^#define FLOWGNN_EMB_DIM_OGB\s+300\b", text, re.M)
    assert re.search(r"^int flowgnn_set_emb_dim\(flowgnn_engine\* e, int emb_dim\);", text, re.M)
    assert re.search(r"^int flowgnn_emb_dim\(const flowgnn_engine\* e\);", text, re.M)
    assert re.search(r"^int flowgnn_group_set_emb_dim\(flowgnn_group\* g, int emb_dim\);", text, re.M)
    assert text.index("int flowgnn_num_tasks(") < text.index("int flowgnn_set_emb_dim(")  # placed behind flowgnn_set_num_tasks, which it follows


def test_library_exports_them_and_null_handles_answer():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f), f
    null = C.c_void_p()
    assert lib.flowgnn_set_emb_dim(null, 300) == ERR_ARG
    assert lib.flowgnn_emb_dim(null) == -1
    assert lib.flowgnn_group_set_emb_dim(null, 300) == ERR_ARG


def test_the_models_default_width_is_what_it_was():
    assert embedding_dim("GIN") == 100 and embedding_dim("GIN-VN") == 100 and embedding_dim("GCN") == 100


def test_prototypes():
    lib = _lib.load()
    assert lib.flowgnn_set_emb_dim.argtypes == [C.c_void_p, C.c_int]
    assert lib.flowgnn_emb_dim.argtypes == [C.c_void_p]
    assert lib.flowgnn_group_set_emb_dim.argtypes == [C.c_void_p, C.c_int]
    for f in FUNCS:
        assert getattr(lib, f).restype == C.c_int, f


def test_python_wrappers_exist():
    assert callable(Engine.set_emb_dim) and callable(EngineGroup.set_emb_dim)
    assert isinstance(Engine.emb_dim, property) and isinstance(EngineGroup.emb_dim, property)
    assert inspect.signature(weights.synth_gin_weights).parameters["emb_dim"].default == 100
    assert inspect.signature(weights.load_gin_weights).parameters["emb_dim"].default == 100
    assert inspect.signature(weights.save_gin_weights).parameters["emb_dim"].default is None
    assert weights.GIN_EMB_DIMS == (100, 300)
    assert weights.gin_files(100) == weights.GIN_FILES
    assert weights.gin_eps_file(300) == "gin_ep1_eps_dim300.bin" and weights.gin_eps_file(100) == weights.GIN_EPS_FILE


def test_host_cli_knows_the_flag():
    text = open(os.path.join(ROOT, "flowgnn_amd", "csrc", "host_main.cpp")).read()
    assert '"--emb-dim"' in text and "[--emb-dim 100|300]" in text and "flowgnn_group_set_emb_dim" in text


def test_the_build_lists_agree():
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    make = open(os.path.join(src, "Makefile")).read()
    units = re.search(r"^SRCS := (.*)$", make, re.M).group(1).split()
    loop = re.search(r"^for f in (.*); do$", open(os.path.join(ROOT, "scripts", "dev", "devlib.sh")).read(), re.M).group(1).split()
    assert "gin_wide.hip" in units and "gin_wide" in loop and os.path.exists(os.path.join(src, "gin_wide.hip"))


def test_the_width_is_written_once():
    """gin_wide.hip's kernels are templates on D: the literal widths appear in the one instantiation only."""
    text = open(os.path.join(ROOT, "flowgnn_amd", "csrc", "gin_wide.hip")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert len(re.findall(r"\b300\b", code)) == 2, re.findall(r".*\b300\b.*", code)  # `emb_dim == 300` and `GinWideModel<300>`
    for n in ("600", "320", "608"):
        assert not re.search(r"\b" + n + r"\b", code), n


# ---------------------------------------------------------------- with a device (no kernel is launched)
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
    e = Engine("GIN")
    try:
        assert e.emb_dim == 100
        for bad in (0, 200, -1):
            rc, text = _rc(lambda: e.set_emb_dim(bad))
            assert rc == ERR_ARG and "100" in text and "300" in text, (bad, rc, text)
            assert e.emb_dim == 100
        e.set_emb_dim(300)
        assert e.emb_dim == 300 and embedding_dim("GIN") == 100
        e.set_emb_dim(100)
        assert e.emb_dim == 100
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["GIN-VN", "GCN", "GAT", "PNA", "DGN"])
def test_other_models_refuse(model):
    e = Engine(model)
    try:
        rc, text = _rc(lambda: e.set_emb_dim(300))
        assert rc == ERR_UNSUPPORTED and "GIN" in text, (rc, text)
        assert e.emb_dim == embedding_dim(model)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["q6.10", "f16"])
def test_numeric_modes_refuse_in_both_orders(mode):
    e = Engine("GIN")
    try:
        e.set_emb_dim(300)
        rc, text = _rc(lambda: e.set_numeric_mode(mode))
        assert rc == ERR_UNSUPPORTED and "300" in text, (rc, text)
        e.set_numeric_mode("f32")
        e.set_emb_dim(100)
        e.set_numeric_mode(mode)
        rc, text = _rc(lambda: e.set_emb_dim(300))
        assert rc == ERR_UNSUPPORTED and "numeric" in text, (rc, text)
        assert e.emb_dim == 100
        e.set_emb_dim(100)  # the width it has: a no-op in any mode
    finally:
        e.close()


@pytest.mark.gpu
def test_ogb_virtual_node_refuses_in_both_orders():
    e = Engine("GIN")
    try:
        e.set_emb_dim(300)
        rc, text = _rc(lambda: e.set_ogb_virtual_node(_vn()))
        assert rc == ERR_UNSUPPORTED and "100 wide" in text, (rc, text)
        e.set_ogb_virtual_node(None)  # off stays accepted
        e.set_emb_dim(100)
        e.set_ogb_virtual_node(_vn())
        rc, text = _rc(lambda: e.set_emb_dim(300))
        assert rc == ERR_UNSUPPORTED and "virtual node" in text, (rc, text)
        assert e.emb_dim == 100
    finally:
        e.close()


@pytest.mark.gpu
def test_aggregation_probes_refuse():
    e = Engine("GIN")
    try:
        e.set_emb_dim(300)
        lib, ms = e.lib, C.c_float()
        assert lib.flowgnn_run_aggregation_only(e._h, 0, 1, C.byref(ms)) == ERR_UNSUPPORTED
        assert b"300" in lib.flowgnn_last_error(e._h)
        d0, d1 = C.c_int(), C.c_int()
        assert lib.flowgnn_get_aggregate(e._h, 0, None, C.byref(d0), None, C.byref(d1)) == ERR_UNSUPPORTED
        assert b"300" in lib.flowgnn_last_error(e._h)
    finally:
        e.close()


@pytest.mark.gpu
def test_the_same_width_twice_keeps_weights_and_batch():
    """A no-op returns FLOWGNN_OK and drops nothing; a change drops the weights and the batch: FLOWGNN_ERR_STATE on flowgnn_run until
    both are set again."""
    b = gp.synth_molhiv_batch(4, seed=1)
    e = Engine("GIN")
    try:
        e.set_weights(weights.synth_gin_weights(seed=7))
        e.set_batch(b)
        e.set_emb_dim(100)
        assert e.lib.flowgnn_run(e._h) == OK
        e.sync()
        e.set_emb_dim(300)
        assert e.lib.flowgnn_run(e._h) == ERR_STATE
        e.set_batch(b)
        assert e.lib.flowgnn_run(e._h) == ERR_STATE  # the weights went with the width
        e.set_weights(weights.synth_gin_weights(seed=7, emb_dim=300))
        assert e.lib.flowgnn_run(e._h) == OK
        e.sync()
        e.set_emb_dim(300)
        assert e.lib.flowgnn_run(e._h) == OK
        e.sync()
        e.set_emb_dim(100)
        assert e.lib.flowgnn_run(e._h) == ERR_STATE
        e.set_weights(weights.synth_gin_weights(seed=7))
        assert e.lib.flowgnn_run(e._h) == ERR_STATE  # ... and the batch
        e.set_batch(b)
        assert e.lib.flowgnn_run(e._h) == OK
        e.sync()
    finally:
        e.close()


@pytest.mark.gpu
def test_group_form():
    g = EngineGroup("GIN", [0, 0])
    try:
        assert g.emb_dim == 100
        g.set_emb_dim(300)
        assert g.emb_dim == 300
        rc, _ = _rc(lambda: g.set_emb_dim(200))
        assert rc == ERR_ARG
    finally:
        g.close()
    g = EngineGroup("GCN", [0])
    try:
        rc, _ = _rc(lambda: g.set_emb_dim(300))
        assert rc == ERR_UNSUPPORTED
    finally:
        g.close()
