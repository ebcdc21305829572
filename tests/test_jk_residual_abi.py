"""OGB's JK="sum" and residual=True (flowgnn.h: flowgnn_set_jk_residual): the header, the library's exports and
the wrappers without a GPU; then, marked gpu because flowgnn_create needs the device but with no kernel launched, every status code
and refusal, in both orders where there are two calls, with the words the text must contain, and that (FLOWGNN_JK_LAST, 0) restores
each refused call.  The arithmetic is tests/test_jk_residual_gpu.py's."""
import ctypes as C
import os
import re

import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, _lib, export

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_set_jk_residual", "flowgnn_jk_residual", "flowgnn_group_set_jk_residual"]
NEW_UNITS = ["gin_wide_jk.hip"]
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 8
LAST, SUM = 0, 1
ON = [(LAST, 1), (SUM, 0), (SUM, 1)]
gpu = pytest.mark.gpu


# ---------------------------------------------------------------- no GPU
def test_header_declares_the_three_calls_and_the_two_constants():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "flowgnn.h")).read())
    assert "#define FLOWGNN_JK_LAST 0" in text and "#define FLOWGNN_JK_SUM 1" in text
    assert "int flowgnn_set_jk_residual(flowgnn_engine* e, int emb_dim, int jk, int residual);" in text
    assert "int flowgnn_jk_residual(const flowgnn_engine* e, int* jk_out, int* residual_out);" in text
    assert "int flowgnn_group_set_jk_residual(flowgnn_group* g, int emb_dim, int jk, int residual);" in text
    assert "range(num_layer + 1)" in text and "six terms" in text  # which of OGB's two JK sums this is
    assert "NOT what the readout pools" in text                      # flowgnn_get_h under JK sum


def test_library_exports_them_and_null_handles_answer():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f), f
        assert getattr(lib, f).restype == C.c_int, f
    null = C.c_void_p()
    for jk, res in ON + [(LAST, 0)]:
        assert lib.flowgnn_set_jk_residual(null, 300, jk, res) == ERR_ARG
        assert lib.flowgnn_group_set_jk_residual(null, 300, jk, res) == ERR_ARG
    assert lib.flowgnn_jk_residual(null, None, None) == -1
    assert lib.flowgnn_set_jk_residual.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int]
    assert lib.flowgnn_group_set_jk_residual.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int]
    assert lib.flowgnn_jk_residual.argtypes == [C.c_void_p, _lib.p_int, _lib.p_int]


def test_python_wrappers_exist():
    import inspect
    for name in ("set_jk_residual", "jk_residual"):
        assert callable(getattr(Engine, name)), name
    assert callable(EngineGroup.set_jk_residual)
    for cls in (Engine, EngineGroup):
        p = inspect.signature(cls.set_jk_residual).parameters
        assert (p["jk"].default, p["residual"].default, p["emb_dim"].default) == ("last", False, 300)
    assert "set_jk_residual" in export.export_weights.__doc__  # the flags are not in a state_dict: the caller passes them


def test_host_cli_and_build_know_it():
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    text = open(os.path.join(src, "host_main.cpp")).read()
    assert '"--jk"' in text and '"--residual"' in text and "flowgnn_group_set_jk_residual" in text
    make = open(os.path.join(src, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", make, re.M).group(1).split()
    for unit in NEW_UNITS:
        assert unit in srcs and os.path.exists(os.path.join(src, unit)), unit
    for header in ("gin_wide_jk.h", "gin_wide_body.h", "gin_wide_f16_body.h"):
        assert os.path.exists(os.path.join(src, header)) and header in make, header


# ---------------------------------------------------------------- status codes (no kernel is launched)
@pytest.fixture(scope="module")
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


def _set(e, d, jk, res):
    rc = e.lib.flowgnn_set_jk_residual(e._h, d, jk, res)
    return rc, (e.lib.flowgnn_last_error(e._h) or b"").decode()


def _get(e):
    jk, res = C.c_int(-7), C.c_int(-7)
    rc = e.lib.flowgnn_jk_residual(e._h, C.byref(jk), C.byref(res))
    assert e.lib.flowgnn_jk_residual(e._h, None, None) == rc  # the outs may be NULL
    return rc, jk.value, res.value


@gpu
def test_argument_errors_and_state(torch_context_first):
    e = Engine("GIN")
    try:
        assert _get(e) == (0, LAST, 0) and e.jk_residual() == ("last", False)
        for jk in (-1, 2, 7):
            for d in (100, 300):
                rc, text = _set(e, d, jk, 0)
                assert rc == ERR_ARG and "jk" in text and str(jk) in text and "FLOWGNN_JK_SUM" in text, (rc, text)
        for res in (-1, 2):
            rc, text = _set(e, 300, SUM, res)
            assert rc == ERR_ARG and "residual" in text and str(res) in text, (rc, text)
        for bad in (0, 200, -300, 301):
            for jk, res in ON + [(LAST, 0)]:
                rc, text = _set(e, bad, jk, res)
                assert rc == ERR_ARG and "100" in text and "300" in text, (bad, rc, text)
        for jk, res in ON:
            rc, text = _set(e, 300, jk, res)  # an engine at width 100 asked for 300: the text names both widths
            assert rc == ERR_ARG and "300" in text and "100" in text, (rc, text)
            rc, text = _set(e, 100, jk, res)  # width 100 has no instance
            assert rc == ERR_UNSUPPORTED and "300" in text and "resident" in text and "flowgnn_set_emb_dim" in text, (rc, text)
        assert _set(e, 100, LAST, 0)[0] == OK and _set(e, 300, LAST, 0)[0] == OK  # the default: accepted with either width argument
        assert _get(e) == (0, LAST, 0)
        e.set_emb_dim(300)
        for jk, res in ON:
            rc, text = _set(e, 100, jk, res)  # ... and at width 300, asked for 100
            assert rc == ERR_ARG and "100" in text and "300" in text, (rc, text)
            assert _set(e, 300, jk, res)[0] == OK and _get(e) == (1, jk, res)
            assert e.jk_residual() == ("sum" if jk else "last", bool(res))
        assert _set(e, 100, LAST, 0)[0] == OK and _get(e) == (0, LAST, 0)  # off through either width argument
        with pytest.raises(ValueError):
            e.set_jk_residual("max")
        with pytest.raises(ValueError):
            e.set_jk_residual("concat")
        e.set_jk_residual("sum", True)
        assert e.jk_residual() == ("sum", True)
        e.set_jk_residual()
        assert e.jk_residual() == ("last", False)
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("model", ["GIN-VN", "GCN", "GAT", "PNA", "DGN"])
def test_other_models_refuse(model, torch_context_first):
    e = Engine(model)
    try:
        if model == "GCN":
            e.set_model_emb_dim(300)
        for d in (100, 300):
            for jk, res in ON:
                rc, text = _set(e, d, jk, res)
                assert rc == ERR_UNSUPPORTED and "FLOWGNN_MODEL_GIN" in text, (rc, text)
                if model == "GCN":  # why: its rows in HBM are post-linear, and the form does not exist yet
                    assert "post-linear" in text and "does not exist yet" in text, text
            assert _set(e, d, LAST, 0)[0] == OK  # the default is a no-op for any model
        assert _get(e) == (0, LAST, 0)
    finally:
        e.close()


@gpu
def test_width_change_is_refused_while_on_and_off_restores(torch_context_first):
    e = Engine("GIN")
    try:
        e.set_emb_dim(300)
        for jk, res in (("last", True), ("sum", False), ("sum", True)):
            e.set_jk_residual(jk, res)
            for set_width in (e.set_emb_dim, e.set_model_emb_dim):
                rc, text = _rc(lambda: set_width(100))
                assert rc == ERR_UNSUPPORTED and "flowgnn_set_jk_residual" in text and "100" in text and "turn it off" in text, (rc, text)
                assert e.emb_dim == 300 and e.jk_residual() == (jk, res)
                set_width(300)  # the width it has: a no-op
        # ---- it combines with everything else at this width: none of these calls is refused, in either order
        e.set_pooling("max")
        e.set_pooling("mean")
        e.set_numeric_mode("f16", emb_dim=300)
        e.set_numeric_mode("f32", emb_dim=300)
        e.set_node_embeddings(True)
        e.set_node_logits(True)
        e.set_embeddings(True)
        e.set_num_tasks(3)
        e.set_num_tasks(1)
        e.set_jk_residual("last", True)
        e.set_node_embeddings(False)
        e.set_node_logits(False)
        e.set_embeddings(False)
        assert e.jk_residual() == ("last", True)
        # ---- (LAST, 0) restores the refused call
        e.set_jk_residual("last", False)
        e.set_emb_dim(100)
        assert e.emb_dim == 100
        # ---- the other order: at width 100 the setting is refused, the width first and then the setting is accepted
        rc, text = _rc(lambda: e.set_jk_residual("sum", True, emb_dim=100))
        assert rc == ERR_UNSUPPORTED and e.jk_residual() == ("last", False), (rc, text)
        e.set_emb_dim(300)
        e.set_jk_residual("sum", True)
        assert e.jk_residual() == ("sum", True)
        e.set_jk_residual()
        e.set_model_emb_dim(100)
        assert e.emb_dim == 100
    finally:
        e.close()


@gpu
def test_group_form(torch_context_first):
    g = EngineGroup("GIN", [0, 0])
    try:
        rc, _ = _rc(lambda: g.set_jk_residual("sum", True))  # the members are 100 wide
        assert rc == ERR_ARG
        g.set_emb_dim(300)
        g.set_jk_residual("sum", True)
        for i in range(2):
            assert g.lib.flowgnn_jk_residual(g.lib.flowgnn_group_engine(g._h, i), None, None) == 1
        rc, text = _rc(lambda: g.set_emb_dim(100))
        assert rc == ERR_UNSUPPORTED and g.emb_dim == 300, (rc, text)
        assert g.lib.flowgnn_group_set_jk_residual(g._h, 200, 1, 1) == ERR_ARG
        assert g.lib.flowgnn_group_set_jk_residual(g._h, 300, 2, 0) == ERR_ARG
        assert g.lib.flowgnn_group_set_jk_residual(g._h, 300, 0, 2) == ERR_ARG
        g.set_jk_residual()
        for i in range(2):
            assert g.lib.flowgnn_jk_residual(g.lib.flowgnn_group_engine(g._h, i), None, None) == 0
        g.set_emb_dim(100)
    finally:
        g.close()
