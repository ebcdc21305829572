"""OGB's JK="sum" and residual=True for GCN at width 300 (flowgnn.h: flowgnn_set_model_jk_residual): the header,
the library's exports, the wrappers, the host and the Makefile without a GPU; then, marked gpu because flowgnn_create needs the device
but with no kernel launched, every status code and refusal, in both orders where two calls meet, with the words the text must contain,
and that (FLOWGNN_JK_LAST, 0) restores each refused call.  The arithmetic is tests/test_gcn_jk_residual_gpu.py's."""
import ctypes as C
import inspect
import os
import re

import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, _lib, export

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_set_model_jk_residual", "flowgnn_group_set_model_jk_residual"]
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 8
LAST, SUM = 0, 1
ON = [(LAST, 1), (SUM, 0), (SUM, 1)]
gpu = pytest.mark.gpu


# ---------------------------------------------------------------- no GPU
def test_header_declares_the_two_calls():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "flowgnn.h")).read())
    assert "int flowgnn_set_model_jk_residual(flowgnn_engine* e, int emb_dim, int jk, int residual);" in text
    assert "int flowgnn_group_set_model_jk_residual(flowgnn_group* g, int emb_dim, int jk, int residual);" in text
    assert "int flowgnn_set_jk_residual(flowgnn_engine* e, int emb_dim, int jk, int residual);" in text  # the old call stays
    assert "UNPROJECTED" in text and "section 4.25" in text and "flowgnn_set_gcn_virtual_node_dim" in text
    assert "flowgnn_jk_residual serves both" in text


def test_library_exports_them_and_null_handles_answer():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f), f
        assert getattr(lib, f).restype == C.c_int, f
    null = C.c_void_p()
    for jk, res in ON + [(LAST, 0)]:
        assert lib.flowgnn_set_model_jk_residual(null, 300, jk, res) == ERR_ARG
        assert lib.flowgnn_group_set_model_jk_residual(null, 300, jk, res) == ERR_ARG
    assert lib.flowgnn_set_model_jk_residual.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int]
    assert lib.flowgnn_group_set_model_jk_residual.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int]


def test_python_wrappers_keep_their_signature_and_use_the_model_form_for_gcn():
    for cls in (Engine, EngineGroup):
        p = inspect.signature(cls.set_jk_residual).parameters
        assert list(p) == ["self", "jk", "residual", "emb_dim"]
        assert (p["jk"].default, p["residual"].default, p["emb_dim"].default) == ("last", False, 300)
        src = inspect.getsource(cls.set_jk_residual)
        assert "set_model_jk_residual" in src and '"GCN"' in src, cls
    doc = export.export_weights.__doc__
    assert "flowgnn_set_model_jk_residual" in doc and "host GCN --emb-dim 300 [--ogb-vn] --jk sum --residual" in doc


def test_host_cli_and_build_know_it():
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    text = open(os.path.join(src, "host_main.cpp")).read()
    assert "flowgnn_group_set_model_jk_residual" in text and "flowgnn_group_set_jk_residual" in text
    make = open(os.path.join(src, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", make, re.M).group(1).split()
    assert "gcn_wide_jk.hip" in srcs and os.path.exists(os.path.join(src, "gcn_wide_jk.hip"))
    for header in ("gcn_wide_jk.h", "gcn_wide_body.h"):
        assert os.path.exists(os.path.join(src, header)) and header in make, header
    dev = open(os.path.join(ROOT, "scripts", "dev", "devlib.sh")).read()
    assert " gcn_wide_jk " in dev


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


def _set(e, d, jk, res, fn="flowgnn_set_model_jk_residual"):
    rc = getattr(e.lib, fn)(e._h, d, jk, res)
    return rc, (e.lib.flowgnn_last_error(e._h) or b"").decode()


def _get(e):
    jk, res = C.c_int(-7), C.c_int(-7)
    rc = e.lib.flowgnn_jk_residual(e._h, C.byref(jk), C.byref(res))
    assert e.lib.flowgnn_jk_residual(e._h, None, None) == rc  # the outs may be NULL
    return rc, jk.value, res.value


@gpu
def test_gcn_argument_errors_and_state(torch_context_first):
    e = Engine("GCN")
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
            rc, text = _set(e, 100, jk, res)  # GCN at width 100 has no instance
            assert rc == ERR_UNSUPPORTED and "flowgnn_set_model_emb_dim" in text and "300" in text, (rc, text)
            assert _get(e) == (0, LAST, 0)
        assert _set(e, 100, LAST, 0)[0] == OK and _set(e, 300, LAST, 0)[0] == OK  # the default: accepted with either width argument
        e.set_model_emb_dim(300)
        for jk, res in ON:
            rc, text = _set(e, 100, jk, res)  # ... and at width 300, asked for 100
            assert rc == ERR_ARG and "100" in text and "300" in text, (rc, text)
            assert _set(e, 300, jk, res)[0] == OK and _get(e) == (1, jk, res)
            assert e.jk_residual() == ("sum" if jk else "last", bool(res))
        assert _set(e, 100, LAST, 0)[0] == OK and _get(e) == (0, LAST, 0)  # off through either width argument
        with pytest.raises(ValueError):
            e.set_jk_residual("cat")
        e.set_jk_residual("sum", True)  # the wrapper takes the model form for GCN
        assert e.jk_residual() == ("sum", True) and _get(e) == (1, SUM, 1)
        e.set_jk_residual()
        assert e.jk_residual() == ("last", False)
    finally:
        e.close()


@gpu
def test_the_old_call_keeps_its_answer_on_gcn_and_names_the_new_one(torch_context_first):
    e = Engine("GCN")
    try:
        e.set_model_emb_dim(300)
        for order in (0, 1):  # with the setting off, and with it on through the new call
            if order:
                assert _set(e, 300, SUM, 1)[0] == OK
            for d in (100, 300):
                for jk, res in ON:
                    rc, text = _set(e, d, jk, res, fn="flowgnn_set_jk_residual")
                    assert rc == ERR_UNSUPPORTED, (rc, text)
                    for phrase in ("FLOWGNN_MODEL_GIN", "post-linear", "does not exist yet", "flowgnn_set_model_jk_residual"):
                        assert phrase in text, (phrase, text)
            assert _get(e) == ((1, SUM, 1) if order else (0, LAST, 0))  # a refusal changes nothing
        # (LAST, 0) is the same state through either call
        assert _set(e, 300, LAST, 0, fn="flowgnn_set_jk_residual")[0] == OK and _get(e) == (0, LAST, 0)
    finally:
        e.close()


@gpu
def test_on_a_gin_engine_the_new_call_is_the_old_one(torch_context_first):
    e = Engine("GIN")
    try:
        for fn in ("flowgnn_set_jk_residual", "flowgnn_set_model_jk_residual"):
            for jk, res in ON:
                rc, text = _set(e, 300, jk, res, fn=fn)
                assert rc == ERR_ARG and "300" in text and "100" in text, (fn, rc, text)
                rc, text = _set(e, 100, jk, res, fn=fn)
                assert rc == ERR_UNSUPPORTED and "resident" in text and "flowgnn_set_emb_dim" in text, (fn, rc, text)
        e.set_emb_dim(300)
        for jk, res in ON:
            assert _set(e, 300, jk, res)[0] == OK and _get(e) == (1, jk, res)          # set through the new call ...
            assert _set(e, 300, LAST, 0, fn="flowgnn_set_jk_residual")[0] == OK and _get(e) == (0, LAST, 0)   # ... cleared through the old
            assert _set(e, 300, jk, res, fn="flowgnn_set_jk_residual")[0] == OK and _get(e) == (1, jk, res)   # and the other way round
            assert _set(e, 300, LAST, 0)[0] == OK and _get(e) == (0, LAST, 0)
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("model", ["GIN-VN", "GAT", "PNA", "DGN"])
def test_other_models_refuse_the_new_call(model, torch_context_first):
    e = Engine(model)
    try:
        for d in (100, 300):
            for jk, res in ON:
                rc, text = _set(e, d, jk, res)
                assert rc == ERR_UNSUPPORTED and "FLOWGNN_MODEL_GIN" in text and "FLOWGNN_MODEL_GCN" in text, (rc, text)
            assert _set(e, d, LAST, 0)[0] == OK  # the default is a no-op for any model
        assert _get(e) == (0, LAST, 0)
    finally:
        e.close()


@gpu
def test_width_change_is_refused_while_on_and_off_restores(torch_context_first):
    e = Engine("GCN")
    try:
        e.set_model_emb_dim(300)
        for jk, res in (("last", True), ("sum", False), ("sum", True)):
            e.set_jk_residual(jk, res)
            rc, text = _rc(lambda: e.set_model_emb_dim(100))
            assert rc == ERR_UNSUPPORTED and "flowgnn_set_model_jk_residual" in text and "100" in text and "turn it off" in text, (rc, text)
            assert e.emb_dim == 300 and e.jk_residual() == (jk, res)
            e.set_model_emb_dim(300)  # the width it has: a no-op
        # ---- it combines with everything else at this width: none of these calls is refused, in either order
        e.set_pooling("max")
        e.set_pooling("mean")
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
        e.set_model_emb_dim(100)
        assert e.emb_dim == 100
        # ---- the other order: at width 100 the setting is refused, the width first and then the setting is accepted
        rc, text = _rc(lambda: e.set_jk_residual("sum", True, emb_dim=100))
        assert rc == ERR_UNSUPPORTED and e.jk_residual() == ("last", False), (rc, text)
        e.set_model_emb_dim(300)
        e.set_jk_residual("sum", True)
        assert e.jk_residual() == ("sum", True)
        e.set_jk_residual()
        e.set_model_emb_dim(100)
        assert e.emb_dim == 100
    finally:
        e.close()


@gpu
def test_group_form(torch_context_first):
    g = EngineGroup("GCN", [0, 0])
    try:
        rc, _ = _rc(lambda: g.set_jk_residual("sum", True))  # the members are 100 wide
        assert rc == ERR_ARG
        g.set_model_emb_dim(300)
        g.set_jk_residual("sum", True)
        for i in range(2):
            assert g.lib.flowgnn_jk_residual(g.lib.flowgnn_group_engine(g._h, i), None, None) == 1
        rc, text = _rc(lambda: g.set_model_emb_dim(100))
        assert rc == ERR_UNSUPPORTED and g.emb_dim == 300, (rc, text)
        assert g.lib.flowgnn_group_set_jk_residual(g._h, 300, 1, 1) == ERR_UNSUPPORTED  # the old group call refuses GCN too
        assert g.lib.flowgnn_group_set_model_jk_residual(g._h, 200, 1, 1) == ERR_ARG
        assert g.lib.flowgnn_group_set_model_jk_residual(g._h, 300, 2, 0) == ERR_ARG
        assert g.lib.flowgnn_group_set_model_jk_residual(g._h, 300, 0, 2) == ERR_ARG
        g.set_jk_residual()
        for i in range(2):
            assert g.lib.flowgnn_jk_residual(g.lib.flowgnn_group_engine(g._h, i), None, None) == 0
        g.set_model_emb_dim(100)
    finally:
        g.close()
