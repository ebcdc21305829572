"""OGB's set2set readout (flowgnn.h: flowgnn_set_set2set_pooling): the header, the library's exports and the
wrappers without a GPU; then, marked gpu because flowgnn_create needs the device but with no kernel launched, every status code and
refusal, in both orders where there are two calls, with the words the text must contain, and that turning the readout off restores
each refused call.  The arithmetic is tests/test_set2set_gpu.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, _lib, export, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_set_set2set_pooling", "flowgnn_set2set_pooling", "flowgnn_group_set_set2set_pooling"]
KEYS = ("w_ih", "w_hh", "b_ih", "b_hh", "head_w", "head_b")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 8
gpu = pytest.mark.gpu


# ---------------------------------------------------------------- no GPU
def test_header_declares_the_three_calls():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "flowgnn.h")).read())
    tensors = "const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* head_w, const float* head_b);"
    assert "int flowgnn_set_set2set_pooling(flowgnn_engine* e, int emb_dim, int steps, int num_tasks, " + tensors in text
    assert "int flowgnn_set2set_pooling(const flowgnn_engine* e);" in text
    assert "int flowgnn_group_set_set2set_pooling(flowgnn_group* g, int emb_dim, int steps, int num_tasks, " + tensors in text
    assert "pool.lstm.weight_ih_l0" in text and "(z_i, z_f, z_g, z_o)" in text and "#define FLOWGNN_SET2SET_MAX_STEPS 8" in text


def test_library_exports_them_and_null_handles_answer():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f), f
        assert getattr(lib, f).restype == C.c_int, f
    null = C.c_void_p()
    assert lib.flowgnn_set_set2set_pooling(null, 300, 2, 1, *[None] * 6) == ERR_ARG
    assert lib.flowgnn_set2set_pooling(null) == -1
    assert lib.flowgnn_group_set_set2set_pooling(null, 300, 2, 1, *[None] * 6) == ERR_ARG
    assert lib.flowgnn_set_set2set_pooling.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int] + [_lib.p_float] * 6
    assert lib.flowgnn_group_set_set2set_pooling.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int] + [_lib.p_float] * 6


def test_python_wrappers_exist():
    for name in ("set_set2set_pooling", "set2set_pooling"):
        assert callable(getattr(Engine, name)), name
    assert callable(EngineGroup.set_set2set_pooling)
    for name in ("synth_set2set", "save_set2set", "load_set2set", "checked_set2set", "set2set_shapes", "set2set_file"):
        assert callable(getattr(weights, name)), name
    assert weights.SET2SET_KEYS == KEYS
    assert callable(export.set2set_from_ogb_state_dict)
    assert weights.set2set_file("GIN") == "gin_ep1_set2set_dim300.bin" and weights.set2set_file("GCN") == "gcn_ep1_set2set_dim300.bin"


def test_host_cli_and_build_know_it():
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    text = open(os.path.join(src, "host_main.cpp")).read()
    assert '"--set2set"' in text and '"--set2set-steps"' in text and "flowgnn_group_set_set2set_pooling" in text
    make = open(os.path.join(src, "Makefile")).read()
    assert "wide_s2s.hip" in re.search(r"^SRCS := (.*)$", make, re.M).group(1).split()
    assert os.path.exists(os.path.join(src, "wide_s2s.hip")) and os.path.exists(os.path.join(src, "wide_s2s.h"))


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


def _s2s(d=300, t=1):
    return weights.synth_set2set(seed=d + t, emb_dim=d, num_tasks=t)


def _ptrs(s):
    assert all(a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] for a in s.values())
    return [s[k].ctypes.data_as(_lib.p_float) for k in KEYS]


def _set(e, d, p, steps=2, t=1):
    rc = e.lib.flowgnn_set_set2set_pooling(e._h, d, steps, t, *p)
    return rc, (e.lib.flowgnn_last_error(e._h) or b"").decode()


def _call(e, name, *args):
    rc = getattr(e.lib, name)(e._h, *args)
    return rc, (e.lib.flowgnn_last_error(e._h) or b"").decode()


def _wide(model):
    e = Engine(model)
    (e.set_emb_dim if model == "GIN" else e.set_model_emb_dim)(300)
    return e


@gpu
@pytest.mark.parametrize("model", ["GIN", "GCN"])
def test_argument_errors(model, torch_context_first):
    s100, s300 = _s2s(100), _s2s(300)
    p100, p300, none = _ptrs(s100), _ptrs(s300), [None] * 6
    e = Engine(model)
    try:
        for bad in (0, 200, -300, 301):
            for p in (p300, none):
                rc, text = _set(e, bad, p)
                assert rc == ERR_ARG and "100" in text and "300" in text, (bad, rc, text)
        rc, text = _set(e, 300, p300)  # an engine at width 100, tensors 300 wide: the text names both widths
        assert rc == ERR_ARG and "300" in text and "100" in text, (rc, text)
        rc, text = _set(e, 100, p100)  # tensors of the engine's width 100: only the 300-wide models have this readout
        assert rc == ERR_UNSUPPORTED and "300" in text and ("flowgnn_set_emb_dim" in text and "flowgnn_set_model_emb_dim" in text), (rc, text)
        assert e.set2set_pooling() == 0
        assert _set(e, 100, none)[0] == OK and _set(e, 300, none, steps=0, t=0)[0] == OK  # all NULL: off at any width, a no-op
        (e.set_emb_dim if model == "GIN" else e.set_model_emb_dim)(300)
        rc, text = _set(e, 100, p100)  # ... and at width 300, tensors 100 wide
        assert rc == ERR_ARG and "100" in text and "300" in text, (rc, text)
        for steps in (0, -1, 9, 100):
            rc, text = _set(e, 300, p300, steps=steps)
            assert rc == ERR_ARG and "steps" in text and str(steps) in text and "8" in text, (rc, text)
        for t in (0, -2, 2, 3):  # the engine's NUM_TASK is 1: the text names both numbers
            rc, text = _set(e, 300, p300, t=t)
            assert rc == ERR_ARG and str(t) in text and "1" in text and "flowgnn_set_num_tasks" in text, (rc, text)
        for k in range(6):
            for some in ([x if i != k else None for i, x in enumerate(p300)], [x if i == k else None for i, x in enumerate(p300)]):
                rc, text = _set(e, 300, some)
                assert rc == ERR_ARG and "NULL" in text, (rc, text)
        for value in (np.nan, np.inf, -np.inf):
            for key, at in (("w_ih", (1199, 599)), ("w_hh", (0, 299)), ("b_ih", (1199,)), ("b_hh", (0,)), ("head_w", (0, 599)), ("head_b", (0,))):
                bad = {k: v.copy() for k, v in s300.items()}
                bad[key][at] = value
                rc, text = _set(e, 300, _ptrs(bad))
                assert rc == ERR_ARG and "finite" in text and key in text, (rc, text)
        assert e.set2set_pooling() == 0
        for steps in (1, 2, 8):
            assert _set(e, 300, p300, steps=steps)[0] == OK and e.set2set_pooling() == steps
        assert _set(e, 100, none)[0] == OK and e.set2set_pooling() == 0  # off through either width argument
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("model", ["GIN-VN", "GAT", "PNA", "DGN"])
def test_other_models_refuse(model, torch_context_first):
    e = Engine(model)
    try:
        for d in (100, 300):
            rc, text = _set(e, d, _ptrs(_s2s(d)))
            assert rc == ERR_UNSUPPORTED and "GIN" in text and "GCN" in text, (rc, text)
        assert e.set2set_pooling() == 0
        assert _set(e, 300, [None] * 6)[0] == OK  # off is a no-op for any model
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("model", ["GIN", "GCN"])
def test_refusals_in_both_orders_and_off_restores(model, torch_context_first):
    s2s, gate = _s2s(300), weights.synth_attention_pooling()
    e = _wide(model)
    try:
        before = (e.attention_pooling(), e.pooling(), e.lib.flowgnn_num_tasks(e._h))
        # ---- the readout first, then the other call
        e.set_set2set_pooling(s2s, steps=3)
        assert e.set2set_pooling() == 3
        for mode in ("sum", "max"):
            rc, text = _rc(lambda: e.set_pooling(mode))
            assert rc == ERR_UNSUPPORTED and "pooling" in text and "set2set" in text, (rc, text)
        e.set_pooling("mean")  # the one accepted value
        assert e.pooling() == "mean"
        assert e.lib.flowgnn_set_pooling(e._h, 3) == ERR_ARG  # a bad mode stays an argument error
        rc, text = _call(e, "flowgnn_set_node_logits", 1)
        assert rc == ERR_UNSUPPORTED and "node logits" in text and "flowgnn_set_set2set_pooling" in text, (rc, text)
        assert _call(e, "flowgnn_set_node_logits", 0)[0] == OK  # off is always accepted
        rc, text = _call(e, "flowgnn_set_embeddings", 1)
        assert rc == ERR_UNSUPPORTED and "600" in text and "300" in text and "flowgnn_set_set2set_pooling" in text, (rc, text)
        assert _call(e, "flowgnn_set_embeddings", 0)[0] == OK
        rc, text = _rc(lambda: e.set_attention_pooling(gate))
        assert rc == ERR_UNSUPPORTED and "flowgnn_set_set2set_pooling" in text and "exclude" in text and e.attention_pooling() is False, (rc, text)
        e.set_attention_pooling(None)  # off is always accepted
        set_width = e.set_emb_dim if model == "GIN" else e.set_model_emb_dim
        rc, text = _rc(lambda: set_width(100))
        assert rc == ERR_UNSUPPORTED and "300" in text and "set2set" in text and e.emb_dim == 300, (rc, text)
        set_width(300)  # the width it has: a no-op
        rc, text = _call(e, "flowgnn_set_num_tasks", 3)
        assert rc == ERR_UNSUPPORTED and "set2set" in text and "3" in text and "1" in text, (rc, text)
        assert _call(e, "flowgnn_set_num_tasks", 1)[0] == OK  # the number it has
        assert e.set2set_pooling() == 3
        e.set_node_embeddings(True)  # combines
        e.set_node_embeddings(False)
        # ---- off restores each refused call, and leaves the other settings as they were
        e.set_set2set_pooling(None)
        assert e.set2set_pooling() == 0
        assert (e.attention_pooling(), e.pooling(), e.lib.flowgnn_num_tasks(e._h)) == before
        e.set_pooling("sum")
        # ---- the other call first, then the readout
        rc, text = _rc(lambda: e.set_set2set_pooling(s2s))
        assert rc == ERR_UNSUPPORTED and "pooling" in text and e.set2set_pooling() == 0, (rc, text)
        e.set_pooling("max")
        rc, text = _rc(lambda: e.set_set2set_pooling(s2s))
        assert rc == ERR_UNSUPPORTED and "pooling" in text, (rc, text)
        e.set_pooling("mean")
        assert _call(e, "flowgnn_set_node_logits", 1)[0] == OK
        rc, text = _rc(lambda: e.set_set2set_pooling(s2s))
        assert rc == ERR_UNSUPPORTED and "node logits" in text and e.set2set_pooling() == 0, (rc, text)
        assert _call(e, "flowgnn_set_node_logits", 0)[0] == OK
        assert _call(e, "flowgnn_set_embeddings", 1)[0] == OK
        rc, text = _rc(lambda: e.set_set2set_pooling(s2s))
        assert rc == ERR_UNSUPPORTED and "flowgnn_set_embeddings" in text and "600" in text and e.set2set_pooling() == 0, (rc, text)
        assert _call(e, "flowgnn_set_embeddings", 0)[0] == OK
        e.set_attention_pooling(gate)
        rc, text = _rc(lambda: e.set_set2set_pooling(s2s))
        assert rc == ERR_UNSUPPORTED and "flowgnn_set_attention_pooling" in text and "exclude" in text and e.set2set_pooling() == 0, (rc, text)
        assert e.attention_pooling() is True  # the refused call left the other readout on
        e.set_attention_pooling(None)
        e.set_num_tasks(3)
        rc, text = _rc(lambda: e.set_set2set_pooling(s2s))  # one task against the engine's three
        assert rc == ERR_ARG and "3" in text and "1" in text, (rc, text)
        e.set_set2set_pooling(_s2s(300, 3))
        assert e.set2set_pooling() == 2
        e.set_set2set_pooling(None)
        e.set_num_tasks(1)
        set_width(100)
        assert e.emb_dim == 100
    finally:
        e.close()


@gpu
def test_wrapper_reads_width_and_tasks_off_the_tensors(torch_context_first):
    e = Engine("GIN")
    try:
        rc, text = _rc(lambda: e.set_set2set_pooling(_s2s(100)))  # 100-wide tensors reach the C call, which refuses them by name
        assert rc == ERR_UNSUPPORTED and "300" in text, (rc, text)
        rc, text = _rc(lambda: e.set_set2set_pooling(_s2s(300)))
        assert rc == ERR_ARG and "100" in text and "300" in text, (rc, text)
        with pytest.raises(ValueError):
            e.set_set2set_pooling(dict(_s2s(300), b_ih=_s2s(100)["b_ih"]))
        with pytest.raises(ValueError):
            e.set_set2set_pooling({"w_ih": _s2s(300)["w_ih"]})
    finally:
        e.close()


@gpu
def test_group_form(torch_context_first):
    g = EngineGroup("GIN", [0, 0])
    try:
        rc, _ = _rc(lambda: g.set_set2set_pooling(_s2s(300)))  # the members are 100 wide
        assert rc == ERR_ARG
        g.set_emb_dim(300)
        g.set_set2set_pooling(_s2s(300), steps=4)
        for i in range(2):
            assert g.lib.flowgnn_set2set_pooling(g.lib.flowgnn_group_engine(g._h, i)) == 4
        rc, text = _rc(lambda: g.set_emb_dim(100))
        assert rc == ERR_UNSUPPORTED and g.emb_dim == 300, (rc, text)
        rc, text = _rc(lambda: g.set_pooling("sum"))
        assert rc == ERR_UNSUPPORTED and "pooling" in text, (rc, text)
        rc, text = _rc(lambda: g.set_attention_pooling(weights.synth_attention_pooling()))
        assert rc == ERR_UNSUPPORTED and "set2set" in text, (rc, text)
        rc, text = _rc(lambda: g.set_embeddings(True))
        assert rc == ERR_UNSUPPORTED, (rc, text)
        assert g.lib.flowgnn_group_set_set2set_pooling(g._h, 200, 2, 1, *[None] * 6) == ERR_ARG
        assert g.lib.flowgnn_group_set_set2set_pooling(g._h, 300, 9, 1, *_ptrs(_s2s(300))) == ERR_ARG
        g.set_set2set_pooling(None)
        for i in range(2):
            assert g.lib.flowgnn_set2set_pooling(g.lib.flowgnn_group_engine(g._h, i)) == 0
        g.set_emb_dim(100)
    finally:
        g.close()
