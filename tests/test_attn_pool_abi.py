"""OGB's attention readout (flowgnn.h: flowgnn_set_attention_pooling): the header, the library's exports and
the wrappers without a GPU; then, marked gpu because flowgnn_create needs the device but with no kernel launched, every status code
and refusal, in both orders where there are two calls, with the words the text must contain, and that turning the readout off restores
each refused call.  The arithmetic is tests/test_attn_pool_gpu.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, _lib, export, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_set_attention_pooling", "flowgnn_attention_pooling", "flowgnn_group_set_attention_pooling"]
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 8
gpu = pytest.mark.gpu


# ---------------------------------------------------------------- no GPU
def test_header_declares_the_three_calls():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    assert re.search(r"^int flowgnn_set_attention_pooling\(flowgnn_engine\* e, int emb_dim, const float\* w1, const float\* b1, const float\* w2\);", text, re.M)
    assert re.search(r"^int flowgnn_attention_pooling\(const flowgnn_engine\* e\);", text, re.M)
    assert re.search(r"^int flowgnn_group_set_attention_pooling\(flowgnn_group\* g, int emb_dim, const float\* w1, const float\* b1, const float\* w2\);", text, re.M)
    assert "pool.gate_nn.3.bias" in text  # the header says that the last bias cancels and is not taken


def test_library_exports_them_and_null_handles_answer():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f), f
        assert getattr(lib, f).restype == C.c_int, f
    null = C.c_void_p()
    assert lib.flowgnn_set_attention_pooling(null, 300, None, None, None) == ERR_ARG
    assert lib.flowgnn_attention_pooling(null) == -1
    assert lib.flowgnn_group_set_attention_pooling(null, 300, None, None, None) == ERR_ARG
    assert lib.flowgnn_set_attention_pooling.argtypes == [C.c_void_p, C.c_int] + [_lib.p_float] * 3
    assert lib.flowgnn_group_set_attention_pooling.argtypes == [C.c_void_p, C.c_int] + [_lib.p_float] * 3


def test_python_wrappers_exist():
    for name in ("set_attention_pooling", "attention_pooling"):
        assert callable(getattr(Engine, name)), name
    assert callable(EngineGroup.set_attention_pooling)
    for name in ("synth_attention_pooling", "save_attention_pooling", "load_attention_pooling"):
        assert callable(getattr(weights, name)), name
    assert callable(export.attention_pooling_from_ogb_state_dict)
    assert weights.attention_pooling_file("GIN") == "gin_ep1_attnpool_dim300.bin" and weights.attention_pooling_file("GCN") == "gcn_ep1_attnpool_dim300.bin"


def test_host_cli_and_build_know_it():
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    text = open(os.path.join(src, "host_main.cpp")).read()
    assert '"--attn-pool"' in text and "flowgnn_group_set_attention_pooling" in text
    make = open(os.path.join(src, "Makefile")).read()
    assert "wide_attn.hip" in re.search(r"^SRCS := (.*)$", make, re.M).group(1).split()
    assert os.path.exists(os.path.join(src, "wide_attn.hip")) and os.path.exists(os.path.join(src, "wide_attn.h"))


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


def _gate(d=300):
    rng = np.random.default_rng(d)
    return {"w1": rng.standard_normal((2 * d, d)).astype(np.float32), "b1": rng.standard_normal(2 * d).astype(np.float32),
            "w2": rng.standard_normal(2 * d).astype(np.float32)}


def _ptrs(g):
    assert all(a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] for a in g.values())
    return [g[k].ctypes.data_as(_lib.p_float) for k in ("w1", "b1", "w2")]


def _set(e, d, p):
    rc = e.lib.flowgnn_set_attention_pooling(e._h, d, *p)
    return rc, (e.lib.flowgnn_last_error(e._h) or b"").decode()


def _nlog(e, on):
    rc = e.lib.flowgnn_set_node_logits(e._h, on)
    return rc, (e.lib.flowgnn_last_error(e._h) or b"").decode()


def _wide(model):
    e = Engine(model)
    if model == "GIN":
        e.set_emb_dim(300)
    else:
        e.set_model_emb_dim(300)
    return e


@gpu
@pytest.mark.parametrize("model", ["GIN", "GCN"])
def test_argument_errors(model, torch_context_first):
    g100, g300 = _gate(100), _gate(300)
    p100, p300, none = _ptrs(g100), _ptrs(g300), [None] * 3
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
        assert e.attention_pooling() is False
        assert _set(e, 100, none)[0] == OK and _set(e, 300, none)[0] == OK  # all NULL: off at any width, a no-op
        (e.set_emb_dim if model == "GIN" else e.set_model_emb_dim)(300)
        rc, text = _set(e, 100, p100)  # ... and at width 300, tensors 100 wide
        assert rc == ERR_ARG and "100" in text and "300" in text, (rc, text)
        for some in ([p300[0], None, p300[2]], [None, None, p300[2]], [None] + p300[1:], [p300[0], p300[1], None]):
            rc, text = _set(e, 300, some)
            assert rc == ERR_ARG and "NULL" in text, (rc, text)
        for value in (np.nan, np.inf, -np.inf):
            for key, at in (("w1", (599, 299)), ("b1", (599,)), ("w2", (0,))):
                bad = {k: v.copy() for k, v in g300.items()}
                bad[key][at] = value
                rc, text = _set(e, 300, _ptrs(bad))
                assert rc == ERR_ARG and "finite" in text and key in text, (rc, text)
        assert e.attention_pooling() is False
        assert _set(e, 300, p300)[0] == OK and e.attention_pooling() is True
        assert _set(e, 100, none)[0] == OK and e.attention_pooling() is False  # off through either width argument
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("model", ["GIN-VN", "GAT", "PNA", "DGN"])
def test_other_models_refuse(model, torch_context_first):
    e = Engine(model)
    try:
        for d in (100, 300):
            rc, text = _set(e, d, _ptrs(_gate(d)))
            assert rc == ERR_UNSUPPORTED and "GIN" in text and "GCN" in text, (rc, text)
        assert e.attention_pooling() is False
        assert _set(e, 300, [None] * 3)[0] == OK  # off is a no-op for any model
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("model", ["GIN", "GCN"])
def test_refusals_in_both_orders_and_off_restores(model, torch_context_first):
    gate = _gate(300)
    e = _wide(model)
    try:
        # ---- the readout first, then the other call
        e.set_attention_pooling(gate)
        assert e.attention_pooling() is True
        for mode in ("sum", "max"):
            rc, text = _rc(lambda: e.set_pooling(mode))
            assert rc == ERR_UNSUPPORTED and "pooling" in text and "attention" in text, (rc, text)
        e.set_pooling("mean")  # the one accepted value
        assert e.pooling() == "mean"  # flowgnn_pooling keeps reporting what flowgnn_set_pooling said
        rc, text = _nlog(e, 1)
        assert rc == ERR_UNSUPPORTED and "node logits" in text, (rc, text)
        assert _nlog(e, 0)[0] == OK  # off is always accepted
        set_width = e.set_emb_dim if model == "GIN" else e.set_model_emb_dim
        rc, text = _rc(lambda: set_width(100))
        assert rc == ERR_UNSUPPORTED and "300" in text and "attention" in text and e.emb_dim == 300, (rc, text)
        set_width(300)  # the width it has: a no-op
        assert e.attention_pooling() is True
        assert e.lib.flowgnn_set_pooling(e._h, 3) == ERR_ARG  # a bad mode stays an argument error
        # ---- off restores each refused call
        e.set_attention_pooling(None)
        assert e.attention_pooling() is False
        e.set_pooling("sum")
        assert e.pooling() == "sum"
        # ---- the other call first, then the readout
        rc, text = _rc(lambda: e.set_attention_pooling(gate))
        assert rc == ERR_UNSUPPORTED and "pooling" in text and e.attention_pooling() is False, (rc, text)
        e.set_pooling("max")
        rc, text = _rc(lambda: e.set_attention_pooling(gate))
        assert rc == ERR_UNSUPPORTED and "pooling" in text, (rc, text)
        e.set_pooling("mean")
        assert _nlog(e, 1)[0] == OK
        rc, text = _rc(lambda: e.set_attention_pooling(gate))
        assert rc == ERR_UNSUPPORTED and "node logits" in text and e.attention_pooling() is False, (rc, text)
        assert _nlog(e, 0)[0] == OK
        e.set_attention_pooling(gate)
        assert e.attention_pooling() is True
        e.set_attention_pooling(None)
        set_width(100)
        assert e.emb_dim == 100
    finally:
        e.close()


@gpu
def test_wrapper_reads_the_width_off_w1(torch_context_first):
    e = Engine("GIN")
    try:
        rc, text = _rc(lambda: e.set_attention_pooling(_gate(100)))  # 100-wide tensors reach the C call, which refuses them by name
        assert rc == ERR_UNSUPPORTED and "300" in text, (rc, text)
        rc, text = _rc(lambda: e.set_attention_pooling(_gate(300)))
        assert rc == ERR_ARG and "100" in text and "300" in text, (rc, text)
        with pytest.raises(ValueError):
            e.set_attention_pooling(dict(_gate(300), b1=_gate(100)["b1"]))
        with pytest.raises(ValueError):
            e.set_attention_pooling({"w1": _gate(300)["w1"]})
    finally:
        e.close()


@gpu
def test_group_form(torch_context_first):
    g = EngineGroup("GIN", [0, 0])
    try:
        rc, _ = _rc(lambda: g.set_attention_pooling(_gate(300)))  # the members are 100 wide
        assert rc == ERR_ARG
        g.set_emb_dim(300)
        g.set_attention_pooling(_gate(300))
        for i in range(2):
            assert g.lib.flowgnn_attention_pooling(g.lib.flowgnn_group_engine(g._h, i)) == 1
        rc, text = _rc(lambda: g.set_emb_dim(100))
        assert rc == ERR_UNSUPPORTED and g.emb_dim == 300, (rc, text)
        rc, text = _rc(lambda: g.set_pooling("sum"))
        assert rc == ERR_UNSUPPORTED and "pooling" in text, (rc, text)
        assert g.lib.flowgnn_group_set_attention_pooling(g._h, 200, None, None, None) == ERR_ARG
        g.set_attention_pooling(None)
        g.set_emb_dim(100)
    finally:
        g.close()
