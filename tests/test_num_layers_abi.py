"""OGB's num_layer (flowgnn.h: flowgnn_set_num_layers): the header, the library's exports, the null handles and
the wrappers without a GPU; then, marked gpu because flowgnn_create needs the device but with no kernel launched, every status code and
refusal, in both orders where there are two calls, with the words the text must contain, and that depth 5 restores each refused call.
The arithmetic is tests/test_num_layers_gpu.py's."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, _lib, export, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_set_num_layers", "flowgnn_num_layers", "flowgnn_group_set_num_layers"]
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 8
gpu = pytest.mark.gpu


# ---------------------------------------------------------------- no GPU
def test_header_declares_the_calls_and_the_constants():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "flowgnn.h")).read())
    assert "#define FLOWGNN_NUM_LAYERS_DEFAULT 5" in text and "#define FLOWGNN_MAX_NUM_LAYERS 8" in text
    assert "int flowgnn_set_num_layers(flowgnn_engine* e, int emb_dim, int num_layers);" in text
    assert "int flowgnn_num_layers(const flowgnn_engine* e);" in text
    assert "int flowgnn_group_set_num_layers(flowgnn_group* g, int emb_dim, int num_layers);" in text
    assert "GNN_node raises below 2" in text and "turn it off, change the depth, set it again" in text
    assert "[flowgnn_num_layers(e)]" in text and "flowgnn_num_layers(e) - 1" in text  # the comments that said [5] and [4]


def test_library_exports_them_and_null_handles_answer():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f) and getattr(lib, f).restype == C.c_int, f
    null = C.c_void_p()
    for n in (1, 2, 5, 8, 9):
        assert lib.flowgnn_set_num_layers(null, 300, n) == ERR_ARG
        assert lib.flowgnn_group_set_num_layers(null, 300, n) == ERR_ARG
    assert lib.flowgnn_num_layers(null) == -1
    assert lib.flowgnn_set_num_layers.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert lib.flowgnn_group_set_num_layers.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert lib.flowgnn_num_layers.argtypes == [C.c_void_p]


def test_python_wrappers_and_cli_exist():
    for cls in (Engine, EngineGroup):
        p = inspect.signature(cls.set_num_layers).parameters
        assert list(p)[1:] == ["n", "emb_dim"] and p["emb_dim"].default == 300
        assert isinstance(inspect.getattr_static(cls, "num_layers"), property)
    assert "flowgnn_set_num_layers" in export.export_weights.__doc__
    for fn in (weights.load_gin_weights, weights.load_gcn_weights, weights.load_gin_eps, weights.load_gin_virtual_node, weights.load_gcn_virtual_node,
               weights.synth_gin_weights, weights.synth_gcn_weights, weights.gin_files, weights.gcn_shapes, weights.gin_virtual_node_shapes):
        assert inspect.signature(fn).parameters["num_layers"].default == 5, fn
    text = open(os.path.join(ROOT, "flowgnn_amd", "csrc", "host_main.cpp")).read()
    assert '"--num-layer"' in text and "flowgnn_group_set_num_layers" in text


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


def _set(e, d, n):
    rc = e.lib.flowgnn_set_num_layers(e._h, d, n)
    return rc, (e.lib.flowgnn_last_error(e._h) or b"").decode()


def _wide(model):
    e = Engine(model)
    (e.set_emb_dim if model == "GIN" else e.set_model_emb_dim)(300)
    return e


@gpu
@pytest.mark.parametrize("model", ["GIN", "GCN"])
def test_argument_errors_and_state(model, torch_context_first):
    e = Engine(model)
    try:
        assert e.num_layers == 5
        for n in (-1, 0, 1, 9, 100):
            for d in (100, 300):
                rc, text = _set(e, d, n)
                assert rc == ERR_ARG and str(n) in text and "2 .. 8" in text, (rc, text)
        for bad in (0, 200, 301):
            rc, text = _set(e, bad, 5)
            assert rc == ERR_ARG and "100" in text and "300" in text, (rc, text)
        rc, text = _set(e, 300, 3)  # an engine at width 100 asked for 300: the text names both widths
        assert rc == ERR_ARG and "300" in text and "100" in text, (rc, text)
        assert _set(e, 100, 5)[0] == OK  # the depth it has, before any state changes
        for n in (2, 3, 4, 6, 7, 8):  # width 100 with a depth other than 5
            rc, text = _set(e, 100, n)
            assert rc == ERR_UNSUPPORTED and "five layers deep" in text and "300" in text, (rc, text)
        assert e.num_layers == 5
        (e.set_emb_dim if model == "GIN" else e.set_model_emb_dim)(300)
        rc, text = _set(e, 100, 3)  # ... and at width 300, asked for 100
        assert rc == ERR_ARG and "100" in text and "300" in text, (rc, text)
        for n in (2, 3, 4, 6, 7, 8, 5):
            assert _set(e, 300, n)[0] == OK and e.num_layers == n
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("model", ["GIN-VN", "GAT", "PNA", "DGN"])
def test_other_models_refuse(model, torch_context_first):
    e = Engine(model)
    try:
        for d in (100, 300):
            rc, text = _set(e, d, 3)
            assert rc == ERR_UNSUPPORTED and "FLOWGNN_MODEL_GIN" in text and "FLOWGNN_MODEL_GCN" in text, (rc, text)
            assert _set(e, d, 5)[0] == OK  # what every engine is: a no-op for any model
        assert e.num_layers == 5
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("model", ["GIN", "GCN"])
def test_change_drops_weights_and_batch_and_keeps_the_settings(model, torch_context_first):
    from flowgnn_amd import graphpack as gp
    e = _wide(model)
    try:
        synth = weights.synth_gin_weights if model == "GIN" else weights.synth_gcn_weights
        e.set_weights(synth(emb_dim=300))
        b = gp.synth_molhiv_batch(4, seed=1)
        e.set_batch(b)
        e.set_pooling("sum")
        e.set_numeric_mode("f16", emb_dim=300)
        e.set_jk_residual("sum", True)
        e.set_num_layers(5)  # the same depth: nothing changes, the batch stays resident
        rc, _ = _rc(e.run)
        assert rc == OK
        e.sync()
        e.set_num_layers(3)
        rc, text = _rc(e.run)  # weights and batch have to be set again
        assert rc != OK, text
        rc, text = _rc(lambda: e.set_batch(b))  # the batch alone: accepted, and the run is still refused -- the weights went with the depth
        assert rc == OK, text
        rc, text = _rc(e.run)
        assert rc != OK and "weights" in text.lower(), (rc, text)
        with pytest.raises(ValueError) as ex:  # a weight set of the old depth never reaches the C call
            e.set_weights(synth(emb_dim=300))
        assert "5 layers" in str(ex.value) and "depth is 3" in str(ex.value), str(ex.value)
        assert e.pooling() == "sum" and e.jk_residual() == ("sum", True) and e.num_layers == 3  # none of them is sized by the depth
        e.set_weights(synth(emb_dim=300, num_layers=3))
        e.set_batch(b)
        e.run()
        e.sync()
    finally:
        e.close()


@gpu
def test_eps_and_virtual_node_belong_to_a_depth_both_orders(torch_context_first):
    for model in ("GIN", "GCN"):
        e = _wide(model)
        try:
            set_vn = e.set_ogb_virtual_node if model == "GIN" else e.set_gcn_virtual_node
            synth_vn = weights.synth_gin_virtual_node if model == "GIN" else weights.synth_gcn_virtual_node
            set_vn(synth_vn(emb_dim=300))
            rc, text = _rc(lambda: e.set_num_layers(3))
            assert rc == ERR_UNSUPPORTED and "virtual node" in text and "turn it off, change the depth, set it again" in text and "5 layers, not 3" in text, (rc, text)
            e.set_num_layers(5)  # the depth it has: accepted while it is on
            set_vn(None)
            e.set_num_layers(3)  # off restores the refused call
            with pytest.raises(ValueError):  # the other order: tensors of depth 5 for an engine of depth 3 never reach the C call
                set_vn(synth_vn(emb_dim=300))
            set_vn(synth_vn(emb_dim=300, num_layers=3))
            rc, text = _rc(lambda: e.set_num_layers(5))
            assert rc == ERR_UNSUPPORTED and "3 layers, not 5" in text, (rc, text)
            set_vn(None)
            if model == "GIN":
                e.set_gin_eps(np.full(3, 0.1, np.float32))
                assert e.gin_eps().shape == (3,) and np.allclose(e.gin_eps(), 0.1)
                with pytest.raises(ValueError):
                    e.set_gin_eps(np.zeros(5, np.float32))
                rc, text = _rc(lambda: e.set_num_layers(6))
                assert rc == ERR_UNSUPPORTED and "flowgnn_set_gin_eps" in text and "turn it off, change the depth, set it again" in text, (rc, text)
                e.set_gin_eps(None)
                e.set_num_layers(6)
                e.set_gin_eps(np.arange(6, dtype=np.float32) / 10)
                assert np.allclose(e.gin_eps(), np.arange(6) / 10)
                e.set_gin_eps(None)
            # ---- the width: to 100 while the depth is not 5 is refused by both width calls, depth 5 restores them
            for set_width in ([e.set_emb_dim, e.set_model_emb_dim] if model == "GIN" else [e.set_model_emb_dim]):
                rc, text = _rc(lambda: set_width(100))
                assert rc == ERR_UNSUPPORTED and "flowgnn_set_num_layers" in text and "five layers deep" in text, (rc, text)
                assert e.emb_dim == 300
            e.set_num_layers(5)
            e.set_model_emb_dim(100)
            assert e.emb_dim == 100 and e.num_layers == 5
            # ---- FLOWGNN_NUMERIC_Q6_10: the fixed-point arithmetic is five layers deep (the mode exists at width 100 alone)
            e.set_numeric_mode("q6.10")
            rc, text = _rc(lambda: e.set_num_layers(3, emb_dim=100))
            assert rc == ERR_UNSUPPORTED and "FLOWGNN_NUMERIC_Q6_10" in text, (rc, text)
            e.set_numeric_mode("f32")
            e.set_model_emb_dim(300)
            e.set_num_layers(3)
            rc, text = _rc(lambda: e.set_numeric_mode("q6.10"))  # the other order: at depth 3 the width is 300, which has no such mode
            assert rc == ERR_UNSUPPORTED, (rc, text)
        finally:
            e.close()


@gpu
def test_group_form(torch_context_first):
    g = EngineGroup("GCN", [0, 0])
    try:
        assert g.num_layers == 5
        rc, _ = _rc(lambda: g.set_num_layers(3))  # the members are 100 wide
        assert rc == ERR_ARG
        g.set_model_emb_dim(300)
        g.set_num_layers(7)
        for i in range(2):
            assert g.lib.flowgnn_num_layers(g.lib.flowgnn_group_engine(g._h, i)) == 7
        assert g.lib.flowgnn_group_set_num_layers(g._h, 300, 9) == ERR_ARG
        assert g.lib.flowgnn_group_set_num_layers(g._h, 200, 3) == ERR_ARG
        rc, text = _rc(lambda: g.set_model_emb_dim(100))
        assert rc == ERR_UNSUPPORTED and g.emb_dim == 300, (rc, text)
        g.set_num_layers(5)
        g.set_model_emb_dim(100)
    finally:
        g.close()
