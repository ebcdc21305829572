"""The width-carrying call of gcn-virtual (flowgnn.h: flowgnn_set_gcn_virtual_node_dim): its status codes in
both call orders, the getter, the group form, off / on / off on a resident batch, flowgnn_set_model_emb_dim's refusal in both
directions, and the old call's refusal text.  Status codes only; marked gpu: flowgnn_create needs the device.  The arithmetic is
tests/test_gcn_wide_vn_gpu.py's."""
import ctypes as C

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, _lib, graphpack as gp, weights
from tests import gcn_wide_vn_ref as V
from tests.parity import REL, assert_close

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 8


@pytest.fixture(scope="module", autouse=True)
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


def _vn(d):
    return weights.synth_gcn_virtual_node(seed=13, emb_dim=d)


def _ptrs(vn):
    """The five tensors as the C call's arguments (contiguous float32 arrays that the caller keeps alive)."""
    assert all(a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] for a in vn.values())
    return [a.ctypes.data_as(_lib.p_float) for a in vn.values()]


def _dim(e, d, p):
    rc = e.lib.flowgnn_set_gcn_virtual_node_dim(e._h, d, *p)
    return rc, (e.lib.flowgnn_last_error(e._h) or b"").decode()


def test_null_handles_and_prototypes():
    lib = _lib.load()
    null = C.c_void_p()
    assert lib.flowgnn_set_gcn_virtual_node_dim(null, 300, None, None, None, None, None) == ERR_ARG
    assert lib.flowgnn_group_set_gcn_virtual_node_dim(null, 300, None, None, None, None, None) == ERR_ARG
    assert lib.flowgnn_set_gcn_virtual_node_dim.argtypes == [C.c_void_p, C.c_int] + [_lib.p_float] * 5
    assert lib.flowgnn_group_set_gcn_virtual_node_dim.argtypes == [C.c_void_p, C.c_int] + [_lib.p_float] * 5
    assert lib.flowgnn_set_gcn_virtual_node_dim.restype == C.c_int and lib.flowgnn_group_set_gcn_virtual_node_dim.restype == C.c_int


def test_status_codes_at_both_widths_and_in_both_orders():
    vn100, vn300 = _vn(100), _vn(300)
    p100, p300, none = _ptrs(vn100), _ptrs(vn300), [None] * 5
    e = Engine("GCN")
    try:
        # ---- at width 100: emb_dim 100 is exactly the old call
        for bad in (0, 200, -300, 301):
            for p in (none, p100):
                rc, text = _dim(e, bad, p)
                assert rc == ERR_ARG and "100" in text and "300" in text, (bad, rc, text)
        rc, text = _dim(e, 300, p300)  # tensors of the other width
        assert rc == ERR_ARG and "300" in text and "100" in text and e.gcn_virtual_node() is False, (rc, text)
        assert _dim(e, 300, none)[0] == OK  # all NULL: off at any width
        assert _dim(e, 100, p100)[0] == OK and e.gcn_virtual_node() is True
        rc, text = _rc(lambda: e.set_model_emb_dim(300))  # the tensors belong to a width
        assert rc == ERR_UNSUPPORTED and "virtual node" in text and e.emb_dim == 100, (rc, text)
        assert _dim(e, 300, none)[0] == OK and e.gcn_virtual_node() is False
        # ---- ... and at width 300, the virtual node before the weights
        e.set_model_emb_dim(300)
        rc, text = _dim(e, 100, p100)
        assert rc == ERR_ARG and "100" in text and "300" in text and e.gcn_virtual_node() is False, (rc, text)
        for some in ([p300[0], p300[1], None, p300[3], p300[4]], [None, None, None, None, p300[4]], [None] + p300[1:]):
            rc, text = _dim(e, 300, some)
            assert rc == ERR_ARG and "NULL" in text and e.gcn_virtual_node() is False, (rc, text)
        for key, val in (("w2", np.nan), ("vn_embedding", np.inf), ("b1", -np.inf)):
            bad = dict(vn300)
            bad[key] = vn300[key].copy()
            bad[key].ravel()[-1] = val
            rc, text = _dim(e, 300, _ptrs(bad))
            assert rc == ERR_ARG and key in text and "finite" in text and e.gcn_virtual_node() is False, (rc, text)
        assert _dim(e, 300, p300)[0] == OK and e.gcn_virtual_node() is True
        e.set_weights(weights.synth_gcn_weights(seed=7, emb_dim=300))  # ... then the weights: the state holds
        assert e.gcn_virtual_node() is True
        rc, text = _rc(lambda: e.set_model_emb_dim(100))  # from 300 with the virtual node on
        assert rc == ERR_UNSUPPORTED and "virtual node" in text and e.emb_dim == 300, (rc, text)
        e.set_model_emb_dim(300)  # the width it has: a no-op
        assert e.gcn_virtual_node() is True
        for mode in ("q6.10", "f16"):  # width 300 keeps refusing the numeric modes
            rc, text = _rc(lambda: e.set_numeric_mode(mode))
            assert rc == ERR_UNSUPPORTED and "300" in text, (rc, text)
        assert _dim(e, 100, none)[0] == OK and e.gcn_virtual_node() is False  # off through either width argument
        e.set_model_emb_dim(100)
        assert e.emb_dim == 100
        # ---- fixed point, in both orders of the two setters
        e.set_numeric_mode("q6.10")
        rc, text = _dim(e, 100, p100)
        assert rc == ERR_UNSUPPORTED and "fixed-point" in text, (rc, text)
        e.set_numeric_mode("f32")
        assert _dim(e, 100, p100)[0] == OK
        rc, text = _rc(lambda: e.set_numeric_mode("q6.10"))
        assert rc == ERR_UNSUPPORTED and "virtual node" in text, (rc, text)
    finally:
        e.close()


@pytest.mark.parametrize("model", ["GIN", "GIN-VN", "GAT", "PNA", "DGN"])
def test_other_models_refuse(model):
    e = Engine(model)
    try:
        for d in (100, 300):
            vn = _vn(d)
            rc, text = _dim(e, d, _ptrs(vn))
            assert rc == ERR_UNSUPPORTED and "GCN" in text, (rc, text)
        assert e.gcn_virtual_node() is False
    finally:
        e.close()


def test_the_old_calls_keep_refusing_and_the_wrapper_picks_the_call():
    e = Engine("GCN")
    try:
        with pytest.raises(ValueError):  # 300-wide tensors on an engine that is not 300 wide: before any C call
            e.set_gcn_virtual_node(_vn(300))
        e.set_model_emb_dim(300)
        rc, text = _rc(lambda: e.set_gcn_virtual_node(_vn(100)))  # (the wrapper sends 100-wide tensors through the old call)
        assert rc == ERR_UNSUPPORTED and "300" in text and "100 wide" in text and "flowgnn_set_gcn_virtual_node_dim" in text, (rc, text)
        vn300 = _vn(300)
        assert e.lib.flowgnn_set_gcn_virtual_node(e._h, *_ptrs(vn300)) == ERR_UNSUPPORTED  # no width argument: 100 wide by contract
        assert e.gcn_virtual_node() is False
        rc, text = _rc(lambda: e.set_ogb_virtual_node(_vn(300)))  # GIN's call on a GCN engine stays refused
        assert rc == ERR_UNSUPPORTED and "GIN" in text, (rc, text)
        e.set_gcn_virtual_node(None)
        e.set_gcn_virtual_node(_vn(300))  # ... and the wrapper sends 300-wide ones through the new call
        assert e.gcn_virtual_node() is True
        with pytest.raises(ValueError):
            e.set_gcn_virtual_node(dict(_vn(300), b2=_vn(100)["b2"]))
        e.set_gcn_virtual_node(None)
        assert e.gcn_virtual_node() is False
    finally:
        e.close()


def test_off_on_off_on_a_resident_batch():
    b = gp.synth_molpcba_batch(24, seed=5)
    w, vn = weights.synth_gcn_weights(seed=7, emb_dim=300), V.shapes_virtual_node()
    ref_on, ref_off = V.forward(b, w, vn), V.forward(b, w, V.zero_virtual_node())
    assert ref_on.operands < 6.0e4 / 2
    e = Engine("GCN")
    try:
        e.set_model_emb_dim(300)
        e.set_weights(w)
        e.set_batch(b)
        e.run()
        first = e.results().copy()
        e.set_gcn_virtual_node(vn)
        e.run()
        on = e.results().copy()
        e.set_weights(w)  # the state is the engine's: it holds across flowgnn_set_weights ...
        e.set_batch(b)    # ... and across batches
        assert e.gcn_virtual_node() is True
        e.run()
        on_again = e.results().copy()
        e.set_gcn_virtual_node(None)
        e.run()
        off = e.results().copy()
        assert e.exact_reruns() == 0
    finally:
        e.close()
    assert np.array_equal(first, off) and np.array_equal(on, on_again) and not np.array_equal(on, off)
    assert_close(on, ref_on.logits, scale=ref_on.scale, rel=REL, what="on, on a resident batch")
    assert_close(off, ref_off.logits, scale=ref_off.scale, rel=REL, what="off again")


def test_group_form():
    g = EngineGroup("GCN", [0, 0])
    try:
        with pytest.raises(ValueError):  # the members are 100 wide
            g.set_gcn_virtual_node(_vn(300))
        assert g.lib.flowgnn_group_set_gcn_virtual_node_dim(g._h, 300, *_ptrs(_vn(300))) == ERR_ARG
        g.set_model_emb_dim(300)
        g.set_gcn_virtual_node(_vn(300))
        assert all(int(g.lib.flowgnn_gcn_virtual_node(g.lib.flowgnn_group_engine(g._h, i))) == 1 for i in range(2))
        rc, text = _rc(lambda: g.set_model_emb_dim(100))
        assert rc == ERR_UNSUPPORTED and g.emb_dim == 300, (rc, text)
        rc, _ = _rc(lambda: g.set_gcn_virtual_node(_vn(100)))  # the old call, at 300
        assert rc == ERR_UNSUPPORTED
        assert g.lib.flowgnn_group_set_gcn_virtual_node_dim(g._h, 200, None, None, None, None, None) == ERR_ARG
        g.set_gcn_virtual_node(None)
        g.set_model_emb_dim(100)
        g.set_gcn_virtual_node(_vn(100))  # emb_dim 100 through the wrapper: the old call
        assert g.lib.flowgnn_group_set_gcn_virtual_node_dim(g._h, 100, *_ptrs(_vn(100))) == OK  # ... and through the new one
    finally:
        g.close()
    g = EngineGroup("GIN", [0])
    try:
        assert g.lib.flowgnn_group_set_gcn_virtual_node_dim(g._h, 300, *_ptrs(_vn(300))) == ERR_UNSUPPORTED
    finally:
        g.close()
