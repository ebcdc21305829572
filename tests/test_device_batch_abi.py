"""flowgnn_set_batch_device without a GPU: the header declares it and its layouts, the library exports it, a null engine is refused,
and GraphBatch.to_pyg / from_pyg round-trip to the reference arrays."""
import ctypes
import os
import re

import numpy as np

from flowgnn_amd import GraphBatch, graphpack as gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "flowgnn_amd", "libflowgnn_hip.so")
HEADER = os.path.join(ROOT, "include", "flowgnn.h")


def test_header_declares_set_batch_device_and_layouts():
    src = open(HEADER).read()
    assert re.search(r"#define\s+FLOWGNN_LAYOUT_REFERENCE\s+0\b", src)
    assert re.search(r"#define\s+FLOWGNN_LAYOUT_PYG\s+1\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+flowgnn_set_batch_device\s*\(([^)]*)\)\s*;", code)
    assert m, "flowgnn_set_batch_device is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9 and args[4].startswith("int layout") and args[8].startswith("const float*")


def test_library_exports_set_batch_device_and_refuses_a_null_engine():
    lib = ctypes.CDLL(LIB)
    fn = lib.flowgnn_set_batch_device
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    assert fn(None, 0, None, None, 1, None, None, None, None) == 1  # FLOWGNN_ERR_ARG
    nn = (ctypes.c_int * 2)(3, 4)
    assert fn(None, 2, nn, nn, 0, None, None, None, None) == 1
    assert fn(None, 2, nn, nn, 7, None, None, None, None) == 1


def test_binding_declares_the_symbol():
    from flowgnn_amd import Engine, _lib
    lib = _lib.load()
    assert lib.flowgnn_set_batch_device.restype is ctypes.c_int
    assert len(lib.flowgnn_set_batch_device.argtypes) == 9
    assert _lib.LAYOUT_IDS == {"reference": 0, "pyg": 1}
    for name in ("set_batch_device", "set_batch_device_ptrs", "forward_device"):
        assert callable(getattr(Engine, name))


def _same(a: GraphBatch, b: GraphBatch):
    for f in ("nums_of_nodes", "nums_of_edges", "node_feature", "edge_list", "edge_attr"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype == np.int32 and np.array_equal(x, y), f
    assert (a.node_eigen is None) == (b.node_eigen is None)
    if a.node_eigen is not None:
        assert np.array_equal(a.node_eigen, b.node_eigen)


def test_to_pyg_layout_and_round_trip_numpy():
    b = gp.synth_molhiv_batch(40, seed=11)
    d = b.to_pyg()
    N, E, G = b.total_nodes, b.total_edges, b.num_graphs
    assert d["x"].dtype == np.int64 and d["x"].shape == (N, 9)
    assert d["edge_index"].dtype == np.int64 and d["edge_index"].shape == (2, E) and d["edge_index"].flags.c_contiguous
    assert d["edge_attr"].dtype == np.int64 and d["edge_attr"].shape == (E, 3)
    assert d["ptr"].dtype == np.int64 and d["ptr"].shape == (G + 1,) and d["ptr"][-1] == N
    # global ids: every edge's endpoints inside its graph's node range, source-major order kept
    gid = np.repeat(np.arange(G), b.nums_of_edges)
    lo, hi = d["ptr"][gid], d["ptr"][gid + 1]
    assert ((d["edge_index"] >= lo) & (d["edge_index"] < hi)).all()
    assert np.array_equal(d["edge_index"].T - lo[:, None], b.edge_list)
    _same(b, GraphBatch.from_pyg(**d))


def test_to_pyg_round_trip_with_eigen_and_edgeless_graphs():
    b = gp.synth_hep10k_batch(6, seed=2)
    # a graph with no edges in the middle and at the end
    one = GraphBatch(np.array([3], np.int32), np.array([0], np.int32), np.zeros((3, 9), np.int32), np.zeros((0, 2), np.int32),
                     np.zeros((0, 3), np.int32), np.zeros((3, 4), np.float32))
    b = gp.concat_batches([b.slice(0, 3), one, b.slice(3, 6), one])
    d = b.to_pyg()
    assert d["node_eigen"].dtype == np.float32 and d["node_eigen"].shape == (b.total_nodes, 4)
    _same(b, GraphBatch.from_pyg(**d))


def test_to_pyg_torch_cpu_tensors():
    torch = __import__("pytest").importorskip("torch")
    b = gp.synth_molpcba_batch(25, seed=4)
    t = b.to_pyg("cpu")
    assert t["x"].dtype == torch.int64 and t["edge_index"].shape == (2, b.total_edges) and t["edge_index"].is_contiguous()
    _same(b, GraphBatch.from_pyg(**{k: v.numpy() for k, v in t.items()}))
