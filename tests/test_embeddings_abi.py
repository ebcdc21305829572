"""Graph embeddings (flowgnn.h: flowgnn_set_embeddings): what can be checked without a GPU -- the header, the library's exports, the
null-handle answers, flowgnn_embedding_dim, the Python wrappers and the host CLI's flag."""
import ctypes as C
import os
import re

import flowgnn_amd
from flowgnn_amd import Engine, EngineGroup, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_embedding_dim", "flowgnn_set_embeddings", "flowgnn_get_embeddings", "flowgnn_embeddings_device",
         "flowgnn_set_embeddings_buffer", "flowgnn_group_set_embeddings", "flowgnn_group_get_embeddings"]


def test_header_declares_the_functions():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    for f in FUNCS:
        assert re.search(r"^int " + f + r"\(", text, re.M), f


def test_library_exports_them_and_null_handles_are_argument_errors():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f), f
    null = C.c_void_p()
    p = C.c_void_p()
    buf = (C.c_float * 4)()
    assert lib.flowgnn_set_embeddings(null, 1) == 1
    assert lib.flowgnn_get_embeddings(null, buf) == 1
    assert lib.flowgnn_embeddings_device(null, C.byref(p)) == 1
    assert lib.flowgnn_set_embeddings_buffer(null, None) == 1
    assert lib.flowgnn_group_set_embeddings(null, 1) == 1
    assert lib.flowgnn_group_get_embeddings(null, buf) == 1


def test_embedding_dim_needs_no_gpu():
    lib = _lib.load()
    assert [lib.flowgnn_embedding_dim(m) for m in range(7)] == [100, 100, 100, 16, 80, 100, -1]
    assert [flowgnn_amd.embedding_dim(m) for m in ("GIN", "GIN-VN", "GCN", "GAT", "PNA", "DGN")] == [100, 100, 100, 16, 80, 100]


def test_python_wrappers_exist():
    for name in ("set_embeddings", "embeddings", "embeddings_device_ptr", "set_embeddings_buffer"):
        assert callable(getattr(Engine, name)), name
    for name in ("set_embeddings", "embeddings"):
        assert callable(getattr(EngineGroup, name)), name
    import inspect
    assert inspect.signature(Engine.forward).parameters["return_embeddings"].default is False
    assert inspect.signature(Engine.forward_device).parameters["return_embeddings"].default is False
    assert "embedding_dim" in flowgnn_amd.__all__


def test_host_cli_knows_the_flag():
    assert '"--embeddings"' in open(os.path.join(ROOT, "flowgnn_amd", "csrc", "host_main.cpp")).read()
