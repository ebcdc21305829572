"""Node logits (flowgnn.h: flowgnn_set_node_logits): what can be checked without a GPU -- the header, the library's exports, the
null-handle answers, the ctypes prototypes, the Python wrappers and the host CLI's flag."""
import ctypes as C
import inspect
import os
import re

from flowgnn_amd import Engine, EngineGroup, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_set_node_logits", "flowgnn_get_node_logits", "flowgnn_node_logits_device", "flowgnn_set_node_logits_buffer",
         "flowgnn_group_set_node_logits", "flowgnn_group_get_node_logits"]


def test_header_declares_the_six_functions():
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
    assert lib.flowgnn_set_node_logits(null, 1) == 1
    assert lib.flowgnn_get_node_logits(null, buf) == 1
    assert lib.flowgnn_node_logits_device(null, C.byref(p)) == 1
    assert lib.flowgnn_set_node_logits_buffer(null, None) == 1
    assert lib.flowgnn_group_set_node_logits(null, 1) == 1
    assert lib.flowgnn_group_get_node_logits(null, buf) == 1


def test_prototypes_mirror_the_node_embedding_calls():
    lib = _lib.load()
    for f in FUNCS:
        twin = getattr(lib, f.replace("node_logits", "node_embeddings"))
        assert getattr(lib, f).argtypes == twin.argtypes and getattr(lib, f).restype == twin.restype == C.c_int, f


def test_python_wrappers_exist():
    for name in ("set_node_logits", "node_logits", "node_logits_device_ptr", "set_node_logits_buffer"):
        assert callable(getattr(Engine, name)), name
    for name in ("set_node_logits", "node_logits"):
        assert callable(getattr(EngineGroup, name)), name
    assert inspect.signature(Engine.forward).parameters["return_node_logits"].default is False
    assert inspect.signature(Engine.forward_device).parameters["return_node_logits"].default is False


def test_host_cli_knows_the_flag():
    text = open(os.path.join(ROOT, "flowgnn_amd", "csrc", "host_main.cpp")).read()
    assert '"--node-logits"' in text and "[--node-logits FILE]" in text
