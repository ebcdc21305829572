"""Attention coefficients (flowgnn.h: flowgnn_set_attention): what can be checked without a GPU -- the header, the library's exports,
flowgnn_attention_shape's values and refusals, the null-handle answers, the Python wrappers and the host CLI's flags."""
import ctypes as C
import inspect
import os
import re

import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, _lib, attention_shape
from flowgnn_amd.engine import attention_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_attention_shape", "flowgnn_set_attention", "flowgnn_get_attention", "flowgnn_attention_device",
         "flowgnn_set_attention_buffers", "flowgnn_group_set_attention", "flowgnn_group_get_attention"]


def test_header_declares_the_functions():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    for f in FUNCS:
        assert re.search(r"^int " + f + r"\(", text, re.M), f


def test_library_exports_them_and_null_handles_are_argument_errors():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f), f
        assert getattr(lib, f).restype == C.c_int, f
    null, p, q = C.c_void_p(), C.c_void_p(), C.c_void_p()
    buf = (C.c_float * 4)()
    assert lib.flowgnn_set_attention(null, 16) == 1
    assert lib.flowgnn_get_attention(null, buf, buf) == 1
    assert lib.flowgnn_attention_device(null, C.byref(p), C.byref(q)) == 1
    assert lib.flowgnn_set_attention_buffers(null, None, None) == 1
    assert lib.flowgnn_group_set_attention(null, 16) == 1
    assert lib.flowgnn_group_get_attention(null, buf, buf) == 1


def test_attention_shape_needs_no_gpu():
    lib = _lib.load()
    layers, heads = C.c_int(-1), C.c_int(-1)
    assert lib.flowgnn_attention_shape(_lib.MODEL_IDS["GAT"], C.byref(layers), C.byref(heads)) == 0
    assert (layers.value, heads.value) == (5, 4)
    assert lib.flowgnn_attention_shape(_lib.MODEL_IDS["GAT"], None, None) == 0
    for model in ("GIN", "GIN-VN", "GCN", "PNA", "DGN"):
        layers.value = heads.value = -1
        assert lib.flowgnn_attention_shape(_lib.MODEL_IDS[model], C.byref(layers), C.byref(heads)) == 8, model
        assert (layers.value, heads.value) == (-1, -1)
        with pytest.raises(FlowGNNError) as ei:
            attention_shape(model)
        assert ei.value.code == 8
    assert lib.flowgnn_attention_shape(12345, C.byref(layers), C.byref(heads)) == 8
    assert attention_shape("gat") == (5, 4)


def test_layer_selection_to_mask():
    assert attention_mask("GAT", "all") == 31 and attention_mask("GAT", "last") == 16
    assert attention_mask("GAT", None) == 0 and attention_mask("GAT", False) == 0
    assert attention_mask("GAT", [0, 4]) == 0b10001 and attention_mask("GAT", (4,)) == 16 and attention_mask("GAT", range(5)) == 31
    for bad in ("first", [5], [-1], [1.5]):
        with pytest.raises(ValueError):
            attention_mask("GAT", bad)


def test_python_wrappers_exist():
    for name in ("set_attention", "attention", "attention_device_ptrs", "set_attention_buffers"):
        assert callable(getattr(Engine, name)), name
    for name in ("set_attention", "attention"):
        assert callable(getattr(EngineGroup, name)), name
    assert inspect.signature(Engine.forward).parameters["return_attention"].default is None
    assert inspect.signature(Engine.forward_device).parameters["return_attention"].default is None


def test_host_cli_knows_the_flags():
    text = open(os.path.join(ROOT, "flowgnn_amd", "csrc", "host_main.cpp")).read()
    assert '"--attention"' in text and '"--attention-layers"' in text and "[--attention FILE [--attention-layers MASK]]" in text


def test_the_build_lists_the_new_translation_unit():
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    assert os.path.exists(os.path.join(src, "gat_attn.hip"))
    assert "gat_attn.hip" in open(os.path.join(src, "Makefile")).read()
    assert "gat_attn" in open(os.path.join(ROOT, "scripts", "dev", "devlib.sh")).read()
