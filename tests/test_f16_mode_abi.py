"""The f16 numeric mode's public surface without a GPU: the header's mode code, the Python bindings' mapping to it, and the host
binary's --numeric choice."""
import ctypes
import os
import re

import pytest

from flowgnn_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "flowgnn_amd", "libflowgnn_hip.so")
HEADER = os.path.join(ROOT, "include", "flowgnn.h")


def header_modes():
    src = open(HEADER).read()
    return {m: int(v) for m, v in re.findall(r"^#define FLOWGNN_NUMERIC_(\w+)\s+(\d+)\s*$", src, flags=re.M)}


def test_header_defines_f16_mode():
    assert header_modes() == {"F32": 0, "Q6_10": 1, "F16": 2}


def test_python_bindings_map_f16_to_the_header_code():
    modes = header_modes()
    assert engine.NUMERIC_MODES == {"f32": modes["F32"], "q6.10": modes["Q6_10"], "f16": modes["F16"]}


def test_host_binary_knows_f16():
    src = open(os.path.join(ROOT, "flowgnn_amd", "csrc", "host_main.cpp")).read()
    assert '"f16" ? FLOWGNN_NUMERIC_F16' in src


@pytest.mark.skipif(not os.path.exists(LIB), reason="libflowgnn_hip.so not built (run __graft_entry__.build())")
def test_null_engine_is_rejected_for_every_mode():
    lib = ctypes.CDLL(LIB)
    lib.flowgnn_set_numeric_mode.argtypes = [ctypes.c_void_p, ctypes.c_int]
    for mode in header_modes().values():
        assert lib.flowgnn_set_numeric_mode(None, mode) == 1  # FLOWGNN_ERR_ARG
