"""Laplacian eigenvectors (flowgnn.h: flowgnn_laplacian_eigen*): what can be checked without a GPU -- the header, the library's
exports, the limit, the null-handle answers, the ctypes prototypes, the Python wrappers, the host CLI's flag and the build lists."""
import ctypes as C
import os
import re

import flowgnn_amd
from flowgnn_amd import Engine, _lib, engine, graphpack as gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_laplacian_eigen_max_nodes", "flowgnn_laplacian_eigen", "flowgnn_laplacian_eigen_device"]


def test_header_declares_the_functions_and_the_limit():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    for f in FUNCS:
        assert re.search(r"^int " + f + r"\(", text, re.M), f
    assert re.search(r"^#define FLOWGNN_EIGEN_MAX_NODES\s+128\b", text, re.M)
    assert re.search(r"^int flowgnn_laplacian_eigen_max_nodes\(void\);", text, re.M)


def test_library_exports_them_and_the_limit_needs_no_gpu():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f), f
        assert getattr(lib, f).restype == C.c_int, f
    assert lib.flowgnn_laplacian_eigen_max_nodes() == 128
    assert engine.laplacian_eigen_max_nodes() == 128 and flowgnn_amd.laplacian_eigen_max_nodes is engine.laplacian_eigen_max_nodes
    assert gp.LAPLACIAN_EIGEN_MAX_NODES == 128


def test_null_engine_is_an_argument_error():
    lib = _lib.load()
    null = C.c_void_p()
    nn, ne = (C.c_int * 1)(2), (C.c_int * 1)(1)
    el = (C.c_int * 2)(0, 1)
    out = (C.c_float * 8)()
    assert lib.flowgnn_laplacian_eigen(null, 1, nn, ne, el, out) == 1
    assert lib.flowgnn_laplacian_eigen_device(null, 1, nn, ne, 0, None, None) == 1
    assert lib.flowgnn_laplacian_eigen(null, 0, None, None, None, None) == 1
    assert not any(out)


def test_prototypes():
    lib = _lib.load()
    eng = C.c_void_p
    assert lib.flowgnn_laplacian_eigen_max_nodes.argtypes in ([], None)
    assert lib.flowgnn_laplacian_eigen.argtypes == [eng, C.c_int, _lib.p_int, _lib.p_int, _lib.p_int, _lib.p_float]
    assert lib.flowgnn_laplacian_eigen_device.argtypes == [eng, C.c_int, _lib.p_int, _lib.p_int, C.c_int, C.c_void_p, C.c_void_p]


def test_python_wrappers_exist():
    for name in ("laplacian_eigen", "laplacian_eigen_device", "laplacian_eigen_device_ptrs"):
        assert callable(getattr(Engine, name)), name
    assert callable(gp.laplacian_eigen) and callable(gp.normalized_laplacian)


def test_host_cli_knows_the_flag():
    text = open(os.path.join(ROOT, "flowgnn_amd", "csrc", "host_main.cpp")).read()
    assert '"--compute-eig"' in text and "flowgnn_laplacian_eigen(" in text


def test_the_kernel_file_is_in_both_build_lists():
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    units = re.search(r"^SRCS := (.*)$", open(os.path.join(src, "Makefile")).read(), re.M).group(1).split()
    loop = re.search(r"^for f in (.*); do$", open(os.path.join(ROOT, "scripts", "dev", "devlib.sh")).read(), re.M).group(1).split()
    assert "eigen.hip" in units and "eigen" in loop and os.path.exists(os.path.join(src, "eigen.hip"))
