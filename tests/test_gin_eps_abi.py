"""A trained eps for GIN / GIN-VN (flowgnn.h: flowgnn_set_gin_eps): what can be checked without a GPU -- the header, the library's
exports, the null-handle and wrong-model answers, the ctypes prototypes, the Python wrappers, the host CLI's flag and the build lists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flowgnn_amd
from flowgnn_amd import Engine, EngineGroup, _lib, engine, export, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_set_gin_eps", "flowgnn_gin_eps", "flowgnn_group_set_gin_eps", "flowgnn_entry_set_gin_eps"]


def test_header_declares_the_four_functions():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    for f in FUNCS:
        assert re.search(r"^int " + f + r"\(", text, re.M), f
    assert re.search(r"^int flowgnn_set_gin_eps\(flowgnn_engine\* e, const float\* eps", text, re.M)
    assert re.search(r"^int flowgnn_gin_eps\(const flowgnn_engine\* e, float\* eps_out", text, re.M)
    assert re.search(r"^int flowgnn_group_set_gin_eps\(flowgnn_group\* g, const float\* eps\);", text, re.M)
    assert re.search(r"^int flowgnn_entry_set_gin_eps\(int model, const float\* eps\);", text, re.M)


def test_library_exports_them_and_null_handles_answer():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f), f
    null = C.c_void_p()
    five = (C.c_float * 5)(0.1, 0.2, 0.3, 0.4, 0.5)
    assert lib.flowgnn_set_gin_eps(null, five) == 1
    assert lib.flowgnn_gin_eps(null, None) == -1
    assert lib.flowgnn_group_set_gin_eps(null, five) == 1
    # the entry points' setting has no handle: a model that does not exist is an argument error, a model without the term refuses,
    # a value that is not finite is an argument error; NULL (off) is accepted for GIN and GIN-VN
    assert lib.flowgnn_entry_set_gin_eps(99, five) == 1
    for m in ("GCN", "GAT", "PNA", "DGN"):
        assert lib.flowgnn_entry_set_gin_eps(_lib.MODEL_IDS[m], five) == 8, m
    nan = (C.c_float * 5)(0.0, float("nan"), 0.0, 0.0, 0.0)
    inf = (C.c_float * 5)(0.0, 0.0, 0.0, float("inf"), 0.0)
    assert lib.flowgnn_entry_set_gin_eps(_lib.MODEL_IDS["GIN"], nan) == 1
    assert lib.flowgnn_entry_set_gin_eps(_lib.MODEL_IDS["GIN-VN"], inf) == 1
    assert lib.flowgnn_entry_set_gin_eps(_lib.MODEL_IDS["GIN"], None) == 0
    assert lib.flowgnn_entry_set_gin_eps(_lib.MODEL_IDS["GIN-VN"], None) == 0


def test_prototypes():
    lib = _lib.load()
    assert lib.flowgnn_set_gin_eps.argtypes == [C.c_void_p, _lib.p_float]
    assert lib.flowgnn_gin_eps.argtypes == [C.c_void_p, _lib.p_float]
    assert lib.flowgnn_group_set_gin_eps.argtypes == [C.c_void_p, _lib.p_float]
    assert lib.flowgnn_entry_set_gin_eps.argtypes == [C.c_int, _lib.p_float]
    for f in FUNCS:
        assert getattr(lib, f).restype == C.c_int, f


def test_python_wrappers_exist():
    for name in ("set_gin_eps", "gin_eps"):
        assert callable(getattr(Engine, name)), name
    assert callable(EngineGroup.set_gin_eps)
    assert callable(engine.entry_set_gin_eps) and flowgnn_amd.entry_set_gin_eps is engine.entry_set_gin_eps
    assert callable(weights.load_gin_eps) and callable(export.gin_eps_from_ogb_state_dict)
    import inspect
    assert inspect.signature(Engine.load_weights_dir).parameters["eps"].default is False
    assert inspect.signature(weights.save_gin_weights).parameters["eps"].default is None
    assert inspect.signature(export.export_weights).parameters["keep_eps"].default is False
    assert inspect.signature(export.gin_weights_from_ogb_state_dict).parameters["keep_eps"].default is False


def test_eps_argument_wants_five_values():
    assert engine._eps_arg(None) is None
    a = engine._eps_arg(np.array([1, 2, 3, 4, 5], np.float64))
    assert list(a) == [1.0, 2.0, 3.0, 4.0, 5.0]
    with pytest.raises(ValueError):
        engine._eps_arg([0.0] * 4)


def test_host_cli_knows_the_flag():
    text = open(os.path.join(ROOT, "flowgnn_amd", "csrc", "host_main.cpp")).read()
    assert '"--eps"' in text and "[--eps]" in text and "gin_ep1_eps_dim100.bin" in text and "flowgnn_group_set_gin_eps" in text


def test_the_build_lists_agree():
    """The eps instances' translation unit is in the Makefile's SRCS, in scripts/dev/devlib.sh's list and named in variant.sh."""
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    make = open(os.path.join(src, "Makefile")).read()
    units = re.search(r"^SRCS := (.*)$", make, re.M).group(1).split()
    loop = re.search(r"^for f in (.*); do$", open(os.path.join(ROOT, "scripts", "dev", "devlib.sh")).read(), re.M).group(1).split()
    assert sorted(u[:-len(".hip")] for u in units) == sorted(loop)
    assert "gin_split_eps.hip" in units and os.path.exists(os.path.join(src, "gin_split_eps.hip"))
    assert re.search(r"^gin_split_eps\.o: gin_split\.hip$", make, re.M)
    assert "gin_split_eps" in open(os.path.join(ROOT, "scripts", "dev", "variant.sh")).read()
