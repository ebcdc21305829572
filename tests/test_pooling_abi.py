"""Readout pooling (flowgnn.h: flowgnn_set_pooling): what can be checked without a GPU -- the header, the library's exports, the
null-handle answers, the ctypes prototypes, the Python wrappers, the mode names and the host CLI's flag."""
import ctypes as C
import os
import re

import flowgnn_amd
from flowgnn_amd import Engine, EngineGroup, _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["flowgnn_set_pooling", "flowgnn_pooling", "flowgnn_group_set_pooling", "flowgnn_entry_set_pooling"]
CONSTANTS = {"FLOWGNN_POOL_MEAN": 0, "FLOWGNN_POOL_SUM": 1, "FLOWGNN_POOL_MAX": 2}


def test_header_declares_the_four_functions_and_three_constants():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    for f in FUNCS:
        assert re.search(r"^int " + f + r"\(", text, re.M), f
    for name, value in CONSTANTS.items():
        assert re.search(r"^#define " + name + r"\s+" + str(value) + r"\b", text, re.M), name
    assert re.search(r"^int flowgnn_pooling\(const flowgnn_engine\* e\);", text, re.M)


def test_library_exports_them_and_null_handles_answer():
    lib = _lib.load()
    for f in FUNCS:
        assert hasattr(lib, f), f
    null = C.c_void_p()
    assert lib.flowgnn_set_pooling(null, 1) == 1
    assert lib.flowgnn_pooling(null) == -1
    assert lib.flowgnn_group_set_pooling(null, 1) == 1
    # the entry points' setting has no handle: a model or a mode that does not exist is an argument error, PNA / DGN refuse the others
    assert lib.flowgnn_entry_set_pooling(99, 0) == 1
    assert lib.flowgnn_entry_set_pooling(0, 3) == 1 and lib.flowgnn_entry_set_pooling(0, -1) == 1
    assert lib.flowgnn_entry_set_pooling(_lib.MODEL_IDS["PNA"], 1) == 8 and lib.flowgnn_entry_set_pooling(_lib.MODEL_IDS["DGN"], 2) == 8
    assert lib.flowgnn_entry_set_pooling(_lib.MODEL_IDS["PNA"], 0) == 0


def test_prototypes():
    lib = _lib.load()
    assert lib.flowgnn_set_pooling.argtypes == lib.flowgnn_set_numeric_mode.argtypes
    assert lib.flowgnn_group_set_pooling.argtypes == lib.flowgnn_group_set_numeric_mode.argtypes
    assert lib.flowgnn_pooling.argtypes == lib.flowgnn_num_tasks.argtypes
    assert lib.flowgnn_entry_set_pooling.argtypes == [C.c_int, C.c_int]
    for f in FUNCS:
        assert getattr(lib, f).restype == C.c_int, f


def test_python_wrappers_exist():
    for name in ("set_pooling", "pooling"):
        assert callable(getattr(Engine, name)), name
    assert callable(EngineGroup.set_pooling)
    assert callable(engine.entry_set_pooling) and flowgnn_amd.entry_set_pooling is engine.entry_set_pooling


def test_pooling_modes_has_the_three_names():
    assert engine.POOLING_MODES == {"mean": 0, "sum": 1, "max": 2}
    assert list(engine.POOLING_MODES) == ["mean", "sum", "max"]


def test_host_cli_knows_the_flag():
    text = open(os.path.join(ROOT, "flowgnn_amd", "csrc", "host_main.cpp")).read()
    assert '"--pooling"' in text and "[--pooling mean|sum|max]" in text


def test_the_build_lists_agree():
    """Every translation unit of the Makefile's SRCS is in scripts/dev/devlib.sh's list too (the default units call into the pooling
    instances' launchers, so a development library without them does not load), and the four new ones exist."""
    src = os.path.join(ROOT, "flowgnn_amd", "csrc")
    make = open(os.path.join(src, "Makefile")).read()
    units = re.search(r"^SRCS := (.*)$", make, re.M).group(1).split()
    loop = re.search(r"^for f in (.*); do$", open(os.path.join(ROOT, "scripts", "dev", "devlib.sh")).read(), re.M).group(1).split()
    assert sorted(u[:-len(".hip")] for u in units) == sorted(loop)
    for u in ("gin_split_poolsum", "gin_split_poolmax", "gcn_poolsum", "gat_poolsum"):
        assert u + ".hip" in units and os.path.exists(os.path.join(src, u + ".hip")), u
