"""The host-side plans of GCN, GAT, DGN and PNA (flowgnn_amd/csrc/gcn_plan.h, gat_plan.h, dgn_plan.h, pna_plan.h) from Python: plain C++, built with g++ and called through
ctypes (tests/resident_plan_shim.cpp).  Shared by test_resident_plan_cpu.py (the plan against the parent's conditions, on every input) and
test_resident_plan_gpu.py (the plan against what a run launches).

A set of cases is a dict of equally long numpy arrays, one per input field; `plan(lib, model, cases)` returns the same for the result fields."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flowgnn_amd", "csrc")
# both sides of the model's fill threshold for its graph-tile kernels, and the threshold
FILLS = {"GCN": np.array([0.49, 0.5, 0.51]), "GAT": np.array([0.49, 0.5, 0.51]), "DGN": np.array([0.39, 0.4, 0.41]), "PNA": np.array([0.39, 0.4, 0.41])}
DGN_JOB_N = 1000  # DGN's density rule (job_e >= 8 job_n) at one job_n: job_e = 8 job_n - 1 + density, density 0, 1, 2
PATHS = ["fixed_point", "resident", "per_layer"]  # enum class GcnPath / GatPath / DgnPath / PnaPath, in order
INSTANCES = {"GCN": ["default", "rows", "pool_sum", "node_logits"],  # enum class GcnResidentInstance, in order
             "GAT": ["default", "pool_sum", "attention", "node_logits"],  # enum class GatResidentInstance
             "DGN": ["default", "emb", "rows"], "PNA": ["default", "emb", "rows"]}  # enum class DgnResidentInstance / PnaResidentInstance
# (name, bits) in the order the shim unpacks / packs them
INPUTS = {"GCN": [(k, 1) for k in ("resident", "tile_build", "binpack", "split", "fused", "table_ok", "qmode", "keep_h", "exact", "tiles",
                                   "bp_lists", "edge_attr", "edges", "emb", "node_emb", "node_logits", "two_tasks")] + [("fill_i", 2), ("pooling", 2)],
          "GAT": [(k, 1) for k in ("resident", "fold_readout", "split", "qmode", "keep_h", "exact", "tiles", "emb", "node_emb", "node_logits",
                                   "attention")] + [("fill_i", 2), ("pooling", 2)],
          # mfma_agg: dgn_mfma_agg + 1 (-1, 0, 1); resident: dgn_resident (0, 1, 2)
          "DGN": [(k, 1) for k in ("fused", "split", "fold_readout", "rowinfo_direct", "binpack", "qmode", "keep_h", "exact", "nonempty", "eigen",
                                   "tiles", "bp_lists", "edges", "csr_built", "emb", "node_emb")]
                 + [("mfma_agg", 2), ("resident", 2), ("fill_i", 2), ("density", 2)],
          "PNA": [(k, 1) for k in ("fused", "split", "resident", "tile_build", "binpack", "qmode", "keep_h", "exact", "tiles", "bp_lists", "emb",
                                   "node_emb")] + [("fill_i", 2)]}
RESULTS = {"GCN": [("path", 2), ("instance", 2)] + [(k, 1) for k in ("needs_csr", "wants_packed_tile_lists", "one_pass", "bin_packed", "sum_from_rows",
                                                                    "fused_encoder", "fused_layers", "folded_last", "multi_task",
                                                                    "node_logits_from_scores", "pool_rows", "node_logits_from_rows")],
           "GAT": [("path", 2), ("instance", 2)] + [(k, 1) for k in ("split_products", "attention_kernels", "fold", "pool_rows",
                                                                    "node_logits_from_scores", "node_logits_from_rows")],
           "DGN": [("path", 2), ("instance", 2)] + [(k, 1) for k in ("needs_csr", "wants_packed_tile_lists", "bin_packed", "fused_layers",
                                                                    "mfma_aggregation", "rowinfo_from_edge_list", "first_layer_makes_rowinfo",
                                                                    "pooled_last", "prepare_aggregate", "edge_scalar", "split_dense", "emb_readout")],
           "PNA": [("path", 2), ("instance", 2)] + [(k, 1) for k in ("needs_csr", "wants_packed_tile_lists", "one_pass", "bin_packed", "fused_layers",
                                                                    "split_dense", "emb_readout")]}


def build_shim(directory):
    so = os.path.join(str(directory), "libresident_plan_test.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, "-o", so,
                           os.path.join(ROOT, "tests", "resident_plan_shim.cpp")])
    lib = C.CDLL(so)
    for fn in (lib.rp_gcn_bulk, lib.rp_gat_bulk, lib.rp_dgn_bulk, lib.rp_pna_bulk):
        fn.argtypes = [C.POINTER(C.c_uint32), C.c_longlong, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        fn.restype = None
    return lib


def full_product(model):
    """Every combination of the model's inputs: each flag both ways, each two-bit input (fill_i over FILLS, pooling, DGN's mfma_agg,
    resident and density) over 0, 1, 2."""
    sizes = [3 if bits == 2 else 2 for _, bits in INPUTS[model]]
    grid = np.indices(sizes, dtype=np.uint8).reshape(len(sizes), -1)
    return {k: grid[i] for i, (k, _) in enumerate(INPUTS[model])}


def plan(lib, model, cases):
    n = len(next(iter(cases.values())))
    words, at = np.zeros(n, np.uint32), 0
    for k, bits in INPUTS[model]:
        words |= np.asarray(cases[k]).astype(np.uint32) << np.uint32(at)
        at += bits
    out = np.zeros(n, np.uint32)
    assert at <= 32
    fn = getattr(lib, f"rp_{model.lower()}_bulk")
    fn(words.ctypes.data_as(C.POINTER(C.c_uint32)), n, FILLS[model].ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    res, at = {}, 0
    for k, bits in RESULTS[model]:
        v = (out >> np.uint32(at)) & np.uint32((1 << bits) - 1)
        res[k] = v.astype(np.uint8) if bits > 1 else v.astype(bool)
        at += bits
    return res


def plan_one(lib, model, **inputs):
    """The plan of one case as {field: value}; inputs left out are 0 -- pass every field that matters."""
    cases = {k: np.array([int(inputs.pop(k, 0))]) for k, _ in INPUTS[model]}
    assert not inputs, f"unknown plan inputs {sorted(inputs)}"
    return {k: v[0].item() for k, v in plan(lib, model, cases).items()}
