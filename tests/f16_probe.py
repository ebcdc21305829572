"""The cases of the f16 exactness probe (tests/test_f16_probe_gpu.py) and their float64 references, shared with the CPU tests that show
what the probe can prove (tests/test_f16_ref_cpu.py).  No GPU here.

A case is one engine configuration in FLOWGNN_NUMERIC_F16 that reaches one F16 instance of gin_split.hip's kernels; its inputs are the
dyadic weights and the power-of-two-sized molecules of tests/test_f16_mode_gpu.py (probe_weights, probe_batch), on which every fp32 sum
of the mode is exact -- tests/f16_ref.gin_forward(check=True) proves it per input, and a case whose figure exceeded 2^24 would prove
nothing.  The batch of every case but one carries a one-node graph in front and behind and a graph without edges in the middle (node
counts 1, 2 and 4 are powers of two as well, so the mean cases keep their exact division).

What tells a right instance from a wrong one is the separation among the references themselves: the `rne` forward (the mode) against
  rtz                      the same with the activations (a, hidden units) rounded toward zero,
  none                     the unrounded forward (what the f32 mode computes),
  a not rounded, hidden units not rounded, weights not rounded, weights rounded toward zero
                           the mode's forward with that one operand point treated otherwise,
  u not rounded, u rounded toward zero       the same for the folded head u = W2^T w, where the readout is the folded one,
and, where the case has a trained eps,
  eps all zero, eps layers 1 and 2 swapped, last eps layer zeroed.
A pair SEPARATES when more than half of the elements differ by more than 100 x the probe's bound 1e-6 (1 + |want|) and the median
does too.  `separation(model, case)` computes that per output and variant; the GPU test asserts exactly the pairs that separate here,
and the pairs that do not are the named list NOT_SEPARATED below, with the fraction the references reached -- the CPU test holds the
list to the computed table in both directions, so no pair can drop out of the GPU test unnamed."""
import functools
from collections import namedtuple

import numpy as np

from flowgnn_amd import graphpack as gp
from tests import f16_ref
from tests.test_f16_mode_gpu import probe_batch, probe_weights
from tests.test_resident_limits_gpu import random_graph

MODELS = ["GIN", "GIN-VN"]
EPS = [0.5, -0.25, 0.25, -0.5, 0.5]  # s_l = 1 + eps[l] of two bits, all five unlike 1, both signs: s_l h stays an fp32 value
WRONG_EPS = {
    "eps all zero": [0.0] * 5,
    "eps layers 1 and 2 swapped": [0.5, 0.25, -0.25, -0.5, 0.5],
    "last eps layer zeroed": [0.5, -0.25, 0.25, -0.5, 0.0],
}
WRONG_POINT = {  # the mode's forward with ONE operand point (f16_ref.POINTS) treated otherwise; u on the folded path only
    "a not rounded": ("a", "none"),
    "hidden units not rounded": ("hid", "none"),
    "weights not rounded": ("w", "none"),
    "weights rounded toward zero": ("w", "rtz"),
    "u not rounded": ("u", "none"),
    "u rounded toward zero": ("u", "rtz"),
}
FACTOR = 100.0  # of the bound, as tests/test_f16_mode_gpu.py::test_exactness_probe has it

Case = namedtuple("Case", "name kind options fwd pooling eps tasks fold batch models")


def case(name, kind, options=None, fwd=(), pooling="mean", eps=False, tasks=1, fold=False, batch="extra", models=tuple(MODELS)):
    """kind: "resident" (the launch check wants gin_resident and no per-layer slot) or "per_layer" (the opposite); fwd: the forward's
    return_* switches; fold: the readout rule of tests/f16_ref.py that the path's written definition names (flowgnn.h)."""
    return Case(name, kind, dict(options or {}), tuple(fwd), pooling, eps, tasks, fold, batch, tuple(models))


EMB, ROWS, TERMS = "return_embeddings", "return_node_embeddings", "return_node_logits"
OUTPUT_OF = {EMB: "pooled", ROWS: "rows", TERMS: "terms"}  # forward switch -> output name of f16_ref.gin_forward

# Instance of gin_split.hip with F16 = true  <-  the case(s) that reach it (GIN: HUBS = false, GIN-VN: HUBS = true; launch_gin_resident
# and launch_gin_layer_split, every f16 branch):
#   gin_resident_f16_kernel, folded, ENC = true (one-pass front end)     test_f16_mode_gpu.py::test_exactness_probe one_pass / gin_vn; "binpack 0"
#   gin_resident_f16_kernel, folded, ENC = false (gin_tile_build 0)       "tile build 0"
#   gin_resident_f16_kernel, un-folded, h_5 rows to HBM                   "node embeddings", "sum, graph embeddings" (test_exactness_probe multi_task_csr)
#   gin_resident_pool_kernel<HUBS, F16>                                   "graph embeddings"
#   gin_resident_poolmax_kernel<HUBS, F16>                                "max", "max, graph embeddings"
#   gin_resident_poolsum_kernel<HUBS, ENC, F16>, ENC = true / false       "sum, tile build 1" / "sum, tile build 0"
#   gin_resident_nlogit_kernel<HUBS, ENC, F16>, ENC = true / false        "node logits, tile build 1" / "node logits, tile build 0"
#   gin_resident_eps_kernel<HUBS, ENC, F16>, ENC = true / false           "eps, tile build 1" / "eps, tile build 0"
#   gin_layer_split_f16_kernel<1, 8> (launch_gin_layer_split_f16)         "gin_resident 0" (GIN also: test_exactness_probe per_layer)
#   gin_layer_split_eps_kernel<1, 8, true>, folded last stage             "eps, gin_resident 0", "eps, sum", "eps, node logits"
#   gin_layer_split_eps_kernel<1, 8, true>, rows out of the last layer    "eps, max" (and below the fill threshold), "eps, graph embeddings", "eps, sum, graph embeddings", "eps, node embeddings",
#                                                                         "eps, NUM_TASK 2", "eps, gin_fold_readout 0"
#   gin_layer_split_eps_kernel<2, 4, true> / <1, 4, true>                 "eps, gin_split_nt 2" / "eps, gin_split_nt 1"
CASES = [
    # ---- graph-resident
    case("tile build 0", "resident", {"gin_tile_build": 0}, fold=True),
    case("binpack 0", "resident", {"gin_binpack": 0}, fold=True),
    case("graph embeddings", "resident", fwd=[EMB]),
    case("node embeddings", "resident", fwd=[ROWS]),
    case("node logits, tile build 1", "resident", {"gin_tile_build": 1}, fwd=[TERMS], fold=True),
    case("node logits, tile build 0", "resident", {"gin_tile_build": 0}, fwd=[TERMS], fold=True),
    case("sum, tile build 1", "resident", {"gin_tile_build": 1}, pooling="sum", fold=True),
    case("sum, tile build 0", "resident", {"gin_tile_build": 0}, pooling="sum", fold=True),
    case("sum, graph embeddings", "resident", fwd=[EMB], pooling="sum"),
    case("max", "resident", pooling="max"),
    case("max, graph embeddings", "resident", fwd=[EMB], pooling="max"),
    case("eps, tile build 1", "resident", {"gin_tile_build": 1}, eps=True, fold=True),
    case("eps, tile build 0", "resident", {"gin_tile_build": 0}, eps=True, fold=True),
    # ---- per-layer
    case("gin_resident 0", "per_layer", {"gin_resident": 0}),
    case("eps, gin_resident 0", "per_layer", {"gin_resident": 0}, eps=True),
    case("eps, sum", "per_layer", pooling="sum", eps=True),
    case("eps, sum, graph embeddings", "per_layer", fwd=[EMB], pooling="sum", eps=True),
    case("eps, max", "per_layer", pooling="max", eps=True),
    case("eps, graph embeddings", "per_layer", fwd=[EMB], eps=True),
    case("eps, node embeddings", "per_layer", fwd=[ROWS], eps=True),
    case("eps, node logits", "per_layer", fwd=[TERMS], eps=True),
    case("eps, NUM_TASK 2", "per_layer", eps=True, tasks=2),
    case("eps, gin_fold_readout 0", "per_layer", {"gin_fold_readout": 0}, eps=True),
    case("eps, gin_split_nt 2", "per_layer", {"gin_resident": 0, "gin_split_nt": 2}, eps=True, models=["GIN"]),
    case("eps, gin_split_nt 1", "per_layer", {"gin_resident": 0, "gin_split_nt": 1}, eps=True, models=["GIN"]),
    # eight graphs of 120 nodes and 650 edges: one per tile by the edge limit (1 280), 47 % full -- under the fill threshold, so the
    # per-layer kernels take the batch with no option set.  The maximum, because a mean or a sum over 120 nodes averages the mode's
    # roundings out (such logits separate from the unrounded forward on half of the graphs only), and sparser graphs would share a
    # tile while denser ones leave the exact range (100 nodes, 700 edges: 2^24.4).  GIN only: a virtual node over 120 nodes leaves it too.
    case("eps, max, graph embeddings, below the fill threshold", "per_layer", fwd=[EMB], pooling="max", eps=True, batch="below_fill", models=["GIN"]),
]
PARAMS = [(m, c) for c in CASES for m in c.models]
IDS = [f"{m}-{c.name}" for m, c in PARAMS]


def outputs_of(c):
    return ("logits",) + tuple(OUTPUT_OF[k] for k in c.fwd)


@functools.lru_cache(maxsize=None)
def batch_of(model, kind):
    if kind == "below_fill":
        assert model == "GIN"
        return gp.concat_batches([random_graph(120, 650, seed=s) for s in range(8)])
    return probe_batch(model == "GIN-VN", extra=True)


@functools.lru_cache(maxsize=None)
def weights_of(tasks):
    """the probe's weights in the form on which the rounding of the weights and of u shows (probe_weights says how)"""
    return probe_weights(num_tasks=tasks, tight=True)


def case_weights(c):
    return weights_of(c.tasks)


@functools.lru_cache(maxsize=None)
def _forward(model, batch, tasks, fold, pooling, rnd, eps, check=True):
    """(every output the rule has, exactness figure or None): computed once per distinct reference and left unchanged"""
    fold = fold and tasks == 1 and pooling != "max"
    names = ("logits", "terms") if fold else f16_ref.OUTPUTS
    if batch == "below_fill":
        names = ("logits", "pooled")  # (what the case returns: no per-graph sums over 120 nodes in the check)
    rnd = rnd if isinstance(rnd, str) else dict(rnd)  # (a tuple of (operand point, rounding) pairs: hashable)
    res = f16_ref.gin_forward(batch_of(model, batch), weights_of(tasks), fold=fold, rnd=rnd, check=check, eps=None if eps is None else list(eps),
                              pooling=pooling, outputs=names)
    out, worst = res if check else (res, None)
    for a in out.values():
        a.setflags(write=False)
    return out, worst


def references(model, c):
    """variant -> (outputs, exactness figure or None): "rne" (the expected values), "rtz", "none", the forwards that are wrong at one
    operand point and, with eps, the three wrong-eps forwards"""
    eps = tuple(EPS) if c.eps else None
    key = (model, c.batch, c.tasks, c.fold, c.pooling)
    refs = {"rne": _forward(*key, "rne", eps)}
    # (rtz rounds the MLP's activations toward zero and leaves the weights and u as the mode has them -- those toward zero are variants
    # of their own, and no fp32-exact ones: such a weight has eleven bits where the mode's has one or two)
    refs["rtz"] = _forward(*key, (("a", "rtz"), ("hid", "rtz")), eps)
    refs["none"] = _forward(*key, "none", eps, False)  # (what fp32 approximates to 1e-5, not what it reproduces: no figure)
    for name, (point, how) in WRONG_POINT.items():
        if point != "u" or c.fold:
            refs[name] = _forward(*key, ((point, how),), eps, False)
    if c.eps:
        for name, wrong in WRONG_EPS.items():
            refs[name] = _forward(*key, "rne", tuple(wrong))
    return refs


def bound(want):
    return 1e-6 * (1.0 + np.abs(want))


def separated(got, other, want):
    """(the pair passes the probe's criterion, fraction of elements beyond FACTOR x the bound, median ratio to the bound)"""
    sep = np.abs(np.asarray(got, np.float64) - other) / bound(want)
    frac, med = float(np.mean(sep > FACTOR)), float(np.median(sep))
    return frac > 0.5 and med > FACTOR, frac, med


def separation(model, c):
    """(output, variant) -> (passes, fraction, median) of the references among themselves, for the outputs the case returns"""
    refs = references(model, c)
    want = refs["rne"][0]
    return {(o, v): separated(want[o], refs[v][0][o], want[o]) for o in outputs_of(c) for v in refs if v != "rne"}


# The pairs that do NOT separate, by name, with the fraction of elements the references reached (tests/test_f16_ref_cpu.py holds this
# list to the computed table in both directions; every other pair is asserted on the GPU).  A logit pair, or a rows / pooled vector
# against rtz, may never be listed: those must separate in every case.  What is listed are vectors against a forward that leaves ONE
# activation unrounded: many entries of a are f16 values as they stand and every h_5 entry reads four hidden units, so a third of the
# rows (and of their maxima) moves at all; and round-to-nearest errors have both signs, so they cancel in a graph's pooled mean or sum
# while the bound grows with it.  The logits and per-node terms of the same cases separate from the same forwards (74 % and more), and
# each of these vectors separates from the unrounded forward, whose weights are all larger by the same 2^-12 (probe_weights, tight).
NOT_SEPARATED = {  # (model, case, output, variant): fraction of elements beyond 100 x the bound (more than 0.5 would pass)
    ("GIN", "graph embeddings", "pooled", "a not rounded"): 0.19,
    ("GIN", "graph embeddings", "pooled", "hidden units not rounded"): 0.16,
    ("GIN-VN", "graph embeddings", "pooled", "a not rounded"): 0.30,
    ("GIN-VN", "graph embeddings", "pooled", "hidden units not rounded"): 0.24,
    ("GIN", "node embeddings", "rows", "a not rounded"): 0.37,
    ("GIN-VN", "node embeddings", "rows", "a not rounded"): 0.36,
    ("GIN", "sum, graph embeddings", "pooled", "a not rounded"): 0.24,
    ("GIN", "sum, graph embeddings", "pooled", "hidden units not rounded"): 0.20,
    ("GIN-VN", "sum, graph embeddings", "pooled", "a not rounded"): 0.30,
    ("GIN-VN", "sum, graph embeddings", "pooled", "hidden units not rounded"): 0.25,
    ("GIN", "max, graph embeddings", "pooled", "a not rounded"): 0.35,
    ("GIN-VN", "max, graph embeddings", "pooled", "a not rounded"): 0.32,
    ("GIN", "eps, sum, graph embeddings", "pooled", "a not rounded"): 0.25,
    ("GIN", "eps, sum, graph embeddings", "pooled", "hidden units not rounded"): 0.21,
    ("GIN-VN", "eps, sum, graph embeddings", "pooled", "a not rounded"): 0.30,
    ("GIN-VN", "eps, sum, graph embeddings", "pooled", "hidden units not rounded"): 0.24,
    ("GIN", "eps, graph embeddings", "pooled", "a not rounded"): 0.21,
    ("GIN", "eps, graph embeddings", "pooled", "hidden units not rounded"): 0.16,
    ("GIN-VN", "eps, graph embeddings", "pooled", "a not rounded"): 0.29,
    ("GIN-VN", "eps, graph embeddings", "pooled", "hidden units not rounded"): 0.24,
    ("GIN", "eps, node embeddings", "rows", "a not rounded"): 0.37,
    ("GIN-VN", "eps, node embeddings", "rows", "a not rounded"): 0.36,
    ("GIN", "eps, max, graph embeddings, below the fill threshold", "pooled", "a not rounded"): 0.37,
}
