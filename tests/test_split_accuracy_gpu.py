"""The split-f16 dense products of all six models, held to fp32 accuracy on the GPU ("Split accuracy").

Every comparison is GPU against the float64 forward of tests/numpy_ref.py with the bound B of tests/split_ref.py (B = sqrt(E_ok E_bad),
from the references alone; tests/test_split_ref_cpu.py proves that B separates the correct arithmetic from every named wrong variant
-- a cross term lost everywhere, in one K-step, in one 16-column tile, in the K tail, in one layer; 1 / scale on the wrong side of the
bias -- each of which passes the suite's 1e-4 parity rule).  max |gpu - f64| / unit <= B, on every output an instance returns.

Inputs (split_ref.batch_of): 64 molhiv-shaped graphs (GIN, GIN-VN, GCN, GAT) or 24 hep10k-shaped ones (PNA, DGN), two seeds, then a
one-node graph without edges and a two-node graph; the rows end inside a 16-row tile.  Weights: the synthetic sets (24-bit mantissas,
nonzero biases), and once per model the pre-scale case (split_ref.weights_of: a layer at 2^-10, largest magnitudes one step below and
one step above a power of two).

Instances (INSTANCES below; from the Makefile's translation units and the launch selection of engine.hip / gin.hip / the models' forward):
the default graph-resident path, its batch-order tiles and three-kernel front end where options exist, the per-layer fallbacks, the
graph-embedding, node-embedding, node-logit, sum-pool and max-pool instances, GIN's un-folded head and readout and its eps instances
(eps = 0: s_l = 1 exactly, so the eps kernels compute the same model), DGN with the walk and with the matrix-pipe aggregation, and the
fp32 matrix-pipe kernels (<model>_mfma 32) against the same B; GIN's per-layer kernel in its three block shapes (gin_split_nt 4, 2, 1);
GAT's attention instance (gat_attn.hip) on its logits; the sum-pool instances of GCN and GAT (gcn_poolsum.hip, gat_poolsum.hip) without
embeddings, which is when they run.  Each case asserts through the profile slots which path ran -- the resident kernel, the fused per-layer
kernel or the separate dense kernel, and none of the other two -- and that no exact re-run happened.  The slots name launch sites, not
template instances: gin_layer_fused covers the split kernel and gin_layer_fused_kernel (fp32, gin_mfma 32) alike, so on GIN's per-layer
path the slot cannot tell a silent fp32 fallback from the split kernel; exact_reruns() sees only the range re-run.

Not covered (not reachable through the ABI with these inputs): gin_resident's hub-row instances beyond what GIN-VN's virtual nodes
select, the development-build ping-pong kernel (gin_pingpong), graphs beyond the tile limits (tests/test_resident_limits_gpu.py runs
those against the oracle), the f16 and fixed-point modes (pinned by tests/test_f16_probe_gpu.py and the Q oracles)."""
from collections import namedtuple

import numpy as np
import pytest

from flowgnn_amd import Engine
from tests import split_ref as sr
from tests.test_embeddings_gpu import launched

pytestmark = pytest.mark.gpu

# what a case does beside the options: fwd = Engine.forward's return_* flags, pooling, eps; outs = the reference names of what forward
# returns, in order; h = also compare flowgnn_get_h's rows (the per-layer kernels repeat the pass with the rows kept)
Inst = namedtuple("Inst", "name options path fwd outs pooling eps h", defaults=((), ("logits",), "mean", False, False))
EMB = (("return_embeddings",), ("logits", "emb"))
ROWS = (("return_node_embeddings",), ("logits", "rows"))
NLOG = (("return_node_logits",), ("logits", "node_logits"))


def _gin():
    return [
        Inst("default", {}, "resident", h=True),
        Inst("batch_order_tiles", {"gin_binpack": 0}, "resident"),
        Inst("three_kernel_front_end", {"gin_tile_build": 0}, "resident"),
        Inst("head_not_folded", {"gin_head_fold": 0}, "resident"),
        Inst("readout_not_folded", {"gin_fold_readout": 0}, "resident"),
        Inst("per_layer", {"gin_resident": 0}, "per_layer", h=True),
        Inst("per_layer_readout_not_folded", {"gin_resident": 0, "gin_fold_readout": 0}, "per_layer"),
        Inst("per_layer_two_tiles_per_wave", {"gin_resident": 0, "gin_split_nt": 2}, "per_layer", h=True),  # gin_layer_split_kernel<2, 4>
        Inst("per_layer_four_waves", {"gin_resident": 0, "gin_split_nt": 1}, "per_layer", h=True),          # <1, 4> (the default 4: <1, 8>)
        Inst("embeddings", {}, "resident", *EMB),
        Inst("node_embeddings", {}, "resident", *ROWS),
        Inst("node_logits", {}, "resident", *NLOG),
        Inst("node_logits_head_not_folded", {"gin_head_fold": 0}, "resident", *NLOG),
        Inst("sum_pool", {}, "resident", (), ("logits_sum",), "sum"),
        Inst("sum_pool_three_kernel_front_end", {"gin_tile_build": 0}, "resident", (), ("logits_sum",), "sum"),
        Inst("sum_pool_embeddings", {}, "resident", ("return_embeddings",), ("logits_sum", "emb_sum"), "sum"),
        Inst("sum_pool_readout_not_folded", {"gin_fold_readout": 0}, "resident", (), ("logits_sum",), "sum"),
        Inst("max_pool", {}, "resident", (), ("logits_max",), "max"),
        Inst("max_pool_embeddings", {}, "resident", ("return_embeddings",), ("logits_max", "emb_max"), "max"),
        Inst("eps", {}, "resident", eps=True),
        Inst("eps_three_kernel_front_end", {"gin_tile_build": 0}, "resident", eps=True),
        Inst("eps_head_not_folded", {"gin_head_fold": 0}, "per_layer", eps=True),
        Inst("eps_per_layer", {"gin_resident": 0}, "per_layer", eps=True),
        Inst("fp32_pipe", {"gin_mfma": 32}, "fp32", h=True),
    ]


INSTANCES = {
    "GIN": _gin(),
    "GIN-VN": _gin(),
    "GCN": [
        Inst("default", {}, "resident", h=True),
        Inst("batch_order_tiles", {"gcn_binpack": 0}, "resident"),
        Inst("three_kernel_front_end", {"gcn_tile_build": 0}, "resident"),
        Inst("per_layer", {"gcn_resident": 0}, "per_layer", h=True),
        Inst("per_layer_unfused", {"gcn_resident": 0, "gcn_unfused": 1}, "unfused"),
        Inst("embeddings", {}, "per_layer", *EMB),  # (graph embeddings alone: the per-layer kernels, pooled from the rows in HBM)
        Inst("node_embeddings", {}, "resident", *ROWS),
        Inst("node_logits", {}, "resident", *NLOG),
        Inst("sum_pool", {}, "resident", (), ("logits_sum",), "sum"),  # gcn_poolsum.hip
        Inst("sum_pool_embeddings", {}, "per_layer", ("return_embeddings",), ("logits_sum", "emb_sum"), "sum"),
        Inst("max_pool", {}, "per_layer", ("return_embeddings",), ("logits_max", "emb_max"), "max"),
        Inst("fp32_pipe", {"gcn_mfma": 32}, "fp32", h=True),
    ],
    "GAT": [
        Inst("default", {}, "resident", h=True),
        Inst("readout_not_folded", {"gat_fold_readout": 0}, "per_layer"),
        Inst("per_layer", {"gat_resident": 0}, "per_layer", h=True),
        Inst("per_layer_readout_not_folded", {"gat_resident": 0, "gat_fold_readout": 0}, "per_layer"),
        Inst("embeddings", {}, "per_layer", *EMB),
        Inst("node_embeddings", {}, "per_layer", *ROWS),
        Inst("node_logits", {}, "resident", *NLOG),  # gat_nlogit.hip
        Inst("attention", {}, "resident", ("return_attention",), ("logits", "_attention")),  # gat_attn.hip: its logits (the coefficients: tests/test_attention_gpu.py)
        Inst("sum_pool", {}, "resident", (), ("logits_sum",), "sum"),  # gat_poolsum.hip
        Inst("sum_pool_embeddings", {}, "per_layer", ("return_embeddings",), ("logits_sum", "emb_sum"), "sum"),
        Inst("max_pool", {}, "per_layer", ("return_embeddings",), ("logits_max", "emb_max"), "max"),
        Inst("fp32_pipe", {"gat_mfma": 32}, "fp32", h=True),
    ],
    "PNA": [
        Inst("default", {}, "resident", h=True),
        Inst("batch_order_tiles", {"pna_binpack": 0}, "resident"),
        Inst("three_kernel_front_end", {"pna_tile_build": 0}, "resident"),
        Inst("per_layer", {"pna_resident": 0}, "per_layer", h=True),
        Inst("per_layer_unfused", {"pna_resident": 0, "pna_fused": 0}, "unfused", h=True),
        Inst("embeddings", {}, "resident", *EMB),
        Inst("node_embeddings", {}, "resident", *ROWS),
        Inst("fp32_pipe", {"pna_mfma": 32}, "fp32", h=True),
    ],
    "DGN": [
        Inst("default", {}, "resident", h=True),
        Inst("batch_order_tiles", {"dgn_binpack": 0}, "resident"),
        Inst("matrix_pipe_aggregation", {"dgn_mfma_agg": 1}, "resident"),
        Inst("in_edge_walk", {"dgn_mfma_agg": 0}, "per_layer", h=True),  # (the walk lives on the per-layer path)
        Inst("per_layer", {"dgn_resident": 0, "dgn_mfma_agg": 1}, "per_layer", h=True),
        Inst("per_layer_readout_not_folded", {"dgn_resident": 0, "dgn_fold_readout": 0}, "per_layer"),
        Inst("per_layer_unfused", {"dgn_resident": 0, "dgn_fused": 0}, "unfused", h=True),
        Inst("embeddings", {}, "resident", *EMB),
        Inst("node_embeddings", {}, "resident", *ROWS),
        Inst("fp32_pipe", {"dgn_mfma": 32}, "fp32", h=True),
    ],
}
PARAMS = [(m, i) for m in sr.MODELS for i in INSTANCES[m]]
IDS = [f"{m}-{i.name}" for m, i in PARAMS]
RESIDENT_SLOT = {m: f"{sr.base(m)}_resident" for m in sr.MODELS}
# the slots that carry a model's dense products off the resident path: the fused per-layer kernel, the separate dense kernel
FUSED_SLOT = {"GIN": "gin_layer_fused", "GIN-VN": "gin_layer_fused", "GCN": "gcn_layer_fused", "GAT": "gat_layer", "PNA": "pna_layer_fused",
              "DGN": "dgn_layer_fused"}
DENSE_SLOT = {"GIN": "gin_mlp", "GIN-VN": "gin_mlp", "GCN": "gcn_dense", "GAT": None, "PNA": "pna_dense", "DGN": "dgn_dense"}
# <model>_mfma 32: GCN, PNA and DGN take the aggregate + fp32 dense kernels, GIN and GAT the fp32 form of the per-layer kernel
FP32_SLOT = {"GIN": "gin_layer_fused", "GIN-VN": "gin_layer_fused", "GCN": "gcn_dense", "GAT": "gat_layer", "PNA": "pna_dense", "DGN": "dgn_dense"}


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def run_instance(model, inst, seed, case="synth"):
    """(name -> float32 array as the engine returned it, profile slots launched, exact re-runs)"""
    b, w = sr.batch_of(model, seed), sr.weights_of(model, case)
    e = Engine(model, device=0, options=inst.options)
    try:
        e.set_weights(w)
        if inst.pooling != "mean":
            e.set_pooling(inst.pooling)
        if inst.eps:
            e.set_gin_eps([0.0] * 5)  # on, with s_l = float32(1 + 0) = 1: the eps kernels, the same model
        e.profile_enable(True)
        got = {}

        def forward():
            ret = e.forward(b, **{k: ("last" if k == "return_attention" else True) for k in inst.fwd})
            ret = ret if isinstance(ret, tuple) else (ret,)
            assert len(ret) == len(inst.outs)
            got.update(zip(inst.outs, ret))

        names = launched(e, forward)
        reruns = e.exact_reruns()
        if inst.h:
            got["h"] = e.final_h()
        reruns_h = e.exact_reruns()
    finally:
        e.close()
    return got, names, (reruns, reruns_h)


def check(model, inst, seed, case="synth"):
    tb, ref = sr.table(model, seed, case), sr.reference(model, seed, case)
    got, names, reruns = run_instance(model, inst, seed, case)
    what = f"{model} / {inst.name} / seed {seed} / {case}"
    worst = {}
    for o, x in got.items():
        if o not in tb:  # (the pre-scale case holds the default outputs only: split_ref.CASE_OUTPUTS)
            continue
        assert np.isfinite(x).all(), (what, o)
        worst[o] = sr.err(x, ref, o) / tb[o].bound
    print(f"\n{what}: ratio to B " + ", ".join(f"{o} {r:.3f}" for o, r in worst.items()) + f"   [{' '.join(sorted(names))}]")
    must = {"resident": RESIDENT_SLOT, "per_layer": FUSED_SLOT, "unfused": DENSE_SLOT, "fp32": FP32_SLOT}[inst.path][model]
    others = {RESIDENT_SLOT[model], FUSED_SLOT[model], DENSE_SLOT[model]} - {must, None}
    assert must in names and not (names & others), (what, inst.path, names)
    assert reruns == (0, 0), (what, "exact re-runs", reruns)  # the bound is met by the kernels asked for, not by a silent fp32 re-run
    for o, r in worst.items():
        assert r <= 1.0, (what, o, f"max |gpu - f64| / unit = {r * tb[o].bound:.3e}, {r:.2f} x B = {tb[o].bound:.3e}",
                          f"E_ok {tb[o].e_ok:.2e}, E_bad {tb[o].e_bad:.2e}")
    assert "logits" in worst or any(o.startswith("logits") for o in worst)


@pytest.mark.parametrize("model,inst", PARAMS, ids=IDS)
def test_instance_meets_the_split_bound(model, inst):
    for seed in sr.SEEDS[model]:
        check(model, inst, seed)


@pytest.mark.parametrize("model", sr.MODELS)
def test_prescale_case(model):
    """Three different power-of-two scales per split matrix (sc, 1 / sc and the biases' pre-scale), on the default path, the per-layer
    path and the node-embedding instance."""
    seed = sr.PRESCALE_SEED[model]
    by_name = {i.name: i for i in INSTANCES[model]}
    for name in ("default", "per_layer", "node_embeddings", "embeddings"):
        check(model, by_name[name], seed, "prescale")
