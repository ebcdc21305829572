"""The host-side plans of GCN, GAT, DGN and PNA (gcn_plan.h, gat_plan.h, dgn_plan.h, pna_plan.h) against what a run actually launches and
computes, on the GPU.

For each configuration below (options, optional outputs, pooling, tasks, numeric mode; three batches) one fresh engine runs the batch once:
- the profile slots that run launched are exactly the ones the plan names for that configuration (the plan through the same shim as
  test_resident_plan_cpu.py; slots_of: the ProfScope names of the parent's forward, gcn.hip / gat.hip at fe3f5ae, and of engine_forward);
- no exact-fp32 re-run happened;
- the logits and every output that is on are BIT-identical to tests/golden/resident_plan.npz: the same configurations run through
  GcnModel::forward / GatModel::forward of the parent commit (fe3f5ae) on an MI355X, recorded with
  `python -m tests.test_resident_plan_gpu <out.npz> GCN GAT` from that commit's tree with this file and tests/resident_plan.py copied into it.
  DGN and PNA, whose plans came later: tests/golden/resident_plan_dgn_pna.npz, from DgnModel::forward / PnaModel::forward of THEIR parent
  commit (1ac249e, whose dgn.hip / pna.hip name the slots), recorded in the same way with `... <out.npz> DGN PNA`.

The configurations reach every path and every resident instance of the four models (asserted)."""
import dataclasses
import os
import sys

import numpy as np
import pytest

from flowgnn_amd import Engine, graphpack as gp, weights
from tests import resident_plan as rp

pytestmark = pytest.mark.gpu
GOLDEN = {m: os.path.join(os.path.dirname(__file__), "golden", f) for f, ms in (("resident_plan.npz", ("GCN", "GAT")),
                                                                              ("resident_plan_dgn_pna.npz", ("DGN", "PNA"))) for m in ms}
THRESHOLD = {"GCN": 0.5, "GAT": 0.5, "DGN": 0.4, "PNA": 0.4}  # the fill under which a model's graph-tile kernels are not used
OUTPUTS = ("emb", "node_emb", "node_logits")


def ring_batch(num_graphs, nodes, seed, reach=1):
    """Ring graphs (reach > 1: every node also joined to the next `reach` ones), both edge directions, random node features and edge
    attributes."""
    rng = np.random.default_rng(seed)
    a = np.tile(np.arange(nodes, dtype=np.int32), reach)
    b = (a + np.repeat(np.arange(1, reach + 1, dtype=np.int32), nodes)) % nodes
    ring = np.stack([np.concatenate([a, b]), np.concatenate([b, a])], axis=1).astype(np.int32)
    n, e = num_graphs * nodes, num_graphs * len(ring)
    nf = (rng.random((n, 9)) * gp.ND_FEATURE_CARD).astype(np.int32)
    ea = (rng.random((e, 3)) * gp.ED_FEATURE_CARD).astype(np.int32)
    return gp.GraphBatch(np.full(num_graphs, nodes, np.int32), np.full(num_graphs, len(ring), np.int32), nf, np.tile(ring, (num_graphs, 1)), ea)


# full: 192 rows, 384 edges -- one full GCN tile, three quarters of a GAT tile.
# sparse: three graphs of 40 nodes and 720 edges.  Two of them exceed a tile's in-edges (GCN 960, GAT 1 280), so every tile holds one:
# 40 rows of 192 / 256, far under the resident paths' 0.5 fill threshold -- the per-layer path.
# tiny: 2 graphs of 5 nodes.  One tile, and a one-tile batch counts as full (tile_pack.cpp): resident, whatever its rows.
# DGN (tiles of 128 rows / 2 560 in-edges) and PNA (256 / 4 608):
# full: two edges per node, under DGN's density rule (job_e >= 8 job_n): the in-edge walk.  The greedy packing's tiles but the last are full.
# sparse: 18 edges per node, over the rule: the matrix pipe.  The three graphs fit one tile of either model: full.
# underfilled: four graphs of 48 nodes and 2 208 edges: by edges one fits a DGN tile and two a PNA tile -- 0.375 of the rows, under the 0.4
# threshold.
BATCHES = {"full": lambda: ring_batch(12, 16, seed=3), "sparse": lambda: ring_batch(3, 40, seed=4, reach=9), "tiny": lambda: ring_batch(2, 5, seed=5),
           "underfilled": lambda: ring_batch(4, 48, seed=6, reach=23)}


def with_eigen(b):
    """DGN's node_eigen as an INPUT: seeded random float32 [N][4] in [-1, 1), not the graphs' eigenvectors (no LAPACK in the golden)."""
    eig = (np.random.default_rng(11).random((b.total_nodes, 4)) * 2.0 - 1.0).astype(np.float32)
    return dataclasses.replace(b, node_eigen=eig)


def density_of(b):
    """rp's density input of a batch that is its whole job: job_e one under, at, or over 8 job_n (0, 1, 2; off the rule by any margin)."""
    return 1 + int(np.sign(b.total_edges - 8 * b.total_nodes))


def cfg(batch="full", pooling="mean", tasks=1, mode="f32", attention=None, emb=False, node_emb=False, node_logits=False, **options):
    return dict(batch=batch, pooling=pooling, tasks=tasks, mode=mode, attention=attention, emb=emb, node_emb=node_emb, node_logits=node_logits,
                options=options)


CONFIGS = {
    "GCN": [
        cfg(), cfg(gcn_binpack=0), cfg(gcn_tile_build=0),
        cfg(node_emb=True), cfg(node_emb=True, emb=True), cfg(node_emb=True, node_logits=True), cfg(node_emb=True, pooling="sum"),
        cfg(pooling="sum"), cfg(node_logits=True),
        cfg(gcn_tile_build=0, node_emb=True, emb=True, node_logits=True), cfg(gcn_tile_build=0, pooling="sum"), cfg(gcn_tile_build=0, node_logits=True),
        cfg(pooling="max"), cfg(pooling="max", emb=True), cfg(emb=True),
        cfg(gcn_resident=0), cfg(gcn_resident=0, node_logits=True), cfg(gcn_resident=0, pooling="sum"), cfg(gcn_resident=0, node_emb=True, node_logits=True),
        cfg(gcn_unfused=1), cfg(gcn_mfma="f32"), cfg(gcn_mfma="f32", emb=True, node_logits=True),
        cfg(tasks=2), cfg(tasks=2, node_logits=True, emb=True), cfg(mode="q6.10"),
        cfg(batch="sparse"), cfg(batch="sparse", emb=True, node_emb=True, node_logits=True), cfg(batch="sparse", pooling="sum"),
        cfg(batch="tiny"),
    ],
    "GAT": [
        cfg(), cfg(pooling="sum"), cfg(attention="last"), cfg(attention="all", node_logits=True), cfg(node_logits=True),
        cfg(pooling="sum", attention=[0, 4]), cfg(pooling="max"), cfg(pooling="max", emb=True), cfg(emb=True), cfg(node_emb=True),
        cfg(node_emb=True, node_logits=True, attention="last"),
        cfg(gat_resident=0), cfg(gat_resident=0, node_logits=True), cfg(gat_resident=0, attention="all"), cfg(gat_resident=0, pooling="sum"),
        cfg(gat_mfma="f32"), cfg(gat_mfma="f32", node_logits=True), cfg(gat_fold_readout=0), cfg(gat_fold_readout=0, node_logits=True, emb=True),
        cfg(mode="q6.10"),
        cfg(batch="sparse"), cfg(batch="sparse", node_logits=True, attention="last"), cfg(batch="sparse", pooling="sum"),
        cfg(batch="tiny"),
    ],
    # (node embeddings on the ten-node batch alone: the golden file stays small)
    "DGN": [
        cfg(), cfg(dgn_resident=2), cfg(dgn_resident=2, dgn_binpack=0), cfg(dgn_resident=2, emb=True),
        cfg(batch="tiny", dgn_resident=2, node_emb=True), cfg(batch="tiny", dgn_resident=2, node_emb=True, emb=True),
        cfg(batch="sparse"), cfg(batch="sparse", emb=True),
        cfg(batch="sparse", dgn_resident=0), cfg(batch="sparse", dgn_resident=0, dgn_rowinfo_direct=0), cfg(batch="sparse", dgn_resident=0, dgn_fold_readout=0),
        cfg(batch="sparse", dgn_resident=0, emb=True), cfg(batch="sparse", dgn_resident=0, dgn_fold_readout=0, emb=True),
        cfg(batch="sparse", dgn_resident=0, dgn_mfma_agg=0),
        cfg(batch="tiny", dgn_resident=0, dgn_mfma_agg=1, node_emb=True), cfg(batch="tiny", dgn_resident=0, dgn_mfma_agg=1, node_emb=True, emb=True),
        cfg(batch="tiny", dgn_resident=0, node_emb=True),
        cfg(dgn_mfma_agg=1), cfg(dgn_resident=0, dgn_mfma_agg=1),
        cfg(dgn_fused=0), cfg(batch="tiny", dgn_fused=0, emb=True, node_emb=True), cfg(dgn_mfma="f32"),
        cfg(mode="q6.10"),
        cfg(batch="underfilled"), cfg(batch="underfilled", dgn_resident=2, emb=True),
        cfg(batch="tiny"),
    ],
    "PNA": [
        cfg(), cfg(pna_binpack=0), cfg(pna_tile_build=0), cfg(emb=True), cfg(pna_tile_build=0, emb=True),
        cfg(batch="tiny", node_emb=True), cfg(batch="tiny", node_emb=True, emb=True), cfg(batch="tiny", pna_tile_build=0, node_emb=True),
        cfg(pna_resident=0), cfg(pna_resident=0, emb=True),
        cfg(batch="tiny", pna_resident=0, node_emb=True), cfg(batch="tiny", pna_resident=0, node_emb=True, emb=True),
        cfg(pna_fused=0), cfg(batch="tiny", pna_fused=0, emb=True, node_emb=True), cfg(pna_mfma="f32"),
        cfg(mode="q6.10"),
        cfg(batch="sparse"), cfg(batch="sparse", pna_binpack=0, emb=True),
        cfg(batch="underfilled"), cfg(batch="underfilled", emb=True),
        cfg(batch="tiny"),
    ],
}
CASES = [(m, i) for m in CONFIGS for i in range(len(CONFIGS[m]))]


def case_id(case):
    m, i = case
    c = CONFIGS[m][i]
    default = cfg()
    on = [k if c[k] is True else f"{k}={c[k]}" for k in c if k != "options" and c[k] != default[k]]
    return f"{m}-{i}-" + (",".join(on + [f"{k}={v}" for k, v in c["options"].items()]) or "default")


def slots_of(model, p):
    """The profile slots one run launches, from the plan's flags (and engine_forward's index build)."""
    path = rp.PATHS[p["path"]]
    if model == "GCN":
        s = {"build_csr"} if p["needs_csr"] else set()
        if path == "fixed_point":
            return s | {"gcnq_forward"}
        if path == "resident":
            s |= {"gcn_tile_build" if p["one_pass"] else "gcn_encoder_projected", "gcn_resident"}
            s |= {"mean_pool_linear"} if p["sum_from_rows"] else set()
        else:  # (every batch has edges: edge_scalar, and the fused layers where the plan fuses at all)
            s |= {"edge_scalar", "mean_pool_linear"}
            s |= {"gcn_encoder_dense"} if p["fused_encoder"] else {"atom_encoder", "gcn_dense"}
            s |= {"gcn_layer_fused"} if p["fused_layers"] else {"gcn_aggregate", "gcn_dense"}
            s |= {"gcn_layer_fused"} if p["folded_last"] else {"gcn_aggregate"}
    elif model in ("DGN", "PNA"):  # (their per-layer readout stores the graph embeddings itself: no slot of its own)
        m = model.lower()
        s = {"build_csr"} if p["needs_csr"] else set()
        if path == "fixed_point":
            return s | {m + "q_forward"}
        if path == "resident":
            front = "dgn_tile_build" if model == "DGN" else "pna_tile_build" if p["one_pass"] else "pna_tile_desc"
            return s | {front, m + "_resident"}
        s |= {"atom_encoder", "pool_mlp3"} | ({m + "_layer_fused"} if p["fused_layers"] else {m + "_aggregate", m + "_dense"})
        if model == "DGN":
            s |= ({"edge_scalar"} if p["edge_scalar"] else set()) | ({"dgn_rowinfo"} if p["rowinfo_from_edge_list"] else set())
        return s
    else:
        s = {"build_csr"}
        if path == "fixed_point":
            return s | {"gatq_forward"}
        if path == "resident":
            return s | {"gat_resident"}
        s |= {"gat_scores0", "gat_layer", "mean_pool_linear"}
        s |= {"gat_attention"} if p["attention_kernels"] else set()
    s |= {"mean_pool_rows"} if p["pool_rows"] else set()
    s |= {"node_logits"} if p["node_logits_from_rows"] or p["node_logits_from_scores"] else set()
    return s


def make_engine(model, c):
    e = Engine(model, device=0, options=c["options"])
    if c["tasks"] != 1:
        e.set_num_tasks(c["tasks"])
    e.set_weights(weights.synth_gcn_weights(seed=7, num_tasks=c["tasks"]) if model == "GCN" else weights.SYNTH[model](seed=7))
    e.set_numeric_mode(c["mode"])
    e.set_pooling(c["pooling"])
    if c["attention"] is not None:
        e.set_attention(c["attention"])
    e.set_embeddings(c["emb"])
    e.set_node_embeddings(c["node_emb"])
    e.set_node_logits(c["node_logits"])
    return e


def run(model, c, b):
    """One run of the configuration on a fresh engine -> (engine facts for the plan, slots launched, {output: array})."""
    e = make_engine(model, c)
    if model == "DGN":
        b = with_eigen(b)
    try:
        e.profile_enable(True)
        e.set_batch(b)
        before = {k: v["launches"] for k, v in e.profile_read().items()}
        e.run()
        out = {"logits": e.results().copy()}
        launched = {k for k, v in e.profile_read().items() if v["launches"] > before.get(k, 0)}
        for k, get in zip(OUTPUTS, (e.embeddings, e.node_embeddings, e.node_logits)):
            if c[k]:
                out[k] = get().copy()
        if c["attention"] is not None:
            out["attn_edge"], out["attn_self"] = (a.copy() for a in e.attention())
        facts = dict(fill=e.graph_tile_fill(b.nums_of_nodes, b.nums_of_edges), tiles=e.batch_tiles(), exact_reruns=e.exact_reruns(), density=density_of(b))
        return facts, launched, out
    finally:
        e.close()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return rp.build_shim(tmp_path_factory.mktemp("resident_plan"))


@pytest.fixture(scope="module")
def batches():
    return {k: f() for k, f in BATCHES.items()}


@pytest.fixture(scope="module")
def golden():
    files = {path: np.load(path) for path in set(GOLDEN.values())}
    return {m: files[path] for m, path in GOLDEN.items()}


def plan_of(lib, model, c, facts):
    o = c["options"]
    fill = facts["fill"]
    at = THRESHOLD[model]
    assert fill <= at - 0.01 or fill >= at + 0.01, fill  # (the plan is pinned AT the threshold on the CPU; here a batch is on one side of it)
    common = dict(tiles=facts["tiles"][0] > 0, fill_i=2 if fill >= at else 0, qmode=c["mode"] == "q6.10", keep_h=0, exact=0)
    if model in ("DGN", "PNA"):  # (the mean alone and no node logits: flowgnn_set_pooling, flowgnn_set_node_logits)
        assert c["pooling"] == "mean" and not c["node_logits"]
        common.update(emb=c["emb"], node_emb=c["node_emb"], bp_lists=facts["tiles"][1] > 0, split=o.get(model.lower() + "_mfma") != "f32",
                      fused=o.get(model.lower() + "_fused", 1), binpack=o.get(model.lower() + "_binpack", 1))
    else:
        common.update(pooling={"mean": 0, "sum": 1, "max": 2}[c["pooling"]], **{k: c[k] for k in OUTPUTS})
    if model == "DGN":  # (a fresh engine's first run of a batch with nodes, edges and the eigenvector column: no CSR of it yet)
        return rp.plan_one(lib, "DGN", mfma_agg=o.get("dgn_mfma_agg", -1) + 1, fold_readout=o.get("dgn_fold_readout", 1),
                           rowinfo_direct=o.get("dgn_rowinfo_direct", 1), resident=o.get("dgn_resident", 1), nonempty=1, eigen=1, edges=1,
                           csr_built=0, density=facts["density"], **common)
    if model == "PNA":
        return rp.plan_one(lib, "PNA", resident=o.get("pna_resident", 1), tile_build=o.get("pna_tile_build", 1), **common)
    if model == "GCN":  # (synth weights: the resident walk's table check passes; the batches have edges and edge attributes)
        return rp.plan_one(lib, "GCN", resident=o.get("gcn_resident", 1), tile_build=o.get("gcn_tile_build", 1), binpack=o.get("gcn_binpack", 1),
                           split=o.get("gcn_mfma") != "f32", fused=not o.get("gcn_unfused", 0), table_ok=1, two_tasks=c["tasks"] == 2,
                           bp_lists=facts["tiles"][1] > 0, edge_attr=1, edges=1, **common)
    return rp.plan_one(lib, "GAT", resident=o.get("gat_resident", 1), fold_readout=o.get("gat_fold_readout", 1), split=o.get("gat_mfma") != "f32",
                       attention=c["attention"] is not None, **common)


def test_the_batches_are_on_the_sides_of_the_fill_threshold_they_are_meant_for(batches):
    assert (batches["full"].total_nodes, batches["full"].total_edges) == (192, 384)
    for model in ("GCN", "GAT"):
        e = Engine(model, device=0)
        try:
            fill = {k: e.graph_tile_fill(b.nums_of_nodes, b.nums_of_edges) for k, b in batches.items()}
            assert fill["full"] == 1.0 and fill["tiny"] == 1.0 and 0.0 < fill["sparse"] <= 0.25, fill
            e.set_batch(batches["sparse"])
            assert e.batch_tiles()[0] == 3
        finally:
            e.close()
    # DGN, PNA: the 0.4 threshold, and the density rule
    assert [density_of(batches[k]) for k in ("full", "sparse", "underfilled", "tiny")] == [0, 2, 2, 0]
    for model in ("DGN", "PNA"):
        e = Engine(model, device=0)
        try:
            fill = {k: e.graph_tile_fill(b.nums_of_nodes, b.nums_of_edges) for k, b in batches.items()}
            assert min(fill["full"], fill["sparse"], fill["tiny"]) >= 0.41 and 0.0 < fill["underfilled"] <= 0.39, fill
        finally:
            e.close()


def plans_without_a_run(lib, model, batches):
    """The plan of every configuration of a model, from what the batches are meant to be (asserted on the engine above)."""
    under = "sparse" if model in ("GCN", "GAT") else "underfilled"
    return [plan_of(lib, model, c, dict(fill=0.2 if c["batch"] == under else 1.0, tiles=(1, 1), density=density_of(batches[c["batch"]])))
            for c in CONFIGS[model]]


def test_the_configurations_reach_every_path_and_instance(lib, batches):
    for model in CONFIGS:
        seen = set()
        for p in plans_without_a_run(lib, model, batches):
            seen.add((rp.PATHS[p["path"]], rp.INSTANCES[model][p["instance"]] if rp.PATHS[p["path"]] == "resident" else None))
        want = {("fixed_point", None), ("per_layer", None)} | {("resident", i) for i in rp.INSTANCES[model]}
        assert seen == want, (model, seen ^ want)


def test_the_dgn_and_pna_configurations_reach_every_branch_of_their_forwards(lib, batches):
    def reached(model, *keys, path=None, **where):
        """The values the plans (of `path`, with the flags of `where`) take in `keys`, and the configurations' options, as a set of tuples."""
        rows = [(c, p) for c, p in zip(CONFIGS[model], plans_without_a_run(lib, model, batches))
                if (path is None or rp.PATHS[p["path"]] == path) and all(p[k] == v for k, v in where.items())]
        return {tuple(p[k] if k in p else c[k] if k in c else c["options"].get(k) for k in keys) for c, p in rows}

    both = {(False,), (True,)}
    # DGN: the walk and the matrix-pipe fused layers; the first layer making the per-row pass or not; the last layer pooled or not (by the
    # option, and by the node embeddings); the three values of dgn_resident; the two-kernel layer by option, its fp32 dense; the tile lists
    assert reached("DGN", "mfma_aggregation", path="per_layer", fused_layers=True) == both
    assert reached("DGN", "first_layer_makes_rowinfo", "dgn_rowinfo_direct", path="per_layer", mfma_aggregation=True) >= {(False, None), (True, 0)}
    assert reached("DGN", "pooled_last", "dgn_fold_readout", "node_emb", path="per_layer", mfma_aggregation=True) >= {
        (True, None, False), (False, 0, False), (False, None, True)}
    assert reached("DGN", "dgn_resident") == {(None,), (0,), (2,)} and (None,) in reached("DGN", "dgn_resident", path="resident")
    assert (0,) in reached("DGN", "dgn_fused", path="per_layer", split_dense=True)
    assert ("f32",) in reached("DGN", "dgn_mfma", path="per_layer", prepare_aggregate=True, split_dense=False)
    assert reached("DGN", "bin_packed", path="resident") == both
    assert reached("DGN", "emb_readout", path="per_layer", pooled_last=True) == both
    # PNA: both front ends of the resident kernel, the tile lists, the per-layer path by option, the two-kernel layer and its fp32 dense,
    # every combination of the two optional outputs on either path
    assert reached("PNA", "one_pass", path="resident") == both and reached("PNA", "bin_packed", path="resident", one_pass=True) == both
    assert (0,) in reached("PNA", "pna_resident", path="per_layer", fused_layers=True)
    assert (0,) in reached("PNA", "pna_fused", path="per_layer", split_dense=True)
    assert ("f32",) in reached("PNA", "pna_mfma", path="per_layer", fused_layers=False, split_dense=False)
    outputs = {(False, False), (True, False), (False, True), (True, True)}
    assert reached("PNA", "emb", "node_emb", path="resident") == outputs and reached("PNA", "emb", "node_emb", path="per_layer") == outputs
    for model in ("DGN", "PNA"):
        assert "fixed_point" in {rp.PATHS[p["path"]] for p in plans_without_a_run(lib, model, batches)}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_run_launches_what_the_plan_names_and_computes_what_the_parent_computed(case, lib, batches, golden):
    model, i = case
    c = CONFIGS[model][i]
    facts, launched, out = run(model, c, batches[c["batch"]])
    p = plan_of(lib, model, c, facts)
    assert facts["exact_reruns"] == 0
    assert launched == slots_of(model, p), (p, sorted(launched))
    for k, got in out.items():
        want = golden[model][f"{model}/{i}/{k}"]
        assert got.shape == want.shape and got.dtype == want.dtype, k
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{k}: max |diff| {np.abs(got - want).max()}"
    assert {k for k in golden[model].files if k.startswith(f"{model}/{i}/")} == {f"{model}/{i}/{k}" for k in out}


def record(path, models):
    """What one file of `golden` holds, from the library of the tree this runs in."""
    b = {k: f() for k, f in BATCHES.items()}
    arrays = {}
    for model, i in (case for case in CASES if case[0] in models):
        c = CONFIGS[model][i]
        facts, _, out = run(model, c, b[c["batch"]])
        assert facts["exact_reruns"] == 0, (model, i)
        arrays.update({f"{model}/{i}/{k}": v for k, v in out.items()})
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(arrays)} arrays of the configurations of {', '.join(models)}")


if __name__ == "__main__":
    record(sys.argv[1], sys.argv[2:])
