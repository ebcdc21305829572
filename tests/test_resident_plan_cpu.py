"""Which kernels a GCN / GAT forward runs (flowgnn_amd/csrc/gcn_plan.h: gcn_plan, gat_plan.h: gat_plan) on the CPU, on EVERY input.

Up to and including commit fe3f5ae the decision was spread over GcnModel / GatModel: use_resident, one_pass, needs_csr,
wants_packed_tile_lists, the instance chains and the post-passes of the resident launch, and the conditions of the per-layer path.
`gcn_parent_plan` / `gat_parent_plan` below transcribe those statement by statement (gcn.hip / gat.hip at fe3f5ae, line numbers in the
comments), vectorised over the cases; the headers' functions must agree with them on the full product of their inputs: every flag both
ways, the tile fill on both sides of the 0.5 threshold and at it, num_tasks 1 and 2, the three pooling modes."""
import numpy as np
import pytest

from tests import resident_plan as rp

MEAN, SUM, MAX = 0, 1, 2  # FLOWGNN_POOL_*
FIXED, RESIDENT, PER_LAYER = range(3)  # rp.PATHS
GCN_DEFAULT, GCN_ROWS, GCN_POOLSUM, GCN_NLOGIT = range(4)  # rp.INSTANCES["GCN"]
GAT_DEFAULT, GAT_POOLSUM, GAT_ATTN, GAT_NLOGIT = range(4)  # rp.INSTANCES["GAT"]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return rp.build_shim(tmp_path_factory.mktemp("resident_plan"))


@pytest.fixture(scope="module")
def gcn(lib):
    cases = rp.full_product("GCN")
    return cases, rp.plan(lib, "GCN", cases)


@pytest.fixture(scope="module")
def gat(lib):
    cases = rp.full_product("GAT")
    return cases, rp.plan(lib, "GAT", cases)


def gcn_parent_plan(c):
    """gcn.hip at fe3f5ae: GcnModel::use_resident .. forward (lines 1322-1499)."""
    f = {k: c[k].astype(bool) for k in c if k not in ("fill_i", "pooling")}
    fill, pooling = rp.FILLS[c["fill_i"]], c["pooling"]
    num_tasks = 1 + c["two_tasks"].astype(int)
    # 1327-1328: use_resident
    use_resident = (f["resident"] & f["table_ok"] & ~f["qmode"] & ~f["keep_h"] & (~f["emb"] | f["node_emb"]) & f["split"] & ~f["exact"] & f["fused"]
                    & (num_tasks == 1) & f["tiles"] & (fill >= 0.5) & (pooling != MAX))
    one_pass = f["tile_build"] & use_resident & f["edge_attr"]  # 1332
    p = {"needs_csr": ~one_pass,  # 1333
         "wants_packed_tile_lists": f["binpack"] & f["tile_build"] & f["resident"] & ~f["qmode"] & (num_tasks == 1)}  # 1334
    # 1341: if (qmode_) return gcnq_forward(...);  1342: if (use_resident(db)) { ... return 0; }  1418-: the per-layer kernels
    p["path"] = np.where(f["qmode"], FIXED, np.where(use_resident, RESIDENT, PER_LAYER))
    res, per = p["path"] == RESIDENT, p["path"] == PER_LAYER
    p["one_pass"] = res & one_pass  # 1344
    p["bin_packed"] = p["one_pass"] & f["binpack"] & f["bp_lists"]  # 1347
    # 1358 / 1363 / 1368 / 1373 behind the one-pass front end, 1384 / 1388 / 1392 / 1396 behind the CSR front end: the same chain
    chain = np.where(f["node_emb"], GCN_ROWS, np.where(pooling == SUM, GCN_POOLSUM, np.where(f["node_logits"], GCN_NLOGIT, GCN_DEFAULT)))
    p["instance"] = np.where(res, chain, GCN_DEFAULT)
    p["sum_from_rows"] = res & f["node_emb"] & (pooling == SUM)  # 1405
    fast = f["split"] & ~f["exact"] & f["fused"]
    p["fused_encoder"] = per & fast  # 1420
    p["fused_layers"] = per & fast & f["edges"]  # 1434
    p["folded_last"] = per & fast & f["edges"] & (num_tasks == 1) & ~f["emb"] & ~f["node_emb"] & (pooling != MAX)  # 1457
    p["node_logits_from_scores"] = p["folded_last"] & f["node_logits"]  # 1471
    unfolded = per & ~p["folded_last"]  # (1475: the folded last stage returns)
    p["multi_task"] = unfolded & (num_tasks > 1)  # 1485
    p["pool_rows"] = (res & f["emb"]) | (unfolded & f["emb"])  # 1401, 1490
    p["node_logits_from_rows"] = (res & f["node_emb"] & f["node_logits"]) | (unfolded & f["node_logits"])  # 1409, 1494
    return p


def gat_parent_plan(c):
    """gat.hip at fe3f5ae: GatModel::forward (lines 1168-1294)."""
    f = {k: c[k].astype(bool) for k in c if k not in ("fill_i", "pooling")}
    fill, pooling = rp.FILLS[c["fill_i"]], c["pooling"]
    # 1188-1189
    resident = (f["resident"] & ~f["keep_h"] & ~f["emb"] & ~f["node_emb"] & f["fold_readout"] & f["split"] & ~f["exact"] & f["tiles"] & (fill >= 0.5)
                & ((pooling == MEAN) | ((pooling == SUM) & ~f["attention"])))
    p = {"path": np.where(f["qmode"], FIXED, np.where(resident, RESIDENT, PER_LAYER))}  # 1181: if (qmode_) return gatq_forward(...); 1188; 1222-
    res, per = p["path"] == RESIDENT, p["path"] == PER_LAYER
    # 1202 / 1205 / 1209 / 1213
    chain = np.where(pooling == SUM, GAT_POOLSUM, np.where(f["attention"], GAT_ATTN, np.where(f["node_logits"], GAT_NLOGIT, GAT_DEFAULT)))
    p["instance"] = np.where(res, chain, GAT_DEFAULT)
    p["fold"] = per & f["fold_readout"] & ~f["emb"] & ~f["node_emb"] & (pooling != MAX)  # 1228
    p["split_products"] = per & f["split"] & ~f["exact"]  # 1241
    p["attention_kernels"] = per & f["attention"]  # 1242: (db.attn_mask >> l) & 1, for some l
    p["pool_rows"] = per & f["emb"]  # 1283
    p["node_logits_from_scores"] = per & f["node_logits"] & p["fold"]  # 1287, 1290
    p["node_logits_from_rows"] = per & f["node_logits"] & ~p["fold"]  # 1287, 1291
    return p


def assert_same(model, cases, got, want):
    assert set(got) == set(want)
    for k in got:
        bad = np.flatnonzero(got[k] != want[k])
        first = {} if not len(bad) else {f: int(cases[f][bad[0]]) for f in cases}
        assert not len(bad), f"{model} plan.{k}: {len(bad)} of {len(got[k])} cases differ from the parent, the first: {first}"


def test_gcn_plan_agrees_with_the_parents_conditions(gcn):
    cases, got = gcn
    assert len(cases["pooling"]) == 2 ** 17 * 3 * 3
    assert_same("GCN", cases, got, gcn_parent_plan(cases))


def test_gat_plan_agrees_with_the_parents_conditions(gat):
    cases, got = gat
    assert len(cases["pooling"]) == 2 ** 11 * 3 * 3
    assert_same("GAT", cases, got, gat_parent_plan(cases))


def test_every_path_and_every_instance_is_reached(gcn, gat):
    for model, (cases, p) in (("GCN", gcn), ("GAT", gat)):
        assert set(np.unique(p["path"])) == {FIXED, RESIDENT, PER_LAYER}
        assert set(np.unique(p["instance"][p["path"] == RESIDENT])) == set(range(len(rp.INSTANCES[model])))
        assert (p["instance"][p["path"] != RESIDENT] == 0).all()  # no instance off the resident path
        for k in p:  # every flag of the plan is set somewhere and clear somewhere
            assert len(np.unique(p[k])) > 1, (model, k)


def test_gcn_needs_csr_is_the_one_pass_resident_forward(gcn):
    """The engine asks needs_csr before forward (engine_forward): both read the one plan, and the index build is skipped exactly where
    that plan runs the resident kernel behind the one-pass front end."""
    _, p = gcn
    assert np.array_equal(~p["needs_csr"], (p["path"] == RESIDENT) & p["one_pass"])
    assert not (p["one_pass"] & (p["path"] != RESIDENT)).any() and not (p["bin_packed"] & ~p["one_pass"]).any()


def engine_allows(model, c):
    """The cases a caller can reach through the C ABI (engine.hip):
    - flowgnn_set_node_logits / flowgnn_set_pooling: no node logits with the sum or the maximum (each refuses while the other is on);
    - flowgnn_set_numeric_mode / flowgnn_set_embeddings / _node_embeddings / _node_logits / _attention / _pooling: in fixed point no
      optional output and no pooling but the mean (each refuses while the other is on); GcnModel::set_numeric_mode / set_num_tasks:
      fixed point is single-task;
    - flowgnn_set_attention: GAT only (GCN's plan has no such input)."""
    q, nl, pooling = c["qmode"].astype(bool), c["node_logits"].astype(bool), c["pooling"]
    extra = c["emb"].astype(bool) | c["node_emb"].astype(bool) | nl
    if model == "GAT":
        extra = extra | c["attention"].astype(bool)
    ok = ~(nl & (pooling != MEAN)) & ~(q & (extra | (pooling != MEAN)))
    if model == "GCN":
        ok &= ~(q & c["two_tasks"].astype(bool))
    return ok


def test_gcn_every_requested_output_has_exactly_one_writer(gcn):
    cases, p = gcn
    ok = engine_allows("GCN", cases)
    assert ok.any() and (~ok).any()
    c = {k: v[ok] for k, v in cases.items()}
    p = {k: v[ok] for k, v in p.items()}
    emb, node_emb, node_logits, pooling = c["emb"].astype(bool), c["node_emb"].astype(bool), c["node_logits"].astype(bool), c["pooling"]
    fixed, res, per = p["path"] == FIXED, p["path"] == RESIDENT, p["path"] == PER_LAYER
    inst = lambda i: res & (p["instance"] == i)
    unfolded = per & ~p["folded_last"]  # the last stage leaves rows (in the caller's node-embedding buffer when that is on)
    # the logits: one path, and on it one readout of the pooling asked for.  The resident kernel's own readout is the mean, the sum
    # instance's the sum; behind the storing instance the sum is taken from the rows, which replaces the kernel's mean
    assert (fixed.astype(int) + res + per == 1).all()
    assert not (res & (pooling == MAX)).any()
    assert np.array_equal(res & (pooling == SUM), inst(GCN_POOLSUM) | p["sum_from_rows"])
    assert not (inst(GCN_POOLSUM) & p["sum_from_rows"]).any() and not (p["sum_from_rows"] & ~inst(GCN_ROWS)).any()
    assert not (per & p["folded_last"] & p["multi_task"]).any()
    assert np.array_equal(per & c["two_tasks"].astype(bool), p["multi_task"])  # two tasks: the multi-task readout, and only there
    # the graph embeddings: pooled from rows that are in HBM
    assert np.array_equal(p["pool_rows"], emb)
    assert not (p["pool_rows"] & ~(inst(GCN_ROWS) | unfolded)).any()
    # the node embeddings: the storing instance, or the un-folded last stage
    assert np.array_equal(inst(GCN_ROWS).astype(int) + (unfolded & node_emb), node_emb.astype(int))
    # the node logits: their instance, or from the rows, or from the folded scores
    writers = inst(GCN_NLOGIT).astype(int) + p["node_logits_from_rows"] + p["node_logits_from_scores"]
    assert np.array_equal(writers, node_logits.astype(int))
    assert not (p["node_logits_from_rows"] & ~(inst(GCN_ROWS) | unfolded)).any()
    assert not (p["node_logits_from_scores"] & ~p["folded_last"]).any()


def test_gat_every_requested_output_has_exactly_one_writer(gat):
    cases, p = gat
    ok = engine_allows("GAT", cases)
    assert ok.any() and (~ok).any()
    c = {k: v[ok] for k, v in cases.items()}
    p = {k: v[ok] for k, v in p.items()}
    emb, node_emb, node_logits, attention = (c[k].astype(bool) for k in ("emb", "node_emb", "node_logits", "attention"))
    pooling = c["pooling"]
    fixed, res, per = p["path"] == FIXED, p["path"] == RESIDENT, p["path"] == PER_LAYER
    inst = lambda i: res & (p["instance"] == i)
    # the logits: one path; the resident kernel's readout is the mean, the sum instance's the sum
    assert (fixed.astype(int) + res + per == 1).all()
    assert not (res & (pooling == MAX)).any()
    assert np.array_equal(res & (pooling == SUM), inst(GAT_POOLSUM))
    # the graph and the node embeddings: the per-layer path's 16-wide rows
    assert np.array_equal(p["pool_rows"], emb) and not (p["pool_rows"] & p["fold"]).any()
    assert np.array_equal(per & ~p["fold"] & node_emb, node_emb)
    # the node logits: their instance, the attention instance (which stores them too), or behind the per-layer readout
    writers = inst(GAT_NLOGIT).astype(int) + (inst(GAT_ATTN) & node_logits) + p["node_logits_from_scores"] + p["node_logits_from_rows"]
    assert np.array_equal(writers, node_logits.astype(int))
    assert not (p["node_logits_from_scores"] & ~p["fold"]).any() and not (p["node_logits_from_rows"] & p["fold"]).any()
    # the attention coefficients: their instance, or one kernel per selected layer
    assert np.array_equal(inst(GAT_ATTN).astype(int) + p["attention_kernels"], attention.astype(int))
