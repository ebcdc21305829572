"""Which kernels a GCN / GAT / DGN / PNA forward runs (flowgnn_amd/csrc/gcn_plan.h: gcn_plan, gat_plan.h: gat_plan, dgn_plan.h: dgn_plan,
pna_plan.h: pna_plan) on the CPU, on EVERY input.

Up to and including commit fe3f5ae the decision was spread over GcnModel / GatModel: use_resident, one_pass, needs_csr,
wants_packed_tile_lists, the instance chains and the post-passes of the resident launch, and the conditions of the per-layer path.
`gcn_parent_plan` / `gat_parent_plan` below transcribe those statement by statement (gcn.hip / gat.hip at fe3f5ae, line numbers in the
comments), vectorised over the cases; the headers' functions must agree with them on the full product of their inputs: every flag both
ways, the tile fill on both sides of the 0.5 threshold and at it, num_tasks 1 and 2, the three pooling modes.

DGN and PNA followed at 1ac249e, where DgnModel / PnaModel still held use_fused, use_mfma_agg, use_resident, needs_csr and forward's own
locals: `dgn_parent_plan` / `pna_parent_plan` transcribe dgn.hip / pna.hip of that commit in the same way.  Their fill threshold is 0.4;
DGN's density rule (job_e >= 8 job_n) is taken one edge under, at and one edge over it, dgn_mfma_agg over -1, 0, 1 and dgn_resident over
0, 1, 2."""
import numpy as np
import pytest

from tests import resident_plan as rp

MEAN, SUM, MAX = 0, 1, 2  # FLOWGNN_POOL_*
FIXED, RESIDENT, PER_LAYER = range(3)  # rp.PATHS
GCN_DEFAULT, GCN_ROWS, GCN_POOLSUM, GCN_NLOGIT = range(4)  # rp.INSTANCES["GCN"]
GAT_DEFAULT, GAT_POOLSUM, GAT_ATTN, GAT_NLOGIT = range(4)  # rp.INSTANCES["GAT"]
INST_DEFAULT, INST_EMB, INST_ROWS = range(3)  # rp.INSTANCES["DGN"], rp.INSTANCES["PNA"]


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


@pytest.fixture(scope="module")
def dgn(lib):
    cases = rp.full_product("DGN")
    return cases, rp.plan(lib, "DGN", cases)


@pytest.fixture(scope="module")
def pna(lib):
    cases = rp.full_product("PNA")
    return cases, rp.plan(lib, "PNA", cases)


def gcn_parent_plan(c):
    """gcn.hip at fe3f5ae: GcnModel::use_resident .. forward (lines 1322-1499)."""
    f = {k: c[k].astype(bool) for k in c if k not in ("fill_i", "pooling")}
    fill, pooling = rp.FILLS["GCN"][c["fill_i"]], c["pooling"]
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
    fill, pooling = rp.FILLS["GAT"][c["fill_i"]], c["pooling"]
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


def dgn_parent_plan(c):
    """dgn.hip at 1ac249e: DgnModel::wants_packed_tile_lists .. forward (lines 1682-1848)."""
    two_bit = ("mfma_agg", "resident", "fill_i", "density")
    f = {k: c[k].astype(bool) for k in c if k not in two_bit}
    fill, mfma_agg, resident = rp.FILLS["DGN"][c["fill_i"]], c["mfma_agg"].astype(int) - 1, c["resident"]
    job_n, job_e = rp.DGN_JOB_N, 8 * rp.DGN_JOB_N - 1 + c["density"].astype(np.int64)
    use_fused = f["fused"] & f["split"] & ~f["exact"] & f["tiles"] & (fill >= 0.4)  # 1686
    use_mfma_agg = np.where(mfma_agg < 0, job_e.astype(float) >= 8.0 * float(job_n), mfma_agg != 0)  # 1689
    use_resident = (resident != 0) & ~f["keep_h"] & ~f["qmode"] & f["eigen"] & use_fused & ((resident == 2) | use_mfma_agg)  # 1694
    p = {"wants_packed_tile_lists": f["fused"] & (resident != 0) & f["binpack"] & ~f["qmode"],  # 1682
         # 1698: if (db.b.n_tot > 0 && use_resident(db)) return false;  1699
         "needs_csr": ~(f["nonempty"] & use_resident)
                      & ~(f["rowinfo_direct"] & ~f["qmode"] & f["nonempty"] & f["eigen"] & use_fused & use_mfma_agg)}
    # 1741: if (n <= 0) return 0;  1742: if (!db.node_eigen) return 1; -- no launch, so no flag of the plan; 1744: if (qmode_) return
    # dgnq_forward(...) (the header names the fixed-point path for every fixed-point input; with 1741 / 1742 in front nothing runs
    # either way);  1746: if (use_resident(db)) return forward_resident(...);  1747-: the per-layer kernels
    runs = f["nonempty"] & f["eigen"]
    p["path"] = np.where(f["qmode"], FIXED, np.where(runs & use_resident, RESIDENT, PER_LAYER))
    res, per = p["path"] == RESIDENT, runs & (p["path"] == PER_LAYER)
    p["bin_packed"] = res & f["binpack"] & f["bp_lists"]  # 1707
    p["instance"] = np.where(res, np.where(f["node_emb"], INST_ROWS, np.where(f["emb"], INST_EMB, INST_DEFAULT)), INST_DEFAULT)  # 1730-1732
    p["fused_layers"] = per & use_fused  # 1751, 1773
    p["prepare_aggregate"] = per & ~use_fused  # 1753
    p["edge_scalar"] = p["prepare_aggregate"] & f["edges"]  # 1662
    direct = p["fused_layers"] & use_mfma_agg & f["rowinfo_direct"] & ~f["csr_built"]  # 1759
    p["rowinfo_from_edge_list"] = direct  # 1760
    p["mfma_aggregation"] = p["fused_layers"] & use_mfma_agg  # 1778-1779
    p["first_layer_makes_rowinfo"] = p["mfma_aggregation"] & ~direct  # 1782: stored = direct || l > 0, at l == 0;  1800: if (!stored)
    p["pooled_last"] = p["mfma_aggregation"] & f["fold_readout"] & ~f["keep_h"] & ~f["node_emb"]  # 1791, at l == DGN_L - 1 (DGN_L = 4 > 1)
    p["split_dense"] = p["prepare_aggregate"] & f["split"] & ~f["exact"]  # 1818
    p["emb_readout"] = per & f["emb"]  # 1834, 1837
    return p


def pna_parent_plan(c):
    """pna.hip at 1ac249e: PnaModel::use_fused .. forward (lines 1193-1309)."""
    f = {k: c[k].astype(bool) for k in c if k != "fill_i"}
    fill = rp.FILLS["PNA"][c["fill_i"]]
    use_fused = f["fused"] & ~f["qmode"] & f["split"] & ~f["exact"] & f["tiles"] & (fill >= 0.4)  # 1194
    use_resident = f["resident"] & ~f["keep_h"] & use_fused  # 1197
    p = {"needs_csr": ~(f["tile_build"] & use_resident),  # 1199
         "wants_packed_tile_lists": f["binpack"] & f["tile_build"] & f["resident"] & f["fused"] & ~f["qmode"]}  # 1201
    # 1248: if (qmode_) return pnaq_forward(...);  1250: if (use_resident(db)) return forward_resident(...);  1251-: the per-layer kernels
    p["path"] = np.where(f["qmode"], FIXED, np.where(use_resident, RESIDENT, PER_LAYER))
    res, per = p["path"] == RESIDENT, p["path"] == PER_LAYER
    p["bin_packed"] = res & f["binpack"] & f["tile_build"] & f["bp_lists"]  # 1206
    p["one_pass"] = res & f["tile_build"]  # 1211
    p["instance"] = np.where(res, np.where(f["node_emb"], INST_ROWS, np.where(f["emb"], INST_EMB, INST_DEFAULT)), INST_DEFAULT)  # 1236-1238
    p["fused_layers"] = per & use_fused  # 1258, 1262
    p["split_dense"] = per & ~use_fused & f["split"] & ~f["exact"]  # 1284
    p["emb_readout"] = per & f["emb"]  # 1301
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


def test_dgn_plan_agrees_with_the_parents_conditions(dgn):
    cases, got = dgn
    assert len(cases["density"]) == 2 ** 16 * 3 ** 4
    assert_same("DGN", cases, got, dgn_parent_plan(cases))


def test_pna_plan_agrees_with_the_parents_conditions(pna):
    cases, got = pna
    assert len(cases["fill_i"]) == 2 ** 12 * 3
    assert_same("PNA", cases, got, pna_parent_plan(cases))


def test_every_path_and_every_instance_is_reached(gcn, gat, dgn, pna):
    for model, (cases, p) in (("GCN", gcn), ("GAT", gat), ("DGN", dgn), ("PNA", pna)):
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


def test_pna_needs_csr_is_the_one_pass_resident_forward(pna):
    _, p = pna
    assert np.array_equal(~p["needs_csr"], (p["path"] == RESIDENT) & p["one_pass"])
    assert not (p["one_pass"] & (p["path"] != RESIDENT)).any() and not (p["bin_packed"] & ~p["one_pass"]).any()


def test_dgn_needs_csr_is_the_resident_forward_or_the_one_eligible_for_the_edge_list_pass(dgn):
    """The engine asks needs_csr before it builds the index, so without csr_built; forward decides on the edge-list pass after, with it.
    The pass runs only where the engine was told to skip the build, and never on a batch whose index an earlier forward had built."""
    c, p = dgn
    eligible = p["mfma_aggregation"] & c["rowinfo_direct"].astype(bool)  # (the matrix-pipe layers of the per-layer path, option on)
    assert np.array_equal(~p["needs_csr"], (p["path"] == RESIDENT) | eligible)
    assert not (p["rowinfo_from_edge_list"] & p["needs_csr"]).any()
    assert not (p["rowinfo_from_edge_list"] & c["csr_built"].astype(bool)).any()
    assert np.array_equal(p["rowinfo_from_edge_list"], eligible & ~c["csr_built"].astype(bool))
    # needs_csr does not move with csr_built: the same answer for the two cases that differ in it alone
    other = {k: v for k, v in c.items() if k != "csr_built"}
    order = np.lexsort([c["csr_built"]] + [v for v in other.values()])
    assert np.array_equal(p["needs_csr"][order][0::2], p["needs_csr"][order][1::2])


def engine_allows(model, c):
    """The cases a caller can reach through the C ABI (engine.hip):
    - flowgnn_set_node_logits / flowgnn_set_pooling: no node logits with the sum or the maximum (each refuses while the other is on);
    - flowgnn_set_numeric_mode / flowgnn_set_embeddings / _node_embeddings / _node_logits / _attention / _pooling: in fixed point no
      optional output and no pooling but the mean (each refuses while the other is on); GcnModel::set_numeric_mode / set_num_tasks:
      fixed point is single-task;
    - flowgnn_set_attention: GAT only (GCN's plan has no such input);
    - flowgnn_set_node_logits / flowgnn_set_pooling: PNA and DGN have the mean alone and no node logits (their plans have no such inputs)."""
    if model in ("DGN", "PNA"):
        return ~(c["qmode"].astype(bool) & (c["emb"].astype(bool) | c["node_emb"].astype(bool)))
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


@pytest.mark.parametrize("model", ["DGN", "PNA"])
def test_dgn_pna_every_requested_output_has_exactly_one_writer(model, dgn, pna):
    cases, p = dgn if model == "DGN" else pna
    ok = engine_allows(model, cases)
    assert ok.any() and (~ok).any()
    if model == "DGN":  # a forward that runs: DgnModel::forward returns before its first launch without nodes or without the eigenvectors
        ok &= cases["nonempty"].astype(bool) & cases["eigen"].astype(bool)
    c = {k: v[ok] for k, v in cases.items()}
    p = {k: v[ok] for k, v in p.items()}
    emb, node_emb = c["emb"].astype(bool), c["node_emb"].astype(bool)
    fixed, res, per = p["path"] == FIXED, p["path"] == RESIDENT, p["path"] == PER_LAYER
    inst = lambda i: res & (p["instance"] == i)
    assert (fixed.astype(int) + res + per == 1).all()
    # the graph embeddings: the Emb instance, the Rows instance (which serves them too), or the per-layer readout
    assert np.array_equal(inst(INST_EMB).astype(int) + (inst(INST_ROWS) & emb) + p["emb_readout"], emb.astype(int))
    assert not (p["emb_readout"] & ~per).any()
    # the node embeddings: the Rows instance, or the last per-layer stage writing into the caller's buffer -- which must then write rows
    assert np.array_equal(inst(INST_ROWS).astype(int) + (per & node_emb), node_emb.astype(int))
    if model == "DGN":
        assert not (p["pooled_last"] & (node_emb | c["keep_h"].astype(bool))).any()
