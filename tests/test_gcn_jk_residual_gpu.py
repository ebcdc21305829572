"""OGB's GNN(JK="sum") and GNN(residual=True) for GCN on the GPU (flowgnn.h: flowgnn_set_model_jk_residual): gcn
and gcn-virtual at emb_dim 300 against the executable torch.nn model of tests/ogb_gcn_jk_torch.py, through the route a user takes --
model.state_dict() -> export_weights("GCN", ..., emb_dim=300[, virtual_node=True, virtual_node_dim=300]) -> .bin files ->
Engine.load_weights_dir -> Engine.set_jk_residual -> kernels.  The batch is tests.ogb_torch.gcn_batch(): 29 graphs, 765 nodes (a one-node
graph, isolated nodes, a 17-node ring, a 129-node path, 765 = 5 x 128 + 125 rows, tiles whose 16 rows belong to several graphs, a last
column tile masked at column 300).

Expected values: the torch model's own float64 forward.  Tolerance: the project's rule, |gpu - torch| <= 1e-4 (scale + |torch|), scale =
the largest magnitude the model's forward hooks saw (tests/parity.py; ogb_gcn_jk_torch.py says which hooks -- the smaller, stricter
set).  tests/test_gcn_jk_residual_cpu.py asserts on the references alone what is relied on here: every wrong form's rows miss that rule
by at least 10 x, the six damped models stay below half the split-f16 threshold, the undamped gcn-virtual ones leave it.  Every
comparison prints its ratio to the bound.  Every test that makes the call fails on a library without it.

  (a) parity of node embeddings (= r), graph embeddings and logits; no exact re-run; only gcn_wide_layer ran; the GPU's rows more than
      5 x the bound from every wrong form's rows.  The same checkpoint with the call not made misses the bound.
  (b) every readout reads r, under (sum, residual): mean / sum / max pooling, NUM_TASK = 3, node logits, and the attention and set2set
      readouts against tests/attn_pool_ref.py / tests/set2set_ref.py fed the float64 r.  The two softmax readouts run on gcn alone
      (section 4.24 says why: on the virtual-node model's r a dot product's fp32 rounding moves a softmax weight by more than the bound).
  (c) the exact (fp32) re-run on the undamped gcn-virtual models, one per setting.
  (d) bits: (LAST, 0) through the call is never calling; the JK store leaves h_5 = pre_4 as it was; placements (gcn: the same bits;
      gcn-virtual: within the bound, since the partial rows are cut at batch-relative tiles, section 4.19); a resident batch across
      settings; option hipgraph.
  (e) `host GCN --emb-dim 300 --ogb-vn --jk sum --residual`.
"""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from flowgnn_amd import Engine, EngineGroup, export, graphpack as gp, weights  # noqa: E402
from tests import attn_pool_ref as A, ogb_gcn_jk_torch as K, ogb_torch as T, set2set_ref as S  # noqa: E402
from tests.parity import assert_close, err_ratio  # noqa: E402
from tests.test_embeddings_gpu import launched  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
MODELS = [(vn, jk, res) for vn in (False, True) for jk, res in K.SETTINGS]
name_of = lambda vn, jk, res: f"gcn{'-virtual' if vn else ''}-{jk}{'-res' if res else ''}"
IDS = [name_of(*m) for m in MODELS]
VN_IDS = ["gcn", "gcn-virtual"]


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    if torch.cuda.is_available():
        torch.cuda.init()


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    """(vn, jk, res, tasks, damped) -> the directory export_weights wrote for that model: each written once."""
    done = {}

    def get(vn, jk="last", res=False, tasks=1, damped=True):
        key = (vn, jk, res, tasks, damped)
        if key not in done:
            d = tmp_path_factory.mktemp("w_" + name_of(vn, jk, res))
            model = K.make_model(vn, jk, res, num_tasks=tasks, damped=damped)
            kw = dict(virtual_node=True, virtual_node_dim=300) if vn else {}
            export.export_weights("GCN", model.state_dict(), str(d), emb_dim=300, multi_task=tasks != 1, **kw)
            done[key] = str(d)
        return done[key]
    return get


def engine(vn, directory, jk="last", res=False, tasks=1, pooling="mean", call=True, profile=True):
    """The width first, then the files, then the flags the model was trained with (they are in no file)."""
    e = Engine("GCN", device=0)
    e.set_model_emb_dim(300)
    if tasks != 1:
        e.set_num_tasks(tasks)
    e.load_weights_dir(directory, virtual_node=vn)
    if pooling != "mean":
        e.set_pooling(pooling)
    if call:
        e.set_jk_residual(jk, res)
        assert e.jk_residual() == (jk, res)
    if profile:
        e.profile_enable(True)
    return e


def group(vn, directory, jk, res):
    g = EngineGroup("GCN", [0, 0])
    g.set_model_emb_dim(300)
    g.load_weights_dir(directory)
    if vn:
        g.set_gcn_virtual_node(weights.load_gcn_virtual_node(directory, emb_dim=300))
    g.set_jk_residual(jk, res)
    return g


def close(got, want, scale, what, rel=1e-4):
    print(what, f"err_ratio {err_ratio(got, want, scale, rel):.4f} (scale {scale:.4g})")
    assert_close(got, want, scale=scale, rel=rel, what=what)


def all_three(e, b=None):
    logits, pooled, rows = (np.array(x) for x in e.forward(T.gcn_batch() if b is None else b, return_embeddings=True, return_node_embeddings=True))
    return logits, pooled, rows


# ---------------------------------------------------------------- (a) parity with the torch model
@pytest.mark.parametrize("vn,jk,res", MODELS, ids=IDS)
def test_checkpoint_parity(vn, jk, res, exported):
    want, scale, _ = K.expected(vn, jk, res)
    e = engine(vn, exported(vn, jk, res), jk, res)
    try:
        logits, pooled, rows = all_three(e)
        names = launched(e, lambda: e.run())
        assert e.exact_reruns() == 0
    finally:
        e.close()
    what = name_of(vn, jk, res)
    close(rows, want.rows, scale, (what, "rows"))
    close(pooled, want.pooled, scale, (what, "pooled"))
    close(logits, want.logits, scale, (what, "logits"))
    assert "gcn_wide_layer" in names and "gcn_wide_layer_f32" not in names and "gcn_wide_x0" in names, names
    for v in K.variants_of(vn, jk, res):
        r = err_ratio(K.variant_rows(vn, jk, res, v), rows, scale)
        print(what, "wrong form", v, f"{r:.1f} x the bound from the GPU's rows")
        assert r > 5.0, (v, r)


@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_the_setting_is_what_makes_the_difference(vn, exported):
    """The same files without the call: the rows of a JK='last', residual=False model miss the bound of the trained one's."""
    want, scale, _ = K.expected(vn, "sum", True)
    e = engine(vn, exported(vn, "sum", True), call=False)
    try:
        assert e.jk_residual() == ("last", False)
        rows = np.array(e.forward(T.gcn_batch(), return_node_embeddings=True)[1])
    finally:
        e.close()
    r = err_ratio(rows, want.rows, scale)
    print(name_of(vn, "sum", True), "without the call", f"{r:.1f} x the bound")
    assert r > 1.0


# ---------------------------------------------------------------- (b) every readout reads r
@pytest.mark.parametrize("pooling", ["mean", "sum", "max"])
@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_every_pooling_pools_r(vn, pooling, exported):
    want, scale, _ = K.expected(vn, "sum", True, pooling=pooling)
    e = engine(vn, exported(vn, "sum", True), "sum", True, pooling=pooling)
    try:
        logits, pooled, rows = all_three(e)
        assert e.exact_reruns() == 0
    finally:
        e.close()
    what = (name_of(vn, "sum", True), pooling)
    close(rows, want.rows, scale, (what, "rows"))
    close(pooled, want.pooled, scale, (what, "pooled"))
    close(logits, want.logits, scale, (what, "logits"))


@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_three_tasks(vn, exported):
    want, scale, _ = K.expected(vn, "sum", True, num_tasks=3)
    e = engine(vn, exported(vn, "sum", True, tasks=3), "sum", True, tasks=3)
    try:
        logits, pooled, rows = all_three(e)
        assert e.exact_reruns() == 0
    finally:
        e.close()
    assert want.logits.shape == (T.gcn_batch().num_graphs, 3) == logits.shape
    close(rows, want.rows, scale, (name_of(vn, "sum", True), "3 tasks", "rows"))
    close(logits, want.logits, scale, (name_of(vn, "sum", True), "3 tasks", "logits"))


@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_node_logits_are_each_nodes_share_of_r(vn, exported):
    want, scale, _ = K.expected(vn, "sum", True)
    d = exported(vn, "sum", True)
    w, _ = K.load(d, vn)
    e = engine(vn, d, "sum", True)
    try:
        logits, rows, terms = (np.array(x) for x in e.forward(T.gcn_batch(), return_node_embeddings=True, return_node_logits=True))
    finally:
        e.close()
    what = name_of(vn, "sum", True)
    close(rows, want.rows, scale, (what, "rows beside node logits"))
    close(terms, K.node_logits(w, want.rows), scale, (what, "node logits"))
    b = T.gcn_batch()
    means = np.add.reduceat(terms.astype(np.float64), b.node_offsets()[:-1]) / b.nums_of_nodes
    close(means, want.logits, scale, (what, "mean of the node logits"))
    close(logits, want.logits, scale, (what, "logits"))


def test_attention_readout_reads_r(exported):
    want, scale, _ = K.expected(False, "sum", True)
    d = exported(False, "sum", True)
    w, _ = K.load(d, False)
    gate, b = weights.synth_attention_pooling(), T.gcn_batch()
    stats = {}
    pooled, logits, _ = A.readout(want.rows, b, gate, w["graph_pred_weights"], w["graph_pred_bias"], stats=stats)
    scale = max(scale, stats["s_max"], stats["hidden_max"])
    e = engine(False, d, "sum", True)
    try:
        e.set_attention_pooling(gate)
        got, emb, rows = all_three(e)
        names = launched(e, lambda: e.run())
    finally:
        e.close()
    assert "attn_gate" in names and "attn_pool_rows" in names, names
    close(rows, want.rows, scale, ("attention", "rows"))
    close(emb, pooled, scale, ("attention", "pooled"))
    close(got, logits, scale, ("attention", "logits"))


def test_set2set_readout_reads_r(exported):
    want, scale, _ = K.expected(False, "sum", True)
    d = exported(False, "sum", True)
    s2s, b = weights.synth_set2set(), T.gcn_batch()
    stats = {}
    q, logits, _ = S.readout(want.rows, b, s2s, steps=2, stats=stats)
    scale = max(scale, stats["q_max"], stats["e_max"], float(np.abs(logits).max()))
    e = engine(False, d, "sum", True)
    try:
        e.set_set2set_pooling(s2s, steps=2)
        got, rows = (np.array(x) for x in e.forward(b, return_node_embeddings=True))
        names = launched(e, lambda: e.run())
    finally:
        e.close()
    assert "s2s_lstm" in names and "s2s_head" in names, names
    close(rows, want.rows, scale, ("set2set", "rows"))
    close(got, logits, scale, ("set2set", "logits"))


# ---------------------------------------------------------------- (c) the exact re-run
@pytest.mark.parametrize("jk,res", K.SETTINGS, ids=[f"{jk}{'-res' if res else ''}" for jk, res in K.SETTINGS])
def test_exact_rerun(jk, res, exported):
    """The undamped gcn-virtual models (tests/test_gcn_jk_residual_cpu.py asserts that their largest split operand passes the
    threshold): the pass is repeated once on the fp32 pipe, with the adds of gin_wide_jk.hip's element-wise kernel in the fast path's
    order, and lands inside the same bound."""
    want, scale, _ = K.expected(True, jk, res, damped=False)
    e = engine(True, exported(True, jk, res, damped=False), jk, res)
    try:
        logits, pooled, rows = all_three(e)
        reruns = e.exact_reruns()
        names = launched(e, lambda: e.run())
    finally:
        e.close()
    what = (name_of(True, jk, res), "undamped")
    print(what, "exact_reruns", reruns)
    assert reruns == 1 and "gcn_wide_layer_f32" in names, (reruns, names)
    close(rows, want.rows, scale, (what, "rows"))
    close(pooled, want.pooled, scale, (what, "pooled"))
    close(logits, want.logits, scale, (what, "logits"))


# ---------------------------------------------------------------- (d) bits
@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_the_default_through_the_call_is_never_calling(vn, exported):
    d = exported(vn)
    outs, slots = [], []
    for call in (False, True):
        e = engine(vn, d, "last", False, call=call)
        try:
            outs.append(all_three(e))
            slots.append({k: v["launches"] for k, v in e.profile_read().items()})
        finally:
            e.close()
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    assert slots[0] == slots[1] and "gcn_wide_x0" not in slots[0], slots


@pytest.mark.parametrize("node_emb", [False, True], ids=["", "node-embeddings"])
@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_the_jk_store_leaves_h5_as_it_was(vn, node_emb, exported):
    """(sum, off): final_h() is the plain run's pre_4 byte for byte, and the plain run's node embeddings ARE that pre_4."""
    d, b = exported(vn), T.gcn_batch()
    plain = engine(vn, d, call=False)
    try:
        plain.forward(b)
        h5 = plain.final_h().copy()
        rows_plain = np.array(plain.forward(b, return_node_embeddings=True)[1])
    finally:
        plain.close()
    assert h5.tobytes() == rows_plain.tobytes()
    e = engine(vn, d, "sum", False)
    try:
        r = np.array(e.forward(b, return_node_embeddings=True)[1]) if node_emb else None
        if not node_emb:
            e.forward(b)
        got = e.final_h().copy()
    finally:
        e.close()
    assert got.tobytes() == h5.tobytes()
    if node_emb:
        assert r.tobytes() != h5.tobytes()  # the node embeddings are the sum, not h_5


@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_placements(vn, exported):
    """A host batch, both device layouts and two runs: the same bits.  A permuted batch, a slice and a two-member group give each graph
    the same bits for plain gcn; for gcn-virtual they agree within the bound only (the partial rows are cut at batch-relative tiles)."""
    from tests.test_device_batch_gpu import device_args
    want, scale, _ = K.expected(vn, "sum", True)
    d, b = exported(vn, "sum", True), T.gcn_batch()
    G, off = b.num_graphs, b.node_offsets()
    perm = np.random.default_rng(5).permutation(G)
    shuffled = gp.concat_batches([b.slice(int(i), int(i) + 1) for i in perm])
    e = engine(vn, d, "sum", True)
    try:
        logits, pooled, rows = all_three(e)
        again = all_three(e)
        for layout in ("pyg", "reference"):
            args, kw = device_args(b, layout, "GCN")
            got = e.forward_device(*args, return_embeddings=True, return_node_embeddings=True, **kw)
            e.sync()
            for x, y in zip(got, (logits, pooled, rows)):
                assert np.array_equal(x.cpu().numpy().reshape(y.shape), y), layout
        s_logits, s_pooled, s_rows = all_three(e, shuffled)
        e.set_job_totals(b.total_nodes, b.total_edges)
        p_logits, p_pooled, p_rows = all_three(e, b.slice(5, 27))
        e.set_job_totals(-1, -1)
        assert e.exact_reruns() == 0
    finally:
        e.close()
    for x, y in zip(again, (logits, pooled, rows)):
        assert x.tobytes() == y.tobytes()
    g = group(vn, d, "sum", True)
    try:
        g.set_embeddings(True)
        g.set_node_embeddings(True)
        g_logits = np.array(g.forward(b))
        g_pooled, g_rows = np.array(g.embeddings()), np.array(g.node_embeddings()).reshape(rows.shape)
    finally:
        g.close()
    soff = shuffled.node_offsets()
    s_rows_back = np.concatenate([s_rows[soff[k]:soff[k + 1]] for k in np.argsort(perm)])
    inv = np.argsort(perm)
    pairs = [("permuted logits", s_logits[inv], logits), ("permuted pooled", s_pooled[inv], pooled), ("permuted rows", s_rows_back, rows),
             ("slice logits", p_logits, logits[5:27]), ("slice pooled", p_pooled, pooled[5:27]), ("slice rows", p_rows, rows[off[5]:off[27]]),
             ("group logits", g_logits, logits), ("group pooled", g_pooled, pooled), ("group rows", g_rows, rows)]
    for what, x, y in pairs:
        if vn:
            close(x, y, scale, (name_of(vn, "sum", True), what))
        else:
            assert np.array_equal(x, y), what


@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_the_setting_changes_between_runs_on_a_resident_batch(vn, exported):
    d, b = exported(vn, "sum", True), T.gcn_batch()
    plain = engine(vn, d, call=False)
    try:
        base = [x.copy() for x in all_three(plain)]
    finally:
        plain.close()
    e = engine(vn, d, "sum", True)
    try:
        e.set_embeddings(True)
        e.set_node_embeddings(True)
        e.set_batch(b)
        runs = []
        for jk, res in (("sum", True), ("last", False), ("sum", True), ("last", True), ("sum", False)):
            e.set_jk_residual(jk, res)
            e.run()
            runs.append([np.array(x).copy() for x in (e.results(), e.embeddings(), e.node_embeddings())])
    finally:
        e.close()
    for x, y in zip(runs[0], runs[2]):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(runs[1], base):
        assert x.tobytes() == y.tobytes()
    assert len({r[0].tobytes() for r in runs}) == 4  # four settings, four answers


def test_hipgraph_replay_follows_the_setting(exported):
    """Option hipgraph: the call drops the recorded launch sequence, and the new one is recorded and replayed in its turn."""
    d, b = exported(True, "sum", True), T.gcn_batch()
    direct = engine(True, d, "sum", True)
    try:
        expected = np.array(direct.forward(b)).copy()
    finally:
        direct.close()
    h = Engine("GCN", device=0, options={"hipgraph": 2})  # (no profiling: a profiled run is launched directly)
    try:
        h.set_model_emb_dim(300)
        h.load_weights_dir(d, virtual_node=True)
        h.set_batch(b)
        for _ in range(3):
            h.run()
        last = h.results().copy()
        assert h.graph_replays() >= 1
        h.set_jk_residual("sum", True)  # drops the recorded sequence
        h.run()
        first = h.results().copy()
        before = h.graph_replays()
        outs = []
        for _ in range(3):
            h.run()
            outs.append(h.results().copy())
        assert h.graph_replays() > before
        h.set_jk_residual("last", False)
        h.run()
        off = h.results().copy()
    finally:
        h.close()
    assert np.array_equal(first, expected) and all(np.array_equal(o, expected) for o in outs)
    assert np.array_equal(off, last) and not np.array_equal(first, last)


# ---------------------------------------------------------------- (e) the host CLI
@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_host_cli_300_jk_residual(vn, exported, tmp_path):
    """`host GCN --emb-dim 300 [--ogb-vn] --jk sum --residual` on a written pack and the exported directory."""
    want, scale, _ = K.expected(vn, "sum", True)
    gdir, out = tmp_path / "graphs", tmp_path / "HLS_output.txt"
    gp.write_pack(T.gcn_batch(), str(gdir))
    p = subprocess.run([HOST, "GCN", "--emb-dim", "300"] + (["--ogb-vn"] if vn else []) +
                       ["--jk", "sum", "--residual", "--graphs", str(gdir), "--weights", exported(vn, "sum", True), "--trials", "1", "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    close(got, want.logits, scale, (name_of(vn, "sum", True), "host CLI"))
