"""OGB's GNN(JK="sum") and GNN(residual=True) on the GPU (flowgnn.h: flowgnn_set_jk_residual): gin and gin-virtual
at emb_dim 300 against the executable torch.nn model of tests/ogb_jk_torch.py, through the route a user takes -- model.state_dict()
-> export_weights -> .bin files -> Engine.load_weights_dir -> Engine.set_jk_residual -> kernels.  The batch is tests.ogb_torch.gin_batch():
30 graphs, 771 nodes (a one-node graph, isolated nodes, a 17-node ring, a 129-node path, 771 = 6 x 128 + 3 rows, tiles whose 16 rows
belong to several graphs, a last column tile masked at column 300).

Expected values: the torch model's own float64 forward.  Tolerance: the project's rule, |gpu - torch| <= 1e-4 (scale + |torch|), scale =
the largest magnitude the model's forward hooks saw (tests/parity.py; ogb_jk_torch.py says which hooks -- the smaller, stricter set).
tests/test_jk_residual_cpu.py asserts on the references alone what is relied on here: every wrong form's rows miss that rule by at
least 10 x (smallest 12.7), the six damped models stay below half the split-f16 threshold, the two undamped ones leave it.  Every
comparison prints its ratio to the bound.  Every test here fails on a library without the call.

  (a) parity of logits, node embeddings (= r) and graph embeddings; no exact re-run; the GPU's rows more than 5 x the bound from every
      wrong form's rows (>= 10 x between the references, <= 1 x between the GPU and the right one).
  (b) every readout reads r, under (sum, residual): mean / sum / max pooling, NUM_TASK = 3, the attention and set2set readouts against
      tests/attn_pool_ref.py / tests/set2set_ref.py fed the float64 r, node logits.  The two softmax readouts run on gin alone: on
      gin-virtual's r (magnitudes of 5e3) a dot product's fp32 rounding, 1e-7 x 5e3 x sqrt(300), moves a softmax weight by 1e-2 and the
      weighted sum by 50, a hundred times the bound -- a property of that readout on such rows in fp32, whichever kernel computes it.
  (c) the f16 mode: logits within the project's f16 rule, 2e-4 (scale + |f64|) (F16_REL of tests/test_gin_wide_f16_gpu.py); rows printed
      with their ratio, not asserted (as section 4.22 does); only the f16 slot ran.
  (d) the exact (fp32) re-run on the undamped gin-virtual models.
  (e) bits: (LAST, 0) through the call is never calling; the JK store leaves h_5 as it was; placements; a resident batch across
      settings; option hipgraph.
  (f) `host GIN --emb-dim 300 --eps --ogb-vn --jk sum --residual`.
"""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from flowgnn_amd import Engine, EngineGroup, export, graphpack as gp, weights  # noqa: E402
from tests import attn_pool_ref as A, ogb_jk_torch as J, ogb_torch as T, set2set_ref as S  # noqa: E402
from tests.parity import assert_close, err_ratio  # noqa: E402
from tests.test_embeddings_gpu import launched  # noqa: E402
from tests.test_gin_wide_f16_gpu import F16_REL  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
MODELS = [(vn, jk, res) for vn in (False, True) for jk, res in J.SETTINGS]
name_of = lambda vn, jk, res: f"gin{'-virtual' if vn else ''}-{jk}{'-res' if res else ''}"
IDS = [name_of(*m) for m in MODELS]
VN_IDS = ["gin", "gin-virtual"]


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
            model = J.make_model(vn, jk, res, num_tasks=tasks, damped=damped)
            kw = dict(virtual_node=True, virtual_node_dim=300) if vn else {}
            export.export_weights("GIN", model.state_dict(), str(d), keep_eps=True, multi_task=tasks != 1, **kw)
            done[key] = str(d)
        return done[key]
    return get


def engine(vn, directory, jk="last", res=False, tasks=1, pooling="mean", f16=False, call=True, profile=True):
    """The width first, then the files, then the flags the model was trained with (they are in no file)."""
    e = Engine("GIN", device=0)
    e.set_emb_dim(300)
    if tasks != 1:
        e.set_num_tasks(tasks)
    e.load_weights_dir(directory, eps=True, virtual_node=vn)
    if pooling != "mean":
        e.set_pooling(pooling)
    if f16:
        e.set_numeric_mode("f16", emb_dim=300)
    if call:
        e.set_jk_residual(jk, res)
        assert e.jk_residual() == (jk, res)
    if profile:
        e.profile_enable(True)
    return e


def group(vn, directory, jk, res):
    g = EngineGroup("GIN", [0, 0])
    g.set_emb_dim(300)
    g.load_weights_dir(directory)
    g.set_gin_eps(weights.load_gin_eps(directory, emb_dim=300))
    if vn:
        g.set_ogb_virtual_node(weights.load_gin_virtual_node(directory, emb_dim=300))
    g.set_jk_residual(jk, res)
    return g


def close(got, want, scale, what, rel=1e-4):
    print(what, f"err_ratio {err_ratio(got, want, scale, rel):.4f} (scale {scale:.4g})")
    assert_close(got, want, scale=scale, rel=rel, what=what)


def all_three(e, b=None):
    logits, pooled, rows = (np.array(x) for x in e.forward(T.gin_batch() if b is None else b, return_embeddings=True, return_node_embeddings=True))
    return logits, pooled, rows


# ---------------------------------------------------------------- (a) parity with the torch model
@pytest.mark.parametrize("vn,jk,res", MODELS, ids=IDS)
def test_checkpoint_parity(vn, jk, res, exported):
    want, scale, _ = J.expected(vn, jk, res)
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
    assert "gin_wide_layer" in names and "gin_wide_layer_f32" not in names and "gin_wide_layer_f16" not in names, names
    for v in J.variants_of(vn, jk, res):
        r = err_ratio(J.variant_rows(vn, jk, res, v), rows, scale)
        print(what, "wrong form", v, f"{r:.1f} x the bound from the GPU's rows")
        assert r > 5.0, (v, r)


def test_the_setting_is_what_makes_the_difference(exported):
    """The same files without the call: the logits of a JK='last', residual=False model, far from the trained one's."""
    want, scale, _ = J.expected(True, "sum", True)
    e = engine(True, exported(True, "sum", True), call=False)
    try:
        assert e.jk_residual() == ("last", False)
        rows = np.array(e.forward(T.gin_batch(), return_node_embeddings=True)[1])
    finally:
        e.close()
    assert err_ratio(rows, want.rows, scale) > 100.0


# ---------------------------------------------------------------- (b) every readout reads r
@pytest.mark.parametrize("pooling", ["mean", "sum", "max"])
@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_every_pooling_pools_r(vn, pooling, exported):
    want, scale, _ = J.expected(vn, "sum", True, pooling=pooling)
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
    want, scale, _ = J.expected(vn, "sum", True, num_tasks=3)
    e = engine(vn, exported(vn, "sum", True, tasks=3), "sum", True, tasks=3)
    try:
        logits, pooled, rows = all_three(e)
        assert e.exact_reruns() == 0
    finally:
        e.close()
    assert want.logits.shape == (T.gin_batch().num_graphs, 3) == logits.shape
    close(rows, want.rows, scale, (name_of(vn, "sum", True), "3 tasks", "rows"))
    close(logits, want.logits, scale, (name_of(vn, "sum", True), "3 tasks", "logits"))


@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_node_logits_are_each_nodes_share_of_r(vn, exported):
    want, scale, _ = J.expected(vn, "sum", True)
    d = exported(vn, "sum", True)
    w, _, _ = J.load(d, vn)
    e = engine(vn, d, "sum", True)
    try:
        logits, rows, terms = (np.array(x) for x in e.forward(T.gin_batch(), return_node_embeddings=True, return_node_logits=True))
    finally:
        e.close()
    what = name_of(vn, "sum", True)
    close(rows, want.rows, scale, (what, "rows beside node logits"))
    close(terms, J.node_logits(w, want.rows), scale, (what, "node logits"))
    b = T.gin_batch()
    means = np.add.reduceat(terms.astype(np.float64), b.node_offsets()[:-1]) / b.nums_of_nodes
    close(means, want.logits, scale, (what, "mean of the node logits"))
    close(logits, want.logits, scale, (what, "logits"))


def test_attention_readout_reads_r(exported):
    want, scale, _ = J.expected(False, "sum", True)
    d = exported(False, "sum", True)
    w, _, _ = J.load(d, False)
    gate, b = weights.synth_attention_pooling(), T.gin_batch()
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
    want, scale, _ = J.expected(False, "sum", True)
    d = exported(False, "sum", True)
    s2s, b = weights.synth_set2set(), T.gin_batch()
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


# ---------------------------------------------------------------- (c) the f16 mode
@pytest.mark.parametrize("vn,jk,res", MODELS, ids=IDS)
def test_f16_mode(vn, jk, res, exported):
    want, scale, _ = J.expected(vn, jk, res)
    e = engine(vn, exported(vn, jk, res), jk, res, f16=True)
    try:
        logits, pooled, rows = all_three(e)
        names = launched(e, lambda: e.run())
        reruns = e.exact_reruns()
    finally:
        e.close()
    what = name_of(vn, jk, res)
    print(what, "f16 rows", f"{err_ratio(rows, want.rows, scale, F16_REL):.4f} x the f16 rule (printed, not asserted)")
    print(what, "f16 logits", f"{err_ratio(logits, want.logits, scale, F16_REL):.4f} x the f16 rule (scale {scale:.4g})")
    assert reruns == 0
    assert "gin_wide_layer_f16" in names and "gin_wide_layer" not in names and "gin_wide_layer_f32" not in names, names
    assert_close(logits, want.logits, scale=scale, rel=F16_REL, what=(what, "f16 logits"))


# ---------------------------------------------------------------- (d) the exact re-run
@pytest.mark.parametrize("jk", ["last", "sum"])
def test_exact_rerun(jk, exported):
    """The undamped gin-virtual models (tests/test_jk_residual_cpu.py asserts that they leave the f16 range): the pass is repeated on
    the fp32 pipe, with the adds of gin_wide_jk.hip's element-wise kernel, and lands inside the same bound."""
    want, scale, _ = J.expected(True, jk, True, damped=False)
    assert scale > 1.2e5
    e = engine(True, exported(True, jk, True, damped=False), jk, True)
    try:
        logits, pooled, rows = all_three(e)
        reruns = e.exact_reruns()
        names = launched(e, lambda: e.run())
    finally:
        e.close()
    what = (name_of(True, jk, True), "undamped")
    print(what, "exact_reruns", reruns)
    assert reruns >= 1 and "gin_wide_layer_f32" in names, (reruns, names)
    close(rows, want.rows, scale, (what, "rows"))
    close(logits, want.logits, scale, (what, "logits"))


# ---------------------------------------------------------------- (e) bits
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
    assert slots[0] == slots[1], slots


@pytest.mark.parametrize("node_emb", [False, True], ids=["", "node-embeddings"])
@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_the_jk_store_leaves_h5_as_it_was(vn, node_emb, exported):
    """(sum, off): final_h() is the plain run's h_5 byte for byte, and the plain run's node embeddings ARE that h_5."""
    d, b = exported(vn), T.gin_batch()
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
def test_placements_give_each_graph_the_same_bits(vn, exported):
    from tests.test_device_batch_gpu import device_args
    d, b = exported(vn, "sum", True), T.gin_batch()
    G, off = b.num_graphs, b.node_offsets()
    perm = np.random.default_rng(5).permutation(G)
    shuffled = gp.concat_batches([b.slice(int(i), int(i) + 1) for i in perm])
    e = engine(vn, d, "sum", True)
    try:
        logits, pooled, rows = all_three(e)
        for layout in ("pyg", "reference"):
            args, kw = device_args(b, layout, "GIN")
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
    assert np.array_equal(s_logits, logits[perm]) and np.array_equal(s_pooled, pooled[perm])
    soff = shuffled.node_offsets()
    for k, i in enumerate(perm):
        assert np.array_equal(s_rows[soff[k]:soff[k + 1]], rows[off[i]:off[i + 1]]), (k, i)
    assert np.array_equal(p_logits, logits[5:27]) and np.array_equal(p_pooled, pooled[5:27]) and np.array_equal(p_rows, rows[off[5]:off[27]])
    g = group(vn, d, "sum", True)
    try:
        g.set_embeddings(True)
        g.set_node_embeddings(True)
        g_logits = np.array(g.forward(b))
        g_pooled, g_rows = np.array(g.embeddings()), np.array(g.node_embeddings())
    finally:
        g.close()
    assert np.array_equal(g_logits, logits) and np.array_equal(g_pooled, pooled) and np.array_equal(g_rows.reshape(rows.shape), rows)


@pytest.mark.parametrize("vn", [False, True], ids=VN_IDS)
def test_the_setting_changes_between_runs_on_a_resident_batch(vn, exported):
    d, b = exported(vn, "sum", True), T.gin_batch()
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
        for jk, res in (("sum", True), ("last", False), ("sum", True)):
            e.set_jk_residual(jk, res)
            e.run()
            runs.append([np.array(x).copy() for x in (e.results(), e.embeddings(), e.node_embeddings())])
    finally:
        e.close()
    for x, y in zip(runs[0], runs[2]):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(runs[1], base):
        assert x.tobytes() == y.tobytes()
    assert runs[0][0].tobytes() != runs[1][0].tobytes()


def test_hipgraph_replay_follows_the_setting(exported):
    """Option hipgraph: the call drops the recorded launch sequence, and the new one is recorded and replayed in its turn."""
    d, b = exported(True, "sum", True), T.gin_batch()
    direct = engine(True, d, "sum", True)
    try:
        expected = np.array(direct.forward(b)).copy()
    finally:
        direct.close()
    h = Engine("GIN", device=0, options={"hipgraph": 2})  # (no profiling: a profiled run is launched directly)
    try:
        h.set_emb_dim(300)
        h.load_weights_dir(d, eps=True, virtual_node=True)
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


# ---------------------------------------------------------------- (f) the host CLI
def test_host_cli_300_jk_residual(exported, tmp_path):
    """`host GIN --emb-dim 300 --eps --ogb-vn --jk sum --residual` on a written pack and the exported directory."""
    want, scale, _ = J.expected(True, "sum", True)
    gdir, out = tmp_path / "graphs", tmp_path / "HLS_output.txt"
    gp.write_pack(T.gin_batch(), str(gdir))
    p = subprocess.run([HOST, "GIN", "--emb-dim", "300", "--eps", "--ogb-vn", "--jk", "sum", "--residual", "--graphs", str(gdir), "--weights",
                        exported(True, "sum", True), "--trials", "1", "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    close(got, want.logits, scale, (name_of(True, "sum", True), "host CLI"))
