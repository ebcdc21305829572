"""OGB's attention readout at width 300 on the GPU (flowgnn.h: flowgnn_set_attention_pooling; kernels: flowgnn_amd/csrc/wide_attn.hip,
DESIGN.md section 4.20), for gin, gin-virtual, gcn and gcn-virtual.

Expected values: the float64 forwards of the wide references (tests/gin_wide_ref.py, gin_wide_vn_ref.py, gcn_wide_ref.py,
gcn_wide_vn_ref.py) for the rows, then tests/attn_pool_ref.readout on them.  Tolerance: the project's rule and nothing else,
|gpu - want| <= REL (scale + |want|), REL = 1e-4, scale = the reference's activation scale extended by max |s| and the largest hidden
value of the gate (tests/parity.py); the readout-arithmetic case uses B = sqrt(E_ok * E_bad) of attn_pool_ref.table on the rows the
engine itself returned, which comes from the references alone.  tests/test_attn_pool_cpu.py shows that every semantic wrong form of
the readout is at least 50 x the rule away.  Every comparison prints its worst ratio to the bound.

Shapes: tests/ogb_torch.gin_batch() / gcn_batch() -- a one-node graph, three nodes without an edge, a 17-node ring (one past a wave's
16-row tile), a 129-node path (one past the 128-row workgroup tile, longer than a wavefront) and a graph count that is no multiple of
four.  Every test here fails on a library without flowgnn_set_attention_pooling."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, export, graphpack as gp, weights
from tests import attn_pool_ref as A, gcn_wide_ref as C, gcn_wide_vn_ref as CV, gin_wide_ref as W, gin_wide_vn_ref as V, ogb_torch as T, split_ref
from tests.parity import REL, assert_close, err_ratio
from tests.test_embeddings_gpu import launched

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
GATE, POOL, MEAN = "attn_gate", "attn_pool_rows", "mean_pool_rows"
EPS = np.asarray(W.TRAINED_EPS, np.float32)
KINDS = [("gin", False), ("gin", True), ("gcn", False), ("gcn", True)]
name_of = lambda kind, vn: f"{kind}{'-virtual' if vn else ''}"
VN_W1 = 1.0 / 64  # the virtual node's first linear layer (tests/gin_wide_vn_ref.shapes_virtual_node): t of a 129-node graph stays in the split's range


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def close(got, want, scale, what, rel=REL):
    print(what, f"worst ratio to the bound {err_ratio(got, want, scale, rel):.3f}")
    assert_close(got, want, scale=scale, rel=rel, what=what)


@pytest.fixture(scope="module")
def gate():
    return weights.synth_attention_pooling(seed=11)


def tensors(kind, vn, tasks=1):
    """(weights, virtual node or None) of a model: the seeded synthetic sets at width 300."""
    if kind == "gin":
        return weights.synth_gin_weights(seed=7, num_tasks=tasks, emb_dim=300), (V.shapes_virtual_node(w1_scale=VN_W1) if vn else None)
    return weights.synth_gcn_weights(seed=7, num_tasks=tasks, emb_dim=300), (CV.shapes_virtual_node(w1_scale=VN_W1) if vn else None)


def reference(kind, vn, b, w, vnt, g, tasks=1):
    """(rows, pooled, logits, scale) in float64: the wide reference's forward for the rows, then the readout on them."""
    if kind == "gin":
        ref = V.forward(b, w, vnt, eps=EPS, num_tasks=tasks) if vn else W.forward(b, w, eps=EPS, num_tasks=tasks)
    else:
        ref = CV.forward(b, w, vnt, num_tasks=tasks) if vn else C.forward(b, w, num_tasks=tasks)
    stats = {}
    pooled, logits, s = A.readout(ref.rows, b, g, w["graph_pred_weights"], w["graph_pred_bias"], stats=stats)
    # the gate kernel's own operands are in range: the rows, and the hidden values times W1's power-of-two pre-scale
    assert max(float(np.abs(ref.rows).max()), split_ref.pow2_scale(g["w1"]) * stats["hidden_max"]) < 6.0e4 / 2
    return ref.rows, pooled, logits, max(ref.scale, stats["s_max"], stats["hidden_max"])


def configure(e, kind, vn, w, vnt, g, tasks=1):
    """Width, NUM_TASK, weights, eps (GIN), the virtual node, the readout: on an Engine or an EngineGroup."""
    (e.set_emb_dim if kind == "gin" else e.set_model_emb_dim)(300)
    if tasks != 1:
        e.set_num_tasks(tasks)
    e.set_weights(w)
    if kind == "gin":
        e.set_gin_eps(EPS)
    if vn:
        (e.set_ogb_virtual_node if kind == "gin" else e.set_gcn_virtual_node)(vnt)
    if g is not None:
        e.set_attention_pooling(g)


def make(kind, vn, w, vnt, g, tasks=1, options=None):
    e = Engine(kind.upper(), device=0, options=options or {})
    configure(e, kind, vn, w, vnt, g, tasks)
    e.profile_enable(True)
    return e


def run(e, b, expect_reruns=0, **fwd):
    """One forward with the readout on: its two slots ran, the mean's did not."""
    res = {}
    before = e.exact_reruns()
    names = launched(e, lambda: res.update(got=e.forward(b, **fwd)))
    assert {GATE, POOL, "pooled_head"} <= names and MEAN not in names, names
    assert e.exact_reruns() - before == expect_reruns, (e.exact_reruns(), before)
    return res["got"]


# ---------------------------------------------------------------- 1. parity on the shapes where the kernels can go wrong
@pytest.mark.parametrize("tasks", [1, 3])
@pytest.mark.parametrize("kind,vn", KINDS, ids=[name_of(k, v) for k, v in KINDS])
def test_parity(kind, vn, tasks, gate):
    b = T.batch_of(kind)
    assert b.num_graphs % 4 != 0 and 1 in b.nums_of_nodes and 17 in b.nums_of_nodes and 129 in b.nums_of_nodes
    w, vnt = tensors(kind, vn, tasks)
    rows, pooled, logits, scale = reference(kind, vn, b, w, vnt, gate, tasks)
    e = make(kind, vn, w, vnt, gate, tasks)
    try:
        got, emb, nemb = run(e, b, return_embeddings=True, return_node_embeddings=True)
        assert e.exact_reruns() == 0
        h = e.final_h()  # flowgnn_get_h still returns what it did (GIN: h_5, the pooled rows; GCN: x_4)
    finally:
        e.close()
    what = (name_of(kind, vn), f"NUM_TASK {tasks}")
    assert got.shape == ((b.num_graphs, tasks) if tasks > 1 else (b.num_graphs,))
    close(nemb, rows, scale, what + ("node embeddings",))
    close(emb, pooled, scale, what + ("graph embeddings",))
    close(got, logits, scale, what + ("logits",))
    assert np.isfinite(h).all() and (kind != "gin" or np.array_equal(h, nemb))


@pytest.mark.parametrize("kind,vn", KINDS, ids=[name_of(k, v) for k, v in KINDS])
def test_host_batch_device_batch_and_group_give_the_same_bits(kind, vn, gate):
    pytest.importorskip("torch")
    from tests.test_device_batch_gpu import device_args
    b = T.batch_of(kind)
    w, vnt = tensors(kind, vn)
    e = make(kind, vn, w, vnt, gate)
    try:
        want, want_emb = [x.copy() for x in run(e, b, return_embeddings=True)]
        for layout in ("pyg", "reference"):
            args, kw = device_args(b, layout, kind.upper())
            got, emb = e.forward_device(*args, return_embeddings=True, **kw)
            e.sync()
            assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(emb.cpu().numpy(), want_emb), layout
        assert e.exact_reruns() == 0
    finally:
        e.close()
    g = EngineGroup(kind.upper(), [0, 0])
    try:
        configure(g, kind, vn, w, vnt, gate)
        g.set_embeddings(True)
        got = g.forward(b)
        emb = g.embeddings()
        g.set_attention_pooling(None)
        off = g.forward(b)
    finally:
        g.close()
    same = np.array_equal(got, want) and np.array_equal(emb, want_emb)
    print(name_of(kind, vn), "group [0, 0]: the bits of one engine" if same else "group [0, 0]: other bits than one engine")
    if kind == "gcn" and vn and not same:
        # gcn-virtual's LAYERS cut the virtual node's per-graph sums at the batch's 16-node tiles (flowgnn.h, flowgnn_set_gcn_virtual_node_dim;
        # tests/test_gcn_wide_vn_gpu.test_group_within_the_bound): its rows agree within fp32 rounding between two cuts, whatever the readout
        _, pooled, logits, scale = reference(kind, vn, b, w, vnt, gate)
        close(got, logits, scale, "gcn-virtual, group")
        close(emb, pooled, scale, "gcn-virtual, group, embeddings")
    else:
        assert np.array_equal(got, want) and np.array_equal(emb, want_emb)  # a graph's bits do not depend on where the group cuts the batch
    assert not np.array_equal(off, want)


# ---------------------------------------------------------------- 2. the readout's arithmetic alone
@pytest.mark.parametrize("seed", [5, 7])
def test_readout_arithmetic(seed, gate):
    """err <= B = sqrt(E_ok * E_bad) for `pooled` and `logits`, with the rows the engine itself returned as the readout's input: closer
    to float64 than every wrong variant of the three-product split, by the margin the references leave."""
    b = gp.synth_molhiv_batch(64, seed=seed)
    w, _ = tensors("gin", False)
    e = make("gin", False, w, None, gate)
    try:
        logits, emb, rows = run(e, b, return_embeddings=True, return_node_embeddings=True)
    finally:
        e.close()
    pw, pb = w["graph_pred_weights"], w["graph_pred_bias"]
    want_pooled, want_logits, _ = A.readout(rows, b, gate, pw, pb)
    t = A.table(rows, b, gate, pw, pb)
    for name, got, want in (("pooled", emb, want_pooled), ("logits", logits, want_logits)):
        r = t[name]
        err = A.err(got, want, r.unit)
        print(f"seed {seed} {name}: err {err:.3e}  E_ok {r.e_ok:.3e}  B {r.bound:.3e}  E_bad {r.e_bad:.3e}  ratio {r.e_bad / r.e_ok:.1f}")
        assert r.e_bad / r.e_ok >= 16.0, (name, r.e_ok, r.e_bad)  # (a condition on the references: split_ref.LOW_RATIO's value)
        assert err <= r.bound, (name, err, r.bound)


# ---------------------------------------------------------------- 3. exactness and position independence
def test_one_node_graphs_have_the_bits_of_the_mean_readout(gate):
    """e = 1 and Z = 1: pooled = r[v] exactly, so the logit is the mean readout's, bit for bit, from the same engine, with the readout
    switched off, on and off again."""
    singles = [T._graph(1, [], 40 + i) for i in range(5)]
    b = gp.concat_batches([T.gin_batch()] + singles[:2] + [gp.synth_molhiv_batch(6, seed=2)] + singles[2:])
    one = np.nonzero(np.asarray(b.nums_of_nodes) == 1)[0]
    assert len(one) == 6
    w, _ = tensors("gin", False)
    e = make("gin", False, w, None, None)
    try:
        off, off_emb = [x.copy() for x in e.forward(b, return_embeddings=True)]
        e.set_attention_pooling(gate)
        on, on_emb = [x.copy() for x in run(e, b, return_embeddings=True)]
        e.set_attention_pooling(None)
        names = launched(e, lambda: e.forward(b, return_embeddings=True))
        off2, off2_emb = e.results().copy(), e.embeddings().copy()
    finally:
        e.close()
    assert MEAN in names and not names & {GATE, POOL}, names
    assert np.array_equal(on[one], off[one]) and np.array_equal(on_emb[one], off_emb[one])
    many = np.nonzero(np.asarray(b.nums_of_nodes) > 2)[0]
    assert not np.any(on[many] == off[many])
    assert np.array_equal(off2, off) and np.array_equal(off2_emb, off_emb)  # off -> on -> off reproduces the mean's result


@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_slice_as_a_shard_and_off_on_off(kind, gate):
    b = T.batch_of(kind)
    w, _ = tensors(kind, False)
    e = make(kind, False, w, None, gate)
    try:
        whole, whole_emb = [x.copy() for x in run(e, b, return_embeddings=True)]
        e.set_job_totals(b.total_nodes, b.total_edges)
        part, part_emb = [x.copy() for x in run(e, b.slice(5, 27), return_embeddings=True)]
        e.set_job_totals(-1, -1)
        e.set_attention_pooling(None)
        off = e.forward(b).copy()
        e.set_attention_pooling(gate)
        again = run(e, b).copy()
        e.set_attention_pooling(None)
        off2 = e.forward(b).copy()
    finally:
        e.close()
    assert np.array_equal(part, whole[5:27]) and np.array_equal(part_emb, whole_emb[5:27])
    assert np.array_equal(again, whole) and np.array_equal(off2, off) and not np.array_equal(off, whole)


def test_hipgraph_replay_equals_direct_launches(gate):
    b = T.gin_batch()
    w, _ = tensors("gin", False)
    plain = make("gin", False, w, None, gate)
    try:
        expected = run(plain, b).copy()
    finally:
        plain.close()
    h = Engine("GIN", device=0, options={"hipgraph": 2})
    try:
        configure(h, "gin", False, w, None, None)
        h.set_batch(b)
        for _ in range(3):
            h.run()
        mean = h.results().copy()
        assert h.graph_replays() >= 1
        h.set_attention_pooling(gate)  # drops the recorded sequence
        h.run()
        first = h.results().copy()
        before = h.graph_replays()
        outs = []
        for _ in range(3):
            h.run()
            outs.append(h.results().copy())
        assert h.graph_replays() > before  # the new sequence is recorded and replayed in its turn
        h.set_attention_pooling(None)
        h.run()
        off = h.results().copy()
    finally:
        h.close()
    assert np.array_equal(first, expected) and all(np.array_equal(o, expected) for o in outs)
    assert np.array_equal(off, mean) and not np.array_equal(first, mean)


# ---------------------------------------------------------------- 4. saturation and the range fallback
def test_saturated_softmax(gate):
    """w2 x 64: alpha is nearly one-hot and exp underflows for most nodes; the result is finite and within the rule."""
    b = gp.synth_molhiv_batch(64, seed=5)
    g = dict(gate, w2=gate["w2"] * np.float32(64))
    w, _ = tensors("gin", False)
    rows, pooled, logits, scale = reference("gin", False, b, w, None, g)
    s = A.readout(rows, b, g, w["graph_pred_weights"], w["graph_pred_bias"])[2]
    off = b.node_offsets()
    seg = np.repeat(np.arange(b.num_graphs), np.diff(off))
    d = s - np.maximum.reduceat(s, off[:-1])[seg]
    assert np.mean(d < -104) > 0.5  # exp(-104) < the smallest fp32 subnormal: most nodes' weights are zero in fp32
    e = make("gin", False, w, None, g)
    try:
        got, emb = run(e, b, return_embeddings=True)
    finally:
        e.close()
    assert np.isfinite(got).all() and np.isfinite(emb).all()
    close(emb, pooled, scale, "saturated, graph embeddings")
    close(got, logits, scale, "saturated, logits")


def test_range_fallback(gate):
    """b1 = 1e5 on eight hidden units whose w2 entries are 0: the gate scores are unchanged and a hidden value leaves the f16 range --
    one exact re-run, and the results within the rule of the same reference."""
    b = gp.synth_molhiv_batch(64, seed=7)
    g = {k: v.copy() for k, v in gate.items()}
    units = np.array([3, 64, 130, 255, 301, 448, 590, 599])
    g["b1"][units] = np.float32(1e5)
    g["w2"][units] = np.float32(0)
    base = dict(gate, w2=g["w2"])
    w, _ = tensors("gin", False)
    pw, pb = w["graph_pred_weights"], w["graph_pred_bias"]
    ref = W.forward(b, w, eps=EPS)
    stats = {}
    pooled, logits, s = A.readout(ref.rows, b, g, pw, pb, stats=stats)
    assert np.abs(s - A.readout(ref.rows, b, base, pw, pb)[2]).max() == 0.0 and stats["hidden_max"] > 6.6e4  # the scores are unchanged
    scale = max(ref.scale, stats["s_max"], stats["hidden_max"])
    e = make("gin", False, w, None, g)
    try:
        res = {}
        names = launched(e, lambda: res.update(got=e.forward(b, return_embeddings=True)))
        assert e.exact_reruns() == 1 and {GATE, POOL, "gin_wide_layer_f32"} <= names, (e.exact_reruns(), names)
        got, emb = res["got"]
    finally:
        e.close()
    close(emb, pooled, scale, "range fallback, graph embeddings")
    close(got, logits, scale, "range fallback, logits")


# ---------------------------------------------------------------- 5. end to end: torch model -> files -> host CLI
@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_end_to_end(kind, tmp_path):
    pytest.importorskip("torch")
    model = A.attention_model(kind, False, emb_dim=300)
    b = T.batch_of(kind)
    want, scale, _ = T.run(model, b)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    kw = dict(keep_eps=True) if kind == "gin" else dict(emb_dim=300)
    export.export_weights(kind.upper(), model.state_dict(), str(wdir), attention_pooling=True, **kw)
    out = tmp_path / "HLS_output.txt"
    flags = ["--eps"] if kind == "gin" else []
    p = subprocess.run([HOST, kind.upper(), "--emb-dim", "300"] + flags + ["--attn-pool", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1",
                        "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    cli = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    e = Engine(kind.upper(), device=0)
    try:
        (e.set_emb_dim if kind == "gin" else e.set_model_emb_dim)(300)
        e.load_weights_dir(str(wdir), eps=kind == "gin", attention_pooling=True)
        assert e.attention_pooling() is True
        e.profile_enable(True)
        got, emb, rows = run(e, b, return_embeddings=True, return_node_embeddings=True)
        print(kind, "exact_reruns", e.exact_reruns())
    finally:
        e.close()
    assert np.abs(cli - got).max() <= 1e-8, np.abs(cli - got).max()  # the file's 8 decimals
    close(rows, want.rows, scale, (kind, "end to end, rows"))
    close(emb, want.pooled, scale, (kind, "end to end, pooled"))
    close(got, want.logits, scale, (kind, "end to end, logits"))
    close(cli, want.logits, scale, (kind, "host --attn-pool"))


# ---------------------------------------------------------------- 6. speed guard
def test_speed_guard(gate):
    """attn_gate + attn_pool_rows <= the average time of one gin_wide_layer launch in the same process: the gate has about half of a
    layer's MFMAs and no gather, so a gate slower than a whole layer of the unchanged kernel means spills or a serialised stream.  Device
    events, best of three medians of seven (tests/test_f16_mode_gpu.test_speed_guard)."""
    b = gp.synth_molhiv_batch(1 << 14, seed=3)
    w, _ = tensors("gin", False)
    e = make("gin", False, w, None, gate)
    try:
        e.set_batch(b)
        e.run()
        e.results()
        assert e.exact_reruns() == 0
        slots = ("gin_wide_layer", GATE, POOL)

        def medians(runs=7):
            ms = {k: [] for k in slots}
            for _ in range(runs):
                t0 = e.profile_read()
                e.run()
                e.results()
                t1 = e.profile_read()
                for k in slots:
                    ms[k].append(t1[k]["total_ms"] - t0[k]["total_ms"])
            return {k: float(np.median(v)) for k, v in ms.items()}

        best = {k: np.inf for k in slots}
        for _ in range(3):
            m = medians()
            for k in slots:
                best[k] = min(best[k], m[k])
    finally:
        e.close()
    layer = best["gin_wide_layer"] / 5
    print(f"attn_gate {best[GATE]:.4f} ms + attn_pool_rows {best[POOL]:.4f} ms against one gin_wide_layer launch {layer:.4f} ms")
    assert best[GATE] + best[POOL] <= layer, best
