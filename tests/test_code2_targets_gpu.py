"""The vocabulary head scoring given target tokens on the GPU (flowgnn.h: flowgnn_set_vocab_targets; kernels: flowgnn_amd/csrc/
wide_vocab_score.hip) against float64 NumPy: tests/code2_ref.head_logits on the pooled rows the engine
returns, their max-shifted log-sum-exp, and the rank under (larger value, then lower index).  Every (graph, position) is held to
check_scores' conditions, none excluded; on inputs whose fp32 sums are exact the rank and the logit must be equal.  Every test here
fails on a library without the call."""
import numpy as np
import pytest

from flowgnn_amd import Engine
from flowgnn_amd.engine import FlowGNNError
from tests import code2_ref as R, parity
from tests.test_code2_gpu import ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, engine, pooled_of, shared, w300
from tests.test_embeddings_gpu import launched, torch_context_first  # noqa: F401  (torch's context before the first engine: see there)
from tests.wide_cases import many

pytestmark = pytest.mark.gpu
ERR_NODE_FEAT = 4
SPLIT, EXACT = {"vocab_target", "vocab_score"}, {"vocab_score_f32"}


def at(logits, t):
    """the float64 logit at t [G][P]; NaN where t is -1"""
    x = np.take_along_axis(logits, np.maximum(t, 0)[..., None].astype(np.int64), axis=2)[..., 0]
    return np.where(t >= 0, x, np.nan)


def rank_ref(logits, t):
    """entries v != t before t under (larger value, then lower index), in float64; -1 where t is -1"""
    x, idx = at(logits, t)[..., None], np.arange(logits.shape[2])
    return np.where(t >= 0, ((logits > x) | ((logits == x) & (idx < t[..., None]))).sum(axis=2), -1)


def seeded_targets(seed, G, P, V):
    """[G][P] int32 in 0 .. V - 1, a fifth of them -1; the last one is -1 and the first V - 1 (one position: the first wins)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, V, (G, P)).astype(np.int32)
    t[rng.random((G, P)) < 0.2] = -1
    t[-1, -1], t[0, 0] = -1, V - 1
    return t


def run_targets(e, batch, w, b, t):
    """((tokens, scores), (logit, lse, rank), launched slots) of a run with targets t"""
    e.set_vocab_head(w, b)
    res = {}
    names = launched(e, lambda: (e.forward(batch, targets=t), res.update(tok=e.tokens(), sc=e.target_scores())))
    assert not {"vocab_head", "vocab_head_fold", "vocab_head_f32"} & names, names
    return res["tok"], res["sc"], names


def check_scores(tok, sc, logits, t, what=""):
    """(a) to (d) of section 4.36 for every (g, p); returns where the float64 band of (d) is a single rank"""
    (ids, scores), (logit, lse, rank) = tok, sc
    G, P, V = logits.shape
    has = t >= 0
    assert logit.shape == lse.shape == rank.shape == (G, P) and rank.dtype == np.int32 and logit.dtype == lse.dtype == np.float32, what
    assert (rank[~has] == -1).all() and np.isnan(logit[~has]).all() and np.isfinite(logit[has]).all() and np.isfinite(lse).all(), what
    x, top, scale = at(logits, t), logits.max(axis=2), parity.oracle_scale(logits)
    r1 = parity.err_ratio(logit[has], x[has], scale)
    r3 = parity.err_ratio(lse, top + np.log(np.exp(logits - top[..., None]).sum(axis=2)), scale)
    hit = has & (ids == t)
    assert np.array_equal(has & (rank == 0), hit) and np.array_equal(logit[hit].view(np.int32), scores[hit].view(np.int32)), (what, "(c)")
    band = 2 * parity.REL * (scale + np.abs(top))[..., None]
    other = np.arange(V) != t[..., None]
    lo, hi = (logits > x[..., None] + band).sum(axis=2), ((logits >= x[..., None] - band) & other).sum(axis=2)
    print(what, f"logit at the target: {r1:.4f} of the bound; lse: {r3:.4f} of the bound; single-rank bands: {float((lo == hi)[has].mean()) if has.any() else 1.0:.3f}")
    assert r1 <= 1.0 and r3 <= 1.0 and ((lo <= rank) & (rank <= hi))[has].all(), (what, r1, r3)
    return (lo == hi)[has]


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("V", [1, 15, 17, 5002])
@pytest.mark.parametrize("G", [1, 17, 129])
def test_shapes(G, V, P):
    batch, pooled = pooled_of(G)
    w, b = R.head(P, V, 3000 * P + V + G)
    t = seeded_targets(V + G + P, G, P, V)
    logits = R.head_logits(pooled, w, b)
    e = shared()
    e.set_vocab_head(w, b)
    e.forward(batch)
    plain = e.tokens()
    tok, sc, names = run_targets(e, batch, w, b, t)
    assert SPLIT <= names and not EXACT & names and ("vocab_score_fold" in names) == (V > 64), names
    assert all(np.array_equal(a.view(np.int32), c.view(np.int32)) for a, c in zip(tok, plain)), "(e): tokens or scores differ from a run without targets"
    R.check_tokens(*tok, logits, what=f"G {G} V {V} P {P}")
    single = check_scores(tok, sc, logits, t, what=f"G {G} V {V} P {P}")
    assert V > 17 or single.size == 0 or single.mean() >= 0.5, "the float64 band of (d) is too wide to tell a wrong count"


@pytest.mark.parametrize("V", [337, 5002])
def test_exact_rank(V):
    """Inputs on which every fp32 sum of the split arithmetic is exact (test_code2_head_f16_gpu.test_exactness_probe's): the logits are
    the float64 ones, so the rank and the target's logit are equal to the reference's; biases on a 2^-12 grid make ties frequent"""
    rng = np.random.default_rng(V)
    P, D, G = 5, 300, 17
    w = np.zeros((P, V, D), np.float32)
    for p in range(P):
        for v in range(V):
            k = rng.choice(D, 2 + (p + v) % 3, replace=False)
            w[p, v, k] = rng.choice([-0.5, -0.25, 0.25, 0.5], len(k))
    b = (rng.integers(-4096, 4096, (P, V)) / 4096.0).astype(np.float32)
    wts = dict(w300())
    w2, b2 = np.array(wts["node_mlp_2_weights"]), np.array(wts["node_mlp_2_bias"])
    w2[-1] = 0.0  # the last layer's rows are its bias: 12 significant bits each
    b2[-1] = (rng.choice([-1.0, 1.0], D) * (2 * rng.integers(1024, 2048, D) + 1) / 2048.0 * 2.0 ** rng.integers(-2, 2, D)).astype(np.float32)
    wts["node_mlp_2_weights"], wts["node_mlp_2_bias"] = w2, b2
    e = engine(wts)
    e.set_pooling("sum")  # pooled[g] = n_g b2: up to 15 significant bits, hi and lo halves hold them exactly
    batch = many(G, 4)
    pooled = e.forward(batch, return_embeddings=True)[1]
    assert np.array_equal(pooled, np.asarray(batch.nums_of_nodes, np.float32)[:, None] * b2[-1][None])
    logits = R.head_logits(pooled, w, b)
    t = rng.integers(0, V, (G, P)).astype(np.int32)
    for g, p in np.ndindex(G, P):  # every other (g, p): a target whose logit another entry shares, where there is one
        _, inv, cnt = np.unique(logits[g, p], return_inverse=True, return_counts=True)
        twins = np.flatnonzero(cnt[inv] > 1)
        if twins.size and (g + p) % 2 == 0:
            t[g, p] = rng.choice(twins)
    assert ((logits == at(logits, t)[..., None]).sum(axis=2) > 1).any(), "no (g, p) has a tie with its target"
    tok, (logit, lse, rank), names = run_targets(e, batch, w, b, t)
    assert SPLIT | {"vocab_score_fold"} <= names and e.exact_reruns() == 0, names
    assert np.array_equal(rank, rank_ref(logits, t)) and np.array_equal(logit.astype(np.float64), at(logits, t))
    assert np.array_equal(tok[0], logits.argmax(axis=2)) and np.array_equal(tok[1].astype(np.float64), logits.max(axis=2))


@pytest.mark.parametrize("lo,mid,hi", [(4, 5, 6), (3, 9, 14), (3, 20, 40), (70, 2500, 4999)])
def test_ties(lo, mid, hi):
    """Three identical rows planted as the maximum -- in one lane's rows, in three lanes of a tile, in three tiles, in three slices --
    and each of them the target of one position: only the lower-indexed copies count"""
    batch, pooled = pooled_of(17)
    w, b = R.head(3, 5002, 5)
    b = R.plant(w, b, pooled, [mid, mid, mid])
    for v in (lo, hi):
        w[:, v], b[:, v] = w[:, mid], b[:, mid]
    t = np.tile(np.array([lo, mid, hi], np.int32), (17, 1))
    tok, (logit, lse, rank), names = run_targets(shared(), batch, w, b, t)
    assert "vocab_score_fold" in names, names
    assert (rank == [0, 1, 2]).all() and (tok[0] == lo).all() and np.array_equal(logit.view(np.int32), tok[1].view(np.int32)), rank[0]
    check_scores(tok, (logit, lse, rank), R.head_logits(pooled, w, b), t, what=f"tie {lo} {mid} {hi}")


def test_planted():
    batch, pooled = pooled_of(17)
    V = 5002
    w, b = R.head(2, V, 9)
    b = R.plant(w, b, pooled, [2501, 2501])
    L = R.head_logits(pooled, w, b)
    b[1, 77] -= np.float32(L[:, 1, 77].max() - L[:, 1].min() + 0.05 * (parity.oracle_scale(L) + np.abs(L).max()))  # below every other, as far
    t = np.tile(np.array([2501, 77], np.int32), (17, 1))
    tok, sc, _ = run_targets(shared(), batch, w, b, t)
    assert (sc[2] == [0, V - 1]).all(), sc[2]
    check_scores(tok, sc, R.head_logits(pooled, w, b), t, what="planted")


def test_range_guard():
    wts = dict(w300())
    b2 = np.array(wts["node_mlp_2_bias"])
    b2[-1, 7] = 1.0e5  # test_code2_gpu.test_range_guard's model: pooled[:, 7] is beyond 6e4, no layer operand is
    wts["node_mlp_2_bias"] = b2
    e = engine(wts)
    batch = many(17, 3)
    pooled = e.forward(batch, return_embeddings=True)[1]
    assert np.abs(pooled[:, 7]).min() > 6.0e4 and e.exact_reruns() == 0
    w, b = R.head(5, 5002, 8)
    t = seeded_targets(8, 17, 5, 5002)
    tok, sc, names = run_targets(e, batch, w, b, t)
    assert EXACT <= names and e.exact_reruns() == 1, (names, e.exact_reruns())
    R.check_tokens(*tok, R.head_logits(pooled, w, b), what="pooled value of 1e5")
    check_scores(tok, sc, R.head_logits(pooled, w, b), t, what="pooled value of 1e5")


def test_state():
    import torch

    def refused(code, fn, *words):
        with pytest.raises(FlowGNNError) as x:
            fn()
        assert x.value.code == code and len(str(x.value)) > 40 and all(s in str(x.value) for s in words), x.value

    batch, pooled = pooled_of(17)
    V = 37
    w, b = R.head(2, V, 80)
    t = np.random.default_rng(1).integers(-1, V, (17, 2)).astype(np.int32)
    gcn = Engine("GCN", device=0)
    gcn.set_model_emb_dim(300)
    gcn.set_batch(batch)
    refused(ERR_UNSUPPORTED, lambda: gcn.set_vocab_targets(t))
    narrow = Engine("GIN", device=0)  # width 100
    narrow.set_batch(batch)
    refused(ERR_UNSUPPORTED, lambda: narrow.set_vocab_targets(t))
    e = engine()
    assert e.lib.flowgnn_set_vocab_targets(e._h, t.ctypes.data_as(e.lib.flowgnn_set_vocab_targets.argtypes[1]), 2, 0) == ERR_STATE  # no batch
    refused(ERR_STATE, e.target_scores)
    # targets before the head, then the head; and the other order: the same bits; a device tensor: the same bits again
    e.set_batch(batch)
    e.set_vocab_targets(t)
    assert e.vocab_targets
    e.set_vocab_head(w, b)
    e.run()
    first = e.target_scores()
    _, second, names = run_targets(e, batch, w, b, t)
    assert SPLIT <= names
    e.forward(batch, targets=torch.from_numpy(t).to(f"cuda:{e.device}"))
    third = e.target_scores()
    for other in (second, third):
        assert all(np.array_equal(a.view(np.int32), c.view(np.int32)) for a, c in zip(first, other))
    check_scores(e.tokens(), first, R.head_logits(pooled, w, b), t, what="state")
    # the results die with the batch, the head and the targets
    e.set_batch(many(5, 2))
    assert not e.vocab_targets
    refused(ERR_STATE, e.target_scores)
    e.forward(batch, targets=t)
    e.set_vocab_head(w, b)
    refused(ERR_STATE, e.target_scores)
    e.forward(batch, targets=t)
    e.set_vocab_targets(None)
    refused(ERR_STATE, e.target_scores)
    names = launched(e, lambda: e.forward(batch))  # no targets: the head's own launches and nothing of this file's
    assert "vocab_head" in names and not {n for n in names if n.startswith(("vocab_score", "vocab_target"))}, names
    refused(ERR_STATE, e.target_scores)
    # what is refused, and where
    refused(ERR_STATE, lambda: e.forward(batch, targets=t[:, :1]), "flowgnn_run", "positions")
    for bad in (V, -2):
        tb = t.copy()
        tb[3, 1] = bad
        refused(ERR_ARG, lambda: e.forward(batch, targets=tb), "flowgnn_set_vocab_targets")
    tb[3, 1] = V
    e.set_vocab_head(None, None)
    e.set_batch(batch)
    e.set_vocab_targets(tb)  # no head yet: V is unknown
    e.set_vocab_head(w, b)
    refused(ERR_ARG, e.run, "flowgnn_run")
    e.set_vocab_targets(t)
    for beside in ("topk", "f16"):
        e.set_vocab_topk(2) if beside == "topk" else e.set_vocab_head_numeric("f16")
        refused(ERR_STATE, e.run, "flowgnn_set_vocab_targets", "flowgnn_set_vocab_topk", "flowgnn_set_vocab_head_numeric")
        e.set_vocab_targets(None)
        e.forward(batch)  # clean after detaching
        assert e.tokens()[0].shape == (17, 2)
        e.set_vocab_topk(0) if beside == "topk" else e.set_vocab_head_numeric("f32")
        e.set_vocab_targets(t)
    # a device value of V: the batch's error word, reported as the AST encoder reports a bad index
    dev = engine()
    dev.set_vocab_head(w, b)
    dev.set_batch(batch)
    dev.set_vocab_targets(torch.from_numpy(tb).to(f"cuda:{dev.device}"))
    dev.run()
    refused(ERR_NODE_FEAT, dev.target_scores, "flowgnn_set_vocab_targets")
