"""The vocabulary head's top-k form on the GPU (flowgnn.h: flowgnn_set_vocab_topk; kernels: vh_topk_* in flowgnn_amd/csrc/wide_vocab.hip;
DESIGN.md section 4.34) against float64 NumPy: the logits of tests/code2_ref.head_logits sorted by (-value, index), and their
log-sum-exp with a max shift.  Every (graph, position, rank) is held to check_topk's conditions, none excluded; where winners are
planted far beyond the bound the indices must be equal, in order.  Every test here fails on a library without the call."""
import numpy as np
import pytest

from flowgnn_amd import Engine
from flowgnn_amd.engine import FlowGNNError
from tests import code2_ref as R, parity
from tests.test_code2_gpu import ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, engine, pooled_of, shared, w300
from tests.test_embeddings_gpu import launched, torch_context_first  # noqa: F401  (torch's context before the first engine: see there)
from tests.wide_cases import many

pytestmark = pytest.mark.gpu


def topk_ref(logits, K):
    """(ids [G][P][K], values [G][P][K], lse [G][P]) in float64; (-1, -inf) at ranks at or beyond V"""
    G, P, V = logits.shape
    order = np.lexsort((np.broadcast_to(np.arange(V), logits.shape), -logits), axis=2)[..., :K]  # by -value, then by index
    ids, vals = np.full((G, P, K), -1, np.int64), np.full((G, P, K), -np.inf)
    ids[..., :order.shape[2]], vals[..., :order.shape[2]] = order, np.take_along_axis(logits, order, axis=2)
    top = logits.max(axis=2)
    return ids, vals, top + np.log(np.exp(logits - top[..., None]).sum(axis=2))


def check_topk(ids, scores, lse, logits, K, equal=False, what=""):
    G, P, V = logits.shape
    n = min(K, V)
    ref_ids, ref_vals, ref_lse = topk_ref(logits, K)
    ids, scores, lse = np.asarray(ids), np.asarray(scores, np.float64), np.asarray(lse, np.float64)
    assert ids.shape == scores.shape == (G, P, K) and lse.shape == (G, P) and ids.dtype == np.int32, (what, ids.shape, scores.shape, lse.shape)
    assert (ids[..., n:] == -1).all() and (scores[..., n:] == -np.inf).all(), (what, "a rank beyond the vocabulary is not (-1, -inf)")
    ids, scores = ids[..., :n].astype(np.int64), scores[..., :n]
    assert (ids >= 0).all() and (ids < V).all(), (what, "an index outside the vocabulary", int(ids.min()), int(ids.max()))
    assert (np.sort(ids, axis=2)[..., 1:] != np.sort(ids, axis=2)[..., :-1]).all(), (what, "an index twice in one list")
    down, tie = scores[..., 1:] < scores[..., :-1], scores[..., 1:] == scores[..., :-1]
    assert (down | (tie & (ids[..., 1:] > ids[..., :-1]))).all(), (what, "not in the order (larger value, then lower index)")
    at = np.take_along_axis(logits, ids, axis=2)
    scale = parity.oracle_scale(logits)
    r1 = parity.err_ratio(scores, at, scale)
    r2 = float(((ref_vals[..., :n] - at) / (2 * parity.REL * (scale + np.abs(ref_vals[..., :n])))).max())
    r3 = parity.err_ratio(lse, ref_lse, scale)
    print(what, f"score against its logit: {r1:.4f} of the bound; the logit below the r-th largest: {r2:.4f} of twice the bound; lse: {r3:.4f} of the bound")
    assert np.isfinite(scores).all() and np.isfinite(lse).all() and r1 <= 1.0 and r2 <= 1.0 and r3 <= 1.0, (what, r1, r2, r3)
    if equal:
        assert np.array_equal(ids, ref_ids[..., :n]), (what, "a planted order was missed")


def plant_ranks(w, b, pooled, rows):
    """b with b[p][rows[i]] raised so that rows[0] > rows[1] > .. beat every other entry of every position, for every graph, each by
    code2_ref.plant's margin over the next: far beyond the bound, asserted as plant asserts it"""
    b = np.array(b, np.float32)
    L = R.head_logits(pooled, w, b)
    for p in range(L.shape[1]):
        gap = (L[:, p].max() - L[:, p].min()) + 0.5 * (parity.oracle_scale(L) + np.abs(L[:, p]).max())  # a row's spread over the graphs, and a margin
        for i, v in enumerate(rows):
            b[p, v] += np.float32(L[:, p].max() - L[:, p, v].min() + (len(rows) - i) * gap)
    L = R.head_logits(pooled, w, b)
    won = L[:, :, rows]
    rest = np.delete(L, rows, axis=2).max(axis=2, initial=-np.inf)
    below = np.concatenate([won[..., 1:], rest[..., None]], axis=2)
    assert ((won - below) > 100 * parity.REL * (parity.oracle_scale(L) + np.abs(won))).all()
    return b


def run_topk(e, batch, w, b, K):
    e.set_vocab_head(w, b)
    e.set_vocab_topk(K)
    res = {}
    names = launched(e, lambda: (e.forward(batch), res.update(top=e.topk(), tok=e.tokens())))
    assert np.array_equal(res["tok"][0], res["top"][0][..., 0]) and np.array_equal(res["tok"][1], res["top"][1][..., 0])  # tokens() is rank 0
    return res["top"], names


@pytest.fixture(autouse=True)
def topk_off_afterwards():
    yield
    shared().set_vocab_topk(0)  # the engine is test_code2_gpu's as well


@pytest.mark.parametrize("K", [1, 2, 8])
@pytest.mark.parametrize("V", [1, 15, 17, 5002])
@pytest.mark.parametrize("G", [1, 17, 129])
def test_shapes(G, V, K):
    batch, pooled = pooled_of(G)
    w, b = R.head(2, V, 1000 * K + V + G)
    planted = (G + V + K) % 2 == 0  # half of the cases
    if planted:
        b = plant_ranks(w, b, pooled, [(7 * i + V // 2) % V for i in range(min(K, V))])  # (distinct: 7 divides no V here)
    logits = R.head_logits(pooled, w, b)
    ref = topk_ref(logits, K)
    check_topk(ref[0].astype(np.int32), ref[1], ref[2], logits, K, equal=True, what="the reference against itself")
    e = shared()
    e.set_vocab_head(w, b)
    folds = "vocab_head_fold" in launched(e, lambda: e.forward(batch))  # k = 0: what the plan does with this batch on this device
    top, names = run_topk(e, batch, w, b, K)
    assert "vocab_topk" in names and "vocab_topk_f32" not in names and ("vocab_topk_fold" in names) == folds, names
    assert not {"vocab_head", "vocab_head_fold"} & names, names
    check_topk(*top, logits, K, equal=planted, what=f"G {G} V {V} K {K}")


@pytest.mark.parametrize("V", [17, 5002])
def test_rank0_is_the_argmax_path(V):
    batch, _ = pooled_of(17)
    w, b = R.head(5, V, 60 + V)
    e = shared()
    (ids, scores, _), _ = run_topk(e, batch, w, b, 8)
    e.set_vocab_topk(0)
    e.forward(batch)
    ids0, scores0 = e.tokens()
    assert np.array_equal(ids[..., 0], ids0) and np.array_equal(scores[..., 0].view(np.int32), scores0.view(np.int32))


@pytest.mark.parametrize("v1,v2", [(4, 6), (3, 9), (3, 20), (3, 100), (70, 4999)])
def test_ties(v1, v2):
    """test_code2_gpu.test_ties's placements: the twins are ranks 0 and 1, the lower index first"""
    batch, pooled = pooled_of(17)
    w, b = R.head(2, 5002, 5)
    b = R.plant(w, b, pooled, [v1, v1])
    w[:, v2], b[:, v2] = w[:, v1], b[:, v1]
    (ids, scores, lse), names = run_topk(shared(), batch, w, b, 4)
    assert "vocab_topk_fold" in names, names
    assert (ids[..., 0] == v1).all() and (ids[..., 1] == v2).all() and np.array_equal(scores[..., 0], scores[..., 1]), (v1, v2, ids[0])
    check_topk(ids, scores, lse, R.head_logits(pooled, w, b), 4, what=f"tie {v1} {v2}")


def test_three_equal_maxima():
    batch, pooled = pooled_of(17)
    w, b = R.head(2, 5002, 5)
    b = R.plant(w, b, pooled, [40, 40])
    for v in (7, 2500):
        w[:, v], b[:, v] = w[:, 40], b[:, 40]
    (ids, scores, lse), _ = run_topk(shared(), batch, w, b, 2)
    assert (ids[..., 0] == 7).all() and (ids[..., 1] == 40).all(), ids[0]
    check_topk(ids, scores, lse, R.head_logits(pooled, w, b), 2, what="three equal maxima")


@pytest.mark.parametrize("rising", [True, False])
def test_list_traffic_extremes(rising):
    """A bias that rises with the index: every candidate of a lane evicts; one that falls: none does after the first K.  The step is
    four times the largest |W pooled|, so neighbours are at least half a step apart, hundreds of fp32 roundings of the largest logit"""
    batch, pooled = pooled_of(17)
    V, K = 5002, 8
    w, b = R.head(2, V, 70)
    step = 4 * np.abs(R.head_logits(pooled, w, 0 * b)).max()
    b[:] = (step * (np.arange(V) if rising else np.arange(V)[::-1])).astype(np.float32)
    (ids, scores, lse), _ = run_topk(shared(), batch, w, b, K)
    want = np.arange(V - 1, V - 1 - K, -1) if rising else np.arange(K)
    assert (ids == want).all(), (ids[0], want)
    check_topk(ids, scores, lse, R.head_logits(pooled, w, b), K, equal=True, what=f"bias {'rising' if rising else 'falling'}")


def test_last_tile_all_negative():
    """test_code2_gpu's input: the fifteen rows of the second tile that do not exist would give logit 0, above every real one"""
    batch, pooled = pooled_of(17)
    w, b = R.head(5, 17, 6)
    b -= np.float32(np.abs(R.head_logits(pooled, w, b)).max() + 10.0)
    logits = R.head_logits(pooled, w, b)
    assert (logits < 0).all()
    top, _ = run_topk(shared(), batch, w, b, 8)
    check_topk(*top, logits, 8, what="all negative")


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
    top, names = run_topk(e, batch, w, b, 8)
    assert "vocab_topk_f32" in names and e.exact_reruns() == 1, (names, e.exact_reruns())
    check_topk(*top, R.head_logits(pooled, w, b), 8, what="pooled value of 1e5")


def test_state():
    def refused(code, fn):
        with pytest.raises(FlowGNNError) as x:
            fn()
        assert x.value.code == code and len(str(x.value)) > 40, x.value

    batch, pooled = pooled_of(17)
    w, b = R.head(2, 37, 80)
    e = engine()
    refused(ERR_ARG, lambda: e.set_vocab_topk(9))
    refused(ERR_ARG, lambda: e.set_vocab_topk(-1))
    gcn = Engine("GCN", device=0)
    gcn.set_model_emb_dim(300)
    refused(ERR_UNSUPPORTED, lambda: gcn.set_vocab_topk(3))
    refused(ERR_UNSUPPORTED, lambda: Engine("GIN", device=0).set_vocab_topk(3))  # width 100
    refused(ERR_STATE, e.topk)  # nothing ran
    # head off and k = 3: a run succeeds, launches nothing of the head's and gives the bits of an engine that never saw the call
    e.set_vocab_topk(3)
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(batch)))
    assert e.vocab_topk == 3 and not {n for n in names if n.startswith("vocab_")}, names
    assert np.array_equal(res["got"], engine().forward(batch))
    refused(ERR_STATE, e.topk)
    e.set_vocab_head(w, b)
    e.forward(batch)
    assert e.topk()[0].shape == (17, 2, 3) and e.lib.flowgnn_topk_k(e._h) == 3
    e.set_vocab_topk(2)  # a change of k
    refused(ERR_STATE, e.topk)
    refused(ERR_STATE, e.tokens)
    e.forward(batch)
    assert e.topk()[0].shape == (17, 2, 2)
    e.set_batch(many(5, 2))  # a new batch
    refused(ERR_STATE, e.topk)
    e.forward(batch)
    e.set_vocab_head(None, None)  # the head turned off
    refused(ERR_STATE, e.topk)
    e.set_vocab_head(w, b)
    e.set_vocab_topk(0)  # k = 0: the argmax form's launches and no others, and nothing to fetch
    names = launched(e, lambda: e.forward(batch))
    assert "vocab_head" in names and not {n for n in names if n.startswith("vocab_topk")}, names
    refused(ERR_STATE, e.topk)
    R.check_tokens(*e.tokens(), R.head_logits(pooled, w, b), what="k = 0")
