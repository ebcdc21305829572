"""The vocabulary head's f16 numeric mode on the GPU (flowgnn.h: flowgnn_set_vocab_head_numeric; kernel: flowgnn_amd/csrc/
wide_vocab_f16.hip) against the mode's rule in float64:
    logit = b + sum_k r(W s) / s . r(pooled),   s the power-of-two scale of all of W, r to nearest even to f16
on the pooled rows the engine returned.  Only the fp32 accumulation order differs from the rule, so the shapes are held to
code2_ref.check_tokens' two conditions at parity.REL, and the probe, whose every fp32 sum is exact, to bit equality.  Every test that
runs the mode asserts that its own kernel was launched; on a library without the call each fails with an AttributeError."""
import functools

import numpy as np
import pytest

from flowgnn_amd import Engine
from flowgnn_amd.engine import FlowGNNError
from tests import code2_ref as R, f16_ref as F
from tests.test_code2_gpu import ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, engine, w300
from tests.test_embeddings_gpu import launched, torch_context_first  # noqa: F401  (torch's context before the first engine: see there)
from tests.wide_cases import many

pytestmark = pytest.mark.gpu
T = 2  # the graph tiles of a wave (wide_vocab_f16.hip: FLOWGNN_VHF_TILES): a wave ends at 16 T graphs, a block at 128 T


def rule_logits(pooled, w, b, r_pooled="rne", r_w="rne"):
    """The rule's [G][P][V] in float64; the other roundings: the wrong variants the probe must tell apart from it"""
    s = F.pow2_scale(w)
    return R.head_logits(F.rounder(r_pooled)(pooled), F.rounder(r_w)(R.c(w) * s) / s, b)


@functools.lru_cache(maxsize=None)
def mine():  # this file's engine: the mode stays on it
    return engine()


@functools.lru_cache(maxsize=None)
def pooled_of(G):
    batch, e = many(G, 40 + G), mine()
    e.set_vocab_head(None, None)
    return batch, e.forward(batch, return_embeddings=True)[1]


def run_f16(e, batch, w, b):
    e.set_vocab_head(w, b)
    e.set_vocab_head_numeric("f16")
    res = {}
    names = launched(e, lambda: (e.forward(batch), res.update(tok=e.tokens())))
    return res["tok"], names


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("V", [1, 15, 17, 33, 5002])
@pytest.mark.parametrize("G", [1, 17, 16 * T + 1, 128 * T + 1])
def test_shapes(G, V, P):
    batch, pooled = pooled_of(G)
    w, b = R.head(P, V, 2000 * P + V + G)
    planted = (G + V + P) % 2 == 0  # half of the cases
    if planted:
        b = R.plant(w, b, pooled, [(7 * p + V // 2) % V for p in range(P)])
    (ids, scores), names = run_f16(mine(), batch, w, b)
    assert "vocab_head_f16" in names and not {"vocab_head", "vocab_head_f32"} & names and ("vocab_head_fold" in names) == (V > 64), names
    R.check_tokens(ids, scores, rule_logits(pooled, w, b), equal=planted, what=f"f16 head, G {G} V {V} P {P}")


def test_exactness_probe():
    """Inputs on which every fp32 sum of the rule is exact: scores bit-equal to it, and unequal to three wrong variants' -- pooled
    rounded toward zero, pooled unrounded, weights unrounded -- in more than half of the (g, p)"""
    rng = np.random.default_rng(3)
    P, V, D = 5, 101, 300
    w = np.zeros((P, V, D), np.float32)
    for p in range(P):
        for v in range(V):  # two to four non-zeros in {+-1/4, +-1/2}, times 1 - 2^-12 + 2^-20: to nearest they ARE the few-bit values
            k = rng.choice(D, 2 + (p + v) % 3, replace=False)
            w[p, v, k] = rng.choice([-0.5, -0.25, 0.25, 0.5], len(k)) * (1.0 - 2.0 ** -12 + 2.0 ** -20)
    b = (rng.integers(-4096, 4096, (P, V)) / 4096.0).astype(np.float32)
    wts = dict(w300())
    w2, b2 = np.array(wts["node_mlp_2_weights"]), np.array(wts["node_mlp_2_bias"])
    w2[-1] = 0.0  # the last layer's rows are its bias: 12 significant bits each, the twelfth set
    b2[-1] = (rng.choice([-1.0, 1.0], D) * (2 * rng.integers(1024, 2048, D) + 1) / 2048.0 * 2.0 ** rng.integers(-2, 2, D)).astype(np.float32)
    wts["node_mlp_2_weights"], wts["node_mlp_2_bias"] = w2, b2
    e = engine(wts)
    e.set_pooling("sum")  # pooled[g] = n_g b2, n_g = 1 .. 5: up to 15 significant bits
    batch = many(16 * T + 1, 4)
    pooled = e.forward(batch, return_embeddings=True)[1]
    assert np.array_equal(pooled, np.asarray(batch.nums_of_nodes, np.float32)[:, None] * b2[-1][None])
    (ids, scores), names = run_f16(e, batch, w, b)
    assert "vocab_head_f16" in names and e.exact_reruns() == 0, names
    rule = rule_logits(pooled, w, b)
    assert np.array_equal(scores.astype(np.float64), rule.max(axis=2)) and np.array_equal(ids, rule.argmax(axis=2))
    for what, kw in [("pooled toward zero", dict(r_pooled="rtz")), ("pooled unrounded", dict(r_pooled="none")), ("weights unrounded", dict(r_w="none"))]:
        differs = float((rule_logits(pooled, w, b, **kw).max(axis=2) != rule.max(axis=2)).mean())
        print(what, f"differs from the rule in {differs:.3f} of the (g, p)")
        assert differs > 0.5, (what, differs)


@pytest.mark.parametrize("v1,v2", [(4, 6), (3, 9), (3, 100), (3, 20), (70, 4999)])
def test_ties(v1, v2):
    """Two identical rows planted as the maximum -- in one lane's four rows, in two lanes of a tile, in two tiles, in the two tiles of
    one chunk, in two slices: the lower index comes back, for every graph"""
    batch, pooled = pooled_of(17)
    w, b = R.head(2, 5002, 5)
    b = R.plant(w, b, pooled, [v1, v1])
    w[:, v2], b[:, v2] = w[:, v1], b[:, v1]
    (ids, scores), names = run_f16(mine(), batch, w, b)
    assert {"vocab_head_f16", "vocab_head_fold"} <= names, names  # the slicing is on
    assert (ids == v1).all(), (v1, v2, ids)
    R.check_tokens(ids, scores, rule_logits(pooled, w, b), what=f"tie {v1} {v2}")


def test_last_tile_all_negative():
    """V = 17: fifteen rows of the second tile do not exist; their zero weights and bias would give logit 0, above every real one"""
    batch, pooled = pooled_of(17)
    w, b = R.head(5, 17, 6)
    b -= np.float32(np.abs(rule_logits(pooled, w, b)).max() + 10.0)
    logits = rule_logits(pooled, w, b)
    assert (logits < 0).all()
    (ids, scores), names = run_f16(mine(), batch, w, b)
    assert "vocab_head_f16" in names, names
    R.check_tokens(ids, scores, logits, what="all negative")


def test_range_guard():
    wts = dict(w300())
    b2 = np.array(wts["node_mlp_2_bias"])
    b2[-1, 7] = 1.0e5  # pooled[:, 7] is beyond 6e4, no layer operand is (tests/test_code2_gpu.py)
    wts["node_mlp_2_bias"] = b2
    e = engine(wts)
    batch = many(17, 3)
    pooled = e.forward(batch, return_embeddings=True)[1]
    assert np.abs(pooled[:, 7]).min() > 6.0e4 and e.exact_reruns() == 0
    w, b = R.head(5, 5002, 8)
    (ids, scores), names = run_f16(e, batch, w, b)
    assert {"vocab_head_f16", "vocab_head_f32"} <= names and e.exact_reruns() == 1, (names, e.exact_reruns())
    R.check_tokens(ids, scores, R.head_logits(pooled, w, b), what="pooled value of 1e5: the exact form, unrounded")


def refused(code, fn, names):
    with pytest.raises(FlowGNNError) as x:
        fn()
    assert x.value.code == code and names in str(x.value), x.value


@pytest.mark.parametrize("layers", ["f32", "f16"])
def test_state(layers):
    """Both call orders, both layer modes, off-is-off, the tokens' life across a change of the mode, and the refusals"""
    batch = many(17, 9)
    w, b = R.head(2, 37, 60)
    never = engine()
    never.set_numeric_mode(layers, emb_dim=300)
    never.set_vocab_head(w, b)
    want = never.forward(batch, return_embeddings=True) + never.tokens()
    e = engine()
    e.set_numeric_mode(layers, emb_dim=300)
    e.set_vocab_head_numeric("f16")  # the mode first, the head second
    (ids, scores), names = run_f16(e, batch, w, b)
    assert "vocab_head_f16" in names and e.vocab_head_numeric == "f16", names
    R.check_tokens(ids, scores, rule_logits(want[1], w, b), what=f"layers {layers}, head f16")
    assert all(np.array_equal(x, y) for x, y in zip((ids, scores), run_f16(never, batch, w, b)[0]))  # the head first, the mode second
    e.set_vocab_head_numeric("f32")
    refused(ERR_STATE, e.tokens, "flowgnn_set_vocab_head")  # dropped with the mode
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(batch, return_embeddings=True) + e.tokens()))
    assert "vocab_head" in names and "vocab_head_f16" not in names and e.vocab_head_numeric == "f32", names
    assert all(np.array_equal(x, y) for x, y in zip(res["got"], want))  # the bits of an engine that never saw the call
    raw = lambda dim, mode: e._check(e.lib.flowgnn_set_vocab_head_numeric(e._h, dim, mode), "flowgnn_set_vocab_head_numeric")
    refused(ERR_ARG, lambda: raw(300, 1), "flowgnn_set_numeric_mode")  # Q6.10: the layers' call has it, the head does not
    refused(ERR_ARG, lambda: raw(100, 2), "flowgnn_set_emb_dim")  # another width than the engine's
    e.set_vocab_topk(2)
    refused(ERR_STATE, lambda: e.set_vocab_head_numeric("f16"), "flowgnn_set_vocab_topk")
    e.set_vocab_topk(0)
    e.set_vocab_head_numeric("f16")
    refused(ERR_STATE, lambda: e.set_vocab_topk(2), "flowgnn_set_vocab_head_numeric")
    gcn = Engine("GCN", device=0)
    gcn.set_model_emb_dim(300)
    refused(ERR_UNSUPPORTED, lambda: gcn.set_vocab_head_numeric("f16"), "FLOWGNN_MODEL_GIN")
    refused(ERR_UNSUPPORTED, lambda: Engine("GIN", device=0).set_vocab_head_numeric("f16"), "flowgnn_set_emb_dim")
    Engine("GIN", device=0).set_vocab_head_numeric("f32")  # the default is accepted wherever a handle is valid
