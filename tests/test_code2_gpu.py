"""ogbg-code2 on the 300-wide GIN on the GPU (flowgnn.h: flowgnn_set_vocab_head, flowgnn_set_ast_encoder; kernels: flowgnn_amd/csrc/
wide_vocab.hip) against the float64 NumPy of tests/code2_ref.py.  The head is held to two conditions for every
(graph, position), none excluded (code2_ref.check_tokens); where a winner is planted far beyond the bound the index must be equal.
Every test here fails on a library without the two calls."""
import ctypes
import functools

import numpy as np
import pytest

from flowgnn_amd import Engine, graphpack as gp, weights
from flowgnn_amd.engine import FlowGNNError
from tests import code2_ref as R, gin_edge_linear_ref as EL
from tests.parity import assert_close
from tests.test_embeddings_gpu import launched, torch_context_first  # noqa: F401  (torch's context before the first engine: see there)
from tests.wide_cases import isolated, many, path

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 1, 6, 8


@functools.lru_cache(maxsize=None)
def w300():
    return weights.synth_gin_weights(seed=7, emb_dim=300)


@functools.lru_cache(maxsize=None)
def vn300():
    vn = weights.synth_gin_virtual_node(seed=11, emb_dim=300)  # (w1 / 16: tests/gin_wide_vn_ref.shapes_virtual_node)
    return dict(vn, w1=vn["w1"] * np.float32(1.0 / 16))


def engine(w=None):
    e = Engine("GIN", device=0)
    e.set_emb_dim(300)
    e.set_weights(w or w300())
    e.profile_enable(True)
    return e


@functools.lru_cache(maxsize=None)
def shared():  # the head-alone tests' engine: the model is only there to make pooled rows
    return engine()


@functools.lru_cache(maxsize=None)
def pooled_of(G):
    """The trivial model's batch of G graphs and its pooled rows [G][300], from return_embeddings on a head-less run"""
    batch = many(G, 40 + G)
    e = shared()
    e.set_vocab_head(None, None)
    return batch, e.forward(batch, return_embeddings=True)[1]


def run_head(e, batch, w, b):
    e.set_vocab_head(w, b)
    res = {}
    names = launched(e, lambda: (e.forward(batch), res.update(tok=e.tokens())))
    return res["tok"], names


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("V", [1, 15, 17, 5002])
@pytest.mark.parametrize("G", [1, 15, 17, 129])
def test_head(G, V, P):
    batch, pooled = pooled_of(G)
    w, b = R.head(P, V, 1000 * P + V + G)
    planted = (G + V + P) % 2 == 0  # half of the cases
    if planted:
        b = R.plant(w, b, pooled, [(7 * p + V // 2) % V for p in range(P)])
    logits = R.head_logits(pooled, w, b)
    R.check_tokens(logits.argmax(axis=2).astype(np.int32), logits.max(axis=2), logits, equal=True, what="the reference against itself")
    (ids, scores), names = run_head(shared(), batch, w, b)
    assert "vocab_head" in names and "vocab_head_f32" not in names and ("vocab_head_fold" in names) == (V > 64), names
    R.check_tokens(ids, scores, logits, equal=planted, what=f"G {G} V {V} P {P}")


@pytest.mark.parametrize("v1,v2", [(4, 6), (3, 9), (3, 20), (3, 100), (70, 4999)])
def test_ties(v1, v2):
    """Two identical rows planted as the maximum -- in one lane's four rows, in two lanes of a tile, in two tiles of a slice, in two
    slices: the lower index comes back, for every graph"""
    batch, pooled = pooled_of(17)
    w, b = R.head(2, 5002, 5)
    b = R.plant(w, b, pooled, [v1, v1])
    w[:, v2], b[:, v2] = w[:, v1], b[:, v1]
    (ids, scores), names = run_head(shared(), batch, w, b)
    assert "vocab_head_fold" in names, names  # the slicing is on
    assert (ids == v1).all(), (v1, v2, ids)
    R.check_tokens(ids, scores, R.head_logits(pooled, w, b), what=f"tie {v1} {v2}")


def test_last_tile_all_negative():
    """V = 17: fifteen rows of the second tile do not exist; their zero weights and bias would give logit 0, above every real one"""
    batch, pooled = pooled_of(17)
    w, b = R.head(5, 17, 6)
    b -= np.float32(np.abs(R.head_logits(pooled, w, b)).max() + 10.0)
    logits = R.head_logits(pooled, w, b)
    assert (logits < 0).all()
    (ids, scores), _ = run_head(shared(), batch, w, b)
    R.check_tokens(ids, scores, logits, what="all negative")


def test_range_guard():
    wts = dict(w300())
    b2 = np.array(wts["node_mlp_2_bias"])
    b2[-1, 7] = 1.0e5  # the last layer has no ReLU and feeds nothing but the readout: pooled[:, 7] is beyond 6e4, no layer operand is
    wts["node_mlp_2_bias"] = b2
    e = engine(wts)
    batch = many(17, 3)
    pooled = e.forward(batch, return_embeddings=True)[1]
    assert np.abs(pooled[:, 7]).min() > 6.0e4 and e.exact_reruns() == 0
    w, b = R.head(5, 5002, 8)
    (ids, scores), names = run_head(e, batch, w, b)
    assert "vocab_head_f32" in names and e.exact_reruns() == 1, (names, e.exact_reruns())
    R.check_tokens(ids, scores, R.head_logits(pooled, w, b), what="pooled value of 1e5")


@pytest.mark.parametrize("beside", ["attention", "f16"])
def test_head_beside_the_other_readout_and_the_f16_mode(beside):
    """The head reads whatever [G][300] row the readout pooled: the attention readout's softmax-weighted sums, and the rows of the
    layers' f16 numeric mode, where the head itself stays fp32-accurate -- held to the fp32 bound on the rows the engine returned"""
    e = engine()
    if beside == "attention":
        e.set_attention_pooling(weights.synth_attention_pooling(seed=11))
    else:
        e.set_numeric_mode("f16", emb_dim=300)
    batch = many(17, 9)
    pooled = e.forward(batch, return_embeddings=True)[1]
    w, b = R.head(5, 5002, 50)
    (ids, scores), names = run_head(e, batch, w, b)
    assert "vocab_head" in names and "vocab_head_f32" not in names and e.exact_reruns() == 0, names
    R.check_tokens(ids, scores, R.head_logits(pooled, w, b), what=f"beside {beside}")


def code2_batch():
    return gp.concat_batches([path(15, 1), isolated(2, 2), path(16, 3), path(17, 4), isolated(1, 5), path(129, 6)])


@pytest.mark.parametrize("virtual", [False, True])
def test_whole_model(virtual):
    batch = code2_batch()
    sizes = (98, 10030, 20) if not virtual else (5, 7, 3)  # code2's real tables, once
    P, V = (5, 5002) if not virtual else (3, 37)
    ast, (x, depth) = R.ast_tables(*sizes, seed=20), R.ast_nodes(batch.total_nodes, *sizes, seed=21)
    assert (depth > sizes[2]).any()  # the clamp is hit
    el, ef = EL.edge_linear(5, 2, 22), EL.features(batch.total_edges, 2, 23)
    hw, hb = R.head(P, V, 24)
    vn = vn300() if virtual else None
    ref = R.forward(batch, w300(), el, ef, ast, x, depth, vn=vn)
    e = engine()
    if virtual:
        e.set_ogb_virtual_node(vn)
    e.set_edge_linear(el["w"], el["b"])
    e.set_ast_encoder(*ast)
    e.set_vocab_head(hw, hb)
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(batch, return_embeddings=True, return_node_embeddings=True, edge_features=ef, ast_nodes=(x, depth)),
                                           tok=e.tokens()))
    logits, pooled, rows = res["got"]
    assert {"ast_encoder", "vocab_head"} <= names and "atom_encoder" not in names and e.exact_reruns() == 0, names
    assert_close(rows, ref.rows, scale=ref.scale, what="rows")
    assert_close(pooled, ref.pooled, scale=ref.scale, what="pooled")
    assert_close(logits, ref.logits, scale=ref.scale, what="logits")
    R.check_tokens(*res["tok"], R.head_logits(pooled, hw, hb), what=f"whole model, virtual {virtual}")


def test_off_is_off_and_device_nodes():
    import torch
    batch = code2_batch()
    ast, (x, depth) = R.ast_tables(5, 7, 3, seed=30), R.ast_nodes(batch.total_nodes, 5, 7, 3, seed=31)
    hw, hb = R.head(2, 37, 32)
    e = engine()
    e.set_ast_encoder(*ast)
    e.set_vocab_head(hw, hb)
    host = e.forward(batch, return_node_embeddings=True, ast_nodes=(x, depth)) + e.tokens()
    dev = e.forward(batch, return_node_embeddings=True, ast_nodes=(torch.from_numpy(x).to("cuda:0"), torch.from_numpy(depth).to("cuda:0"))) + e.tokens()
    assert all(np.array_equal(a, b) for a, b in zip(host, dev))
    e.set_ast_encoder(None, None, None)
    e.set_vocab_head(None, None)
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(batch, return_node_embeddings=True)))
    assert e.vocab_head == 0 and not e.ast_encoder and "atom_encoder" in names and not {"ast_encoder", "vocab_head", "vocab_head_fold"} & names, names
    never = engine().forward(batch, return_node_embeddings=True)
    assert all(np.array_equal(a, b) for a, b in zip(res["got"], never))  # the bits of an engine that never saw the two calls


def test_refusals():
    batch = code2_batch()
    ast, hw, hb = R.ast_tables(5, 7, 3, seed=40), *R.head(2, 37, 41)
    zeros = lambda *shape: np.zeros(shape, np.float32)

    def refused(code, fn):
        with pytest.raises(FlowGNNError) as x:
            fn()
        assert x.value.code == code and len(str(x.value)) > 40, x.value

    e = engine()
    refused(ERR_STATE, e.tokens)  # nothing ran
    e.set_ast_encoder(*ast)
    e.set_vocab_head(hw, hb)
    e.set_batch(batch)
    refused(ERR_STATE, e.run)  # no AST nodes
    refused(ERR_ARG, lambda: e.set_vocab_head(zeros(0, 37, 300), zeros(0, 37)))  # P < 1
    refused(ERR_ARG, lambda: e.set_vocab_head(zeros(2, 0, 300), zeros(2, 0)))  # V < 1
    refused(ERR_ARG, lambda: e.set_vocab_head(zeros(2, 37, 100), zeros(2, 37)))  # another width
    refused(ERR_ARG, lambda: e.set_ast_encoder(zeros(5, 100), zeros(7, 100), zeros(4, 100)))
    nan = hw.copy()
    nan[1, 3, 5] = np.nan
    refused(ERR_ARG, lambda: e.set_vocab_head(nan, hb))
    refused(ERR_UNSUPPORTED, lambda: e.set_emb_dim(100))  # while either is on
    s2s = weights.synth_set2set(num_tasks=1)
    refused(ERR_STATE, lambda: e.set_set2set_pooling(s2s, steps=2))  # the head came first
    other = engine()
    other.set_set2set_pooling(s2s, steps=2)
    refused(ERR_STATE, lambda: other.set_vocab_head(hw, hb))  # set2set came first
    x, depth = R.ast_nodes(batch.total_nodes, 5, 7, 3, seed=42)
    e.forward(batch, ast_nodes=(x, depth))  # the engine stays usable, and both are still on
    R.check_tokens(*e.tokens(), R.head_logits(e.forward(batch, return_embeddings=True, ast_nodes=(x, depth))[1], hw, hb), what="after the refusals")
    # the last run's tokens do not outlive a change of the head: another P, then off (each would move or free what that run wrote)
    assert e.tokens()[0].shape == (batch.num_graphs, 2)
    e.set_vocab_head(hw[:1], hb[:1])
    refused(ERR_STATE, e.tokens)
    e.forward(batch, ast_nodes=(x, depth))
    assert e.tokens()[0].shape == (batch.num_graphs, 1)
    e.set_vocab_head(None, None)
    refused(ERR_STATE, e.tokens)
    dev = [ctypes.c_void_p(1), ctypes.c_void_p(1)]
    assert e.lib.flowgnn_tokens_device(e._h, ctypes.byref(dev[0]), ctypes.byref(dev[1])) == ERR_STATE and dev[0].value == dev[1].value == 1
    e.forward(batch, ast_nodes=(x, depth))  # a run with the head off leaves none either
    refused(ERR_STATE, e.tokens)
    e.set_vocab_head(hw, hb)
    # device AST nodes are checked as flowgnn_set_batch_device checks its arrays: pinned host memory is refused, as x or as depth
    import torch
    e.set_batch(batch)
    dx, dd = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(depth).to("cuda:0")
    pinned = torch.from_numpy(x).pin_memory()
    ip = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), ctypes.POINTER(ctypes.c_int))
    assert e.lib.flowgnn_set_ast_nodes(e._h, ip(pinned), ip(dd), 1) == ERR_ARG
    assert e.lib.flowgnn_set_ast_nodes(e._h, ip(dx), ip(pinned), 1) == ERR_ARG
    refused(ERR_STATE, e.run)  # neither call attached anything
    x[3, 1] = 7  # an attribute at its table's size
    e.set_batch(batch)
    e.set_ast_nodes(x, depth)
    e.run()
    refused(4, e.results)  # FLOWGNN_ERR_NODE_FEAT
    gcn = Engine("GCN", device=0)
    gcn.set_model_emb_dim(300)
    refused(ERR_UNSUPPORTED, lambda: gcn.set_ast_encoder(*ast))
    refused(ERR_UNSUPPORTED, lambda: gcn.set_vocab_head(hw, hb))
    narrow = Engine("GIN", device=0)  # width 100
    refused(ERR_UNSUPPORTED, lambda: narrow.set_vocab_head(zeros(2, 37, 100), zeros(2, 37)))
    refused(ERR_UNSUPPORTED, lambda: narrow.set_ast_encoder(zeros(5, 100), zeros(7, 100), zeros(4, 100)))
