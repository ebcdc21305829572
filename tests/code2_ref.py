"""ogbg-code2 on the 300-wide GIN (flowgnn.h: flowgnn_set_vocab_head, flowgnn_set_ast_encoder): the reference side
of tests/test_code2_gpu.py.  Plain float64 NumPy: the AST node encoder, tests/gin_edge_linear_ref's layers, the list head's logits, and
the two conditions a returned (token, score) pair is held to.  No GPU, and nothing here knows what a GPU returns."""
from collections import namedtuple

import numpy as np

from tests import parity
from tests.test_gin_eps import self_scale

Out = namedtuple("Out", "logits rows pooled scale")
c = lambda a: np.asarray(a, np.float64)


def head_logits(pooled, w, b):
    """[G][P][V] = b[p][v] + W[p][v] . pooled[g] in float64 (pooled: what the engine returned, exact in float64)"""
    return np.einsum("pvd,gd->gpv", c(w), c(pooled)) + c(b)[None]


def check_tokens(ids, scores, logits, equal=False, what=""):
    """Every (g, p), none excluded: score is the float64 logit at the returned index within parity's rule, and that logit is no further
    below the float64 maximum than twice that bound.  equal: the index is the float64 argmax's (a planted winner)."""
    G, P, V = logits.shape
    ids, scores = np.asarray(ids), np.asarray(scores, np.float64)
    assert ids.shape == (G, P) and scores.shape == (G, P) and ids.dtype == np.int32, (what, ids.shape, ids.dtype)
    assert (ids >= 0).all() and (ids < V).all(), (what, "an index outside the vocabulary", int(ids.min()), int(ids.max()))
    at = np.take_along_axis(logits, ids[..., None].astype(np.int64), axis=2)[..., 0]
    top = logits.max(axis=2)
    scale = parity.oracle_scale(logits)
    bound = parity.REL * (scale + np.abs(top))
    r1 = parity.err_ratio(scores, at, scale)
    r2 = float(((top - at) / (2 * bound)).max())
    print(what, f"score against its logit: {r1:.4f} of the bound; the logit below the maximum: {r2:.4f} of twice the bound")
    assert np.isfinite(scores).all() and r1 <= 1.0 and r2 <= 1.0, (what, r1, r2)
    if equal:
        assert np.array_equal(ids, logits.argmax(axis=2)), (what, "a planted winner was missed")


def plant(w, b, pooled, rows):
    """b with b[p][rows[p]] raised until that entry beats every other of its position by 500 x the bound, for every graph; the margin"""
    b = np.array(b, np.float32)
    L = head_logits(pooled, w, b)
    scale = parity.oracle_scale(L)
    for p, v in enumerate(rows):
        b[p, v] += np.float32((L[:, p].max() - L[:, p, v].min()) + 0.05 * (scale + np.abs(L[:, p]).max()))
    L = head_logits(pooled, w, b)
    for p, v in enumerate(rows):
        others = np.delete(L[:, p], v, axis=1).max(axis=1) if L.shape[2] > 1 else np.full(L.shape[0], -np.inf)
        assert ((L[:, p, v] - others) > 100 * parity.REL * (parity.oracle_scale(L) + np.abs(L[:, p, v]))).all()  # far beyond the bound
    return b


def forward(batch, w, el, ef, ast, x, depth, vn=None, eps=None):
    """Out(logits, h_L rows [N][D], pooled [G][D], scale): code2's GNN_node -- h0 = type[x0] + attr[x1] + depth[min(d, max_depth)], then
    tests/gin_edge_linear_ref.forward's layers (GINConv with Linear(F, D) on the edge features, OGB's virtual node), mean pool"""
    ty, at, dp = c(ast[0]), c(ast[1]), c(ast[2])
    we, be, ef = c(el["w"]), c(el["b"]), c(ef)
    w1, b1, w2, b2 = c(w["node_mlp_1_weights"]), c(w["node_mlp_1_bias"]), c(w["node_mlp_2_weights"]), c(w["node_mlp_2_bias"])
    L, D = w1.shape[0], ty.shape[1]
    s = np.ones(L) if eps is None else c(self_scale(eps))
    N, G = batch.total_nodes, batch.num_graphs
    u, v = batch.global_edges().T
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    h = ty[x[:, 0]] + at[x[:, 1]] + dp[np.minimum(depth, len(dp) - 1)]
    vec = None if vn is None else np.tile(c(vn["vn_embedding"]).reshape(-1), (G, 1))
    big = [1.0, float(np.abs(h).max())]
    for l in range(L):
        xl = h if vec is None else h + vec[gid]
        m = np.zeros((N, D))
        np.add.at(m, v, np.maximum(xl[u] + ef @ we[l].T + be[l], 0.0))
        a = m + s[l] * xl
        hid = np.maximum(a @ w1[l].T + b1[l], 0.0)
        h = hid @ w2[l].T + b2[l]
        if l != L - 1:
            h = np.maximum(h, 0.0)
        big += [float(np.abs(a).max()), float(hid.max()), float(np.abs(h).max())]
        if vec is not None and l < L - 1:
            t = np.add.reduceat(xl, off[:-1], axis=0) + vec
            thid = np.maximum(t @ c(vn["w1"])[l].T + c(vn["b1"])[l], 0.0)
            vec = np.maximum(thid @ c(vn["w2"])[l].T + c(vn["b2"])[l], 0.0)
            big += [float(np.abs(t).max()), float(thid.max()), float(vec.max())]
    pooled = np.add.reduceat(h, off[:-1], axis=0) / c(batch.nums_of_nodes)[:, None]
    out = pooled @ c(w["graph_pred_weights"]).reshape(-1, D).T + c(w["graph_pred_bias"]).reshape(-1)
    return Out(out[:, 0] if out.shape[1] == 1 else out, h, pooled, max(big))


def head(positions, vocab, seed, width=300):
    """Seeded head tensors at Linear(width, vocab)'s own scale, full fp32 mantissas"""
    u = np.random.default_rng(seed).uniform(-1, 1, (positions, vocab, width + 1)).astype(np.float32) / np.float32(np.sqrt(width))
    return np.ascontiguousarray(u[:, :, :width]), np.ascontiguousarray(u[:, :, width])


def ast_tables(n_types, n_attrs, max_depth, seed, width=300):
    rng = np.random.default_rng(seed)
    return tuple((0.5 * rng.standard_normal((n, width))).astype(np.float32) for n in (n_types, n_attrs, max_depth + 1))


def ast_nodes(num_nodes, n_types, n_attrs, max_depth, seed):
    """x [N][2], depth [N] int32; a third of the depths lie beyond max_depth (the clamp), and both ends of each table are hit"""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.integers(0, n_types, num_nodes), rng.integers(0, n_attrs, num_nodes)], 1).astype(np.int32)
    depth = rng.integers(0, max_depth + max_depth // 2 + 2, num_nodes).astype(np.int32)
    x[0], x[-1], depth[0], depth[-1] = (0, 0), (n_types - 1, n_attrs - 1), 0, max_depth + 7
    return x, depth
