"""GIN at width 300 with OGB's linear edge encoder, the layer of ogbg-ppa (flowgnn.h: flowgnn_set_edge_linear):
the reference side of tests/test_gin_edge_linear_cpu.py and tests/test_gin_edge_linear_gpu.py.  A plain float64 forward:
tests/gin_wide_ref.forward with ee = ef @ W_e[l].T + b_e[l] in place of the table lookup, the depth read off the weights, and OGB's
virtual node as tests/gin_wide_vn_ref.forward has it.  No GPU, and nothing here knows what a GPU returns."""
from collections import namedtuple

import numpy as np

from tests import numpy_ref
from tests.test_gin_eps import self_scale

Out = namedtuple("Out", "logits rows scale max_feature")


def forward(batch, w, el, ef, vn=None, eps=None, eps_f64=False):
    """Out(logits [G] or [G][T], h_L rows [N][D], scale, max |ef|); scale: the largest magnitude of any activation, the `scale` of
    tests/parity.py.  el: {"w": [L][D][F], "b": [L][D]}; ef [E][F] in the batch's edge order; vn: the five tensors of OGB's virtual node."""
    c = lambda a: np.asarray(a, np.float64)
    nemb, we, be, ef = c(w["node_embedding_weight"]), c(el["w"]), c(el["b"]), c(ef)
    w1, b1, w2, b2 = c(w["node_mlp_1_weights"]), c(w["node_mlp_1_bias"]), c(w["node_mlp_2_weights"]), c(w["node_mlp_2_bias"])
    L, D = w1.shape[0], nemb.shape[-1]
    assert we.shape[:2] == (L, D) and ef.shape == (batch.total_edges, we.shape[2]), (we.shape, ef.shape)
    s = np.ones(L) if eps is None else (1.0 + c(eps) if eps_f64 else c(self_scale(eps)))  # (the engine's float32 1 + eps; eps_f64: OGB's)
    N, G = batch.total_nodes, batch.num_graphs
    u, v = batch.global_edges().T
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    h = nemb[batch.node_feature.astype(np.int64) + numpy_ref.ND_OFF[None, :]].sum(axis=1)
    vec = None if vn is None else np.tile(c(vn["vn_embedding"]).reshape(-1), (G, 1))
    big = [1.0, float(np.abs(h).max())]
    for l in range(L):
        x = h if vec is None else h + vec[gid]
        ee = ef @ we[l].T + be[l]
        m = np.zeros((N, D))
        np.add.at(m, v, np.maximum(x[u] + ee, 0.0))
        a = m + s[l] * x
        hid = np.maximum(a @ w1[l].T + b1[l], 0.0)
        h = hid @ w2[l].T + b2[l]
        if l != L - 1:
            h = np.maximum(h, 0.0)
        big += [float(np.abs(a).max()), float(hid.max()), float(np.abs(h).max())]
        if vec is not None and l < L - 1:
            t = np.add.reduceat(x, off[:-1], axis=0) + vec
            thid = np.maximum(t @ c(vn["w1"])[l].T + c(vn["b1"])[l], 0.0)
            vec = np.maximum(thid @ c(vn["w2"])[l].T + c(vn["b2"])[l], 0.0)
            big += [float(np.abs(t).max()), float(thid.max()), float(vec.max())]
    pooled = np.add.reduceat(h, off[:-1], axis=0) / c(batch.nums_of_nodes)[:, None]
    out = pooled @ c(w["graph_pred_weights"]).reshape(-1, D).T + c(w["graph_pred_bias"]).reshape(-1)
    return Out(out[:, 0] if out.shape[1] == 1 else out, h, max(big), float(np.abs(ef).max()) if ef.size else 0.0)


def features(num_edges, dim, seed):
    """Seeded float32 features, mixed in sign, a fifth of them exact zeros, the rest with full fp32 mantissas (not f16-representable)"""
    rng = np.random.default_rng(seed)
    ef = (1.5 * rng.standard_normal((num_edges, dim))).astype(np.float32)
    ef[rng.random((num_edges, dim)) < 0.2] = 0.0
    return ef


def edge_linear(num_layers, dim, seed, width=300):
    """Seeded encoder tensors at Linear(dim, width)'s own scale"""
    u = np.random.default_rng(seed).uniform(-1, 1, (num_layers, width, dim + 1)).astype(np.float32) / np.float32(np.sqrt(dim))
    return {"w": np.ascontiguousarray(u[:, :, :dim]), "b": np.ascontiguousarray(u[:, :, dim])}
