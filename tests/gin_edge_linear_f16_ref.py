"""GIN at width 300 with OGB's linear edge encoder and the f16 node MLP beside it (flowgnn.h: flowgnn_set_edge_linear_numeric; DESIGN.md
section 4.37): the mode's float64 restatement, the reference side of tests/test_gin_edge_linear_f16_gpu.py.  It is
tests/gin_edge_linear_ref.forward with a, the ReLU'd hidden units (in the scaled domain) and both matrices rounded to f16 as
tests/gin_wide_f16_ref.forward rounds them; the encoder, the walk and the virtual node's update are not rounded.  No GPU, and nothing
here knows what a GPU returns."""
import numpy as np

from tests import numpy_ref
from tests.f16_ref import pow2_scale, rounder
from tests.gin_edge_linear_ref import Out
from tests.test_gin_eps import self_scale


def forward(batch, w, el, ef, vn=None, eps=None):
    c, r = lambda a: np.asarray(a, np.float64), rounder("rne")
    nemb, we, be, ef = c(w["node_embedding_weight"]), c(el["w"]), c(el["b"]), c(ef)
    w1, b1, w2, b2 = c(w["node_mlp_1_weights"]), c(w["node_mlp_1_bias"]), c(w["node_mlp_2_weights"]), c(w["node_mlp_2_bias"])
    L, D = w1.shape[0], nemb.shape[-1]
    s = np.ones(L) if eps is None else c(self_scale(eps))
    N, G = batch.total_nodes, batch.num_graphs
    u, v = batch.global_edges().T
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    h = nemb[batch.node_feature.astype(np.int64) + numpy_ref.ND_OFF[None, :]].sum(axis=1)
    vec = None if vn is None else np.tile(c(vn["vn_embedding"]).reshape(-1), (G, 1))
    big = [1.0, float(np.abs(h).max())]
    for l in range(L):
        x = h if vec is None else h + vec[gid]
        m = np.zeros((N, D))
        np.add.at(m, v, np.maximum(x[u] + ef @ we[l].T + be[l], 0.0))
        a = m + s[l] * x
        s1, s2 = pow2_scale(w1[l]), pow2_scale(w2[l])
        hid = r(np.maximum(r(a) @ (r(w1[l] * s1) / s1).T + b1[l], 0.0) * s1) / s1
        h = hid @ (r(w2[l] * s2) / s2).T + b2[l]
        if l != L - 1:
            h = np.maximum(h, 0.0)
        big += [float(np.abs(a).max()), float(hid.max()), float(np.abs(h).max())]
        if vec is not None and l < L - 1:
            t = np.add.reduceat(x, off[:-1], axis=0) + vec
            thid = np.maximum(t @ c(vn["w1"])[l].T + c(vn["b1"])[l], 0.0)
            vec = np.maximum(thid @ c(vn["w2"])[l].T + c(vn["b2"])[l], 0.0)
    pooled = np.add.reduceat(h, off[:-1], axis=0) / c(batch.nums_of_nodes)[:, None]
    out = pooled @ c(w["graph_pred_weights"]).reshape(-1, D).T + c(w["graph_pred_bias"]).reshape(-1)
    return Out(out[:, 0] if out.shape[1] == 1 else out, h, max(big), float(np.abs(ef).max()) if ef.size else 0.0)
