"""GCN at width 300 with OGB's linear edge encoder and the f16 product beside it (flowgnn.h: flowgnn_set_model_edge_linear_numeric;
DESIGN.md section 4.38): the mode's float64 restatement, the reference side of tests/test_gcn_edge_linear_f16_gpu.py.  It is
tests/gcn_edge_linear_ref.forward with the operand a = xin_l and the matrix of the products x_1 .. x_{L-1} rounded to f16 as
tests/gcn_wide_f16_ref.forward rounds them (x_0 is no matrix-pipe product: W_0 is applied to the node table on the host); the encoder,
the walk, the epilogue and the virtual node's update are not rounded.  No GPU, and nothing here knows what a GPU returns."""
import numpy as np

from tests import numpy_ref, split_ref
from tests.f16_ref import pow2_scale, rounder
from tests.gcn_edge_linear_ref import Out


def forward(batch, w, el, ef, vn=None):
    c, r = lambda a: np.asarray(a, np.float64), rounder("rne")
    nemb, we, be, ef = c(w["node_embedding_weight"]), c(el["w"]), c(el["b"]), c(ef)
    cw, cb, root = c(w["convs_weight"]), c(w["convs_bias"]), c(w["convs_root_emb_weight"])
    bnw, bnb, bnm, bnv = c(w["bn_weight"]), c(w["bn_bias"]), c(w["bn_mean"]), c(w["bn_var"])
    L, D = cw.shape[0], nemb.shape[-1]
    N, G = batch.total_nodes, batch.num_graphs
    u, v = batch.global_edges().T
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    outdeg = np.bincount(u, minlength=N).astype(np.float64)
    dinv = np.where(outdeg > 0, 1.0 / np.sqrt(outdeg + 1.0), 0.0)
    norm = dinv[u] * dinv[v]
    h = nemb[batch.node_feature.astype(np.int64) + numpy_ref.ND_OFF[None, :]].sum(axis=1)
    vec = None if vn is None else np.tile(c(vn["vn_embedding"]).reshape(-1), (G, 1))
    big, ops = [1.0, float(np.abs(h).max())], [0.0]
    for l in range(L):
        xin = h if vec is None else h + vec[gid]
        s = pow2_scale(cw[l])
        x = (xin @ cw[l].T if l == 0 else r(xin) @ (r(cw[l] * s) / s).T) + cb[l]
        m = np.zeros((N, D))
        np.add.at(m, v, norm[:, None] * np.maximum(x[u] + ef @ we[l].T + be[l], 0.0))
        pre = ((m + np.maximum(x + root[l], 0.0) / (outdeg[:, None] + 1.0)) - bnm[l]) / np.sqrt(bnv[l] + 2.0 ** -10) * bnw[l] + bnb[l]
        big += [float(np.abs(xin).max()), float(np.abs(x).max()), float(np.abs(m).max()), float(np.abs(pre).max())]
        if l > 0:
            ops.append(float(np.abs(xin).max()))
        if vec is not None and l < L - 1:
            t = np.add.reduceat(xin, off[:-1], axis=0) + vec
            hid = np.maximum(t @ c(vn["w1"])[l].T + c(vn["b1"])[l], 0.0)
            vec = np.maximum(hid @ c(vn["w2"])[l].T + c(vn["b2"])[l], 0.0)
            big += [float(np.abs(t).max()), float(hid.max()), float(vec.max())]
            ops += [float(np.abs(t).max()), split_ref.pow2_scale(np.asarray(vn["w1"], np.float32)[l]) * float(hid.max())]
        h = np.maximum(pre, 0.0)
    pooled = np.add.reduceat(pre, off[:-1], axis=0) / c(batch.nums_of_nodes)[:, None]
    out = pooled @ c(w["graph_pred_weights"]).reshape(-1, D).T + c(w["graph_pred_bias"]).reshape(-1)
    return Out(out[:, 0] if out.shape[1] == 1 else out, pre, max(big + [float(np.abs(pooled).max())]), float(np.abs(ef).max()) if ef.size else 0.0,
               max(ops))
