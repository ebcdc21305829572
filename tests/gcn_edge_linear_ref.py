"""GCN at width 300 with OGB's linear edge encoder, the GCNConv of ogbg-ppa (flowgnn.h: flowgnn_set_model_edge_linear; DESIGN.md section
4.32): the reference side of tests/test_gcn_edge_linear_cpu.py and tests/test_gcn_edge_linear_gpu.py.  A plain float64 forward:
tests/gcn_wide_ref.forward / tests/gcn_wide_vn_ref.forward with ee = ef @ W_e[l].T + b_e[l] in place of the table row, the depth read
off the weights, and the optional virtual node.  No GPU, and nothing here knows what a GPU returns."""
from collections import namedtuple

import numpy as np

from tests import numpy_ref, split_ref

Out = namedtuple("Out", "logits rows scale max_feature operands")


def forward(batch, w, el, ef, vn=None):
    """Out(logits [G] or [G][T], pre_{L-1} rows [N][D], scale, max |ef|, operands).  scale: the largest magnitude of any activation, the
    `scale` of tests/parity.py; operands: the largest value a range guard of the split kernels watches besides the features (xin_l for
    l >= 1, t and the update's pre-scaled hidden values).  el: {"w": [L][D][F], "b": [L][D]}; ef [E][F] in the batch's edge order."""
    c = lambda a: np.asarray(a, np.float64)
    nemb, we, be, ef = c(w["node_embedding_weight"]), c(el["w"]), c(el["b"]), c(ef)
    cw, cb, root = c(w["convs_weight"]), c(w["convs_bias"]), c(w["convs_root_emb_weight"])
    bnw, bnb, bnm, bnv = c(w["bn_weight"]), c(w["bn_bias"]), c(w["bn_mean"]), c(w["bn_var"])
    L, D = cw.shape[0], nemb.shape[-1]
    assert we.shape[:2] == (L, D) and ef.shape == (batch.total_edges, we.shape[2]), (we.shape, ef.shape)
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
        x = xin @ cw[l].T + cb[l]
        ee = ef @ we[l].T + be[l]
        m = np.zeros((N, D))
        np.add.at(m, v, norm[:, None] * np.maximum(x[u] + ee, 0.0))
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
