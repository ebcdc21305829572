"""OGB's GNN(JK=..., residual=...) for gcn and gcn-virtual (flowgnn.h: flowgnn_set_model_jk_residual): the expected
values of tests/test_gcn_jk_residual_cpu.py and tests/test_gcn_jk_residual_gpu.py.  No GPU, and nothing here knows what a GPU returns.

  GNN / make_model / run / expected   tests/ogb_jk_torch.py's GNN_node and GNN_node_Virtualnode -- conv.py's, WITH their JK and residual
               arguments and the seven wrong forms of VARIANTS -- built with gnn_type="gcn": they take their convs from
               tests/ogb_torch._conv, so nothing of the node models is restated here.  The module tree and the construction order are
               tests/ogb_torch.GNN's (OGB's state_dict keys, and with ("last", False) tests/ogb_torch.make_model("gcn", ...) bit for bit).
               make_model follows ogb_torch.make_model's recipe with the flags ON during the SGD step and the settle passes, on
               ogb_torch.gcn_batch(): 29 graphs with a one-node graph, isolated nodes, a 17-node ring and a 129-node path, the
               smallest shapes that cross a 16-row tile, a 128-row workgroup and the masked column tile at 300.  As in ogb_jk_torch.py
               `r` passes through an nn.Identity and the pooled t of the virtual node's update does not, so the scale -- and with it
               every bound of the GPU tests -- is the smaller, stricter one.
  forward      a NumPy float64 restatement in the ENGINE's terms -- x_l, h_{l+1}, vn_l, r and the add order of flowgnn.h -- in the form
               of tests/gcn_wide_vn_ref.forward, on the exported files (the layer BatchNorms unfolded with the engine's 2^-10, the
               update's folded).  `operands`: the largest value the split-f16 kernels' range guards watch (x_1 .. x_4, t, the update's
               pre-scaled hidden units).
  load         the exported files of a directory, as forward takes them.
"""
import copy
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from flowgnn_amd import weights
from tests import gcn_wide_ref as R, numpy_ref, ogb_jk_torch as J, ogb_torch as T, split_ref

JKS, SETTINGS, VARIANTS, variants_of = J.JKS, J.SETTINGS, J.VARIANTS, J.variants_of
L = T.NUM_LAYER
WIDE = 300


class GNN(nn.Module):
    """gnn.py's GNN(gnn_type="gcn" / "gcn-virtual", JK=..., residual=...), mean / sum / max pooling; constructed in tests/ogb_torch.GNN's order"""

    def __init__(self, num_tasks=1, num_layer=L, emb_dim=WIDE, virtual_node=True, drop_ratio=T.DROP_RATIO, graph_pooling="mean", JK="last",
                 residual=False):
        super().__init__()
        if graph_pooling not in ("mean", "sum", "max") or JK not in JKS:
            raise ValueError((graph_pooling, JK))
        node = J.GNN_node_Virtualnode if virtual_node else J.GNN_node
        self.gnn_node = node(num_layer, emb_dim, drop_ratio=drop_ratio, gnn_type="gcn")
        self.gnn_node.JK, self.gnn_node.residual = JK, bool(residual)
        self.graph_pooling = graph_pooling
        self.graph_pred_linear = nn.Linear(emb_dim, num_tasks)
        self.pool = nn.Identity()
        self.jk = nn.Identity()  # (no parameters: a place for run()'s hook, the rows the readout pools)

    embed = J.GNN.embed
    forward = J.GNN.forward


def make_model(virtual_node, jk="last", residual=False, num_tasks=1, pooling="mean", seed=0, damped=True):
    """tests/ogb_torch.make_model("gcn", virtual_node, 300, ...)'s recipe, step for step, on GNN(JK=jk, residual=residual); shared between
    callers, who must not change it (copy.deepcopy first)."""
    return _make_model(bool(virtual_node), jk, bool(residual), int(num_tasks), pooling, int(seed), bool(damped))


@functools.lru_cache(maxsize=None)
def _make_model(virtual_node, jk, residual, num_tasks, pooling, seed, damped):
    if pooling != "mean":
        model = copy.deepcopy(_make_model(virtual_node, jk, residual, num_tasks, "mean", seed, damped))
        model.graph_pooling = pooling
        return model
    torch.manual_seed(seed)
    model = GNN(num_tasks=num_tasks, emb_dim=WIDE, virtual_node=virtual_node, graph_pooling=pooling, JK=jk, residual=residual).double()
    args = T.tensors(T.gcn_batch())
    gen = torch.Generator().manual_seed(1000 + seed)
    labels = torch.randint(0, 2, (T.gcn_batch().num_graphs, num_tasks), generator=gen).double()
    opt = torch.optim.SGD(model.parameters(), lr=T.SGD_LR)
    model.train()
    for _ in range(T.SGD_STEPS):
        opt.zero_grad()
        F.binary_cross_entropy_with_logits(model(*args), labels).backward()
        opt.step()
    with torch.no_grad():  # (GCNConv has no eps: ogb_torch.make_model draws none for it either)
        for bn in T._bn_modules(model):
            bn.weight.mul_(1 + 0.2 * torch.randn(bn.weight.shape, generator=gen).double())
            bn.bias.add_(0.2 * torch.randn(bn.bias.shape, generator=gen).double())
        if virtual_node:
            w = model.gnn_node.virtualnode_embedding.weight
            w.add_(T.VN_EMBEDDING_STD * torch.randn(w.shape, generator=gen).double())
        if damped:
            for _ in range(T.SETTLE_PASSES):
                model(*args)
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


with_variant = J.with_variant
run = T.run  # (Out(logits, rows = r, pooled), scale, tensors): the hooks see every Identity, self.jk included


def expected(virtual_node, jk, residual, num_tasks=1, pooling="mean", damped=True):
    """run(make_model(...), gcn_batch()), computed once and shared."""
    return _expected(bool(virtual_node), jk, bool(residual), int(num_tasks), pooling, bool(damped))


@functools.lru_cache(maxsize=None)
def _expected(virtual_node, jk, residual, num_tasks, pooling, damped):
    return run(make_model(virtual_node, jk, residual, num_tasks=num_tasks, pooling=pooling, damped=damped), T.gcn_batch())


@functools.lru_cache(maxsize=None)
def variant_rows(virtual_node, jk, residual, variant):
    """The rows r of the wrong form `variant` of expected(virtual_node, jk, residual)'s model, on gcn_batch()."""
    return run(with_variant(make_model(virtual_node, jk, residual), variant), T.gcn_batch())[0].rows


# ---------------------------------------------------------------- the engine's terms, in NumPy
Ref = namedtuple("Ref", "logits rows pooled h5 scale operands")
ND_OFF, ED_OFF = numpy_ref.ND_OFF, numpy_ref.ED_OFF


def load(directory, virtual_node, num_tasks=1):
    """(w, vn or None) of an exported directory at width 300"""
    w = weights.load_gcn_weights(directory, num_tasks=num_tasks, emb_dim=WIDE)
    return w, (weights.load_gcn_virtual_node(directory, emb_dim=WIDE) if virtual_node else None)


def forward(batch, w, vn=None, jk="last", residual=False, pooling="mean", bn_eps=2.0 ** -10, drop=None):
    """Ref(logits, r [N][D], pooled [G][D], h_5 [N][D], scale, operands) in float64, flowgnn.h's definition line by line:
        x_0 = h_0 (+ E);  h_{l+1} = y_l (+ x_l);  x_{l+1} = h_{l+1} (+ vn_{l+1}[g]);  vn_{l+1} = (vn_l +) relu(w2 relu(w1 t + b1) + b2)
        r = h_5, or ((((x_0 + x_1) + x_2) + x_3) + x_4) + h_5
    y_l = relu(conv_l(x_l)) for l < 4 and conv_4(x_4), conv_l as tests/gcn_wide_ref.forward has it: the product W_l x + b_l, the walk,
    root, 1 / (deg + 1) and the layer's BatchNorm (bn_eps: the engine's 2^-10 for the exported files, torch's 1e-5 for a state_dict).
    drop: a WRONG form for tests/test_wide_shapes_cpu.py, as tests/ogb_jk_torch.forward takes it."""
    assert jk in JKS, jk
    assert drop is None or (drop[0] == "residual" and residual) or (drop[0] == "jk" and jk == "sum"), drop
    keep_res = 1.0 - drop[1] if drop is not None and drop[0] == "residual" else 1.0
    keep_jk = 1.0 - drop[1] if drop is not None and drop[0] == "jk" else 1.0
    c = lambda a: np.asarray(a, dtype=np.float64)
    nemb, eemb = c(w["node_embedding_weight"]), c(w["edge_embedding_weight"])
    cw, cb, root = c(w["convs_weight"]), c(w["convs_bias"]), c(w["convs_root_emb_weight"])
    bnw, bnb, bnm, bnv = c(w["bn_weight"]), c(w["bn_bias"]), c(w["bn_mean"]), c(w["bn_var"])
    D = nemb.shape[-1]
    assert cw.shape == (L, D, D) and eemb.shape == (L, 13, D) and root.shape == (L, D), (cw.shape, eemb.shape, root.shape)
    pw, pb = c(w["graph_pred_weights"]).reshape(-1, D), c(w["graph_pred_bias"]).reshape(-1)
    N, G = batch.total_nodes, batch.num_graphs
    ge = batch.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    seg = lambda rows: np.add.reduceat(rows, off[:-1], axis=0)  # (every graph has a node)
    outdeg = np.bincount(u, minlength=N).astype(np.float64)
    dinv = np.where(outdeg > 0, 1.0 / np.sqrt(outdeg + 1.0), 0.0)
    norm = dinv[u] * dinv[v]
    bn = lambda t, l: (t - bnm[l]) / np.sqrt(bnv[l] + bn_eps) * bnw[l] + bnb[l]
    h = nemb[batch.node_feature.astype(np.int64) + ND_OFF[None, :]].sum(axis=1)
    big, ops = [1.0, float(np.abs(h).max())], [0.0]
    if vn is not None:
        E = c(vn["vn_embedding"]).reshape(-1)
        v1, c1, v2, c2 = c(vn["w1"]), c(vn["b1"]), c(vn["w2"]), c(vn["b2"])
        vec = np.tile(E, (G, 1))
        x = h + vec[gid]
    else:
        x = h
    r = None
    for l in range(L):
        z = x @ cw[l].T + cb[l]
        ee = eemb[l][batch.edge_attr.astype(np.int64) + ED_OFF[None, :]].sum(axis=1)
        m = np.zeros((N, D))
        np.add.at(m, v, norm[:, None] * np.maximum(z[u] + ee, 0.0))
        pre = bn(m + np.maximum(z + root[l], 0.0) / (outdeg[:, None] + 1.0), l)
        y = np.maximum(pre, 0.0) if l != L - 1 else pre
        h = y + keep_res * x if residual else y
        big.extend([float(np.abs(x).max()), float(np.abs(z).max()), float(np.abs(m).max()), float(np.abs(pre).max()), float(np.abs(h).max())])
        if vn is not None and l < L - 1:
            t = seg(x) + vec
            uh = np.maximum(t @ v1[l].T + c1[l], 0.0)
            upd = np.maximum(uh @ v2[l].T + c2[l], 0.0)
            vec = vec + upd if residual else upd
            big.extend([float(np.abs(t).max()), float(uh.max()), float(vec.max())])
            ops.extend([float(np.abs(t).max()), split_ref.pow2_scale(np.asarray(vn["w1"], np.float32)[l]) * float(uh.max())])
            x_next = h + vec[gid]
        else:
            x_next = h
        if l < L - 1:
            ops.append(float(np.abs(x_next).max()))  # a of stage l: what DS_SPLIT2 splits
        if jk == "sum":
            r = keep_jk * (x if l == 0 else r) + x_next  # (x_next of the last layer is h_5)
        x = x_next
    if jk == "last":
        r = h
    big.append(float(np.abs(r).max()))
    if pooling == "mean":
        pooled = seg(r) / c(batch.nums_of_nodes)[:, None]
    elif pooling == "sum":
        pooled = seg(r)
    else:
        assert pooling == "max", pooling
        pooled = np.maximum.reduceat(r, off[:-1], axis=0)
    big.append(float(np.abs(pooled).max()))
    out = pooled @ pw.T + pb
    return Ref(out[:, 0] if out.shape[1] == 1 else out, r, pooled, h, max(big), max(ops))


def node_logits(w, rows):
    return R.node_logits(w, rows)
