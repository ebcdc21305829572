"""OGB's GNN(JK=..., residual=...) for gin and gin-virtual (flowgnn.h: flowgnn_set_jk_residual): the expected
values of tests/test_jk_residual_cpu.py and tests/test_jk_residual_gpu.py.  No GPU, and nothing here knows what a GPU returns.

  GNN / make_model / run / expected   a float64 `torch.nn` transcription of ogb/examples/graphproppred/mol/conv.py's GNN_node and
               GNN_node_Virtualnode WITH their JK and residual arguments, on tests/ogb_torch.py's convs and encoders (same module
               tree and construction order: OGB's state_dict keys, and with ("last", False) tests/ogb_torch.make_model bit for bit).
               JK "sum" runs over range(num_layer + 1), six terms, as OGB's current source does (older releases: range(num_layer)).
               make_model follows ogb_torch.make_model's recipe with the flags ON during the SGD step and the settle passes, so the
               BatchNorm statistics are those of a residual model's activations.  `r`, the rows the readout pools, passes through
               an nn.Identity, so ogb_torch.run's scale hooks see it.  The pooled t of the virtual node's update does NOT pass through
               ogb_torch's `pool` Identity here: under the residual t is the largest activation by a third (6 394 against 4 947 for
               gin-virtual, sum with residual), so the scale -- and with it every bound of the GPU tests -- is the smaller, stricter one.
  VARIANTS     the wrong forms a flag on the node models expresses (the mutation tests).
  forward      a NumPy float64 restatement in the ENGINE's terms -- x_l, h_{l+1}, vn_l, r and the add order of flowgnn.h -- in the
               form of tests/gin_wide_vn_ref.forward, on the exported weights (BatchNorms folded, eps as (float)(1.0f + eps)); with
               f16=True the node MLP's operands are rounded as tests/gin_wide_f16_ref.forward rounds them.
               `operands`, Ref's last field: the largest value the range guards of the split-f16 / f16 kernels watch (gin_wide_body.h,
               gin_wide_f16_body.h: |a| and the ReLU'd hidden units times the first matrix's power-of-two pre-scale, per layer and
               per update), as tests/ogb_gcn_jk_torch.forward has it for GCN.
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
from tests import f16_ref, gin_wide_vn_ref as V, numpy_ref, ogb_torch as T, split_ref
from tests.test_gin_eps import self_scale

JKS = ("last", "sum")
SETTINGS = (("last", True), ("sum", False), ("sum", True))  # the non-default ones
VARIANTS = ("residual_before_relu", "no_residual_in_last_layer", "residual_without_vn", "vn_update_without_residual",
            "jk_without_last_term", "jk_without_x0", "jk_over_h_without_vn")
# which setting a wrong form differs under at all: (needs residual, needs JK sum, needs the virtual node)
VARIANT_NEEDS = {"residual_before_relu": (True, False, False), "no_residual_in_last_layer": (True, False, False),
                 "residual_without_vn": (True, False, True), "vn_update_without_residual": (True, False, True),
                 "jk_without_last_term": (False, True, False), "jk_without_x0": (False, True, False),
                 "jk_over_h_without_vn": (False, True, True)}
L = T.NUM_LAYER
WIDE = 300


def variants_of(vn, jk, residual):
    """The wrong forms that are a different computation under this setting."""
    return [v for v in VARIANTS if (residual or not VARIANT_NEEDS[v][0]) and (jk == "sum" or not VARIANT_NEEDS[v][1]) and
            (vn or not VARIANT_NEEDS[v][2])]


def _jk(h_list, xs, JK, variant):
    """h_list as OGB has it at the end of the loop: entries 0 .. L - 1 with the virtual node's vector inside (x_l), entry L = h_L;
    xs: the rows WITHOUT the vector (the virtual-node model's wrong form)"""
    if JK == "last":
        return h_list[-1]
    terms = list(xs) + [h_list[-1]] if variant == "jk_over_h_without_vn" else list(h_list)
    if variant == "jk_without_last_term":
        terms = terms[:-1]
    if variant == "jk_without_x0":
        terms = terms[1:]
    out = 0
    for t in terms:
        out = out + t
    return out


class GNN_node(T.GNN_node):
    """conv.py's GNN_node with JK and residual"""
    JK, residual, variant = "last", False, None

    def forward(self, x, edge_index, edge_attr, batch):
        v, last = self.variant, self.num_layer - 1
        h_list = [self.atom_encoder(x)]
        for layer in range(self.num_layer):
            h = self.batch_norms[layer](self.convs[layer](h_list[layer], edge_index, edge_attr))
            res = self.residual and not (v == "no_residual_in_last_layer" and layer == last)
            if res and v == "residual_before_relu":
                h = h + h_list[layer]
            if layer != last:
                h = F.relu(h)
            h = F.dropout(h, self.drop_ratio, training=self.training)
            if res and v != "residual_before_relu":
                h = h + h_list[layer]
            h_list.append(h)
        return _jk(h_list, h_list[:-1], self.JK, v)


class GNN_node_Virtualnode(T.GNN_node_Virtualnode):
    """conv.py's GNN_node_Virtualnode with JK and residual (self.variant: this file's VARIANTS, not ogb_torch's)"""
    JK, residual = "last", False

    def forward(self, x, edge_index, edge_attr, batch):
        v, last = self.variant, self.num_layer - 1
        G = int(batch[-1].item()) + 1
        vn = self.virtualnode_embedding(torch.zeros(G, dtype=torch.long))
        h_list, xs = [self.atom_encoder(x)], []
        for layer in range(self.num_layer):
            xs.append(h_list[layer])
            h_list[layer] = self.rows(h_list[layer] + vn[batch])  # (OGB adds in place: the residual and the JK sum see the sum)
            h = self.batch_norms[layer](self.convs[layer](h_list[layer], edge_index, edge_attr))
            res = self.residual and not (v == "no_residual_in_last_layer" and layer == last)
            skip = xs[layer] if v == "residual_without_vn" else h_list[layer]
            if res and v == "residual_before_relu":
                h = h + skip
            if layer != last:
                h = F.relu(h)
            h = F.dropout(h, self.drop_ratio, training=self.training)
            if res and v != "residual_before_relu":
                h = h + skip
            h_list.append(h)
            if layer < last:
                t = T._scatter_add(h_list[layer], batch, G) + vn
                u = F.dropout(self.mlp_virtualnode_list[layer](t), self.drop_ratio, training=self.training)  # (t is not hooked: below)
                vn = vn + u if (self.residual and v != "vn_update_without_residual") else u
        return _jk(h_list, xs, self.JK, v)


class GNN(nn.Module):
    """gnn.py's GNN(JK=..., residual=...), mean / sum / max pooling; constructed in tests/ogb_torch.GNN's order"""

    def __init__(self, num_tasks=1, num_layer=L, emb_dim=WIDE, virtual_node=True, drop_ratio=T.DROP_RATIO, graph_pooling="mean", JK="last",
                 residual=False):
        super().__init__()
        if graph_pooling not in ("mean", "sum", "max") or JK not in JKS:
            raise ValueError((graph_pooling, JK))
        node = GNN_node_Virtualnode if virtual_node else GNN_node
        self.gnn_node = node(num_layer, emb_dim, drop_ratio=drop_ratio, gnn_type="gin")
        self.gnn_node.JK, self.gnn_node.residual = JK, bool(residual)
        self.graph_pooling = graph_pooling
        self.graph_pred_linear = nn.Linear(emb_dim, num_tasks)
        self.pool = nn.Identity()
        self.jk = nn.Identity()  # (no parameters: a place for run()'s hook, the rows the readout pools)

    def embed(self, x, edge_index, edge_attr, ptr):
        G = ptr.numel() - 1
        batch = torch.repeat_interleave(torch.arange(G), ptr[1:] - ptr[:-1])
        h = self.jk(self.gnn_node(x, edge_index, edge_attr, batch))
        if self.graph_pooling == "max":
            idx = batch.view(-1, 1).expand(-1, h.shape[1])
            pooled = torch.zeros((G, h.shape[1]), dtype=h.dtype).scatter_reduce_(0, idx, h, "amax", include_self=False)
        else:
            pooled = T._scatter_add(h, batch, G)
            if self.graph_pooling == "mean":
                pooled = pooled / (ptr[1:] - ptr[:-1]).to(h.dtype).view(-1, 1)
        return h, self.pool(pooled)

    def forward(self, x, edge_index, edge_attr, ptr):
        return self.graph_pred_linear(self.embed(x, edge_index, edge_attr, ptr)[1])


def make_model(virtual_node, jk="last", residual=False, num_tasks=1, pooling="mean", seed=0, damped=True):
    """tests/ogb_torch.make_model("gin", virtual_node, 300, ...)'s recipe, step for step, on GNN(JK=jk, residual=residual); shared between
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
    args = T.tensors(T.gin_batch())
    gen = torch.Generator().manual_seed(1000 + seed)
    labels = torch.randint(0, 2, (T.gin_batch().num_graphs, num_tasks), generator=gen).double()
    opt = torch.optim.SGD(model.parameters(), lr=T.SGD_LR)
    model.train()
    for _ in range(T.SGD_STEPS):
        opt.zero_grad()
        F.binary_cross_entropy_with_logits(model(*args), labels).backward()
        opt.step()
    with torch.no_grad():
        for conv in model.gnn_node.convs:
            mag = 0.05 + 0.25 * torch.rand(1, generator=gen).double()
            sign = 1.0 if torch.rand(1, generator=gen).item() < 0.5 else -1.0
            conv.eps.copy_(sign * mag)
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


def with_variant(model, variant):
    """A copy of a model that computes the wrong form `variant`."""
    assert variant in VARIANTS, variant
    m = copy.deepcopy(model)
    m.gnn_node.variant = variant
    return m


run = T.run  # (Out(logits, rows = r, pooled), scale, tensors): the hooks see every Identity, self.jk included


def expected(virtual_node, jk, residual, num_tasks=1, pooling="mean", damped=True):
    """run(make_model(...), gin_batch()), computed once and shared."""
    return _expected(bool(virtual_node), jk, bool(residual), int(num_tasks), pooling, bool(damped))


@functools.lru_cache(maxsize=None)
def _expected(virtual_node, jk, residual, num_tasks, pooling, damped):
    return run(make_model(virtual_node, jk, residual, num_tasks=num_tasks, pooling=pooling, damped=damped), T.gin_batch())


@functools.lru_cache(maxsize=None)
def variant_rows(virtual_node, jk, residual, variant):
    """The rows r of the wrong form `variant` of expected(virtual_node, jk, residual)'s model, on gin_batch()."""
    return run(with_variant(make_model(virtual_node, jk, residual), variant), T.gin_batch())[0].rows


# ---------------------------------------------------------------- the engine's terms, in NumPy
Ref = namedtuple("Ref", "logits rows pooled h5 scale operands")
ND_OFF, ED_OFF = numpy_ref.ND_OFF, numpy_ref.ED_OFF


def load(directory, virtual_node, num_tasks=1):
    """(w, vn or None, eps) of an exported directory at width 300"""
    w = weights.load_gin_weights(directory, num_tasks=num_tasks, emb_dim=WIDE)
    vn = weights.load_gin_virtual_node(directory, emb_dim=WIDE) if virtual_node else None
    return w, vn, weights.load_gin_eps(directory, emb_dim=WIDE)


def forward(batch, w, vn=None, eps=None, jk="last", residual=False, pooling="mean", f16=False, eps_f64=False, drop=None):
    """Ref(logits, r [N][D], pooled [G][D], h_5 [N][D], scale, operands) in float64, flowgnn.h's definition line by line:
        x_0 = h_0 (+ E);  h_{l+1} = y_l (+ x_l);  x_{l+1} = h_{l+1} (+ vn_{l+1}[g]);  vn_{l+1} = (vn_l +) relu(w2 relu(w1 t + b1) + b2)
        r = h_5, or ((((x_0 + x_1) + x_2) + x_3) + x_4) + h_5
    f16: a, the ReLU'd hidden units (in the scaled domain) and both matrices of the NODE MLP rounded to f16, to nearest even, as
    tests/gin_wide_f16_ref.forward does; the residual, the JK sum and the virtual node's update stay unrounded.
    eps: s_l = (float)(1.0f + eps[l]) as the engine forms it; eps_f64: 1 + eps[l] in float64, as OGB's own forward has it.
    drop: None, or (term, mask [N][D] of bool) -- a WRONG form for tests/test_wide_shapes_cpu.py: where mask is set, every layer leaves
    out the residual's x_l (term "residual") or the JK store, so that r stays the layer's input sum there (term "jk": r = h_5)."""
    assert jk in JKS, jk
    assert drop is None or (drop[0] == "residual" and residual) or (drop[0] == "jk" and jk == "sum"), drop
    keep_res = 1.0 - drop[1] if drop is not None and drop[0] == "residual" else 1.0
    keep_jk = 1.0 - drop[1] if drop is not None and drop[0] == "jk" else 1.0
    c = lambda a: np.asarray(a, dtype=np.float64)
    rnd = f16_ref.rounder("rne") if f16 else (lambda a: a)
    nemb, eemb = c(w["node_embedding_weight"]), c(w["edge_embedding_weight"])
    w1, b1, w2, b2 = c(w["node_mlp_1_weights"]), c(w["node_mlp_1_bias"]), c(w["node_mlp_2_weights"]), c(w["node_mlp_2_bias"])
    D = nemb.shape[-1]
    pw, pb = c(w["graph_pred_weights"]).reshape(-1, D), c(w["graph_pred_bias"]).reshape(-1)
    s = np.ones(L) if eps is None else (1.0 + np.asarray(eps, np.float64) if eps_f64 else c(self_scale(eps)))
    N, G = batch.total_nodes, batch.num_graphs
    ge = batch.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    seg = lambda rows: np.add.reduceat(rows, off[:-1], axis=0)
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
        ee = eemb[l][batch.edge_attr.astype(np.int64) + ED_OFF[None, :]].sum(axis=1)
        m = np.zeros((N, D))
        np.add.at(m, v, np.maximum(x[u] + ee, 0.0))
        a = m + s[l] * x
        if f16:
            s1, s2 = f16_ref.pow2_scale(w1[l]), f16_ref.pow2_scale(w2[l])
            W1, W2 = c(rnd(w1[l] * s1)) / s1, c(rnd(w2[l] * s2)) / s2
            hid = c(rnd(np.maximum(c(rnd(a)) @ W1.T + b1[l], 0.0) * s1)) / s1
        else:
            W2 = w2[l]
            hid = np.maximum(a @ w1[l].T + b1[l], 0.0)
        y = hid @ W2.T + b2[l]
        if l != L - 1:
            y = np.maximum(y, 0.0)
        h = y + keep_res * x if residual else y
        big.extend([float(np.abs(x).max()), float(np.abs(a).max()), float(hid.max()), float(np.abs(h).max())])
        ops.extend([float(np.abs(a).max()), split_ref.pow2_scale(np.asarray(w["node_mlp_1_weights"], np.float32)[l]) * float(hid.max())])
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
    return V.node_logits(w, rows)
