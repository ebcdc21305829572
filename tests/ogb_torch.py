"""An executable PyTorch model of OGB's molecule GNNs: the expected values of tests/test_ogb_torch_cpu.py and tests/test_ogb_torch_gpu.py.

A plain `torch.nn` transcription of ogb/examples/graphproppred/mol/conv.py and gnn.py (GINConv, GCNConv, GNN_node, GNN_node_Virtualnode,
GNN with JK='last', residual=False, graph_pooling mean / sum / max) and of ogb.graphproppred.mol_encoder's AtomEncoder / BondEncoder.
torch_geometric's message passing, `degree` and `global_*_pool` are written out with index_add_ / scatter_reduce_; nothing else differs,
and the module tree gives OGB's `state_dict()` keys exactly.  It runs in float64 on the CPU, and nothing here knows what a GPU returns.

  make_model   a "trained-looking" model in eval(): a fixed seed, a few SGD steps in train(), seeded perturbations, and (damped) a number
               of no_grad passes in train() that settle the BatchNorm running statistics.
  run          one forward: Out(logits, final rows, pooled vectors), the scale (the largest magnitude seen by forward hooks on every
               encoder, conv aggregate, row operand, Linear, BatchNorm1d and pool: the `scale` of tests/parity.py), and the tensors
               x, edge_index, edge_attr, ptr that the model consumed.
  gin_batch / gcn_batch   the batches of the tests.
  VARIANTS     the wrong forms of the virtual node (tests/ogb_vn_ref.VARIANTS) that a flag on GNN_node_Virtualnode expresses.
"""
import copy
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from flowgnn_amd import graphpack as gp

ATOM_DIMS = (119, 4, 12, 12, 10, 6, 6, 2, 2)  # ogb.utils.features.get_atom_feature_dims()
BOND_DIMS = (5, 6, 2)                          # ogb.utils.features.get_bond_feature_dims()
NUM_LAYER = 5
DROP_RATIO = 0.5
VARIANTS = ("no_add_in_last_layer", "pool_before_add", "t_without_vn", "mean_instead_of_sum", "update_indexed_l_plus_1", "embedding_ignored")

Out = namedtuple("Out", "logits rows pooled")


class AtomEncoder(nn.Module):
    def __init__(self, emb_dim):
        super().__init__()
        self.atom_embedding_list = nn.ModuleList()
        for n in ATOM_DIMS:
            emb = nn.Embedding(n, emb_dim)
            nn.init.xavier_uniform_(emb.weight.data)
            self.atom_embedding_list.append(emb)

    def forward(self, x):
        out = 0
        for i in range(x.shape[1]):
            out = out + self.atom_embedding_list[i](x[:, i])
        return out


class BondEncoder(nn.Module):
    def __init__(self, emb_dim):
        super().__init__()
        self.bond_embedding_list = nn.ModuleList()
        for n in BOND_DIMS:
            emb = nn.Embedding(n, emb_dim)
            nn.init.xavier_uniform_(emb.weight.data)
            self.bond_embedding_list.append(emb)

    def forward(self, edge_attr):
        out = 0
        for i in range(edge_attr.shape[1]):
            out = out + self.bond_embedding_list[i](edge_attr[:, i])
        return out


def _scatter_add(src, index, n):
    return torch.zeros((n, src.shape[1]), dtype=src.dtype).index_add_(0, index, src)


class GINConv(nn.Module):
    def __init__(self, emb_dim):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(emb_dim, 2 * emb_dim), nn.BatchNorm1d(2 * emb_dim), nn.ReLU(), nn.Linear(2 * emb_dim, emb_dim))
        self.eps = nn.Parameter(torch.Tensor([0]))
        self.bond_encoder = BondEncoder(emb_dim)
        self.aggregate = nn.Identity()  # (no parameters: a place for run()'s hook, the MLP's operand)

    def forward(self, x, edge_index, edge_attr):
        e = self.bond_encoder(edge_attr)
        row, col = edge_index[0], edge_index[1]  # messages flow edge_index[0] -> edge_index[1]
        agg = _scatter_add(F.relu(x[row] + e), col, x.shape[0])
        return self.mlp(self.aggregate((1 + self.eps) * x + agg))


class GCNConv(nn.Module):
    def __init__(self, emb_dim):
        super().__init__()
        self.linear = nn.Linear(emb_dim, emb_dim)
        self.root_emb = nn.Embedding(1, emb_dim)
        self.bond_encoder = BondEncoder(emb_dim)
        self.aggregate = nn.Identity()

    def forward(self, x, edge_index, edge_attr):
        x = self.linear(x)
        e = self.bond_encoder(edge_attr)
        row, col = edge_index[0], edge_index[1]
        deg = torch.zeros(x.shape[0], dtype=x.dtype).index_add_(0, row, torch.ones(row.shape[0], dtype=x.dtype)) + 1  # degree(row) + 1
        deg_inv_sqrt = deg.pow(-0.5)
        deg_inv_sqrt[deg_inv_sqrt == float("inf")] = 0
        norm = deg_inv_sqrt[row] * deg_inv_sqrt[col]
        agg = _scatter_add(norm.view(-1, 1) * F.relu(x[row] + e), col, x.shape[0])
        return self.aggregate(agg + F.relu(x + self.root_emb.weight) * 1.0 / deg.view(-1, 1))


def _conv(gnn_type, emb_dim):
    if gnn_type == "gin":
        return GINConv(emb_dim)
    if gnn_type == "gcn":
        return GCNConv(emb_dim)
    raise ValueError(f"Undefined GNN type called {gnn_type}")


class GNN_node(nn.Module):
    def __init__(self, num_layer, emb_dim, drop_ratio=DROP_RATIO, gnn_type="gin"):
        super().__init__()
        self.num_layer, self.drop_ratio = num_layer, drop_ratio
        self.atom_encoder = AtomEncoder(emb_dim)
        self.convs = nn.ModuleList(_conv(gnn_type, emb_dim) for _ in range(num_layer))
        self.batch_norms = nn.ModuleList(nn.BatchNorm1d(emb_dim) for _ in range(num_layer))

    def forward(self, x, edge_index, edge_attr, batch):
        h = self.atom_encoder(x)
        for layer in range(self.num_layer):
            h = self.batch_norms[layer](self.convs[layer](h, edge_index, edge_attr))
            if layer != self.num_layer - 1:
                h = F.relu(h)
            h = F.dropout(h, self.drop_ratio, training=self.training)
        return h  # JK 'last'


class GNN_node_Virtualnode(nn.Module):
    def __init__(self, num_layer, emb_dim, drop_ratio=DROP_RATIO, gnn_type="gin"):
        super().__init__()
        self.num_layer, self.drop_ratio = num_layer, drop_ratio
        self.atom_encoder = AtomEncoder(emb_dim)
        self.virtualnode_embedding = nn.Embedding(1, emb_dim)
        nn.init.constant_(self.virtualnode_embedding.weight.data, 0)
        self.convs = nn.ModuleList(_conv(gnn_type, emb_dim) for _ in range(num_layer))
        self.batch_norms = nn.ModuleList(nn.BatchNorm1d(emb_dim) for _ in range(num_layer))
        self.mlp_virtualnode_list = nn.ModuleList(
            nn.Sequential(nn.Linear(emb_dim, 2 * emb_dim), nn.BatchNorm1d(2 * emb_dim), nn.ReLU(),
                          nn.Linear(2 * emb_dim, emb_dim), nn.BatchNorm1d(emb_dim), nn.ReLU()) for _ in range(num_layer - 1))
        self.rows = nn.Identity()  # (no parameters: places for run()'s hooks, h_l + vn[batch] and the pooled t)
        self.pool = nn.Identity()
        self.variant = None  # one of VARIANTS: a wrong form, for the mutation test only

    def forward(self, x, edge_index, edge_attr, batch):
        v, last = self.variant, self.num_layer - 1
        G = int(batch[-1].item()) + 1
        vn = self.virtualnode_embedding(torch.zeros(G, dtype=torch.long))
        if v == "embedding_ignored":
            vn = torch.zeros_like(vn)
        h = self.atom_encoder(x)
        for layer in range(self.num_layer):
            h_in = h
            if not (v == "no_add_in_last_layer" and layer == last):
                h = h + vn[batch]
            h = self.rows(h)
            out = self.batch_norms[layer](self.convs[layer](h, edge_index, edge_attr))
            if layer != last:
                out = F.relu(out)
            out = F.dropout(out, self.drop_ratio, training=self.training)
            if layer < last:
                t = _scatter_add(h_in if v == "pool_before_add" else h, batch, G)  # global_add_pool(h_list[layer], batch)
                if v == "mean_instead_of_sum":
                    t = t / torch.bincount(batch, minlength=G).to(t.dtype).view(-1, 1)
                if v != "t_without_vn":
                    t = t + vn
                k = (layer + 1) % last if v == "update_indexed_l_plus_1" else layer
                vn = F.dropout(self.mlp_virtualnode_list[k](self.pool(t)), self.drop_ratio, training=self.training)
            h = out
        return h


class GNN(nn.Module):
    def __init__(self, num_tasks=1, num_layer=NUM_LAYER, emb_dim=300, gnn_type="gin", virtual_node=True, drop_ratio=DROP_RATIO,
                 graph_pooling="mean"):
        super().__init__()
        if graph_pooling not in ("mean", "sum", "max"):
            raise ValueError("Invalid graph pooling type.")
        node = GNN_node_Virtualnode if virtual_node else GNN_node
        self.gnn_node = node(num_layer, emb_dim, drop_ratio=drop_ratio, gnn_type=gnn_type)
        self.graph_pooling = graph_pooling
        self.graph_pred_linear = nn.Linear(emb_dim, num_tasks)
        self.pool = nn.Identity()

    def embed(self, x, edge_index, edge_attr, ptr):
        G = ptr.numel() - 1
        batch = torch.repeat_interleave(torch.arange(G), ptr[1:] - ptr[:-1])
        h = self.gnn_node(x, edge_index, edge_attr, batch)
        if self.graph_pooling == "max":
            idx = batch.view(-1, 1).expand(-1, h.shape[1])
            pooled = torch.zeros((G, h.shape[1]), dtype=h.dtype).scatter_reduce_(0, idx, h, "amax", include_self=False)
        else:
            pooled = _scatter_add(h, batch, G)
            if self.graph_pooling == "mean":
                pooled = pooled / (ptr[1:] - ptr[:-1]).to(h.dtype).view(-1, 1)
        return h, self.pool(pooled)

    def forward(self, x, edge_index, edge_attr, ptr):
        return self.graph_pred_linear(self.embed(x, edge_index, edge_attr, ptr)[1])


# ---------------------------------------------------------------- batches
def tensors(batch):
    """x int64 [N][9], edge_index int64 [2][E] with batch-global ids, edge_attr int64 [E][3], ptr int64 [G + 1]: a PyG Batch's fields."""
    d = batch.to_pyg("cpu")
    return d["x"], d["edge_index"], d["edge_attr"], d["ptr"]


def _graph(n, edges, seed):
    """One graph of n nodes with the directed edges [(src, dst)], seeded atom and bond features."""
    rng = np.random.default_rng(seed)
    nf = np.stack([rng.integers(0, c, n) for c in ATOM_DIMS], 1).astype(np.int32)
    el = np.asarray(edges, np.int32).reshape(-1, 2)
    ea = np.stack([rng.integers(0, c, len(el)) for c in BOND_DIMS], 1).astype(np.int32).reshape(-1, 3)
    return gp.GraphBatch(np.array([n], np.int32), np.array([len(el)], np.int32), nf, el, ea)


def _both(pairs):
    return list(pairs) + [(b, a) for a, b in pairs]


@functools.lru_cache(maxsize=None)
def gcn_batch():
    """24 molhiv-shaped graphs, a one-node graph, three nodes without an edge, a 17-node ring (one past a wave's 16-row tile), a 129-node
    path (one past the wide kernels' 128-row workgroup tile), and nine nodes with self loops and duplicated edges.  Both directions of
    every edge are listed (a self loop is its own reverse): tests/test_ogb_torch_cpu.py says why GCN needs that."""
    ring = [(i, (i + 1) % 17) for i in range(17)]
    path = [(i, i + 1) for i in range(128)]
    messy = _both([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 0), (0, 1), (2, 3), (2, 3)]) + [(4, 4), (7, 7), (7, 7)]
    return gp.concat_batches([gp.synth_molhiv_batch(24, seed=31), _graph(1, [], 1), _graph(3, [], 2), _graph(17, _both(ring), 3),
                              _graph(129, _both(path), 4), _graph(9, messy, 5)])


@functools.lru_cache(maxsize=None)
def gin_batch():
    """gcn_batch and a six-node graph whose edges are listed in one direction only (GIN sums what arrives, whatever leaves)."""
    return gp.concat_batches([gcn_batch(), _graph(6, [(0, 1), (1, 2), (2, 3), (3, 1), (4, 1), (0, 5)], 6)])


def batch_of(kind):
    return gin_batch() if kind == "gin" else gcn_batch()


# ---------------------------------------------------------------- the model of the tests
SGD_STEPS, SGD_LR = 1, 0.01
SETTLE_PASSES = 40  # momentum 0.1: 0.9^40 = 1.5 % of the initial (0, 1) statistics are left
VN_EMBEDDING_STD = 2.0


def _bn_modules(model):
    return [m for m in model.modules() if isinstance(m, nn.BatchNorm1d)]


def make_model(kind, virtual_node, emb_dim, num_tasks=1, pooling="mean", seed=0, damped=True, zero_eps=False):
    """A trained-looking OGB model in eval(), float64; shared between callers, who must not change it (copy.deepcopy first).  The recipe:
      1. torch.manual_seed(seed); OGB's own initialisation (xavier tables, torch's Linear default, a zero virtual-node embedding).
      2. SGD_STEPS steps of plain SGD (lr SGD_LR) in train(), dropout on, on the model's own test batch (batch_of(kind): the running
         statistics then know a 129-node graph, as those of a model trained on a dataset with large molecules do) with seeded 0/1
         labels and OGB's BCEWithLogitsLoss: every parameter has moved, num_batches_tracked counts.
      3. Seeded perturbations of what a small step leaves almost untouched: every eps gets a value of magnitude 0.05 .. 0.3, every
         BatchNorm's weight a factor 1 + 0.2 N(0, 1) and its bias 0.2 N(0, 1), the virtual-node embedding VN_EMBEDDING_STD N(0, 1) per
         component (zero_eps: eps = 0 instead, the one model the reference's GIN file set can hold without an eps file).
      4. damped: SETTLE_PASSES no_grad passes in train() over the same graphs, which bring the BatchNorm running statistics to those of
         the model's own activations, as training for epochs does.  Without them (damped=False) the one step leaves 90 % of the
         initial (0, 1) in every running mean and variance, eval() normalises sums over a graph's nodes by far too small a variance,
         and the virtual node's vector grows from update to update: the model of the fallback tests, whose pooled t passes the
         split-f16 kernels' threshold.  (SGD_STEPS is 1 for that reason: after three steps 73 % is left, and the undamped models' scales
         are 2.3e4 .. 6.5e4 -- neither inside half the threshold nor safely past it; after one step they are 1.3e5 .. 2.7e5.)"""
    return _make_model(kind, bool(virtual_node), int(emb_dim), int(num_tasks), pooling, int(seed), bool(damped), bool(zero_eps))


@functools.lru_cache(maxsize=None)
def _make_model(kind, virtual_node, emb_dim, num_tasks, pooling, seed, damped, zero_eps):
    if pooling != "mean":  # (the same trained-looking parameters under another readout: the node rows are those of the mean model)
        model = copy.deepcopy(_make_model(kind, virtual_node, emb_dim, num_tasks, "mean", seed, damped, zero_eps))
        model.graph_pooling = pooling
        return model
    torch.manual_seed(seed)
    model = GNN(num_tasks=num_tasks, emb_dim=emb_dim, gnn_type=kind, virtual_node=virtual_node, graph_pooling=pooling).double()
    args = tensors(batch_of(kind))
    gen = torch.Generator().manual_seed(1000 + seed)
    labels = torch.randint(0, 2, (batch_of(kind).num_graphs, num_tasks), generator=gen).double()
    opt = torch.optim.SGD(model.parameters(), lr=SGD_LR)
    model.train()
    for _ in range(SGD_STEPS):
        opt.zero_grad()
        F.binary_cross_entropy_with_logits(model(*args), labels).backward()
        opt.step()
    with torch.no_grad():
        for conv in model.gnn_node.convs:
            if kind == "gin":
                mag = 0.05 + 0.25 * torch.rand(1, generator=gen).double()
                sign = 1.0 if torch.rand(1, generator=gen).item() < 0.5 else -1.0
                conv.eps.copy_(torch.zeros(1) if zero_eps else sign * mag)
        for bn in _bn_modules(model):
            bn.weight.mul_(1 + 0.2 * torch.randn(bn.weight.shape, generator=gen).double())
            bn.bias.add_(0.2 * torch.randn(bn.bias.shape, generator=gen).double())
        if virtual_node:
            w = model.gnn_node.virtualnode_embedding.weight
            w.add_(VN_EMBEDDING_STD * torch.randn(w.shape, generator=gen).double())
        if damped:
            for _ in range(SETTLE_PASSES):
                model(*args)
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def with_variant(model, variant):
    """A copy of a virtual-node model that computes the wrong form `variant`."""
    m = copy.deepcopy(model)
    assert variant in VARIANTS and isinstance(m.gnn_node, GNN_node_Virtualnode), variant
    m.gnn_node.variant = variant
    return m


HOOKED = (AtomEncoder, BondEncoder, nn.Identity, nn.Linear, nn.BatchNorm1d)


def run(model, batch):
    """(Out(logits [G] or [G][T], final rows [N][D], pooled vectors [G][D]) as float64 arrays, scale, (x, edge_index, edge_attr, ptr)).
    The rows are in the order of the batch's nodes.  scale = max(1, the largest magnitude any hooked module returned): the encoders'
    rows, h_l + vn[batch], each conv's aggregate, every Linear's and every BatchNorm1d's output (hidden units, rows, logits), the
    pooled t and the readout's pooled vectors."""
    assert not model.training
    args = tensors(batch)
    seen = [1.0]
    hook = lambda _m, _i, out: seen.append(float(out.abs().max())) if out.numel() else None
    handles = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, HOOKED)]
    try:
        with torch.no_grad():
            rows, pooled = model.embed(*args)
            logits = model.graph_pred_linear(pooled)
    finally:
        for h in handles:
            h.remove()
    logits = logits.numpy()
    return Out(logits[:, 0] if logits.shape[1] == 1 else logits, rows.numpy(), pooled.numpy()), max(seen), args


def expected(kind, virtual_node, emb_dim, num_tasks=1, pooling="mean", damped=True):
    """run(make_model(...), batch_of(kind)), computed once and shared: (Out, scale, tensors)."""
    return _expected(kind, bool(virtual_node), int(emb_dim), int(num_tasks), pooling, bool(damped))


@functools.lru_cache(maxsize=None)
def _expected(kind, virtual_node, emb_dim, num_tasks, pooling, damped):
    return run(make_model(kind, virtual_node, emb_dim, num_tasks=num_tasks, pooling=pooling, damped=damped), batch_of(kind))


def numpy_state_dict(model):
    """model.state_dict() as float64 / int64 arrays under the same keys: what the NumPy restatements index."""
    return {k: v.numpy() for k, v in model.state_dict().items()}
