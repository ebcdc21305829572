"""OGB's GNN(num_layer=L) at width 300 (flowgnn.h: flowgnn_set_num_layers): the expected values of
tests/test_num_layers_cpu.py and tests/test_num_layers_gpu.py.

The executable torch models the suite already has -- tests/ogb_torch.GNN, tests/ogb_jk_torch.GNN and tests/ogb_gcn_jk_torch.GNN -- all take
num_layer; their make_model helpers do not.  make_model here is tests/ogb_torch._make_model's recipe, step for step (the seed, one SGD
step, the seeded perturbations, 40 settling passes), with num_layer=L, on T.batch_of(kind).  float64, CPU; nothing here knows what a
GPU returns.

  DEPTHS    2 (the minimum, even, a single virtual-node update), 3 (odd, below 5), 6 (past the old array size), 8 (the cap)
  out_of_range_model   the virtual-node model pushed past the fast path's range, for the exact re-run's test
  DEFECTS   named wrong forms of the depth itself, as copies of a model: one layer fewer, ReLU kept on the last layer, eps of layer l - 1
            used in layer l; for the virtual node, tests/ogb_torch.VARIANTS
"""
import contextlib
import copy
import functools

import torch
import torch.nn.functional as F

from tests import ogb_gcn_jk_torch as GJ, ogb_jk_torch as J, ogb_torch as T

WIDE = 300
DEPTHS = (2, 3, 6, 8)
KINDS = [("gin", False), ("gin", True), ("gcn", False), ("gcn", True)]
DEFECTS = ("one_layer_fewer", "relu_on_last_layer", "eps_of_previous_layer")
name_of = lambda kind, vn, L: f"{kind}{'-virtual' if vn else ''}-L{L}"


@contextlib.contextmanager
def one_thread():
    """torch on one thread, and the setting put back: for the CPU work of these models inside a parallel test run."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


def make_model(kind, virtual_node, num_layer, jk="last", residual=False, damped=True):
    """A trained-looking GNN(num_layer=num_layer, emb_dim=300) in eval(); shared between callers, who must not change it."""
    return _make_model(kind, bool(virtual_node), int(num_layer), jk, bool(residual), bool(damped))


@functools.lru_cache(maxsize=None)
def _make_model(kind, virtual_node, num_layer, jk, residual, damped):
    # One thread for the recipe: its products are 300 wide on some 800 rows, and under a parallel test run a pool of threads per worker
    # costs far more than it saves (3 to 9 s per model on one thread, by the depth).
    with one_thread():
        return _recipe(kind, virtual_node, num_layer, jk, residual, damped)


def _recipe(kind, virtual_node, num_layer, jk, residual, damped):
    seed, num_tasks = 0, 1
    torch.manual_seed(seed)
    if jk == "last" and not residual:
        model = T.GNN(num_tasks=num_tasks, num_layer=num_layer, emb_dim=WIDE, gnn_type=kind, virtual_node=virtual_node)
    else:
        cls = J.GNN if kind == "gin" else GJ.GNN
        model = cls(num_tasks=num_tasks, num_layer=num_layer, emb_dim=WIDE, virtual_node=virtual_node, JK=jk, residual=residual)
    model = model.double()
    args = T.tensors(T.batch_of(kind))
    gen = torch.Generator().manual_seed(1000 + seed)
    labels = torch.randint(0, 2, (T.batch_of(kind).num_graphs, num_tasks), generator=gen).double()
    opt = torch.optim.SGD(model.parameters(), lr=T.SGD_LR)
    model.train()
    for _ in range(T.SGD_STEPS):
        opt.zero_grad()
        F.binary_cross_entropy_with_logits(model(*args), labels).backward()
        opt.step()
    with torch.no_grad():
        for conv in model.gnn_node.convs:
            if kind == "gin":
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


def expected(kind, virtual_node, num_layer, jk="last", residual=False, damped=True):
    """T.run(make_model(...), T.batch_of(kind)), computed once and shared: (Out(logits, rows, pooled), scale, tensors)."""
    return _expected(kind, bool(virtual_node), int(num_layer), jk, bool(residual), bool(damped))


@functools.lru_cache(maxsize=None)
def _expected(kind, virtual_node, num_layer, jk, residual, damped):
    with one_thread():
        return T.run(make_model(kind, virtual_node, num_layer, jk, residual, damped), T.batch_of(kind))


def untrained_state_dict(kind, virtual_node, num_layer, emb_dim=WIDE):
    """GNN(num_layer=num_layer).state_dict() as OGB initialises it, eps drawn away from zero: the keys and shapes of a checkpoint, for
    what needs no trained-looking values (the exporter's depth, the files' sizes)."""
    torch.manual_seed(num_layer)
    model = T.GNN(num_layer=num_layer, emb_dim=emb_dim, gnn_type=kind, virtual_node=virtual_node).double().eval()
    if kind == "gin":
        with torch.no_grad():
            for l, conv in enumerate(model.gnn_node.convs):
                conv.eps.fill_(0.05 * (l + 1))
    return model.state_dict()


# ---------------------------------------------------------------- out of the fast path's range
def out_of_range_model(kind, num_layer):
    """The damped virtual-node model with update 0 pushed past the split-f16 kernels' range (6e4), the way the width's own fallback
    tests push their NumPy weights.  Shared; callers must not change it.
      gin  tests/test_gin_wide_vn_gpu.py: one hidden unit of update 0 (the largest) gets its bias raised by 7.5e4 -- its BatchNorm's
           bias, which the exporter folds into b1 and nowhere else, so w1 and with it the power-of-two scale of the packed matrix stay
           where they were -- and its outgoing weights zeroed, so vn_1 is the original's without that one of 600 units and the node
           MLPs' operands stay as small as they were: the update kernel alone raises the flag
      gcn  tests/gcn_wide_vn_ref.range_virtual_node: component 17 of update 0's last bias (its second BatchNorm's: folded into b2) set
           to 7e4, so vn_1 has that component in every graph and xin_1 = a_1 + vn_1 leaves the range in the layer kernel's registers"""
    return _out_of_range_model(kind, int(num_layer))


@functools.lru_cache(maxsize=None)
def _out_of_range_model(kind, num_layer):
    m = copy.deepcopy(make_model(kind, True, num_layer))
    mlp = m.gnn_node.mlp_virtualnode_list[0]
    with torch.no_grad(), one_thread():
        if kind == "gin":
            seen = []
            h = mlp[1].register_forward_hook(lambda _m, _i, out: seen.append(out.max(0).values))
            m(*T.tensors(T.batch_of(kind)))
            h.remove()
            j = int(seen[0].argmax())
            mlp[1].bias[j] += 7.5e4
            mlp[3].weight[:, j] = 0.0
        else:
            mlp[4].bias[17] = 7.0e4
    return m


@functools.lru_cache(maxsize=None)
def out_of_range_expected(kind, num_layer):
    """T.run(out_of_range_model(...), T.batch_of(kind)): (Out, scale, tensors)."""
    with one_thread():
        return T.run(out_of_range_model(kind, num_layer), T.batch_of(kind))


# ---------------------------------------------------------------- the named defects
class _ReluLast(torch.nn.Module):
    """BatchNorm followed by a ReLU: in the place of the last layer's BatchNorm it keeps the ReLU on the last layer"""

    def __init__(self, bn):
        super().__init__()
        self.bn = bn

    def forward(self, x):
        return F.relu(self.bn(x))


def defects_of(kind):
    return [d for d in DEFECTS if kind == "gin" or d != "eps_of_previous_layer"]


def with_defect(model, defect):
    """A copy of a JK="last" model that computes the wrong form `defect` (DEFECTS) or, for a virtual-node model, one of T.VARIANTS."""
    if defect in T.VARIANTS:
        return T.with_variant(model, defect)
    m = copy.deepcopy(model)
    node = m.gnn_node
    if defect == "one_layer_fewer":  # (what a loop bound of L - 1 computes: the last conv never runs, the one before it loses its ReLU)
        node.num_layer -= 1
    elif defect == "relu_on_last_layer":
        node.batch_norms[node.num_layer - 1] = _ReluLast(node.batch_norms[node.num_layer - 1])
    elif defect == "eps_of_previous_layer":  # (an eps array indexed one off: layer l scales its self term by eps[l - 1], layer 0 by 0)
        eps = [c.eps.clone() for c in node.convs]
        with torch.no_grad():
            for l, c in enumerate(node.convs):
                c.eps.copy_(eps[l - 1] if l else torch.zeros(1, dtype=eps[0].dtype))
    else:
        raise ValueError(defect)
    return m
