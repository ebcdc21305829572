"""OGB's graph_pooling="attention" readout (flowgnn.h: flowgnn_set_attention_pooling), the reference side of
tests/test_attn_pool_cpu.py and tests/test_attn_pool_gpu.py.  No GPU, and nothing here knows what a GPU returns.

  readout      the definition on given rows: s[v] = w2 . relu(W1 r[v] + b1), a softmax over each graph's nodes, pooled[g] = sum alpha r,
               the model's linear head -- in float64, or with `dense` a tests/split_ref.py-style product for W1 r, or all in fp32 with the
               sums taken serially in node order.  Each wrong form of it is a keyword (WRONG).
  table        the separation of tests/split_ref.py for this readout alone: E_ok / E_bad / B = sqrt(E_ok E_bad) of `pooled` and `logits`
               on given rows.
  AttentionGNN a torch.nn model: tests/ogb_torch.GNN with OGB's GlobalAttention as its `pool`, so that state_dict() has OGB's
               `pool.gate_nn.*` keys and embed() applies the softmax readout.
"""
import copy
from collections import namedtuple

import numpy as np

from tests import split_ref

# the wrong forms, each a keyword of `readout`
WRONG = ("uniform", "whole_batch", "unnormalised", "negated", "no_relu", "no_b1", "relu_rows", "hard_argmax")
WRONG_NAMES = {"uniform": "uniform alpha (the mean)", "whole_batch": "softmax over the whole batch", "unnormalised": "alpha not normalised",
               "negated": "-s", "no_relu": "no ReLU", "no_b1": "b1 omitted", "relu_rows": "rows ReLU'd first", "hard_argmax": "hard arg-max"}


def _offsets(batch):
    return np.asarray(batch.node_offsets(), np.int64)


def _serial_segment_sum(x, off, dtype):
    """Per graph, the rows of x added one after the other in node order, in `dtype` (np.add.reduceat sums pairwise)."""
    G = len(off) - 1
    acc = np.zeros((G,) + x.shape[1:], dtype)
    n = off[1:] - off[:-1]
    for k in range(int(n.max()) if G else 0):
        live = np.nonzero(n > k)[0]
        acc[live] = (acc[live] + x[off[live] + k]).astype(dtype)
    return acc


def readout(rows, batch, gate, pw, pb, dense=None, dtype=np.float64, stats=None, uniform=False, whole_batch=False, unnormalised=False,
            negated=False, no_relu=False, no_b1=False, relu_rows=False, hard_argmax=False):
    """(pooled [G][D], logits [G] or [G][T], s [N]) by the definition.  gate: {"w1" [H][D], "b1" [H], "w2" [H]}; pw [T][D], pb [T].
    dense: (a [N][K], W [O][K]) -> [N][O] for the first product (None: the matmul in `dtype`).  dtype float32: every operation in fp32,
    the two per-graph sums serial in node order.  stats: a dict that receives hidden_max (the largest hidden value of the gate) and
    s_max (max |s|), what a test extends its activation scale by."""
    c = lambda a: np.asarray(a, dtype=dtype)
    r = c(rows)
    if relu_rows:
        r = np.maximum(r, 0)
    w1, b1, w2 = c(gate["w1"]), c(gate["b1"]), c(gate["w2"]).reshape(-1)
    D = r.shape[1]
    assert w1.shape == (2 * D, D) and b1.shape == (2 * D,) and w2.shape == (2 * D,), (w1.shape, b1.shape, w2.shape)
    off = _offsets(batch)
    assert off[-1] == r.shape[0], (off[-1], r.shape)
    G = len(off) - 1
    seg = np.repeat(np.arange(G), off[1:] - off[:-1])
    z = (r @ w1.T if dense is None else np.asarray(dense(r, w1), dtype=dtype))
    if not no_b1:
        z = z + b1
    hid = z if no_relu else np.maximum(z, 0)
    s = c(hid @ w2)
    if stats is not None:
        stats["hidden_max"] = float(np.abs(hid).max())
        stats["s_max"] = float(np.abs(s).max())
    t = -s if negated else s
    if uniform:
        e = np.ones_like(t)
    elif hard_argmax:
        first = np.full(G, -1, np.int64)
        m = np.maximum.reduceat(t, off[:-1])
        for v in np.nonzero(t == m[seg])[0][::-1]:
            first[seg[v]] = v
        e = np.zeros_like(t)
        e[first] = 1
    else:
        m = np.full(G, t.max(), dtype) if whole_batch else np.maximum.reduceat(t, off[:-1])
        e = c(np.exp(t - m[seg]))
    if dtype is np.float32:
        Z = _serial_segment_sum(e, off, dtype)
        num = _serial_segment_sum((e[:, None] * r).astype(dtype), off, dtype)
    else:
        Z = np.add.reduceat(e, off[:-1])
        num = np.add.reduceat(e[:, None] * r, off[:-1], axis=0)
    if whole_batch:
        Z = np.full(G, e.sum(), dtype)
    pooled = num if unnormalised else num / Z[:, None]
    pw2 = c(pw).reshape(-1, D)
    out = c(pooled @ pw2.T + c(pb).reshape(-1))
    return c(pooled), (out[:, 0] if out.shape[1] == 1 else out), s


# ---------------------------------------------------------------- split-f16 separation of the readout alone
Row = namedtuple("Row", "e_ok e_bad bound ok bad unit")
OUTPUTS = ("pooled", "logits")


def variants():
    """split_ref.VARIANTS as they apply to the gate's one product: everywhere, in one K-step, in one 16-column tile; K = 300 is padded
    with zero weights to whole K-steps, so there is no fp32 K tail to get wrong, and the readout has no "last layer"."""
    return [s for s in split_ref.VARIANTS if s.where in ("all", "kstep", "tile") and s.tail != "single"]


def table(rows, batch, gate, pw, pb):
    """output name -> Row(E_ok, E_bad, B, per-restatement errors, per-variant errors, unit), from the readout alone on the given rows
    (which are taken as exact: float32 values in float64).  err = max |x - f64| / unit; unit = max(max |rows|, max |s|) for `pooled`,
    max(1, max |logits|) for `logits`.  The correct forms: everything in fp32, the serial fp32 sums included, and split_ref.OK_SPECS
    through split_ref.SplitDense("GIN", spec).  The wrong forms: `variants`."""
    rows = np.asarray(rows, np.float32)
    ref = dict(zip(("pooled", "logits", "s"), readout(rows, batch, gate, pw, pb)))
    unit = {"pooled": max(float(np.abs(rows).max()), float(np.abs(ref["s"]).max())), "logits": max(1.0, float(np.abs(ref["logits"]).max()))}
    ok = {"all fp32": readout(rows, batch, gate, pw, pb, dense=split_ref.dense_fp32, dtype=np.float32)}
    for spec in split_ref.OK_SPECS:
        ok[spec.name] = readout(rows, batch, gate, pw, pb, dense=split_ref.SplitDense("GIN", spec))
    bad = {spec.name: readout(rows, batch, gate, pw, pb, dense=split_ref.SplitDense("GIN", spec)) for spec in variants()}
    out = {}
    for i, name in enumerate(OUTPUTS):
        err = lambda got: float(np.abs(np.asarray(got[i], np.float64) - ref[name]).max()) / unit[name]
        eo = {k: err(v) for k, v in ok.items()}
        eb = {k: err(v) for k, v in bad.items()}
        e_ok, e_bad = max(eo.values()), min(eb.values())
        out[name] = Row(e_ok, e_bad, float(np.sqrt(e_ok * e_bad)), eo, eb, unit[name])
    return out


def err(got, want, unit):
    return float(np.abs(np.asarray(got, np.float64).reshape(np.shape(want)) - want).max()) / unit


# ---------------------------------------------------------------- the torch.nn model
def attention_model(kind, virtual_node, emb_dim=300, num_tasks=1, seed=0):
    """tests/ogb_torch.make_model(kind, virtual_node, emb_dim, num_tasks) -- the trained-looking model of the other tests -- under
    OGB's attention readout: an AttentionGNN with those parameters and a seeded gate whose BatchNorm has non-trivial running statistics
    and affine parameters.  eval(), float64."""
    import torch
    from tests import ogb_torch as T

    class GlobalAttention(torch.nn.Module):
        """torch_geometric.nn.GlobalAttention(gate_nn) as OGB builds it, written out: softmax of gate_nn(x) over each graph's nodes
        (PyG's softmax: exp(s - max) / (sum + 1e-16)), then the weighted sum."""

        def __init__(self, emb_dim):
            super().__init__()
            nn = torch.nn
            self.gate_nn = nn.Sequential(nn.Linear(emb_dim, 2 * emb_dim), nn.BatchNorm1d(2 * emb_dim), nn.ReLU(), nn.Linear(2 * emb_dim, 1))
            self.gates = nn.Identity()  # (no parameters: a place for run()'s hook, the gate scores)

        def forward(self, h, batch, G):
            s = self.gates(self.gate_nn(h)).view(-1)
            m = torch.full((G,), -float("inf"), dtype=s.dtype).scatter_reduce_(0, batch, s, "amax", include_self=True)
            e = torch.exp(s - m[batch])
            Z = torch.zeros(G, dtype=s.dtype).index_add_(0, batch, e) + 1e-16
            alpha = e / Z[batch]
            return T._scatter_add(alpha.view(-1, 1) * h, batch, G)

    class AttentionGNN(T.GNN):
        def __init__(self, **kw):
            super().__init__(graph_pooling="mean", **kw)
            self.graph_pooling = "attention"
            self.pool = GlobalAttention(kw["emb_dim"])
            self.pooled = torch.nn.Identity()

        def embed(self, x, edge_index, edge_attr, ptr):
            G = ptr.numel() - 1
            batch = torch.repeat_interleave(torch.arange(G), ptr[1:] - ptr[:-1])
            h = self.gnn_node(x, edge_index, edge_attr, batch)
            return h, self.pooled(self.pool(h, batch, G))

    base = T.make_model(kind, virtual_node, emb_dim, num_tasks=num_tasks)
    torch.manual_seed(7000 + seed)
    model = AttentionGNN(num_tasks=num_tasks, emb_dim=emb_dim, gnn_type=kind, virtual_node=virtual_node).double()
    missing, unexpected = model.load_state_dict(copy.deepcopy(base.state_dict()), strict=False)
    assert not unexpected and all(k.startswith("pool.gate_nn.") for k in missing), (missing, unexpected)
    gen = torch.Generator().manual_seed(7100 + seed)
    with torch.no_grad():
        lin0, bn, lin3 = model.pool.gate_nn[0], model.pool.gate_nn[1], model.pool.gate_nn[3]
        lin0.weight.copy_(torch.randn(lin0.weight.shape, generator=gen).double() / np.sqrt(emb_dim))
        lin0.bias.copy_(0.5 * torch.randn(lin0.bias.shape, generator=gen).double())
        bn.weight.copy_(1 + 0.2 * torch.randn(bn.weight.shape, generator=gen).double())
        bn.bias.copy_(0.2 * torch.randn(bn.bias.shape, generator=gen).double())
        bn.running_mean.copy_(0.3 * torch.randn(bn.running_mean.shape, generator=gen).double())
        bn.running_var.copy_(0.5 + torch.rand(bn.running_var.shape, generator=gen).double())
        lin3.weight.copy_(4.0 * torch.randn(lin3.weight.shape, generator=gen).double() / np.sqrt(2 * emb_dim))
        lin3.bias.fill_(0.37)  # (cancels in the softmax: the exporter drops it)
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model
