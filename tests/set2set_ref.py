"""OGB's graph_pooling="set2set" readout (flowgnn.h: flowgnn_set_set2set_pooling), the reference side of
tests/test_set2set_cpu.py and tests/test_set2set_gpu.py.  No GPU, and nothing here knows what a GPU returns.

  readout        the definition on given rows, in float64 or all in float32 (the per-graph sums serial in node order): per step the LSTM
                 cell on q*, e[v] = r[v] . h_t[g(v)], a softmax over each graph's nodes, r_t = sum a r, q* = [h_t, r_t]; then the
                 Linear(2D, T) head.  Each wrong form of it is a name in WRONG.
  set2set_model  a torch.nn model: tests/ogb_torch.GNN with PyG's Set2Set written out as its `pool` -- a real torch.nn.LSTM(2D, D) driven
                 exactly as torch_geometric.nn.Set2Set.forward drives it -- and a Linear(2D, T) head, so that state_dict() has OGB's
                 `pool.lstm.*` and `graph_pred_linear.*` keys.
"""
import copy

import numpy as np

# the wrong forms, each a value of readout's `wrong`
WRONG = ("gates_ifog", "gates_igfo", "no_b_hh", "no_w_hh", "c_not_carried", "uniform", "whole_batch", "q_r_h", "one_step_fewer")
WRONG_NAMES = {"gates_ifog": "gate order i, f, o, g", "gates_igfo": "gate order i, g, f, o", "no_b_hh": "b_hh omitted", "no_w_hh": "W_hh h omitted",
               "c_not_carried": "c not carried", "uniform": "uniform a", "whole_batch": "softmax over the whole batch", "q_r_h": "q* = [r, h]",
               "one_step_fewer": "one step fewer"}
_GATES = {None: (0, 1, 2, 3), "gates_ifog": (0, 1, 3, 2), "gates_igfo": (0, 2, 1, 3)}  # where i, f, g, o are taken from in the 4D axis


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return (1 / (1 + np.exp(-x))).astype(x.dtype)


def _tanh(x):
    return np.tanh(x).astype(x.dtype)


def readout(rows, batch, s2s, steps=2, dtype=np.float64, wrong=None, stats=None):
    """(q* [G][2D], logits [G] or [G][T], e [N] of the last step) by the definition.  s2s: the six tensors of weights.SET2SET_KEYS.
    dtype float32: every operation in fp32; the per-graph sums are serial in node order in either dtype (np.add.at).  wrong: None or
    one of WRONG.  stats: a dict that receives q_max (max |q*| over all steps) and e_max (max |e| over all steps)."""
    assert wrong is None or wrong in WRONG, wrong
    c = lambda a: np.asarray(a, dtype=dtype)
    r = c(rows)
    D = r.shape[1]
    w_ih, w_hh, b_ih, b_hh = c(s2s["w_ih"]), c(s2s["w_hh"]), c(s2s["b_ih"]), c(s2s["b_hh"])
    head_w, head_b = c(s2s["head_w"]).reshape(-1, 2 * D), c(s2s["head_b"]).reshape(-1)
    assert w_ih.shape == (4 * D, 2 * D) and w_hh.shape == (4 * D, D) and b_ih.shape == b_hh.shape == (4 * D,), (w_ih.shape, w_hh.shape)
    off = np.asarray(batch.node_offsets(), np.int64)
    assert off[-1] == r.shape[0], (off[-1], r.shape)
    G = len(off) - 1
    seg = np.repeat(np.arange(G), off[1:] - off[:-1])
    gi, gf, gg, go = _GATES.get(wrong, _GATES[None])
    h, cc, q = np.zeros((G, D), dtype), np.zeros((G, D), dtype), np.zeros((G, 2 * D), dtype)
    e = np.zeros(r.shape[0], dtype)
    q_max = e_max = 0.0
    for _ in range(steps - 1 if wrong == "one_step_fewer" else steps):
        z = c(q @ w_ih.T) + b_ih
        if wrong != "no_w_hh":
            z = z + c(h @ w_hh.T)
        if wrong != "no_b_hh":
            z = z + b_hh
        z = c(z).reshape(G, 4, D)
        c_prev = np.zeros_like(cc) if wrong == "c_not_carried" else cc
        cc = c(_sigmoid(z[:, gf]) * c_prev + _sigmoid(z[:, gi]) * _tanh(z[:, gg]))
        h = c(_sigmoid(z[:, go]) * _tanh(cc))
        e = c((r * h[seg]).sum(axis=1))
        if wrong == "uniform":
            a = np.ones_like(e)
        else:
            m = np.full(G, -np.inf, dtype)
            np.maximum.at(m, seg, e)
            if wrong == "whole_batch" and e.size:
                m[:] = e.max()
            a = c(np.exp(e - m[seg]))
        Z, num = np.zeros(G, dtype), np.zeros((G, D), dtype)
        np.add.at(Z, seg, a)
        np.add.at(num, seg, c(a[:, None] * r))
        if wrong == "whole_batch":
            Z[:] = a.sum()
        rt = np.zeros((G, D), dtype)  # (a graph without nodes: r_t = 0)
        live = Z > 0
        rt[live] = c(num[live] / Z[live, None])
        q = c(np.concatenate([rt, h] if wrong == "q_r_h" else [h, rt], axis=1))
        q_max, e_max = max(q_max, float(np.abs(q).max())), max(e_max, float(np.abs(e).max()) if e.size else 0.0)
    if stats is not None:
        stats["q_max"], stats["e_max"] = q_max, e_max
    out = c(q @ head_w.T + head_b)
    return q, (out[:, 0] if out.shape[1] == 1 else out), e


def folded(s2s):
    """(W [4D][2D], b [4D]): W_hh added to the first D columns of W_ih and the two biases to one, in float64 and rounded once to
    float32 -- what the engine packs (q*'s first half is h)."""
    w = np.asarray(s2s["w_ih"], np.float64).copy()
    D = w.shape[1] // 2
    w[:, :D] += np.asarray(s2s["w_hh"], np.float64)
    return w.astype(np.float32), (np.asarray(s2s["b_ih"], np.float64) + np.asarray(s2s["b_hh"], np.float64)).astype(np.float32)


# ---------------------------------------------------------------- the torch.nn model
def set2set_model(kind, virtual_node, num_tasks=1, steps=2, seed=0, emb_dim=300):
    """tests/ogb_torch.make_model(kind, virtual_node, emb_dim, num_tasks) -- the trained-looking model of the other tests -- under
    OGB's set2set readout: its `pool` is PyG's Set2Set(emb_dim, processing_steps=steps) written out around a real torch.nn.LSTM, its
    head a Linear(2 emb_dim, num_tasks); the LSTM keeps torch's initialisation (seeded) with 0.3 N(0, 1) added to both biases, so that
    the gates are not all near 1/2.  eval(), float64."""
    import torch
    from tests import ogb_torch as T

    class Set2Set(torch.nn.Module):
        """torch_geometric.nn.Set2Set.forward, written out: the LSTM is called on q* [1][G][2D] with the carried (h, c); PyG's softmax is
        exp(e - max) / (sum + 1e-16); scatter-add for r."""

        def __init__(self, in_channels, processing_steps):
            super().__init__()
            self.in_channels, self.out_channels, self.processing_steps = in_channels, 2 * in_channels, processing_steps
            self.lstm = torch.nn.LSTM(self.out_channels, in_channels, num_layers=1)
            self.dots = torch.nn.Identity()  # (no parameters: a place for run()'s hook, e)

        def forward(self, x, batch, G):
            h = (x.new_zeros((1, G, self.in_channels)), x.new_zeros((1, G, self.in_channels)))
            q_star = x.new_zeros(G, self.out_channels)
            for _ in range(self.processing_steps):
                q, h = self.lstm(q_star.unsqueeze(0), h)
                q = q.view(G, self.in_channels)
                e = self.dots((x * q[batch]).sum(dim=-1))
                m = torch.full((G,), -float("inf"), dtype=e.dtype).scatter_reduce_(0, batch, e, "amax", include_self=True)
                a = torch.exp(e - m[batch])
                a = a / (torch.zeros(G, dtype=e.dtype).index_add_(0, batch, a) + 1e-16)[batch]
                r = T._scatter_add(a.view(-1, 1) * x, batch, G)
                q_star = torch.cat([q, r], dim=-1)
            return q_star

    class Set2SetGNN(T.GNN):
        def __init__(self, steps, **kw):
            super().__init__(graph_pooling="mean", **kw)
            self.graph_pooling = "set2set"
            self.pool = Set2Set(kw["emb_dim"], processing_steps=steps)
            self.graph_pred_linear = torch.nn.Linear(2 * kw["emb_dim"], kw["num_tasks"])
            self.pooled = torch.nn.Identity()  # (q*)

        def embed(self, x, edge_index, edge_attr, ptr):
            G = ptr.numel() - 1
            batch = torch.repeat_interleave(torch.arange(G), ptr[1:] - ptr[:-1])
            h = self.gnn_node(x, edge_index, edge_attr, batch)
            return h, self.pooled(self.pool(h, batch, G))

    base = T.make_model(kind, virtual_node, emb_dim, num_tasks=num_tasks)
    torch.manual_seed(9000 + seed)
    model = Set2SetGNN(steps, num_tasks=num_tasks, emb_dim=emb_dim, gnn_type=kind, virtual_node=virtual_node).double()
    sd = {k: v for k, v in copy.deepcopy(base.state_dict()).items() if not k.startswith("graph_pred_linear.")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith(("pool.lstm.", "graph_pred_linear.")) for k in missing), (missing, unexpected)
    gen = torch.Generator().manual_seed(9100 + seed)
    with torch.no_grad():
        for b in (model.pool.lstm.bias_ih_l0, model.pool.lstm.bias_hh_l0):
            b.add_(0.3 * torch.randn(b.shape, generator=gen).double())
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def s2s_of(model):
    """The six tensors (weights.SET2SET_KEYS) of a set2set_model, float64, straight from its parameters."""
    sd = {k: v.numpy() for k, v in model.state_dict().items()}
    return {"w_ih": sd["pool.lstm.weight_ih_l0"], "w_hh": sd["pool.lstm.weight_hh_l0"], "b_ih": sd["pool.lstm.bias_ih_l0"],
            "b_hh": sd["pool.lstm.bias_hh_l0"], "head_w": sd["graph_pred_linear.weight"], "head_b": sd["graph_pred_linear.bias"]}
