"""An executable PyTorch model of OGB's ogbg-code2 GNN: the expected values of tests/test_code2_export_cpu.py.

A plain `torch.nn` transcription of ogb/examples/graphproppred/code2: utils.py's ASTNodeEncoder, conv.py's GINConv (edge_encoder =
Linear(2, emb_dim)) and GNN_node, gnn.py's GNN with graph_pooling='mean' and graph_pred_linear_list = max_seq_len x Linear(emb_dim,
num_vocab).  torch_geometric's message passing and global_mean_pool are written out with index_add_; nothing else differs, and the
module tree gives OGB's `state_dict()` keys exactly.  Float64 on the CPU, seeded, small tables; nothing here knows what a GPU returns."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn


class ASTNodeEncoder(nn.Module):
    def __init__(self, emb_dim, num_nodetypes, num_nodeattributes, max_depth):
        super().__init__()
        self.max_depth = max_depth
        self.type_encoder = nn.Embedding(num_nodetypes, emb_dim)
        self.attribute_encoder = nn.Embedding(num_nodeattributes, emb_dim)
        self.depth_encoder = nn.Embedding(max_depth + 1, emb_dim)

    def forward(self, x, depth):
        depth = depth.clamp(max=self.max_depth)  # (OGB: depth[depth > self.max_depth] = self.max_depth)
        return self.type_encoder(x[:, 0]) + self.attribute_encoder(x[:, 1]) + self.depth_encoder(depth)


class GINConv(nn.Module):
    def __init__(self, emb_dim):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(emb_dim, 2 * emb_dim), nn.BatchNorm1d(2 * emb_dim), nn.ReLU(), nn.Linear(2 * emb_dim, emb_dim))
        self.eps = nn.Parameter(torch.Tensor([0]))
        self.edge_encoder = nn.Linear(2, emb_dim)

    def forward(self, x, edge_index, edge_attr):
        row, col = edge_index[0], edge_index[1]  # messages flow edge_index[0] -> edge_index[1]
        msg = F.relu(x[row] + self.edge_encoder(edge_attr))
        return self.mlp((1 + self.eps) * x + torch.zeros_like(x).index_add_(0, col, msg))


class GNN_node(nn.Module):
    def __init__(self, num_layer, emb_dim, node_encoder):
        super().__init__()
        self.node_encoder = node_encoder
        self.convs = nn.ModuleList(GINConv(emb_dim) for _ in range(num_layer))
        self.batch_norms = nn.ModuleList(nn.BatchNorm1d(emb_dim) for _ in range(num_layer))

    def forward(self, x, depth, edge_index, edge_attr):
        h = self.node_encoder(x, depth)
        for layer, (conv, bn) in enumerate(zip(self.convs, self.batch_norms)):
            h = bn(conv(h, edge_index, edge_attr))
            if layer != len(self.convs) - 1:
                h = F.relu(h)
        return h  # JK 'last'; dropout is the identity in eval()


class GNN(nn.Module):
    def __init__(self, num_vocab, max_seq_len, node_encoder, num_layer=5, emb_dim=300):
        super().__init__()
        self.gnn_node = GNN_node(num_layer, emb_dim, node_encoder)
        self.graph_pred_linear_list = nn.ModuleList(nn.Linear(emb_dim, num_vocab) for _ in range(max_seq_len))

    def forward(self, x, depth, edge_index, edge_attr, batch, num_graphs):
        h = self.gnn_node(x, depth, edge_index, edge_attr)
        ones = torch.ones(h.shape[0], dtype=h.dtype)
        pooled = torch.zeros((num_graphs, h.shape[1]), dtype=h.dtype).index_add_(0, batch, h)
        pooled = pooled / torch.zeros(num_graphs, dtype=h.dtype).index_add_(0, batch, ones)[:, None]  # global_mean_pool
        return h, pooled, torch.stack([lin(pooled) for lin in self.graph_pred_linear_list], dim=1)  # rows, pooled, [G][P][V]


def make_model(num_vocab, max_seq_len, n_types, n_attrs, max_depth, seed=0, emb_dim=300, num_layer=5):
    """A trained-looking model in eval(): seeded initialisation, then seeded BatchNorm statistics and affine terms and a non-zero eps per
    layer, so that no fold of the exporter is the identity"""
    torch.manual_seed(seed)
    model = GNN(num_vocab, max_seq_len, ASTNodeEncoder(emb_dim, n_types, n_attrs, max_depth), num_layer, emb_dim).double()
    g = torch.Generator().manual_seed(seed + 1)
    rnd = lambda t: torch.randn(t.shape, generator=g, dtype=torch.float64)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm1d):
                for t, base in ((m.weight, 1.0), (m.bias, 0.0), (m.running_mean, 0.0), (m.running_var, 1.0)):
                    t.copy_(base + 0.1 * rnd(t))
            if isinstance(m, GINConv):
                m.eps.copy_(0.1 * rnd(m.eps))
            if isinstance(m, nn.Embedding):
                m.weight.mul_(0.3)
    return model.eval()


def run(model, batch, x, depth, edge_features):
    """(rows [N][D], pooled [G][D], logits [G][P][V]) of one forward on a flowgnn_amd GraphBatch, as float64 arrays"""
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    gid = np.repeat(np.arange(batch.num_graphs), batch.nums_of_nodes)
    with torch.no_grad():
        out = model(t(x, torch.int64), t(depth, torch.int64), t(batch.global_edges().T, torch.int64), t(edge_features, torch.float64),
                    t(gid, torch.int64), batch.num_graphs)
    return tuple(o.numpy() for o in out)

