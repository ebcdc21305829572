"""OGB's virtual node for GCN (flowgnn.h: flowgnn_set_gcn_virtual_node), the expected values of tests/test_gcn_vn_cpu.py and
tests/test_gcn_vn_gpu.py: a float64 forward of the definition from engine-format weights, the wrong forms a careless implementation
computes instead (`variant=`), an OGB gcn-virtual state_dict with BatchNorm statistics, and the float64 forward of that state_dict
with nothing folded (ogb/examples/graphproppred/mol/conv.py, GNN_node_Virtualnode with GCNConv, in eval mode).

The oracle has no such model (the reference has none).  With the five tensors zero the forward below IS tests/numpy_ref.gcn_forward,
which the oracle tests pin; tests/test_gcn_vn_cpu.py checks that before anything relies on it."""
from collections import OrderedDict

import numpy as np

from flowgnn_amd import graphpack as gp, weights
from tests import numpy_ref
from tests.test_export import D, L, _bn, _bn_params, ogb_state_dict
from tests.test_gin_eps import one_node
from tests.test_resident_limits_gpu import random_graph

ND_OFF, ED_OFF = numpy_ref.ND_OFF, numpy_ref.ED_OFF
# the wrong forms (tests/test_gcn_vn_cpu.py: the fixed input tells each of them from the definition)
VARIANTS = ["no_add_in_last_layer", "pool_before_add", "t_without_vn", "mean_instead_of_sum", "update_indexed_l_plus_1", "embedding_ignored",
            "added_behind_the_linear_map", "added_in_front_of_the_relu"]


def fixed_batch():
    """One-node graphs at both ends, 300 molhiv-shaped graphs, every size from 2 to 5: 16-node tiles that hold many graphs, graphs that
    straddle one and two tile edges, and a last tile that ends in the middle."""
    tiny = [random_graph(n, n + k, seed=40 + 2 * n + k) for n in (2, 3, 4, 5) for k in (0, 1)]
    return gp.concat_batches([one_node(1), gp.synth_molhiv_batch(300, seed=13), one_node(2)] + tiny + [one_node(3)])


def fixed_weights(num_tasks=1):
    w = weights.synth_gcn_weights(seed=7, num_tasks=num_tasks)
    w["graph_pred_weights"] = (np.asarray(w["graph_pred_weights"], np.float32) * np.float32(8)).astype(np.float32)
    return w


def fixed_virtual_node():
    """weights.synth_gcn_virtual_node's random tensors, scaled per tensor until the fixed input tells every wrong form from the
    definition (tests/test_gcn_vn_cpu.py proves that it does): `t` is a SUM over 1 .. 80 nodes, so the first linear layer is scaled
    down until vn neither dies out nor explodes over four updates; leaving `+ vn_l` out of t changes t by one part in n + 1 only, so
    the later updates are scaled up until vn outweighs the rows it is added to; the biases are scaled down so that they do not drown
    it; and the embedding row is scaled up so that dropping E shows."""
    vn = weights.synth_gcn_virtual_node(seed=13)
    f32 = np.float32
    vn["vn_embedding"] = vn["vn_embedding"] * f32(8)
    vn["w1"] = vn["w1"] * f32(0.03)
    vn["w2"] = vn["w2"] * f32(0.5)
    vn["w2"][2] *= f32(3)
    vn["w2"][3] *= f32(32)
    vn["b1"] = vn["b1"] * f32(0.1)
    vn["b2"] = vn["b2"] * f32(0.1)
    return OrderedDict((k, np.ascontiguousarray(v, dtype=np.float32)) for k, v in vn.items())


def zero_virtual_node():
    return OrderedDict((k, np.zeros(s, np.float32)) for k, s in weights.GIN_VIRTUAL_NODE_SHAPES.items())


def range_virtual_node():
    """Zero but for one component of update 0's second bias: vn_1 = relu(b2[0]) has a component of 7e4 in every graph while every h_l
    is as small as without it, so x_1 = h_1 + vn_1 leaves the f16 split's range (6e4) in the registers of the fused kernel's VN
    instance and nowhere else in front of it.  The component is POSITIVE: vn_l is behind a ReLU for every l >= 1, and vn_0 = E, which
    may be negative, never reaches those registers (it is folded into layer 0's bias) -- so relu(a) + vn_l cannot go below zero there,
    and the kernel's |.| in the range tracking is a guard that no input reaches."""
    vn = zero_virtual_node()
    vn["b2"][0, 17] = np.float32(7.0e4)
    return vn


def forward(batch, w, vn, pooling="mean", num_tasks=1, variant=None, return_x4=False):
    """(logits [G] or [G][T], the last rows [N][100] -- BN_4(...), what the readout pools --, scale) in float64; scale = the largest
    magnitude of any activation (rows, projected rows, aggregates, t and the virtual node's hidden vector included): the `scale` of
    tests/parity.py.  return_x4: the projected rows of the last layer too (flowgnn_get_h), behind the scale."""
    assert variant is None or variant in VARIANTS, variant
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    nemb, eemb = f64(w["node_embedding_weight"]), f64(w["edge_embedding_weight"])
    cw, cb, root = f64(w["convs_weight"]), f64(w["convs_bias"]), f64(w["convs_root_emb_weight"])
    bnw, bnb, bnm, bnv = f64(w["bn_weight"]), f64(w["bn_bias"]), f64(w["bn_mean"]), f64(w["bn_var"])
    pw, pb = f64(w["graph_pred_weights"]).reshape(num_tasks, 100), f64(w["graph_pred_bias"]).reshape(num_tasks)
    E = f64(vn["vn_embedding"]).reshape(100)
    v1, c1, v2, c2 = f64(vn["w1"]), f64(vn["b1"]), f64(vn["w2"]), f64(vn["b2"])
    if variant == "embedding_ignored":
        E = np.zeros(100)
    N, G = batch.total_nodes, batch.num_graphs
    ge = batch.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    nn = f64(batch.nums_of_nodes)[:, None]
    seg = lambda rows: np.add.reduceat(rows, off[:-1], axis=0)  # (every graph has a node)
    outdeg = np.bincount(u, minlength=N).astype(np.float64)
    dinv = np.where(outdeg > 0, 1.0 / np.sqrt(outdeg + 1.0), 0.0)
    norm = dinv[u] * dinv[v]
    bn = lambda t, l: (t - bnm[l]) / np.sqrt(bnv[l] + 2.0 ** -10) * bnw[l] + bnb[l]
    h = nemb[batch.node_feature.astype(np.int64) + ND_OFF[None, :]].sum(axis=1)
    pre_relu = None  # BN_{l-1}(...) in front of the ReLU that gives h_l
    vec = np.tile(E, (G, 1))
    big = [float(np.abs(h).max()), float(np.abs(vec).max())]
    x4 = None
    for l in range(5):
        add = vec[gid]
        if l == 4 and variant == "no_add_in_last_layer":
            add = np.zeros_like(add)
        if variant == "added_in_front_of_the_relu" and pre_relu is not None:
            xin = np.maximum(pre_relu + add, 0.0)
        elif variant == "added_behind_the_linear_map":
            xin = h
        else:
            xin = h + add
        x = xin @ cw[l].T + cb[l]
        if variant == "added_behind_the_linear_map":
            x = x + add
        x4 = x
        ee = eemb[l][batch.edge_attr.astype(np.int64) + ED_OFF[None, :]].sum(axis=1)
        m = np.zeros((N, 100))
        np.add.at(m, v, norm[:, None] * np.maximum(x[u] + ee, 0.0))
        pre = bn(m + np.maximum(x + root[l], 0.0) / (outdeg[:, None] + 1.0), l)
        big.extend([float(np.abs(xin).max()), float(np.abs(x).max()), float(np.abs(m).max()), float(np.abs(pre).max())])
        if l < 4:
            rows = h if variant == "pool_before_add" else h + add
            t = seg(rows) / nn if variant == "mean_instead_of_sum" else seg(rows)
            if variant != "t_without_vn":
                t = t + vec
            k = (l + 1) % 4 if variant == "update_indexed_l_plus_1" else l
            hid = np.maximum(t @ v1[k].T + c1[k], 0.0)
            vec = np.maximum(hid @ v2[k].T + c2[k], 0.0)
            big.extend([float(np.abs(t).max()), float(hid.max()), float(vec.max())])
        pre_relu = pre
        h = np.maximum(pre, 0.0)
    if pooling == "mean":
        pooled = seg(pre) / nn
    elif pooling == "sum":
        pooled = seg(pre)
    else:
        pooled = np.maximum.reduceat(pre, off[:-1], axis=0)
    big.append(float(np.abs(pooled).max()))
    out = pooled @ pw.T + pb
    res = ((out[:, 0] if num_tasks == 1 else out), pre, max([1.0] + big))
    return res + (x4,) if return_x4 else res


# ---------------------------------------------------------------- the OGB side
def vn_state_dict(seed=4, with_bn=True, tasks=1):
    """tests.test_export.ogb_state_dict("gcn", ...) with gcn-virtual's keys: a non-zero embedding row and four
    Linear-BatchNorm-ReLU-Linear-BatchNorm-ReLU blocks (without BatchNorm: Linear-ReLU-Linear-ReLU)."""
    sd = ogb_state_dict("gcn", seed, tasks=tasks)
    rng = np.random.default_rng(seed + 1000)
    sd["gnn_node.virtualnode_embedding.weight"] = 0.5 * rng.standard_normal((1, D))
    for l in range(L - 1):
        m = f"gnn_node.mlp_virtualnode_list.{l}"
        second = 3 if with_bn else 2
        sd[f"{m}.0.weight"] = 0.02 * rng.standard_normal((2 * D, D))
        sd[f"{m}.0.bias"] = 0.5 * rng.standard_normal(2 * D)
        sd[f"{m}.{second}.weight"] = 0.03 * rng.standard_normal((D, 2 * D))
        sd[f"{m}.{second}.bias"] = 0.3 * rng.standard_normal(D)
        if with_bn:
            _bn_params(rng, f"{m}.1", 2 * D, sd)
            _bn_params(rng, f"{m}.4", D, sd)
    return sd


def ogb_vn_forward(sd, batch):
    """Inference of the OGB example GNN with gnn_type='gcn-virtual' (JK='last', no residual, mean pooling), float64, nothing folded:
    tests.test_export.ogb_forward's GCN layer with GNN_node_Virtualnode's additions."""
    ge = batch.global_edges()
    row, col = ge[:, 0], ge[:, 1]
    N, G = batch.total_nodes, batch.num_graphs
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    h = sum(sd[f"gnn_node.atom_encoder.atom_embedding_list.{k}.weight"][batch.node_feature[:, k]] for k in range(9))
    vec = np.tile(np.asarray(sd["gnn_node.virtualnode_embedding.weight"], np.float64).reshape(1, D), (G, 1))  # embedding(zeros(G))
    deg = np.bincount(row, minlength=N) + 1.0
    norm = deg[row] ** -0.5 * deg[col] ** -0.5
    for l in range(L):
        c = f"gnn_node.convs.{l}"
        h = h + vec[gid]
        e = sum(sd[f"{c}.bond_encoder.bond_embedding_list.{k}.weight"][batch.edge_attr[:, k]] for k in range(3))
        x = h @ sd[f"{c}.linear.weight"].T + sd[f"{c}.linear.bias"]
        z = np.zeros((N, D))
        np.add.at(z, col, norm[:, None] * np.maximum(x[row] + e, 0.0))
        z = z + np.maximum(x + sd[f"{c}.root_emb.weight"], 0.0) / deg[:, None]
        z = _bn(sd, f"gnn_node.batch_norms.{l}", z)
        if l < L - 1:
            m = f"gnn_node.mlp_virtualnode_list.{l}"
            t = np.add.reduceat(h, off[:-1], axis=0) + vec  # global_add_pool(h_list[layer], batch) + virtualnode_embedding
            t = t @ sd[f"{m}.0.weight"].T + sd[f"{m}.0.bias"]
            if f"{m}.1.weight" in sd:
                t = np.maximum(_bn(sd, f"{m}.1", t), 0.0) @ sd[f"{m}.3.weight"].T + sd[f"{m}.3.bias"]
                vec = np.maximum(_bn(sd, f"{m}.4", t), 0.0)
            else:
                vec = np.maximum(np.maximum(t, 0.0) @ sd[f"{m}.2.weight"].T + sd[f"{m}.2.bias"], 0.0)
        h = z if l == L - 1 else np.maximum(z, 0.0)
    pooled = np.add.reduceat(h, off[:-1], axis=0) / batch.nums_of_nodes[:, None]
    out = pooled @ sd["graph_pred_linear.weight"].T + sd["graph_pred_linear.bias"]
    return out[:, 0] if out.shape[1] == 1 else out
