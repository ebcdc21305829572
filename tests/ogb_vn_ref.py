"""OGB's virtual node for GIN (flowgnn.h: flowgnn_set_ogb_virtual_node), the expected values of tests/test_ogb_vn_cpu.py and
tests/test_ogb_vn_gpu.py: a float64 forward of the definition from engine-format weights, the wrong forms a careless implementation
computes instead (`variant=`), an OGB gin-virtual state_dict with BatchNorm statistics, and the float64 forward of that state_dict
with nothing folded (ogb/examples/graphproppred/mol/conv.py, GNN_node_Virtualnode, in eval mode).

The oracle has no such model (the reference has none).  With the five tensors zero the forward below IS tests.test_gin_eps.gin_eps_forward,
which reproduces tests/numpy_ref.py and the oracle; tests/test_ogb_vn_cpu.py checks that before anything relies on it."""
from collections import OrderedDict

import numpy as np

from flowgnn_amd import weights
from tests import numpy_ref
from tests.test_export import D, L, _bn, _bn_params, ogb_state_dict
from tests.test_gin_eps import self_scale

ND_OFF, ED_OFF = numpy_ref.ND_OFF, numpy_ref.ED_OFF
# the wrong forms (tests/test_ogb_vn_cpu.py: the fixed input tells each of them from the definition)
VARIANTS = ["no_add_in_last_layer", "pool_before_add", "t_without_vn", "mean_instead_of_sum", "update_indexed_l_plus_1", "embedding_ignored"]
NOOP_VARIANT = "update_after_layer_4"  # an update behind the last layer feeds nothing: the same result


def fixed_virtual_node():
    """The virtual node of the fixed input: weights.synth_gin_virtual_node's random tensors, scaled per tensor so that the input can
    tell every wrong form from the definition (tests/test_ogb_vn_cpu.py proves that it does).  What the scaling has to achieve: `t`
    is a SUM over 1 .. 80 nodes, so the first linear layer is scaled down until vn neither dies out nor explodes over four updates
    (a trained model's BatchNorm does that); leaving `+ vn_l` out of t changes t by one part in n + 1 only, so the last two updates
    are scaled up until vn_3 and vn_4 outweigh the rows they are added to and that part reaches the logits; the biases are scaled
    down so that they do not drown it; and the embedding row is scaled up so that dropping E shows."""
    vn = weights.synth_gin_virtual_node(seed=11)
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


def forward(batch, w, vn, eps=None, pooling="mean", num_tasks=1, variant=None):
    """(logits [G] or [G][T], h_5 rows [N][100], scale) in float64; scale = the largest magnitude of any activation (rows, aggregates,
    hidden values, t and the virtual node's hidden vector included): the `scale` of tests/parity.py."""
    assert variant is None or variant in VARIANTS or variant == NOOP_VARIANT, variant
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    s = np.ones(5) if eps is None else f64(self_scale(eps))
    nemb, eemb = f64(w["node_embedding_weight"]), f64(w["edge_embedding_weight"])
    w1, b1 = f64(w["node_mlp_1_weights"]), f64(w["node_mlp_1_bias"])
    w2, b2 = f64(w["node_mlp_2_weights"]), f64(w["node_mlp_2_bias"])
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
    h = nemb[batch.node_feature.astype(np.int64) + ND_OFF[None, :]].sum(axis=1)
    vec = np.tile(E, (G, 1))
    big = [float(np.abs(h).max()), float(np.abs(vec).max())]

    def update(l, x, h_in, vec):
        rows = h_in if variant == "pool_before_add" else x
        t = seg(rows) / nn if variant == "mean_instead_of_sum" else seg(rows)
        if variant != "t_without_vn":
            t = t + vec
        k = (l + 1) % 4 if variant == "update_indexed_l_plus_1" else l
        hid = np.maximum(t @ v1[k].T + c1[k], 0.0)
        out = np.maximum(hid @ v2[k].T + c2[k], 0.0)
        big.extend([float(np.abs(t).max()), float(hid.max()), float(out.max())])
        return out

    for l in range(5):
        x = h if (l == 4 and variant == "no_add_in_last_layer") else h + vec[gid]
        ee = eemb[l][batch.edge_attr.astype(np.int64) + ED_OFF[None, :]].sum(axis=1)
        m = np.zeros((N, 100))
        np.add.at(m, v, np.maximum(x[u] + ee, 0.0))
        a = m + s[l] * x
        hid = np.maximum(a @ w1[l].T + b1[l], 0.0)
        h_next = hid @ w2[l].T + b2[l]
        if l != 4:
            h_next = np.maximum(h_next, 0.0)
        big.extend([float(np.abs(x).max()), float(np.abs(a).max()), float(hid.max()), float(np.abs(h_next).max())])
        if l < 4:
            vec = update(l, x, h, vec)
        elif variant == NOOP_VARIANT:
            update(3, x, h, vec)  # computed and dropped
        h = h_next
    if pooling == "mean":
        pooled = seg(h) / nn
    elif pooling == "sum":
        pooled = seg(h)
    else:
        pooled = np.maximum.reduceat(h, off[:-1], axis=0)
    big.append(float(np.abs(pooled).max()))
    out = pooled @ pw.T + pb
    return (out[:, 0] if num_tasks == 1 else out), h, max([1.0] + big)


# ---------------------------------------------------------------- the OGB side
def vn_state_dict(seed=3, with_bn=True, tasks=1):
    """tests.test_export.ogb_state_dict("gin", ...) with a trained eps and gin-virtual's keys: a non-zero embedding row and four
    Linear-BatchNorm-ReLU-Linear-BatchNorm-ReLU blocks (without BatchNorm: Linear-ReLU-Linear-ReLU)."""
    sd = ogb_state_dict("gin", seed, with_bn=with_bn, tasks=tasks)
    rng = np.random.default_rng(seed + 1000)
    for l, e in enumerate([0.12, -0.07, 0.3, -0.21, 0.05]):
        sd[f"gnn_node.convs.{l}.eps"] = np.array([e])
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
    """Inference of the OGB example GNN with gnn_type='gin-virtual' (JK='last', no residual, mean pooling), float64, nothing folded:
    tests.test_export.ogb_forward's GIN layer with GNN_node_Virtualnode's additions."""
    ge = batch.global_edges()
    row, col = ge[:, 0], ge[:, 1]
    N, G = batch.total_nodes, batch.num_graphs
    off = batch.node_offsets()
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    h = sum(sd[f"gnn_node.atom_encoder.atom_embedding_list.{k}.weight"][batch.node_feature[:, k]] for k in range(9))
    vec = np.tile(np.asarray(sd["gnn_node.virtualnode_embedding.weight"], np.float64).reshape(1, D), (G, 1))  # embedding(zeros(G))
    for l in range(L):
        c = f"gnn_node.convs.{l}"
        h = h + vec[gid]
        e = sum(sd[f"{c}.bond_encoder.bond_embedding_list.{k}.weight"][batch.edge_attr[:, k]] for k in range(3))
        agg = np.zeros((N, D))
        np.add.at(agg, col, np.maximum(h[row] + e, 0.0))
        z = ((1.0 + sd[f"{c}.eps"][0]) * h + agg) @ sd[f"{c}.mlp.0.weight"].T + sd[f"{c}.mlp.0.bias"]
        if f"{c}.mlp.1.weight" in sd:
            z = np.maximum(_bn(sd, f"{c}.mlp.1", z), 0.0) @ sd[f"{c}.mlp.3.weight"].T + sd[f"{c}.mlp.3.bias"]
        else:
            z = np.maximum(z, 0.0) @ sd[f"{c}.mlp.2.weight"].T + sd[f"{c}.mlp.2.bias"]
        if f"gnn_node.batch_norms.{l}.weight" in sd:
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
