"""Producer side of the reference's file formats -- the part the reference repo does not ship.

The reference consumes raw float32 `.bin` weight files (GIN/src/host_load.cc:24-58, GCN/src/host_load.cc:31-170) and a
per-graph pack (`graph_info/g%d_info.txt`, `graph_bin/g%d_*.bin`, GIN/src/host_load.cc:100-143).  Its GCN file is, float for
float, the flattened `state_dict` of the OGB `GNN(gnn_type='gcn', num_layer=5, emb_dim=100)` example model (BatchNorm blocks
of 4 x 100 floats + the `num_batches_tracked` counter: the 401-float stride of GCN/src/host_load.cc:118-166); its GIN files
are the same model family trained without BatchNorm.  This module writes those files from

  * a PyTorch `state_dict` (tensors or arrays) with the OGB example's parameter names -- for GIN, BatchNorm layers (inference
    statistics) are folded into the adjacent linear layers, which is exact, because the reference's GIN has no BatchNorm;
  * any sequence of graph objects with PyG `Data` attributes (`x`, `edge_index`, `edge_attr`, optional `eig`).

Nothing here needs torch, torch_geometric or ogb to be installed: tensors are taken through `numpy()` when they have it.
Host-side tooling only; the device path never imports this module.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Iterable, Mapping, Optional

import numpy as np

from . import weights as _weights
from .graphpack import GraphBatch, write_pack

ATOM_DIMS = (119, 4, 12, 12, 10, 6, 6, 2, 2)  # OGB AtomEncoder tables = offsets {0,119,123,...,171} of GIN/src/host_load.cc:5
BOND_DIMS = (5, 6, 2)                          # OGB BondEncoder tables = offsets {0,5,11} of GIN/src/message_passing.cc:3
BN_EPS = 1e-5                                  # torch.nn.BatchNorm1d default
REF_BN_EPS = 2.0 ** -10                        # what the reference adds to var (GCN/src/load_inputs.cc:32)


class ExportError(ValueError):
    pass


def _np(t) -> np.ndarray:
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def _get(sd: Mapping, key: str) -> np.ndarray:
    if key not in sd:
        raise ExportError(f"state_dict has no '{key}'")
    return _np(sd[key])


def _tables(sd: Mapping, prefix: str, dims) -> np.ndarray:
    """Concatenate the per-feature embedding tables of an OGB Atom/BondEncoder into the reference's single table."""
    rows = []
    for k, n in enumerate(dims):
        t = _get(sd, f"{prefix}.{k}.weight")
        if t.shape[0] != n:
            raise ExportError(f"{prefix}.{k}.weight has {t.shape[0]} rows, the reference's offsets need {n}")
        rows.append(t)
    return np.concatenate(rows, axis=0)


def _fold_bn(w: np.ndarray, b: np.ndarray, sd: Mapping, prefix: str):
    """BatchNorm(inference)(W x + b) as one linear layer (W', b')."""
    g, beta = _get(sd, prefix + ".weight"), _get(sd, prefix + ".bias")
    mean, var = _get(sd, prefix + ".running_mean"), _get(sd, prefix + ".running_var")
    s = g / np.sqrt(var + BN_EPS)
    return w * s[:, None], (b - mean) * s + beta


def gin_eps_from_ogb_state_dict(sd: Mapping, num_layers: int = 5) -> np.ndarray:
    """The trained `gnn_node.convs.l.eps` of an OGB GIN state_dict as float32[num_layers] (0 where a layer has none): what
    Engine.set_gin_eps / flowgnn_set_gin_eps take, and what export_weights(..., keep_eps=True) writes into the eps file."""
    out = np.zeros(num_layers, np.float32)
    for l in range(num_layers):
        k = f"gnn_node.convs.{l}.eps"
        if k in sd:
            out[l] = np.float32(_np(sd[k]).ravel()[0])
    if not np.isfinite(out).all():
        raise ExportError("eps: non-finite values")
    return out


def num_layers_of_ogb_state_dict(sd: Mapping) -> int:
    """OGB's num_layer read off a GNN(...) state_dict: the number of `gnn_node.convs.<l>` blocks, which must be numbered 0 .. L - 1."""
    idx = set()
    for k in sd:
        parts = str(k).split(".")
        if len(parts) > 3 and parts[0] == "gnn_node" and parts[1] == "convs" and parts[2].isdigit():
            idx.add(int(parts[2]))
    if not idx:
        raise ExportError("state_dict has no 'gnn_node.convs.<l>.*' keys: not an OGB GNN(...) model")
    if idx != set(range(len(idx))):
        raise ExportError(f"'gnn_node.convs' has the layers {sorted(idx)}: wanted 0 .. {len(idx) - 1}")
    return len(idx)


def _checked_depth(num_layers: int, width: int) -> int:
    """The depths the engine runs (flowgnn_set_num_layers): 2 .. 8 at width 300, 5 alone at width 100."""
    try:
        return _weights._depth(num_layers, width)
    except ValueError as e:
        raise ExportError(f"{e}: the state_dict is {num_layers} layers deep and {width} wide")


VN_KEY = "gnn_node.virtualnode_embedding.weight"  # what tells a gin-virtual state_dict from a gin one


def _vn_dim(virtual_node_dim) -> int:
    d = int(virtual_node_dim)
    if d not in _weights.GIN_EMB_DIMS:
        raise ExportError(f"virtual_node_dim {virtual_node_dim}: the engine's virtual node is {_weights.GIN_EMB_DIMS[0]} or {_weights.GIN_EMB_DIMS[1]} wide")
    return d


def _virtual_node_from_ogb_state_dict(sd: Mapping, num_layers: int, dim: int = 100) -> Dict[str, np.ndarray]:
    """GNN_node_Virtualnode's own keys are the same whatever gnn_type the convolutions have: the folding of both exporters below."""
    emb = _get(sd, VN_KEY).reshape(-1)
    if emb.size != dim:
        raise ExportError(f"'{VN_KEY}' is {emb.size} wide and virtual_node_dim is {dim}" +
                          (": the virtual node's tensors are 100-wide unless virtual_node_dim=300 says otherwise" if dim == 100 else ""))
    w1s, b1s, w2s, b2s = [], [], [], []
    for l in range(num_layers - 1):
        m = f"gnn_node.mlp_virtualnode_list.{l}"
        w1, b1 = _get(sd, f"{m}.0.weight"), _get(sd, f"{m}.0.bias")
        if f"{m}.1.running_mean" in sd:
            w1, b1 = _fold_bn(w1, b1, sd, f"{m}.1")
            w2, b2 = _get(sd, f"{m}.3.weight"), _get(sd, f"{m}.3.bias")
            if f"{m}.4.running_mean" in sd:
                w2, b2 = _fold_bn(w2, b2, sd, f"{m}.4")
        else:
            w2, b2 = _get(sd, f"{m}.2.weight"), _get(sd, f"{m}.2.bias")
        w1s.append(w1); b1s.append(b1); w2s.append(w2); b2s.append(b2)
    out = OrderedDict([("vn_embedding", emb), ("w1", np.stack(w1s)), ("b1", np.stack(b1s)), ("w2", np.stack(w2s)), ("b2", np.stack(b2s))])
    return _checked(out, _weights.gin_virtual_node_shapes(dim, _checked_depth(num_layers, dim)), lambda k, v: v)


def gin_virtual_node_from_ogb_state_dict(sd: Mapping, num_layers: int = 5, virtual_node_dim: int = 100) -> Dict[str, np.ndarray]:
    """The virtual node of an OGB `GNN(gnn_type='gin-virtual')` state_dict as the five tensors Engine.set_ogb_virtual_node /
    flowgnn_set_ogb_virtual_node take: `gnn_node.virtualnode_embedding.weight` [1][100] and, per update l < num_layers - 1,
    `gnn_node.mlp_virtualnode_list.l` = Linear-BatchNorm-ReLU-Linear-BatchNorm-ReLU (OGB: .0 .1 .3 .4) or Linear-ReLU-Linear-ReLU
    (.0 .2).  Both BatchNorms (inference statistics) sit in front of a ReLU and are folded into the linear layer before them: exact.
    virtual_node_dim: the width the caller expects, 100 or 300 (flowgnn_set_ogb_virtual_node_dim); a state_dict of another width is refused."""
    return _virtual_node_from_ogb_state_dict(sd, num_layers, _vn_dim(virtual_node_dim))


def gcn_virtual_node_from_ogb_state_dict(sd: Mapping, num_layers: int = 5, virtual_node_dim: int = 100) -> Dict[str, np.ndarray]:
    """The same five tensors of an OGB `GNN(gnn_type='gcn-virtual')` state_dict, for Engine.set_gcn_virtual_node /
    flowgnn_set_gcn_virtual_node (the virtual node's keys and its MLP do not depend on the convolution).
    virtual_node_dim: the width the caller expects, 100 or 300 (flowgnn_set_gcn_virtual_node_dim); a state_dict of another width is refused."""
    return _virtual_node_from_ogb_state_dict(sd, num_layers, _vn_dim(virtual_node_dim))


ATTN_KEY = "pool.gate_nn.0.weight"  # what tells a graph_pooling="attention" state_dict from the others


def attention_pooling_from_ogb_state_dict(sd: Mapping, emb_dim: int = 300) -> Dict[str, np.ndarray]:
    """The gate of an OGB `GNN(graph_pooling='attention')` state_dict as the three tensors Engine.set_attention_pooling /
    flowgnn_set_attention_pooling take: `pool.gate_nn` = Linear(D, 2D)-BatchNorm1d(2D)-ReLU-Linear(2D, 1) (OGB: .0 .1 .3).  The
    BatchNorm (inference statistics) sits in front of the ReLU and is folded into the first linear layer: exact.  `pool.gate_nn.3.bias`
    adds the same number to every gate of a graph and cancels in the softmax: it is dropped, here and in the engine.
    emb_dim: the width the caller expects (300: only the 300-wide models have this readout); a state_dict of another width is refused."""
    try:
        shapes = _weights.attention_pooling_shapes(emb_dim)
    except ValueError as e:
        raise ExportError(str(e))
    d = int(emb_dim)
    if ATTN_KEY not in sd:
        raise ExportError(f"state_dict has no '{ATTN_KEY}': it is not a graph_pooling='attention' model (its keys are pool.gate_nn.*)")
    w1, b1 = _get(sd, "pool.gate_nn.0.weight"), _get(sd, "pool.gate_nn.0.bias")
    if w1.shape != (2 * d, d):
        raise ExportError(f"'pool.gate_nn.0.weight' is {w1.shape} and emb_dim is {d}: wanted ({2 * d}, {d})")
    if b1.shape != (2 * d,):
        raise ExportError(f"'pool.gate_nn.0.bias' is {b1.shape}, wanted ({2 * d},)")
    for k in ("weight", "bias", "running_mean", "running_var"):
        t = _get(sd, f"pool.gate_nn.1.{k}")
        if t.shape != (2 * d,):
            raise ExportError(f"'pool.gate_nn.1.{k}' is {t.shape}, wanted ({2 * d},)")
    if (_get(sd, "pool.gate_nn.1.running_var") + BN_EPS <= 0).any():
        raise ExportError("'pool.gate_nn.1.running_var' is not positive")
    w1, b1 = _fold_bn(w1, b1, sd, "pool.gate_nn.1")
    w2 = _get(sd, "pool.gate_nn.3.weight")
    if w2.size != 2 * d or w2.shape[0] != 1:
        raise ExportError(f"'pool.gate_nn.3.weight' is {w2.shape}, wanted (1, {2 * d})")
    out = OrderedDict([("w1", w1), ("b1", b1), ("w2", w2.reshape(-1))])
    return _checked(out, shapes, lambda k, v: v)


S2S_KEY = "pool.lstm.weight_ih_l0"  # what tells a graph_pooling="set2set" state_dict from the others
_S2S_SD_KEYS = OrderedDict([("w_ih", "pool.lstm.weight_ih_l0"), ("w_hh", "pool.lstm.weight_hh_l0"), ("b_ih", "pool.lstm.bias_ih_l0"),
                            ("b_hh", "pool.lstm.bias_hh_l0"), ("head_w", "graph_pred_linear.weight"), ("head_b", "graph_pred_linear.bias")])


def set2set_from_ogb_state_dict(sd: Mapping, emb_dim: int = 300) -> Dict[str, np.ndarray]:
    """The readout of an OGB `GNN(graph_pooling='set2set')` state_dict as the six tensors Engine.set_set2set_pooling /
    flowgnn_set_set2set_pooling take: PyG's `pool.lstm` = torch.nn.LSTM(2D, D) (weight_ih_l0 [4D][2D], weight_hh_l0 [4D][D], bias_ih_l0,
    bias_hh_l0 [4D]; gate order i, f, g, o) and OGB's `graph_pred_linear` = Linear(2D, NUM_TASK), every row of it.  The tensors are taken
    as they are; the number of processing steps is no tensor (OGB: 2) and is given to the engine.
    emb_dim: the width the caller expects (300: only the 300-wide models have this readout); a state_dict of another width is refused."""
    d = int(emb_dim)
    if S2S_KEY not in sd:
        raise ExportError(f"state_dict has no '{S2S_KEY}': it is not a graph_pooling='set2set' model (its keys are pool.lstm.*)")
    out = OrderedDict((k, _get(sd, name)) for k, name in _S2S_SD_KEYS.items())
    t = out["head_w"].shape[0] if out["head_w"].ndim == 2 else 0
    try:
        shapes = _weights.set2set_shapes(d, max(1, t))
    except ValueError as e:
        raise ExportError(str(e))
    for k, shp in shapes.items():
        if out[k].shape != shp:
            raise ExportError(f"'{_S2S_SD_KEYS[k]}' is {out[k].shape} and emb_dim is {d}: wanted {shp}")
    return _checked(out, shapes, lambda k, v: v)


def _mean_head_zeroed(sd: Mapping, emb_dim: int) -> Dict:
    """`sd` with graph_pred_linear replaced by an all-zero [T][D] head and bias: what the model's own set carries beside a set2set file"""
    t = _get(sd, "graph_pred_linear.weight").shape[0]
    out = dict(sd)
    out["graph_pred_linear.weight"] = np.zeros((t, int(emb_dim)), np.float32)
    out["graph_pred_linear.bias"] = np.zeros(t, np.float32)
    return out


def gin_weights_from_ogb_state_dict(sd: Mapping, num_layers: int = 5, eps_tol: float = 0.0, multi_task: bool = False,
                                    keep_eps: bool = False, virtual_node: bool = False, virtual_node_dim: int = 100) -> Dict[str, np.ndarray]:
    """OGB `GNN(gnn_type='gin', virtual_node=False, JK='last', residual=False, graph_pooling='mean')` -> the reference's
    GIN weight set.  `convs.l.mlp` may be Linear-BatchNorm-ReLU-Linear (OGB) or Linear-ReLU-Linear; `batch_norms.l`
    (applied to the conv output before the ReLU) is folded into the second linear layer when present.
    multi_task: keep every row of graph_pred_linear (ogbg-molpcba: 128 tasks) -- graph_pred_weights becomes [NUM_TASK][100], for
    an engine with flowgnn_set_num_tasks(NUM_TASK); without it a head with more than one task is refused (the reference's NUM_TASK is 1).
    The reference ignores GIN's eps (GIN/src/host_load.cc reads it, nothing uses it): a trained |eps| > eps_tol is refused, unless
    keep_eps says that the engine will apply it (gin_eps_from_ogb_state_dict + flowgnn_set_gin_eps).
    A gin-virtual state_dict (it has `gnn_node.virtualnode_embedding.weight`) is refused -- the weight set alone is a model nobody
    trained -- unless virtual_node says that the engine will run the virtual node too (gin_virtual_node_from_ogb_state_dict +
    flowgnn_set_ogb_virtual_node).
    The width is read off `atom_embedding_list.0.weight`: 100 (the reference's) or 300 (OGB's default; the tensors are then the
    300-wide set of flowgnn_set_emb_dim(FLOWGNN_EMB_DIM_OGB)).  A 300-wide gin-virtual state_dict exports only with virtual_node=True
    AND virtual_node_dim=300 (the engine then takes its virtual node through flowgnn_set_ogb_virtual_node_dim); without the keyword
    the virtual node's tensors are 100-wide and the state_dict is refused.  A virtual_node_dim other than the state_dict's width is
    refused too."""
    vdim = _vn_dim(virtual_node_dim)
    p = "gnn_node"
    width = int(_get(sd, f"{p}.atom_encoder.atom_embedding_list.0.weight").shape[-1])
    if width not in _weights.GIN_EMB_DIMS:
        raise ExportError(f"atom_embedding_list.0.weight is {width} wide: the engine runs GIN at emb_dim 100 (the reference's width) "
                          f"and at emb_dim 300 (OGB's default), no other")
    if vdim != 100 and vdim != width:
        raise ExportError(f"virtual_node_dim is {vdim} and the state_dict is {width} wide")
    if VN_KEY in sd and width != vdim:
        raise ExportError(f"the state_dict has '{VN_KEY}' and is {width} wide: the engine's virtual node (flowgnn_set_ogb_virtual_node) "
                          f"has 100-wide tensors unless told otherwise, so a {width}-wide gin-virtual model exports only with "
                          f"virtual_node=True, virtual_node_dim={width} (flowgnn_set_ogb_virtual_node_dim)")
    if VN_KEY in sd and not virtual_node:
        raise ExportError(f"the state_dict has '{VN_KEY}': it is OGB's gin-virtual, and these weights without its virtual node are "
                          f"a model nobody trained; pass virtual_node=True and give the engine gin_virtual_node_from_ogb_state_dict(sd) "
                          f"(Engine.set_ogb_virtual_node)")
    out = OrderedDict()
    out["node_embedding_weight"] = _tables(sd, f"{p}.atom_encoder.atom_embedding_list", ATOM_DIMS)
    ed, w1s, b1s, w2s, b2s = [], [], [], [], []
    for l in range(num_layers):
        c = f"{p}.convs.{l}"
        if not keep_eps and f"{c}.eps" in sd and abs(float(_np(sd[f"{c}.eps"]).ravel()[0])) > eps_tol:
            raise ExportError(f"{c}.eps = {float(_np(sd[c + '.eps']).ravel()[0]):g}: the reference's GIN has no eps term")
        ed.append(_tables(sd, f"{c}.bond_encoder.bond_embedding_list", BOND_DIMS))
        w1, b1 = _get(sd, f"{c}.mlp.0.weight"), _get(sd, f"{c}.mlp.0.bias")
        if f"{c}.mlp.1.running_mean" in sd:
            w1, b1 = _fold_bn(w1, b1, sd, f"{c}.mlp.1")
            w2, b2 = _get(sd, f"{c}.mlp.3.weight"), _get(sd, f"{c}.mlp.3.bias")
        else:
            w2, b2 = _get(sd, f"{c}.mlp.2.weight"), _get(sd, f"{c}.mlp.2.bias")
        if f"{p}.batch_norms.{l}.running_mean" in sd:
            w2, b2 = _fold_bn(w2, b2, sd, f"{p}.batch_norms.{l}")
        w1s.append(w1); b1s.append(b1); w2s.append(w2); b2s.append(b2)
    out["edge_embedding_weight"] = np.stack(ed)
    out["node_mlp_1_weights"], out["node_mlp_1_bias"] = np.stack(w1s), np.stack(b1s)
    out["node_mlp_2_weights"], out["node_mlp_2_bias"] = np.stack(w2s), np.stack(b2s)
    pw, pb = _get(sd, "graph_pred_linear.weight"), _get(sd, "graph_pred_linear.bias")
    if pw.shape[0] != 1 and not multi_task:
        raise ExportError(f"graph_pred_linear has {pw.shape[0]} tasks; the reference is built with NUM_TASK = 1 (GIN/src/dcl.h:25): "
                          f"pass multi_task=True for an engine with flowgnn_set_num_tasks({pw.shape[0]})")
    out["graph_pred_weights"], out["graph_pred_bias"] = pw, pb
    return _checked(out, _weights.gin_files(width, _checked_depth(num_layers, width)), lambda k, v: _weights._task_shape(k, v[1], pw.shape[0]))


def gcn_weights_from_ogb_state_dict(sd: Mapping, num_layers: int = 5, multi_task: bool = False,
                                    virtual_node: bool = False, emb_dim: int = 100, virtual_node_dim: int = 100) -> Dict[str, np.ndarray]:
    """OGB `GNN(gnn_type='gcn', ...)` -> the reference's GCN weight set.  BatchNorm stays a separate step in the
    reference (GCN/src/node_embedding.cc:123-138) but with 2^-10 added to the variance instead of torch's 1e-5
    (GCN/src/load_inputs.cc:32): the exported variance is shifted by the difference so that both normalise alike.
    A gcn-virtual state_dict (it has `gnn_node.virtualnode_embedding.weight`) is refused -- the weight set alone is a model nobody
    trained -- unless virtual_node says that the engine will run the virtual node too (gcn_virtual_node_from_ogb_state_dict +
    flowgnn_set_gcn_virtual_node).
    emb_dim: the width the caller expects, 100 or 300 (OGB's default, for an engine with flowgnn_set_model_emb_dim(300)); a state_dict
    of another width is refused.  A 300-wide gcn-virtual state_dict exports only with virtual_node=True, emb_dim=300 AND
    virtual_node_dim=300 (the engine then takes its virtual node through flowgnn_set_gcn_virtual_node_dim); without that keyword the
    virtual node's tensors are 100 wide and the state_dict is refused.  A virtual_node_dim other than emb_dim is refused too."""
    p = "gnn_node"
    vdim = _vn_dim(virtual_node_dim)
    if int(emb_dim) not in _weights.GCN_EMB_DIMS:
        raise ExportError(f"emb_dim {emb_dim}: the engine runs GCN at emb_dim {_weights.GCN_EMB_DIMS[0]} (the reference's width) and "
                          f"{_weights.GCN_EMB_DIMS[1]} (OGB's default), no other")
    emb_dim = int(emb_dim)
    shapes = _weights.gcn_shapes(emb_dim, _checked_depth(num_layers, emb_dim))
    if vdim != 100 and vdim != emb_dim:
        raise ExportError(f"virtual_node_dim is {vdim} and emb_dim is {emb_dim}: the virtual node has the model's width")
    if emb_dim != 100:
        if virtual_node and vdim != emb_dim:
            raise ExportError(f"virtual_node=True at emb_dim {emb_dim}: the virtual node's tensors are 100 wide unless told otherwise, and the "
                              f"engine runs those at emb_dim 100 only; a {emb_dim}-wide gcn-virtual model exports with "
                              f"virtual_node_dim={emb_dim} beside emb_dim={emb_dim} (flowgnn_set_gcn_virtual_node_dim)")
        width = int(_get(sd, f"{p}.atom_encoder.atom_embedding_list.0.weight").shape[-1])
        if width != emb_dim:
            raise ExportError(f"atom_embedding_list.0.weight is {width} wide and emb_dim is {emb_dim}")
    if VN_KEY in sd and not virtual_node:
        raise ExportError(f"the state_dict has '{VN_KEY}': it is OGB's gcn-virtual, and these weights without its virtual node are "
                          f"a model nobody trained; pass virtual_node=True and give the engine gcn_virtual_node_from_ogb_state_dict(sd) "
                          f"(Engine.set_gcn_virtual_node)")
    out = OrderedDict()
    out["node_embedding_weight"] = _tables(sd, f"{p}.atom_encoder.atom_embedding_list", ATOM_DIMS)
    cols = {k: [] for k in ("edge_embedding_weight", "convs_weight", "convs_bias", "convs_root_emb_weight", "bn_weight", "bn_bias",
                            "bn_mean", "bn_var")}
    for l in range(num_layers):
        c, bn = f"{p}.convs.{l}", f"{p}.batch_norms.{l}"
        cols["edge_embedding_weight"].append(_tables(sd, f"{c}.bond_encoder.bond_embedding_list", BOND_DIMS))
        cols["convs_weight"].append(_get(sd, f"{c}.linear.weight"))
        cols["convs_bias"].append(_get(sd, f"{c}.linear.bias"))
        cols["convs_root_emb_weight"].append(_get(sd, f"{c}.root_emb.weight").reshape(-1))
        cols["bn_weight"].append(_get(sd, f"{bn}.weight"))
        cols["bn_bias"].append(_get(sd, f"{bn}.bias"))
        cols["bn_mean"].append(_get(sd, f"{bn}.running_mean"))
        var = _get(sd, f"{bn}.running_var") + (BN_EPS - REF_BN_EPS)
        if (var + REF_BN_EPS <= 0).any():
            raise ExportError(f"{bn}.running_var is not positive")
        cols["bn_var"].append(var)
    for k, v in cols.items():
        out[k] = np.stack(v)
    pw, pb = _get(sd, "graph_pred_linear.weight"), _get(sd, "graph_pred_linear.bias")
    if pw.shape[0] != 1 and not multi_task:
        raise ExportError(f"graph_pred_linear has {pw.shape[0]} tasks; the reference is built with NUM_TASK = 1 (GCN/src/dcl.h): "
                          f"pass multi_task=True for an engine with flowgnn_set_num_tasks({pw.shape[0]})")
    out["graph_pred_weights"], out["graph_pred_bias"] = pw, pb
    ordered = OrderedDict((k, out[k]) for k in shapes)
    return _checked(ordered, shapes, lambda k, v: _weights._task_shape(k, v, pw.shape[0]))


def _checked(w: Dict[str, np.ndarray], spec: Mapping, shape_of) -> Dict[str, np.ndarray]:
    res = OrderedDict()
    for k, v in spec.items():
        shp = tuple(shape_of(k, v))
        a = np.asarray(w[k], dtype=np.float64)
        if a.size != int(np.prod(shp)):
            raise ExportError(f"{k}: {a.shape} does not fit the reference's {shp}")
        if not np.isfinite(a).all():
            raise ExportError(f"{k}: non-finite values")
        res[k] = np.ascontiguousarray(a.reshape(shp), dtype=np.float32)
    return res


def export_weights(model: str, sd: Mapping, directory: str, multi_task: bool = False, keep_eps: bool = False,
                   virtual_node: bool = False, virtual_node_dim: int = 100, emb_dim: int = 100,
                   attention_pooling: bool = False, set2set: bool = False) -> Dict[str, np.ndarray]:
    """Write the `.bin` file(s) `host` / `flowgnn_load_weights_dir` read for `model` ('GIN', 'GIN-VN' or 'GCN').
    multi_task: keep all rows of the prediction head (the engine then needs flowgnn_set_num_tasks(rows) before loading).
    keep_eps (GIN, GIN-VN): a trained eps is not refused; the eps file holds the trained values, for `host --eps` /
    Engine.load_weights_dir(dir, eps=True) to apply (flowgnn_set_gin_eps).  A 300-wide GIN state_dict (OGB's default emb_dim) gives the
    dim300 file set, for an engine with flowgnn_set_emb_dim(300) / `host GIN --emb-dim 300`.
    virtual_node (GIN): the state_dict is OGB's gin-virtual; its virtual node goes into gin_ep1_virtualnode_dim100.bin beside the
    others, for `host GIN --ogb-vn` / Engine.load_weights_dir(dir, virtual_node=True) to apply (flowgnn_set_ogb_virtual_node).
    virtual_node_dim (GIN): 300 for a 300-wide gin-virtual state_dict, whose virtual node goes into gin_ep1_virtualnode_dim300.bin
    (flowgnn_set_ogb_virtual_node_dim; `host GIN --emb-dim 300 --eps --ogb-vn`); without it such a state_dict is refused.
    virtual_node (GCN): likewise OGB's gcn-virtual, into gcn_ep1_virtualnode_dim100.bin (flowgnn_set_gcn_virtual_node).
    virtual_node_dim (GCN): 300 beside emb_dim=300 for a 300-wide gcn-virtual state_dict, whose virtual node goes into
    gcn_ep1_virtualnode_dim300.bin (flowgnn_set_gcn_virtual_node_dim; `host GCN --emb-dim 300 --ogb-vn`); without it such a
    state_dict is refused, and so is a virtual_node_dim other than emb_dim.
    emb_dim (GCN): 300 for a 300-wide gcn state_dict, which goes into gcn_ep1_dim300.weights.all.bin, for an engine with
    flowgnn_set_model_emb_dim(300) / `host GCN --emb-dim 300`; without it such a state_dict is refused.  (GIN reads its width off the
    state_dict and takes no emb_dim.)
    attention_pooling (GIN, GCN at width 300): the state_dict was trained with graph_pooling='attention'; its gate goes into
    gin_ep1_attnpool_dim300.bin / gcn_ep1_attnpool_dim300.bin beside the others (attention_pooling_from_ogb_state_dict), for
    `host GIN|GCN --emb-dim 300 --attn-pool` / Engine.load_weights_dir(dir, attention_pooling=True) to apply
    (flowgnn_set_attention_pooling).  Without the keyword such a state_dict is refused: its head was never trained on the mean.
    set2set (GIN, GCN at width 300): the state_dict was trained with graph_pooling='set2set'; its LSTM and its Linear(2D, NUM_TASK) head
    go into gin_ep1_set2set_dim300.bin / gcn_ep1_set2set_dim300.bin beside the others (set2set_from_ogb_state_dict), for
    `host GIN|GCN --emb-dim 300 --set2set` / Engine.load_weights_dir(dir, set2set=True) to apply (flowgnn_set_set2set_pooling).  The
    model's own set then carries an all-zero [NUM_TASK][D] head and bias -- the 2D-wide head does not fit it -- so a run that forgets the
    flag gives zeros, not plausible numbers.  Without the keyword such a state_dict is refused, and so is set2set together with
    attention_pooling.
    OGB's GNN(JK=..., residual=...) need nothing here: neither flag adds a parameter, so neither is in a state_dict and the files of
    such a model are those of a JK='last', residual=False one.  The CALLER passes the flags the model was trained with to the engine
    (Engine.set_jk_residual / flowgnn_set_jk_residual; `host GIN --emb-dim 300 --jk sum --residual`); nothing can check them.  That
    holds for GCN too (gcn and gcn-virtual at width 300): Engine.set_jk_residual / flowgnn_set_model_jk_residual;
    `host GCN --emb-dim 300 [--ogb-vn] --jk sum --residual`.
    OGB's num_layer is read off the state_dict (num_layers_of_ogb_state_dict: the `gnn_node.convs.<l>` blocks) and sizes every per-layer
    tensor, the eps file and the virtual node's file; the file names stay the same.  A depth other than 5 is for an engine with
    flowgnn_set_num_layers(300, depth) / Engine.set_num_layers(depth) / `host GIN|GCN --emb-dim 300 --num-layer depth`; a depth outside
    2 .. 8, and a depth other than 5 at width 100, are refused before any file is written."""
    m = model.upper()
    if set2set and m not in ("GIN", "GCN"):
        raise ExportError(f"set2set=True is GIN's and GCN's (flowgnn_set_set2set_pooling); {model} has no such readout")
    if set2set and attention_pooling:
        raise ExportError("set2set=True and attention_pooling=True: a model has one readout (flowgnn_set_set2set_pooling and "
                          "flowgnn_set_attention_pooling exclude each other)")
    if S2S_KEY in sd and not set2set:
        raise ExportError(f"the state_dict has '{S2S_KEY}': it was trained with graph_pooling='set2set', and its head is 2 x emb_dim wide, "
                          f"on the LSTM's query vector; pass set2set=True (flowgnn_set_set2set_pooling; 300-wide GIN and GCN)")
    if attention_pooling and m not in ("GIN", "GCN"):
        raise ExportError(f"attention_pooling=True is GIN's and GCN's (flowgnn_set_attention_pooling); {model} has no such readout")
    if ATTN_KEY in sd and not attention_pooling:
        raise ExportError(f"the state_dict has '{ATTN_KEY}': it was trained with graph_pooling='attention', and its head on a mean readout "
                          f"is a model nobody trained; pass attention_pooling=True (flowgnn_set_attention_pooling; 300-wide GIN and GCN)")
    if int(emb_dim) != 100 and m != "GCN":
        raise ExportError(f"emb_dim={emb_dim} is GCN's keyword; {model} reads its width off the state_dict")
    if _vn_dim(virtual_node_dim) != 100 and m not in ("GIN", "GCN"):
        raise ExportError(f"virtual_node_dim={virtual_node_dim} is GIN's and GCN's (flowgnn_set_ogb_virtual_node_dim, "
                          f"flowgnn_set_gcn_virtual_node_dim); {model} has no such virtual node")
    if virtual_node and m not in ("GIN", "GCN"):
        raise ExportError(f"virtual_node=True is OGB's gin-virtual or gcn-virtual, which the engine runs as GIN or GCN (not {model})")
    depth = num_layers_of_ogb_state_dict(sd) if m in ("GIN", "GIN-VN", "GCN") else 5
    if m in ("GIN", "GIN-VN", "GCN"):  # (before any file is written; the width as the two exporters below read it)
        width = int(emb_dim) if m == "GCN" else int(_get(sd, "gnn_node.atom_encoder.atom_embedding_list.0.weight").shape[-1])
        if not _weights.MIN_NUM_LAYERS <= depth <= _weights.MAX_NUM_LAYERS:
            raise ExportError(f"the state_dict is {depth} layers deep (gnn_node.convs.*): flowgnn_set_num_layers takes "
                              f"{_weights.MIN_NUM_LAYERS} .. {_weights.MAX_NUM_LAYERS}")
        if depth != 5 and (width == 100 or m == "GIN-VN"):
            raise ExportError(f"the state_dict is {depth} layers deep (gnn_node.convs.*) and {'GIN-VN' if m == 'GIN-VN' else '100 wide'}: only the 300-wide GIN and GCN "
                              f"run a depth other than 5 (flowgnn_set_num_layers)")
    s2s = None
    if set2set:  # (before any file is written; the width: GIN's own, read off the state_dict as gin_weights_from_ogb_state_dict reads it)
        s2s = set2set_from_ogb_state_dict(sd, emb_dim=_get(sd, "gnn_node.atom_encoder.atom_embedding_list.0.weight").shape[1] if m == "GIN" else int(emb_dim))
        sd = _mean_head_zeroed(sd, s2s["w_hh"].shape[1])
    if m in ("GIN", "GIN-VN"):
        w = gin_weights_from_ogb_state_dict(sd, num_layers=depth, multi_task=multi_task, keep_eps=keep_eps, virtual_node=virtual_node,
                                            virtual_node_dim=virtual_node_dim)
        vn = gin_virtual_node_from_ogb_state_dict(sd, num_layers=depth, virtual_node_dim=virtual_node_dim) if virtual_node else None  # (before any file is written)
        gate = attention_pooling_from_ogb_state_dict(sd, emb_dim=_weights.gin_emb_dim_of(w)) if attention_pooling else None  # (likewise)
        _weights.save_gin_weights(w, directory, eps=gin_eps_from_ogb_state_dict(sd, num_layers=depth) if keep_eps else None)
        if virtual_node:
            _weights.save_gin_virtual_node(vn, directory)
        if attention_pooling:
            _weights.save_attention_pooling(gate, directory, model="GIN")
        if set2set:
            _weights.save_set2set(s2s, directory, model="GIN")
    elif m == "GCN":
        w = gcn_weights_from_ogb_state_dict(sd, num_layers=depth, multi_task=multi_task, virtual_node=virtual_node, emb_dim=emb_dim, virtual_node_dim=virtual_node_dim)
        vn = gcn_virtual_node_from_ogb_state_dict(sd, num_layers=depth, virtual_node_dim=virtual_node_dim) if virtual_node else None  # (before any file is written)
        gate = attention_pooling_from_ogb_state_dict(sd, emb_dim=int(emb_dim)) if attention_pooling else None  # (likewise)
        _weights.save_gcn_weights(w, directory)
        if virtual_node:
            _weights.save_gcn_virtual_node(vn, directory, emb_dim=int(virtual_node_dim))
        if attention_pooling:
            _weights.save_attention_pooling(gate, directory, model="GCN")
        if set2set:
            _weights.save_set2set(s2s, directory, model="GCN")
    else:
        raise ExportError(f"no OGB example model corresponds to the reference's {model} (its PNA/DGN/GAT checkpoints are already "
                          f"flat files: use flowgnn_amd.weights.save_*_weights)")
    return w


def _arr(g, name: str):
    v = g[name] if isinstance(g, Mapping) else getattr(g, name, None)
    if v is None:
        return None
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.asarray(v)


def batch_from_graphs(graphs: Iterable, with_eigen: bool = False) -> GraphBatch:
    """PyG-style graphs (`x` [N, 9] ints, `edge_index` [2, E] with both directions listed, `edge_attr` [E, 3] ints,
    optionally `eig` [N, >= 2] floats -- the DGN eigenvector file's columns) -> one GraphBatch with node ids local to each
    graph, the encoding of GIN/src/host_load.cc:100-143."""
    nn, ne, nf, el, ea, eg = [], [], [], [], [], []
    for i, g in enumerate(graphs):
        x, ei, at = _arr(g, "x"), _arr(g, "edge_index"), _arr(g, "edge_attr")
        if x is None or ei is None:
            raise ExportError(f"graph {i}: needs x and edge_index")
        if x.ndim != 2 or x.shape[1] != 9:
            raise ExportError(f"graph {i}: x is {x.shape}, the reference reads 9 integer features per node")
        if ei.ndim != 2 or ei.shape[0] != 2:
            raise ExportError(f"graph {i}: edge_index is {ei.shape}, wanted [2, E]")
        n, e = x.shape[0], ei.shape[1]
        if e and (ei.min() < 0 or ei.max() >= n):
            raise ExportError(f"graph {i}: edge_index refers to nodes outside [0, {n})")
        if at is None:
            at = np.zeros((e, 3), np.int64)
        if at.shape != (e, 3):
            raise ExportError(f"graph {i}: edge_attr is {at.shape}, wanted ({e}, 3)")
        nn.append(n); ne.append(e)
        nf.append(x.astype(np.int32)); el.append(ei.T.astype(np.int32)); ea.append(at.astype(np.int32))
        if with_eigen:
            v = _arr(g, "eig")
            if v is None or v.shape[0] != n or v.ndim != 2 or v.shape[1] < 2:
                raise ExportError(f"graph {i}: DGN needs eig [N, >= 2]")
            pad = np.zeros((n, 4), np.float32)
            pad[:, :min(4, v.shape[1])] = v[:, :4]
            eg.append(pad)
    cat = lambda xs, shp, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(shp, dt)
    return GraphBatch(np.asarray(nn, np.int32), np.asarray(ne, np.int32), cat(nf, (0, 9), np.int32), cat(el, (0, 2), np.int32),
                      cat(ea, (0, 3), np.int32), cat(eg, (0, 4), np.float32) if with_eigen else None)


def export_dataset(graphs: Iterable, root: str, eig_dir: Optional[str] = None) -> GraphBatch:
    """Write the pack `host` reads: root/graph_info/g%d_info.txt, root/graph_bin/g%d_{node_feature,edge_list,edge_attr}.bin
    (1-based), root/dataset_size.txt, and eig_dir/g%d.txt for DGN."""
    b = batch_from_graphs(graphs, with_eigen=eig_dir is not None)
    write_pack(b, root, eig_dir=eig_dir)
    return b
