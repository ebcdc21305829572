"""Weight sets in the reference's raw little-endian float32 `.bin` layouts (no header),
plus seeded synthetic weights with the same shapes and scales.

Readers follow the reference host loaders:
  GIN   nine separate files                         GIN/src/host_load.cc:24-58
  GCN   one file, hard-coded float offsets          GCN/src/host_load.cc:31-170

Every weight set is an OrderedDict whose key order is the argument order of the model's
<M>_compute_graphs entry point (include/flowgnn.h).
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Dict

import numpy as np

# name -> (file, shape); order = argument order of flowgnn_set_weights_gin / GIN_compute_graphs
GIN_FILES = OrderedDict([
    ("node_embedding_weight", ("gin_ep1_nd_embed_dim100.bin", (173, 100))),
    ("edge_embedding_weight", ("gin_ep1_ed_embed_dim100.bin", (5, 13, 100))),
    ("node_mlp_1_weights", ("gin_ep1_mlp_1_weights_dim100.bin", (5, 200, 100))),
    ("node_mlp_1_bias", ("gin_ep1_mlp_1_bias_dim100.bin", (5, 200))),
    ("node_mlp_2_weights", ("gin_ep1_mlp_2_weights_dim100.bin", (5, 100, 200))),
    ("node_mlp_2_bias", ("gin_ep1_mlp_2_bias_dim100.bin", (5, 100))),
    ("graph_pred_weights", ("gin_ep1_pred_weights_dim100.bin", (1, 100))),
    ("graph_pred_bias", ("gin_ep1_pred_bias_dim100.bin", (1,))),
])


def _read(path: str, shape, offset_floats: int = 0) -> np.ndarray:
    count = int(np.prod(shape))
    arr = np.fromfile(path, dtype="<f4", count=count, offset=4 * offset_floats)
    if arr.size != count:
        raise IOError(f"{path}: wanted {count} floats at offset {offset_floats}, got {arr.size}")
    return np.ascontiguousarray(arr.reshape(shape), dtype=np.float32)


def _task_shape(k: str, shp, num_tasks: int):
    """graph_pred_weights [NUM_TASK][D] / graph_pred_bias [NUM_TASK]: NUM_TASK is 1 in the reference (GIN/src/dcl.h:25), a
    run-time dimension here (flowgnn_set_num_tasks)."""
    if k == "graph_pred_weights":
        return (num_tasks,) + tuple(shp[1:])
    if k == "graph_pred_bias":
        return (num_tasks,)
    return tuple(shp)


NUM_LAYERS_DEFAULT, MIN_NUM_LAYERS, MAX_NUM_LAYERS = 5, 2, 8  # flowgnn.h: FLOWGNN_NUM_LAYERS_DEFAULT, FLOWGNN_MIN_NUM_LAYERS, FLOWGNN_MAX_NUM_LAYERS


def _depth(num_layers, emb_dim) -> int:
    """OGB's num_layer as the loaders and savers take it (flowgnn_set_num_layers): 2 .. 8, and 5 alone at width 100."""
    n = int(num_layers)
    if not MIN_NUM_LAYERS <= n <= MAX_NUM_LAYERS:
        raise ValueError(f"num_layers {num_layers} is outside {MIN_NUM_LAYERS} .. {MAX_NUM_LAYERS} (flowgnn_set_num_layers)")
    if n != NUM_LAYERS_DEFAULT and int(emb_dim) == 100:
        raise ValueError(f"num_layers {n} at emb_dim 100: the 100-wide kernels are five layers deep; only the 300-wide models have a "
                         f"depth other than 5 (flowgnn_set_num_layers)")
    return n


def _check_depth_of_file(path: str, fixed: int, per_layer: int, num_layers: int, shift: int = 0) -> None:
    """Refuse a file whose size is fixed + (k + shift) per_layer floats for a depth k other than num_layers: both depths are named.
    (Any other size is left to the reads, which refuse a short file.)  shift: -1 for the virtual node's files, one block per update."""
    if not os.path.exists(path) or os.path.getsize(path) % 4:
        return
    floats = os.path.getsize(path) // 4
    if floats == fixed + (num_layers + shift) * per_layer:
        return
    for k in range(MIN_NUM_LAYERS, MAX_NUM_LAYERS + 1):
        if floats == fixed + (k + shift) * per_layer:
            raise ValueError(f"{path} holds the tensors of a model {k} layers deep, and num_layers is {num_layers} (flowgnn_set_num_layers)")


GIN_EMB_DIMS = (100, 300)  # the reference's width, and OGB's default (flowgnn_set_emb_dim: FLOWGNN_EMB_DIM_REFERENCE / _OGB)


_GIN_PER_LAYER = ("edge_embedding_weight", "node_mlp_1_weights", "node_mlp_1_bias", "node_mlp_2_weights", "node_mlp_2_bias")


def gin_files(emb_dim: int = 100, num_layers: int = 5):
    """GIN_FILES at width emb_dim and depth num_layers: the reference's names with dim<emb_dim> in place of dim100 (the depth is not in
    a name), the shapes with 100 -> D, 200 -> 2 D and the leading 5 of the per-layer tensors -> num_layers."""
    d = int(emb_dim)
    if d not in GIN_EMB_DIMS:
        raise ValueError(f"GIN: emb_dim {emb_dim} is not one of {GIN_EMB_DIMS}")
    n = _depth(num_layers, d)
    grow = {100: d, 200: 2 * d}
    out = OrderedDict()
    for k, (f, shp) in GIN_FILES.items():
        wide = tuple(grow.get(x, x) for x in shp)
        out[k] = (f.replace("dim100", f"dim{d}"), (n,) + wide[1:] if k in _GIN_PER_LAYER else wide)
    return out


def gin_num_layers_of(w) -> int:
    """The depth of a GIN or GCN weight set: the leading dimension of its per-layer edge table."""
    return int(np.asarray(w["edge_embedding_weight"]).shape[0])


def gin_emb_dim_of(w) -> int:
    """The width of a GIN weight set: the row length of its atom-embedding table."""
    return int(np.asarray(w["node_embedding_weight"]).shape[-1])


def load_gin_weights(directory: str, num_tasks: int = 1, emb_dim: int = 100, num_layers: int = 5) -> Dict[str, np.ndarray]:
    """num_layers: the depth the files were written for (flowgnn_set_num_layers); a per-layer file of another depth is refused."""
    files = gin_files(emb_dim, num_layers)
    for k in _GIN_PER_LAYER:
        _check_depth_of_file(os.path.join(directory, files[k][0]), 0, int(np.prod(files[k][1][1:])), int(num_layers))
    return OrderedDict((k, _read(os.path.join(directory, f), _task_shape(k, shp, num_tasks))) for k, (f, shp) in files.items())


GIN_EPS_FILE = "gin_ep1_eps_dim100.bin"  # five LE float32, one per layer: read by the reference host and never used


def gin_eps_file(emb_dim: int = 100) -> str:
    return GIN_EPS_FILE.replace("dim100", f"dim{int(emb_dim)}")


def load_gin_eps(directory: str, emb_dim: int = 100, num_layers: int = 5) -> np.ndarray:
    """The eps values of a GIN / GIN-VN weights directory, float32[num_layers] -- five unless the depth says otherwise (for
    Engine.set_gin_eps: flowgnn_set_gin_eps); a file of another depth is refused."""
    n = _depth(num_layers, emb_dim)
    path = os.path.join(directory, gin_eps_file(emb_dim))
    _check_depth_of_file(path, 0, 1, n)
    return _read(path, (n,))


def save_gin_weights(w: Dict[str, np.ndarray], directory: str, eps=None, emb_dim=None, num_layers=None) -> None:
    """eps: the trained values, one per layer, for the eps file (None: zeros, what the reference's own sets carry).  Nothing applies the
    file unless asked to: `host --eps`, Engine.load_weights_dir(dir, eps=True).  emb_dim: None = the arrays' own width (which names the
    files: dim100 / dim300).  num_layers: None = the arrays' own depth; a number must agree with it."""
    tasks = int(np.asarray(w["graph_pred_bias"]).size)
    d = gin_emb_dim_of(w) if emb_dim is None else int(emb_dim)
    n = gin_num_layers_of(w)
    if num_layers is not None and int(num_layers) != n:
        raise ValueError(f"GIN: the tensors are {n} layers deep, num_layers says {num_layers}")
    files = gin_files(d, n)  # (a depth that does not exist is refused before anything is created)
    os.makedirs(directory, exist_ok=True)
    for k, (f, shp) in files.items():
        np.asarray(w[k], dtype="<f4").reshape(_task_shape(k, shp, tasks)).tofile(os.path.join(directory, f))
    e = np.zeros(n, dtype="<f4") if eps is None else np.asarray(eps, dtype="<f4").reshape(n)
    e.tofile(os.path.join(directory, gin_eps_file(d)))  # (zeros: read by the reference, never used)


# OGB's virtual node for GIN (flowgnn.h: flowgnn_set_ogb_virtual_node): one file beside the GIN set, the five tensors in the order of the
# C call's arguments, BatchNorms folded; name -> shape
GIN_VIRTUAL_NODE_FILE = "gin_ep1_virtualnode_dim100.bin"
GIN_VIRTUAL_NODE_SHAPES = OrderedDict([
    ("vn_embedding", (100,)), ("w1", (4, 200, 100)), ("b1", (4, 200)), ("w2", (4, 100, 200)), ("b2", (4, 100)),
])
GIN_VIRTUAL_NODE_FLOATS = sum(int(np.prod(s)) for s in GIN_VIRTUAL_NODE_SHAPES.values())  # 161 300


def gin_virtual_node_shapes(emb_dim: int = 100, num_layers: int = 5):
    """GIN_VIRTUAL_NODE_SHAPES at width emb_dim (flowgnn_set_ogb_virtual_node_dim): 100 -> D, 200 -> 2 D; and at depth num_layers
    (flowgnn_set_num_layers): the leading 4 of the four per-update tensors -> num_layers - 1."""
    d = int(emb_dim)
    if d not in GIN_EMB_DIMS:
        raise ValueError(f"virtual node: emb_dim {emb_dim} is not one of {GIN_EMB_DIMS}")
    u = _depth(num_layers, d) - 1
    grow = {100: d, 200: 2 * d}
    return OrderedDict((k, tuple(grow.get(n, n) for n in shp) if k == "vn_embedding" else (u,) + tuple(grow.get(n, n) for n in shp[1:]))
                       for k, shp in GIN_VIRTUAL_NODE_SHAPES.items())


def gin_virtual_node_num_layers_of(vn) -> int:
    """The depth a virtual node's tensors belong to: its updates (the rows of b2) + 1."""
    return int(np.asarray(vn["b2"]).size) // gin_virtual_node_dim_of(vn) + 1


def gin_virtual_node_file(emb_dim: int = 100) -> str:
    """gin_ep1_virtualnode_dim<emb_dim>.bin"""
    gin_virtual_node_shapes(emb_dim)  # (refuses a width that does not exist)
    return GIN_VIRTUAL_NODE_FILE.replace("dim100", f"dim{int(emb_dim)}")


def gin_virtual_node_dim_of(vn) -> int:
    """The width of a virtual node's tensors: the size of its embedding row."""
    return int(np.asarray(vn["vn_embedding"]).size)


def checked_gin_virtual_node(vn, emb_dims=GIN_EMB_DIMS, num_layers=None) -> Dict[str, np.ndarray]:
    """The dict `vn` with exactly the five keys, each as a contiguous float32 array of its shape at the width read off vn_embedding's
    size, which must be one of emb_dims (GCN's callers pass (100,): its call has no wider form).  num_layers: the depth the tensors
    must have (the engine's: it reads num_layers - 1 updates); None = the tensors' own, read off b2."""
    if set(vn) != set(GIN_VIRTUAL_NODE_SHAPES):
        raise ValueError(f"virtual node: wanted the keys {list(GIN_VIRTUAL_NODE_SHAPES)}, got {sorted(vn)}")
    d = gin_virtual_node_dim_of(vn)
    if d not in tuple(emb_dims):
        raise ValueError(f"virtual node: vn_embedding is {np.asarray(vn['vn_embedding']).shape}, wanted a row of one of the widths {tuple(emb_dims)}")
    out = OrderedDict()
    for k, shp in gin_virtual_node_shapes(d, gin_virtual_node_num_layers_of(vn) if num_layers is None else num_layers).items():
        a = np.asarray(vn[k], dtype=np.float32)
        if a.size != int(np.prod(shp)):
            raise ValueError(f"virtual node: {k} is {a.shape}, wanted {shp}")
        out[k] = np.ascontiguousarray(a.reshape(shp))
    return out


def save_gin_virtual_node(vn, directory: str, emb_dim=None) -> None:
    """Write gin_ep1_virtualnode_dim<D>.bin: vn_embedding, w1, b1, w2, b2 end to end, little-endian float32.  emb_dim: None = the
    tensors' own width (which names the file); a width the tensors do not have is refused.  Nothing applies the file unless asked to:
    `host GIN --ogb-vn`, Engine.load_weights_dir(dir, virtual_node=True)."""
    vn = checked_gin_virtual_node(vn)
    d = gin_virtual_node_dim_of(vn)
    if emb_dim is not None and int(emb_dim) != d:
        raise ValueError(f"virtual node: the tensors are {d} wide, emb_dim says {emb_dim}")
    os.makedirs(directory, exist_ok=True)
    flat = np.concatenate([a.ravel() for a in vn.values()]).astype("<f4")
    flat.tofile(os.path.join(directory, gin_virtual_node_file(d)))


def load_gin_virtual_node(directory: str, emb_dim: int = 100, num_layers: int = 5) -> Dict[str, np.ndarray]:
    """The five tensors of a directory's virtual-node file of width emb_dim (for Engine.set_ogb_virtual_node); a short file is refused."""
    path = os.path.join(directory, gin_virtual_node_file(emb_dim))
    d = int(emb_dim)
    _check_depth_of_file(path, d, 4 * d * d + 3 * d, _depth(num_layers, d), shift=-1)  # (per update: w1, w2, b1, b2; a file of another depth is refused)
    out, at = OrderedDict(), 0
    for k, shp in gin_virtual_node_shapes(emb_dim, num_layers).items():
        out[k] = _read(path, shp, at)
        at += int(np.prod(shp))
    return out


def synth_gin_virtual_node(seed: int = 11, scale: float = 1.0, emb_dim: int = 100, num_layers: int = 5) -> Dict[str, np.ndarray]:
    """Random virtual-node tensors at the scales of synth_gin_weights' MLP (the virtual node's MLP has the node MLP's shapes).
    emb_dim 300: the matrices' scales shrink with sqrt(100 / emb_dim), as synth_gin_weights' do (at 100 the values are what they
    always were)."""
    rng = np.random.default_rng(seed)
    s = {"vn_embedding": 0.11, "w1": 0.075, "b1": 0.91, "w2": 0.053, "b2": 0.49}
    if emb_dim != 100:
        for k in ("w1", "w2"):
            s[k] = s[k] * float(np.sqrt(100.0 / emb_dim))
    return OrderedDict((k, (rng.standard_normal(shp) * s[k] * scale).astype(np.float32)) for k, shp in gin_virtual_node_shapes(emb_dim, num_layers).items())


# ... and for GCN (flowgnn.h: flowgnn_set_gcn_virtual_node): the same five tensors in the same order, one file beside the GCN file
GCN_VIRTUAL_NODE_FILE = "gcn_ep1_virtualnode_dim100.bin"


def gcn_virtual_node_file(emb_dim: int = 100) -> str:
    """gcn_ep1_virtualnode_dim<emb_dim>.bin"""
    gin_virtual_node_shapes(emb_dim)  # (refuses a width that does not exist)
    return GCN_VIRTUAL_NODE_FILE.replace("dim100", f"dim{int(emb_dim)}")


def save_gcn_virtual_node(vn, directory: str, emb_dim: int = 100) -> None:
    """Write gcn_ep1_virtualnode_dim<emb_dim>.bin, as save_gin_virtual_node writes GIN's.  The width is the keyword's, 100 unless it
    says 300 (flowgnn_set_gcn_virtual_node_dim): tensors of another width are refused before anything is created.  Nothing applies
    the file unless asked to: `host GCN --ogb-vn`, Engine.load_weights_dir(dir, virtual_node=True)."""
    name = gcn_virtual_node_file(emb_dim)
    flat = np.concatenate([a.ravel() for a in checked_gin_virtual_node(vn, emb_dims=(int(emb_dim),)).values()]).astype("<f4")  # (refused before anything is created)
    os.makedirs(directory, exist_ok=True)
    flat.tofile(os.path.join(directory, name))


def load_gcn_virtual_node(directory: str, emb_dim: int = 100, num_layers: int = 5) -> Dict[str, np.ndarray]:
    """The five tensors of a directory's GCN virtual-node file of width emb_dim (for Engine.set_gcn_virtual_node); a short file is refused."""
    path = os.path.join(directory, gcn_virtual_node_file(emb_dim))
    d = int(emb_dim)
    _check_depth_of_file(path, d, 4 * d * d + 3 * d, _depth(num_layers, d), shift=-1)  # (per update: w1, w2, b1, b2; a file of another depth is refused)
    out, at = OrderedDict(), 0
    for k, shp in gin_virtual_node_shapes(emb_dim, num_layers).items():
        out[k] = _read(path, shp, at)
        at += int(np.prod(shp))
    return out


def synth_gcn_virtual_node(seed: int = 13, scale: float = 1.0, emb_dim: int = 100, num_layers: int = 5) -> Dict[str, np.ndarray]:
    """Random virtual-node tensors for GCN: synth_gin_virtual_node's scales (the MLP is the same), another seed."""
    return synth_gin_virtual_node(seed=seed, scale=scale, emb_dim=emb_dim, num_layers=num_layers)


# OGB's attention readout for GIN and GCN at width 300 (flowgnn.h: flowgnn_set_attention_pooling): one file beside the model's set, the
# gate's three tensors in the order of the C call's arguments, its BatchNorm folded; the last Linear's bias cancels in the softmax and
# is not stored
ATTENTION_POOLING_KEYS = ("w1", "b1", "w2")
ATTENTION_POOLING_EMB_DIMS = (300,)
_ATTENTION_POOLING_PREFIX = {"GIN": "gin", "GCN": "gcn"}


def attention_pooling_shapes(emb_dim: int = 300, emb_dims=ATTENTION_POOLING_EMB_DIMS):
    """w1 [2D][D], b1 [2D], w2 [2D] at D = emb_dim, one of emb_dims (the files exist at 300 alone; the C call takes 100-wide tensors
    too, to refuse them by name)."""
    d = int(emb_dim)
    if d not in tuple(emb_dims):
        raise ValueError(f"attention pooling: emb_dim {emb_dim} is not one of {tuple(emb_dims)} (only the 300-wide models have this readout)")
    return OrderedDict([("w1", (2 * d, d)), ("b1", (2 * d,)), ("w2", (2 * d,))])


def attention_pooling_file(model: str = "GIN", emb_dim: int = 300) -> str:
    """gin_ep1_attnpool_dim<emb_dim>.bin / gcn_ep1_attnpool_dim<emb_dim>.bin"""
    attention_pooling_shapes(emb_dim)  # (refuses a width that does not exist)
    if model not in _ATTENTION_POOLING_PREFIX:
        raise ValueError(f"attention pooling: model {model!r} is not one of {sorted(_ATTENTION_POOLING_PREFIX)}")
    return f"{_ATTENTION_POOLING_PREFIX[model]}_ep1_attnpool_dim{int(emb_dim)}.bin"


def checked_attention_pooling(gate) -> Dict[str, np.ndarray]:
    """The dict `gate` with exactly the keys w1, b1, w2, each as a contiguous float32 array of its shape at the width read off w1."""
    if set(gate) != set(ATTENTION_POOLING_KEYS):
        raise ValueError(f"attention pooling: wanted the keys {list(ATTENTION_POOLING_KEYS)}, got {sorted(gate)}")
    w1 = np.asarray(gate["w1"])
    if w1.ndim != 2 or w1.shape[0] != 2 * w1.shape[1]:
        raise ValueError(f"attention pooling: w1 is {w1.shape}, wanted [2D][D]")
    out = OrderedDict()
    for k, shp in attention_pooling_shapes(w1.shape[1], emb_dims=GIN_EMB_DIMS).items():
        a = np.asarray(gate[k], dtype=np.float32)
        if a.size != int(np.prod(shp)):
            raise ValueError(f"attention pooling: {k} is {a.shape}, wanted {shp}")
        out[k] = np.ascontiguousarray(a.reshape(shp))
    return out


def save_attention_pooling(gate, directory: str, model: str = "GIN") -> None:
    """Write <model>_ep1_attnpool_dim300.bin: w1, b1, w2 end to end, little-endian float32 (181 200 of them).  Nothing applies the file
    unless asked to: `host GIN|GCN --emb-dim 300 --attn-pool`, Engine.load_weights_dir(dir, attention_pooling=True)."""
    gate = checked_attention_pooling(gate)
    name = attention_pooling_file(model, gate["w1"].shape[1])  # (refused before anything is created)
    os.makedirs(directory, exist_ok=True)
    np.concatenate([a.ravel() for a in gate.values()]).astype("<f4").tofile(os.path.join(directory, name))


def load_attention_pooling(directory: str, model: str = "GIN", emb_dim: int = 300) -> Dict[str, np.ndarray]:
    """The three tensors of a directory's attention-pooling file (for Engine.set_attention_pooling); a short file is refused."""
    path = os.path.join(directory, attention_pooling_file(model, emb_dim))
    out, at = OrderedDict(), 0
    for k, shp in attention_pooling_shapes(emb_dim).items():
        out[k] = _read(path, shp, at)
        at += int(np.prod(shp))
    return out


def synth_attention_pooling(seed: int = 11, emb_dim: int = 300) -> Dict[str, np.ndarray]:
    """Random gate tensors: w1 = N(0,1) / sqrt(D), b1 = 0.5 N(0,1), w2 = 8 N(0,1) / sqrt(2D), drawn in this order from one
    default_rng(seed) -- gates that spread by a few units inside a molecule, so that the softmax is far from the mean."""
    d = int(emb_dim)
    rng = np.random.default_rng(seed)
    w1 = (rng.standard_normal((2 * d, d)) / np.sqrt(d)).astype(np.float32)
    b1 = (0.5 * rng.standard_normal(2 * d)).astype(np.float32)
    w2 = (8.0 * rng.standard_normal(2 * d) / np.sqrt(2 * d)).astype(np.float32)
    return OrderedDict([("w1", w1), ("b1", b1), ("w2", w2)])


# OGB's set2set readout for GIN and GCN at width 300 (flowgnn.h: flowgnn_set_set2set_pooling): one file beside the model's set, PyG's
# Set2Set LSTM (pool.lstm.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0; gate order i, f, g, o) and OGB's Linear(2D, NUM_TASK) head,
# in the order of the C call's arguments.  The number of processing steps is no tensor: it is given where the file is applied
SET2SET_KEYS = ("w_ih", "w_hh", "b_ih", "b_hh", "head_w", "head_b")
SET2SET_EMB_DIMS = (300,)
_SET2SET_PREFIX = {"GIN": "gin", "GCN": "gcn"}


def set2set_shapes(emb_dim: int = 300, num_tasks: int = 1, emb_dims=SET2SET_EMB_DIMS):
    """w_ih [4D][2D], w_hh [4D][D], b_ih [4D], b_hh [4D], head_w [T][2D], head_b [T] at D = emb_dim, one of emb_dims (the files exist
    at 300 alone; the C call takes 100-wide tensors too, to refuse them by name), T = num_tasks."""
    d, t = int(emb_dim), int(num_tasks)
    if d not in tuple(emb_dims):
        raise ValueError(f"set2set: emb_dim {emb_dim} is not one of {tuple(emb_dims)} (only the 300-wide models have this readout)")
    if t < 1:
        raise ValueError(f"set2set: num_tasks is {num_tasks}, wanted at least 1")
    return OrderedDict([("w_ih", (4 * d, 2 * d)), ("w_hh", (4 * d, d)), ("b_ih", (4 * d,)), ("b_hh", (4 * d,)), ("head_w", (t, 2 * d)), ("head_b", (t,))])


def set2set_file(model: str = "GIN", emb_dim: int = 300) -> str:
    """gin_ep1_set2set_dim<emb_dim>.bin / gcn_ep1_set2set_dim<emb_dim>.bin"""
    set2set_shapes(emb_dim)  # (refuses a width that does not exist)
    if model not in _SET2SET_PREFIX:
        raise ValueError(f"set2set: model {model!r} is not one of {sorted(_SET2SET_PREFIX)}")
    return f"{_SET2SET_PREFIX[model]}_ep1_set2set_dim{int(emb_dim)}.bin"


def checked_set2set(s2s) -> Dict[str, np.ndarray]:
    """The dict `s2s` with exactly the keys of SET2SET_KEYS, each as a contiguous float32 array of its shape, the width read off w_hh
    and NUM_TASK off head_b."""
    if set(s2s) != set(SET2SET_KEYS):
        raise ValueError(f"set2set: wanted the keys {list(SET2SET_KEYS)}, got {sorted(s2s)}")
    w_hh = np.asarray(s2s["w_hh"])
    if w_hh.ndim != 2 or w_hh.shape[0] != 4 * w_hh.shape[1]:
        raise ValueError(f"set2set: w_hh is {w_hh.shape}, wanted [4D][D]")
    out = OrderedDict()
    for k, shp in set2set_shapes(w_hh.shape[1], max(1, np.asarray(s2s["head_b"]).size), emb_dims=GIN_EMB_DIMS).items():
        a = np.asarray(s2s[k], dtype=np.float32)
        if a.size != int(np.prod(shp)):
            raise ValueError(f"set2set: {k} is {a.shape}, wanted {shp}")
        out[k] = np.ascontiguousarray(a.reshape(shp))
    return out


def save_set2set(s2s, directory: str, model: str = "GIN") -> None:
    """Write <model>_ep1_set2set_dim300.bin: the six tensors end to end, little-endian float32.  Nothing applies the file unless asked
    to: `host GIN|GCN --emb-dim 300 --set2set`, Engine.load_weights_dir(dir, set2set=True)."""
    s2s = checked_set2set(s2s)
    name = set2set_file(model, s2s["w_hh"].shape[1])  # (refused before anything is created)
    os.makedirs(directory, exist_ok=True)
    np.concatenate([a.ravel() for a in s2s.values()]).astype("<f4").tofile(os.path.join(directory, name))


def load_set2set(directory: str, model: str = "GIN", emb_dim: int = 300) -> Dict[str, np.ndarray]:
    """The six tensors of a directory's set2set file (for Engine.set_set2set_pooling).  NUM_TASK is read off the file's length: the
    LSTM takes 4D (3D + 2) floats and every task 2D + 1 more; another length is refused."""
    path = os.path.join(directory, set2set_file(model, emb_dim))
    d = int(emb_dim)
    floats, lstm = os.path.getsize(path) // 4, 4 * d * (3 * d + 2)
    t = (floats - lstm) // (2 * d + 1)
    if os.path.getsize(path) % 4 or t < 1 or lstm + t * (2 * d + 1) != floats:
        raise ValueError(f"{path}: {os.path.getsize(path)} bytes are not {lstm} + NUM_TASK x {2 * d + 1} little-endian float32")
    out, at = OrderedDict(), 0
    for k, shp in set2set_shapes(d, t).items():
        out[k] = _read(path, shp, at)
        at += int(np.prod(shp))
    return out


def synth_set2set(seed: int = 17, emb_dim: int = 300, num_tasks: int = 1) -> Dict[str, np.ndarray]:
    """Random set2set tensors, drawn in the order of SET2SET_KEYS from one default_rng(seed): the two matrices U(-1/sqrt(D), 1/sqrt(D)),
    torch's initialisation of an LSTM; both biases U(-1/sqrt(D), 1/sqrt(D)) + 0.3 N(0, 1), so that the gates are not all near 1/2;
    head_w = 0.15 N(0, 1) sqrt(100 / D) and head_b = 0.12 N(0, 1), the scales of synth_gin_weights' head."""
    d, t = int(emb_dim), int(num_tasks)
    rng = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(d)
    w_ih = rng.uniform(-k, k, (4 * d, 2 * d)).astype(np.float32)
    w_hh = rng.uniform(-k, k, (4 * d, d)).astype(np.float32)
    b_ih = (rng.uniform(-k, k, 4 * d) + 0.3 * rng.standard_normal(4 * d)).astype(np.float32)
    b_hh = (rng.uniform(-k, k, 4 * d) + 0.3 * rng.standard_normal(4 * d)).astype(np.float32)
    head_w = (0.15 * rng.standard_normal((t, 2 * d)) * np.sqrt(100.0 / d)).astype(np.float32)
    head_b = (0.12 * rng.standard_normal(t)).astype(np.float32)
    return OrderedDict([("w_ih", w_ih), ("w_hh", w_hh), ("b_ih", b_ih), ("b_hh", b_hh), ("head_w", head_w), ("head_b", head_b)])


def synth_gin_weights(seed: int = 7, num_tasks: int = 1, emb_dim: int = 100, num_layers: int = 5) -> Dict[str, np.ndarray]:
    """Random weights with the measured scales of the shipped GIN set:
    W1 s=0.075, b1 s=0.91, W2 s=0.053, b2 s=0.49, node/edge emb s=0.11/0.14, pred s=0.15.
    emb_dim 300: the same scales at OGB's default width, the matrices' scales shrunk by sqrt(100 / emb_dim) so that the activations
    keep their size (the draws, and at 100 the values, are what they always were)."""
    rng = np.random.default_rng(seed)
    scale = {
        "node_embedding_weight": 0.11, "edge_embedding_weight": 0.14,
        "node_mlp_1_weights": 0.075, "node_mlp_1_bias": 0.91,
        "node_mlp_2_weights": 0.053, "node_mlp_2_bias": 0.49,
        "graph_pred_weights": 0.15, "graph_pred_bias": 0.12,
    }
    if emb_dim != 100:
        for k in ("node_mlp_1_weights", "node_mlp_2_weights", "graph_pred_weights"):
            scale[k] = scale[k] * float(np.sqrt(100.0 / emb_dim))
    return OrderedDict((k, (rng.standard_normal(_task_shape(k, shp, num_tasks)) * scale[k]).astype(np.float32))
                       for k, (_, shp) in gin_files(emb_dim, num_layers).items())


# --------------------------------------------------------------------------- GCN
GCN_FILE = "gcn_ep1_dim100.weights.all.bin"
GCN_SHAPES = OrderedDict([
    ("node_embedding_weight", (173, 100)), ("edge_embedding_weight", (5, 13, 100)),
    ("convs_weight", (5, 100, 100)), ("convs_bias", (5, 100)), ("convs_root_emb_weight", (5, 100)),
    ("bn_weight", (5, 100)), ("bn_bias", (5, 100)), ("bn_mean", (5, 100)), ("bn_var", (5, 100)),
    ("graph_pred_weights", (1, 100)), ("graph_pred_bias", (1,)),
])
GCN_EMB_DIMS = (100, 300)  # the reference's width, and OGB's default (flowgnn_set_model_emb_dim: FLOWGNN_EMB_DIM_REFERENCE / _OGB)


def _gcn_dim(emb_dim) -> int:
    d = int(emb_dim)
    if d not in GCN_EMB_DIMS:
        raise ValueError(f"GCN: emb_dim {emb_dim} is not one of {GCN_EMB_DIMS}")
    return d


def gcn_file(emb_dim: int = 100) -> str:
    """gcn_ep1_dim<emb_dim>.weights.all.bin: the reference's one file, with D for 100 in every offset."""
    return GCN_FILE.replace("dim100", f"dim{_gcn_dim(emb_dim)}")


_GCN_WHOLE = ("node_embedding_weight", "graph_pred_weights", "graph_pred_bias")  # every other tensor is per layer


def gcn_shapes(emb_dim: int = 100, num_layers: int = 5):
    """GCN_SHAPES at width emb_dim: 100 -> D; and at depth num_layers (flowgnn_set_num_layers): the leading 5 of the per-layer tensors."""
    d = _gcn_dim(emb_dim)
    n = _depth(num_layers, d)
    return OrderedDict((k, tuple(d if x == 100 else x for x in shp) if k in _GCN_WHOLE else (n,) + tuple(d if x == 100 else x for x in shp[1:]))
                       for k, shp in GCN_SHAPES.items())


def gcn_emb_dim_of(w) -> int:
    """The width of a GCN weight set: the node table's second dimension."""
    return int(np.asarray(w["node_embedding_weight"]).shape[-1])


def _gcn_offsets(num_tasks: int = 1, emb_dim: int = 100, num_layers: int = 5):
    """(name, layer or None) -> float offset in the .all.bin (GCN/src/host_load.cc:34-170, D for 100): node table at 0, layer l at
    173 D + l (D^2 + 15 D), BatchNorm l at 173 D + 5 (D^2 + 15 D) + l (4 D + 1); the head is the last tensor pair of the flattened
    state_dict: weight [NUM_TASK][D] at 173 D + 5 (D^2 + 15 D) + 5 (4 D + 1), bias [NUM_TASK] right behind it.  At D = 100 these are
    17300, 11500, 74800 and 76805.  num_layers: L for every 5 above (flowgnn_set_num_layers) -- the BatchNorm blocks and the head move."""
    d, L = int(emb_dim), int(num_layers)
    layer = d * d + 15 * d
    bn0 = 173 * d + L * layer
    head = bn0 + L * (4 * d + 1)
    off = {("node_embedding_weight", None): 0, ("graph_pred_weights", None): head, ("graph_pred_bias", None): head + d * num_tasks}
    for l in range(L):
        base = 173 * d + layer * l
        off[("convs_weight", l)] = base
        off[("convs_bias", l)] = base + d * d
        off[("convs_root_emb_weight", l)] = base + d * d + d
        off[("edge_embedding_weight", l)] = base + d * d + 2 * d
        bn = bn0 + (4 * d + 1) * l  # 4 x D floats, then one skipped counter (num_batches_tracked)
        off[("bn_weight", l)] = bn
        off[("bn_bias", l)] = bn + d
        off[("bn_mean", l)] = bn + 2 * d
        off[("bn_var", l)] = bn + 3 * d
    return off


def load_gcn_weights(directory: str, num_tasks: int = 1, emb_dim: int = 100, num_layers: int = 5) -> Dict[str, np.ndarray]:
    """num_layers: the depth the file was written for (flowgnn_set_num_layers): every offset behind the layers depends on it, so a file
    whose size is that of another depth is refused."""
    path = os.path.join(directory, gcn_file(emb_dim))
    d, n = _gcn_dim(emb_dim), _depth(num_layers, emb_dim)
    _check_depth_of_file(path, 173 * d + (d + 1) * int(num_tasks), d * d + 15 * d + 4 * d + 1, n)
    off = _gcn_offsets(num_tasks, emb_dim, n)
    w = OrderedDict()
    for k, shp in gcn_shapes(emb_dim, n).items():
        if (k, None) in off:
            w[k] = _read(path, _task_shape(k, shp, num_tasks), off[(k, None)])
        else:
            w[k] = np.stack([_read(path, shp[1:], off[(k, l)]) for l in range(n)])
    return w


def save_gcn_weights(w: Dict[str, np.ndarray], directory: str, emb_dim=None, num_layers=None) -> None:
    """emb_dim: None = the arrays' own width (which names the file); a number must agree with it.  num_layers: likewise the depth."""
    d = gcn_emb_dim_of(w)
    if emb_dim is not None and int(emb_dim) != d:
        raise ValueError(f"GCN: the tensors are {d} wide, emb_dim says {emb_dim}")
    n = gin_num_layers_of(w)
    if num_layers is not None and int(num_layers) != n:
        raise ValueError(f"GCN: the tensors are {n} layers deep, num_layers says {num_layers}")
    shapes = gcn_shapes(d, n)  # (a depth that does not exist is refused before anything is created)
    os.makedirs(directory, exist_ok=True)
    tasks = int(np.asarray(w["graph_pred_bias"]).size)
    off = _gcn_offsets(tasks, d, n)
    buf = np.zeros(off[("graph_pred_weights", None)] + (d + 1) * tasks, dtype="<f4")
    for k, shp in shapes.items():
        a = np.asarray(w[k], dtype=np.float32).reshape(_task_shape(k, shp, tasks))
        if (k, None) in off:
            buf[off[(k, None)]:off[(k, None)] + a.size] = a.ravel()
        else:
            for l in range(n):
                buf[off[(k, l)]:off[(k, l)] + a[l].size] = a[l].ravel()
    buf.tofile(os.path.join(directory, gcn_file(d)))


def synth_gcn_weights(seed: int = 7, num_tasks: int = 1, emb_dim: int = 100, num_layers: int = 5) -> Dict[str, np.ndarray]:
    """emb_dim 300: the same scales at OGB's default width, convs_weight shrunk by sqrt(100 / emb_dim) so that the activations keep
    the size they have at 100 (at 100 the values are what they always were)."""
    rng = np.random.default_rng(seed)
    scale = {"node_embedding_weight": 0.11, "edge_embedding_weight": 0.14, "convs_weight": 0.09, "convs_bias": 0.1,
             "convs_root_emb_weight": 0.3, "bn_weight": 0.2, "bn_bias": 0.2, "bn_mean": 0.3,
             "graph_pred_weights": 0.15, "graph_pred_bias": 0.12}
    if emb_dim != 100:
        scale["convs_weight"] = scale["convs_weight"] * float(np.sqrt(100.0 / emb_dim))
    w = OrderedDict()
    for k, shp in gcn_shapes(emb_dim, num_layers).items():
        shp = _task_shape(k, shp, num_tasks)
        if k == "bn_var":
            w[k] = rng.uniform(0.3, 1.5, shp).astype(np.float32)
        elif k == "bn_weight":
            w[k] = (1.0 + rng.standard_normal(shp) * scale[k]).astype(np.float32)
        else:
            w[k] = (rng.standard_normal(shp) * scale[k]).astype(np.float32)
    return w


# --------------------------------------------------------------------------- PNA
PNA_FILE = "pna_ep1_noBN_dim80.weights.all.bin"
PNA_AVG_DEG = 6.885701656341553  # PNA/src/host_load.cc:127 (host constant, not in the file)
PNA_SHAPES = OrderedDict([
    ("node_embedding_weight", (173, 80)), ("node_conv_weights", (4, 80, 3, 4, 80)), ("node_conv_bias", (4, 80)),
    ("graph_mlp_1_weights", (40, 80)), ("graph_mlp_1_bias", (40,)), ("graph_mlp_2_weights", (20, 40)),
    ("graph_mlp_2_bias", (20,)), ("graph_mlp_3_weights", (1, 20)), ("graph_mlp_3_bias", (1,)), ("avg_deg", (1,)),
])
_PNA_TAIL = OrderedDict([("graph_mlp_1_weights", 321360), ("graph_mlp_1_bias", 324560), ("graph_mlp_2_weights", 324600),
                         ("graph_mlp_2_bias", 325400), ("graph_mlp_3_weights", 325420), ("graph_mlp_3_bias", 325440)])


def load_pna_weights(directory: str) -> Dict[str, np.ndarray]:
    """PNA/src/host_load.cc:23-68: node_emb at 0, layer l weights at 13840 + 76880 l (76800) + bias (80)."""
    path = os.path.join(directory, PNA_FILE)
    w = OrderedDict()
    w["node_embedding_weight"] = _read(path, (173, 80), 0)
    w["node_conv_weights"] = np.stack([_read(path, (80, 3, 4, 80), 13840 + 76880 * l) for l in range(4)])
    w["node_conv_bias"] = np.stack([_read(path, (80,), 13840 + 76880 * l + 76800) for l in range(4)])
    for k, off in _PNA_TAIL.items():
        w[k] = _read(path, PNA_SHAPES[k], off)
    w["avg_deg"] = np.array([PNA_AVG_DEG], dtype=np.float32)
    return w


def save_pna_weights(w: Dict[str, np.ndarray], directory: str) -> None:
    os.makedirs(directory, exist_ok=True)
    buf = np.zeros(325441, dtype="<f4")
    buf[0:13840] = np.asarray(w["node_embedding_weight"], np.float32).ravel()
    for l in range(4):
        base = 13840 + 76880 * l
        buf[base:base + 76800] = np.asarray(w["node_conv_weights"], np.float32)[l].ravel()
        buf[base + 76800:base + 76880] = np.asarray(w["node_conv_bias"], np.float32)[l].ravel()
    for k, off in _PNA_TAIL.items():
        a = np.asarray(w[k], np.float32).ravel()
        buf[off:off + a.size] = a
    buf.tofile(os.path.join(directory, PNA_FILE))


def synth_pna_weights(seed: int = 7) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    scale = {"node_embedding_weight": 0.11, "node_conv_weights": 0.012, "node_conv_bias": 0.1, "graph_mlp_1_weights": 0.1,
             "graph_mlp_1_bias": 0.1, "graph_mlp_2_weights": 0.15, "graph_mlp_2_bias": 0.1, "graph_mlp_3_weights": 0.2,
             "graph_mlp_3_bias": 0.1}
    w = OrderedDict((k, (rng.standard_normal(shp) * scale[k]).astype(np.float32)) for k, shp in PNA_SHAPES.items()
                    if k != "avg_deg")
    w["avg_deg"] = np.array([PNA_AVG_DEG], dtype=np.float32)
    return w


# --------------------------------------------------------------------------- DGN
DGN_FILE = "dgn_ep1_noBN_dim100.weights.all.bin"
DGN_SHAPES = OrderedDict([
    ("embedding_h_atom_embedding_list_weights", (9, 119, 100)),
    ("layers_posttrans_fully_connected_0_linear_weight", (4, 100, 200)),
    ("layers_posttrans_fully_connected_0_linear_bias", (4, 100)),
    ("MLP_layer_FC_layers_0_weight", (50, 100)), ("MLP_layer_FC_layers_0_bias", (50,)),
    ("MLP_layer_FC_layers_1_weight", (25, 50)), ("MLP_layer_FC_layers_1_bias", (25,)),
    ("MLP_layer_FC_layers_2_weight", (1, 25)), ("MLP_layer_FC_layers_2_bias", (1,)),
])
_DGN_TABLE_OFF = [0, 11900, 12300, 13500, 14700, 15700, 16300, 16900, 17100]  # DGN/src/host_load.cc:12-64
_DGN_TAIL = OrderedDict([("MLP_layer_FC_layers_0_weight", 97700), ("MLP_layer_FC_layers_0_bias", 102700),
                         ("MLP_layer_FC_layers_1_weight", 102750), ("MLP_layer_FC_layers_1_bias", 104000),
                         ("MLP_layer_FC_layers_2_weight", 104025), ("MLP_layer_FC_layers_2_bias", 104050)])
_CARD = [119, 4, 12, 12, 10, 6, 6, 2, 2]


def load_dgn_weights(directory: str) -> Dict[str, np.ndarray]:
    path = os.path.join(directory, DGN_FILE)
    emb = np.zeros((9, 119, 100), dtype=np.float32)
    for k in range(9):
        emb[k, :_CARD[k]] = _read(path, (_CARD[k], 100), _DGN_TABLE_OFF[k])
    w = OrderedDict()
    w["embedding_h_atom_embedding_list_weights"] = emb
    w["layers_posttrans_fully_connected_0_linear_weight"] = np.stack(
        [_read(path, (100, 200), 17300 + 20100 * l) for l in range(4)])
    w["layers_posttrans_fully_connected_0_linear_bias"] = np.stack(
        [_read(path, (100,), 17300 + 20100 * l + 20000) for l in range(4)])
    for k, off in _DGN_TAIL.items():
        w[k] = _read(path, DGN_SHAPES[k], off)
    return w


def save_dgn_weights(w: Dict[str, np.ndarray], directory: str) -> None:
    os.makedirs(directory, exist_ok=True)
    buf = np.zeros(104051, dtype="<f4")
    emb = np.asarray(w["embedding_h_atom_embedding_list_weights"], np.float32)
    for k in range(9):
        buf[_DGN_TABLE_OFF[k]:_DGN_TABLE_OFF[k] + _CARD[k] * 100] = emb[k, :_CARD[k]].ravel()
    for l in range(4):
        base = 17300 + 20100 * l
        buf[base:base + 20000] = np.asarray(w["layers_posttrans_fully_connected_0_linear_weight"], np.float32)[l].ravel()
        buf[base + 20000:base + 20100] = np.asarray(w["layers_posttrans_fully_connected_0_linear_bias"], np.float32)[l].ravel()
    for k, off in _DGN_TAIL.items():
        a = np.asarray(w[k], np.float32).ravel()
        buf[off:off + a.size] = a
    buf.tofile(os.path.join(directory, DGN_FILE))


def synth_dgn_weights(seed: int = 7) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    scale = {"embedding_h_atom_embedding_list_weights": 0.11, "layers_posttrans_fully_connected_0_linear_weight": 0.05,
             "layers_posttrans_fully_connected_0_linear_bias": 0.1, "MLP_layer_FC_layers_0_weight": 0.1,
             "MLP_layer_FC_layers_0_bias": 0.1, "MLP_layer_FC_layers_1_weight": 0.15, "MLP_layer_FC_layers_1_bias": 0.1,
             "MLP_layer_FC_layers_2_weight": 0.2, "MLP_layer_FC_layers_2_bias": 0.1}
    w = OrderedDict((k, (rng.standard_normal(shp) * scale[k]).astype(np.float32)) for k, shp in DGN_SHAPES.items())
    for k in range(9):  # rows beyond a table's cardinality do not exist in the file
        w["embedding_h_atom_embedding_list_weights"][k, _CARD[k]:] = 0.0
    return w


# --------------------------------------------------------------------------- GAT
GAT_SHAPES = OrderedDict([
    ("scoring_fn_target", (5, 4, 16)), ("scoring_fn_source", (5, 4, 16)),
    ("linear_proj_weights", (5, 4, 16, 4, 16)), ("skip_proj_weights", (5, 4, 16, 4, 16)),
    ("graph_pred_weights", (1, 16)), ("graph_pred_bias", (1,)),
])
_GAT_FILES = {"graph_pred_weights": "gat_ep1_pred_weights_layer5.bin", "graph_pred_bias": "gat_ep1_pred_bias_layer5.bin",
              "scoring_fn_target": "gat_ep1_scoring_fn_target_layer5.bin",
              "scoring_fn_source": "gat_ep1_scoring_fn_source_layer5.bin"}


def load_gat_weights(directory: str) -> Dict[str, np.ndarray]:
    """GAT/src/host_load.cc:20-91: layer 0 of linear/skip proj is a [4][16][1][9] file placed in the
    [head_out][dim_out][head_in = 0][dim_in < 9] corner of a zero [4][16][4][16] tensor."""
    w = OrderedDict()
    for k in ("scoring_fn_target", "scoring_fn_source"):
        w[k] = _read(os.path.join(directory, _GAT_FILES[k]), GAT_SHAPES[k])
    for k, stem in (("linear_proj_weights", "linear_proj_weight"), ("skip_proj_weights", "skip_proj_weight")):
        full = np.zeros((5, 4, 16, 4, 16), dtype=np.float32)
        full[0, :, :, 0, :9] = _read(os.path.join(directory, f"gat_ep1_{stem}_0_layer5.bin"), (4, 16, 9))
        full[1:] = _read(os.path.join(directory, f"gat_ep1_{stem}_1_layer5.bin"), (4, 4, 16, 4, 16))
        w[k] = full
    for k in ("graph_pred_weights", "graph_pred_bias"):
        w[k] = _read(os.path.join(directory, _GAT_FILES[k]), GAT_SHAPES[k])
    return w


def save_gat_weights(w: Dict[str, np.ndarray], directory: str) -> None:
    os.makedirs(directory, exist_ok=True)
    for k, f in _GAT_FILES.items():
        np.asarray(w[k], dtype="<f4").tofile(os.path.join(directory, f))
    for k, stem in (("linear_proj_weights", "linear_proj_weight"), ("skip_proj_weights", "skip_proj_weight")):
        a = np.asarray(w[k], dtype="<f4")
        np.ascontiguousarray(a[0, :, :, 0, :9]).tofile(os.path.join(directory, f"gat_ep1_{stem}_0_layer5.bin"))
        np.ascontiguousarray(a[1:]).tofile(os.path.join(directory, f"gat_ep1_{stem}_1_layer5.bin"))


def synth_gat_weights(seed: int = 7) -> Dict[str, np.ndarray]:
    """Small weights: the reference feeds raw atom numbers (0..118) into layer 0 and exponentiates the
    attention scores without max subtraction, so the scale has to keep exp() finite."""
    rng = np.random.default_rng(seed)
    scale = {"scoring_fn_target": 0.1, "scoring_fn_source": 0.1, "linear_proj_weights": 0.08, "skip_proj_weights": 0.08,
             "graph_pred_weights": 0.2, "graph_pred_bias": 0.1}
    w = OrderedDict((k, (rng.standard_normal(shp) * scale[k]).astype(np.float32)) for k, shp in GAT_SHAPES.items())
    for k in ("linear_proj_weights", "skip_proj_weights"):
        corner = w[k][0, :, :, 0, :9].copy() * 0.02  # raw integer inputs
        w[k][0] = 0.0
        w[k][0, :, :, 0, :9] = corner
    return w


LOADERS = {"GIN": load_gin_weights, "GIN-VN": load_gin_weights, "GCN": load_gcn_weights, "PNA": load_pna_weights, "DGN": load_dgn_weights, "GAT": load_gat_weights}
SYNTH = {"GIN": synth_gin_weights, "GIN-VN": synth_gin_weights, "GCN": synth_gcn_weights, "PNA": synth_pna_weights, "DGN": synth_dgn_weights, "GAT": synth_gat_weights}
SAVERS = {"GIN": save_gin_weights, "GIN-VN": save_gin_weights, "GCN": save_gcn_weights, "PNA": save_pna_weights, "DGN": save_dgn_weights, "GAT": save_gat_weights}
