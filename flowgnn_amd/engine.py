"""Host-side mirror of the reference's per-model entry points over the C ABI.

`Engine` wraps the handle API (flowgnn_create / set_weights / set_batch / run / get_results);
`compute_graphs` calls the reference-compatible `<M>_compute_graphs` symbol with host arrays,
exactly the argument list of the reference kernel (GIN/src/dcl.h:75-94).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np

from . import _lib
from .graphpack import GraphBatch


# flowgnn_set_numeric_mode codes (flowgnn.h: FLOWGNN_NUMERIC_F32 / _Q6_10 / _F16)
NUMERIC_MODES = {"f32": 0, "q6.10": 1, "f16": 2}
# flowgnn_set_pooling codes (flowgnn.h: FLOWGNN_POOL_MEAN / _SUM / _MAX)
POOLING_MODES = {"mean": 0, "sum": 1, "max": 2}
# flowgnn_set_jk_residual codes (flowgnn.h: FLOWGNN_JK_LAST / _SUM)
JK_MODES = {"last": 0, "sum": 1}
JK_NAMES = {v: k for k, v in JK_MODES.items()}


def _jk_code(jk) -> int:
    """OGB's JK names; an integer goes to the library as it is, which judges it"""
    if isinstance(jk, str):
        if jk not in JK_MODES:
            raise ValueError(f"jk is {jk!r}, wanted one of {sorted(JK_MODES)}")
        return JK_MODES[jk]
    return int(jk)


class FlowGNNError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str = ""):
        self.code = code
        super().__init__(f"{where}: {_lib.STATUS.get(code, code)} {detail}".strip())


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _pi(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_lib.p_int)


def _pf(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_lib.p_float)


def _eps_arg(eps, num_layers: int = 5):
    """None -> NULL (off); else the five values as a float32 array (ctypes takes its pointer for the duration of the call).  "Five" is
    the engine's depth (flowgnn_num_layers): the C call reads that many."""
    if eps is None:
        return None
    a = np.ascontiguousarray(np.asarray(eps, dtype=np.float32).reshape(-1))
    n = int(num_layers)
    if a.size != n:
        raise ValueError(f"eps: {'five' if n == 5 else n} values (one per GIN layer), got {a.size}")
    return (C.c_float * n)(*a.tolist())


def _ogb_vn_args(vn, emb_dims=(100, 300), num_layers: int = 5):
    """None -> five NULLs (off); else the dict's five tensors (weights.GIN_VIRTUAL_NODE_SHAPES) as float32 arrays, in the C call's
    order -- the caller keeps them alive for the duration of the call.  num_layers: the engine's depth (flowgnn_num_layers): the C call
    reads num_layers - 1 updates, so tensors of another depth are refused here, before it sees a pointer."""
    if vn is None:
        return [None] * 5
    from .weights import checked_gin_virtual_node
    return list(checked_gin_virtual_node(vn, emb_dims=emb_dims, num_layers=int(num_layers)).values())


def _attn_pool_args(gate):
    """None -> (300, three NULLs) (off); else the width read off w1 and the dict's three tensors (weights.ATTENTION_POOLING_KEYS) as
    float32 arrays, in the C call's order -- the caller keeps them alive for the duration of the call."""
    if gate is None:
        return 300, [None] * 3
    from .weights import checked_attention_pooling
    a = list(checked_attention_pooling(gate).values())
    return int(a[0].shape[1]), a


def _s2s_args(s2s):
    """None -> (300, 1, six NULLs) (off); else the width read off w_hh, NUM_TASK off head_b and the dict's six tensors
    (weights.SET2SET_KEYS) as float32 arrays, in the C call's order -- the caller keeps them alive for the duration of the call."""
    if s2s is None:
        return 300, 1, [None] * 6
    from .weights import checked_set2set
    a = list(checked_set2set(s2s).values())
    return int(a[1].shape[1]), int(a[5].size), a


def _ogb_vn_dim(a) -> int:
    """The width of _ogb_vn_args' tensors (the embedding row's length); 100 for the five NULLs."""
    return 100 if a[0] is None else int(a[0].size)


def _gcn_vn_args(vn, engine_dim, num_layers: int = 5):
    """_ogb_vn_args for GCN's two calls: 300-wide tensors are for an engine at set_model_emb_dim(300) alone -- on any other they
    are refused here, before a C call sees a pointer."""
    a = _ogb_vn_args(vn, num_layers=num_layers)
    if _ogb_vn_dim(a) != 100 and _ogb_vn_dim(a) != int(engine_dim):
        raise ValueError(f"set_gcn_virtual_node: the tensors are {_ogb_vn_dim(a)} wide and the engine's width is {int(engine_dim)} "
                         "(set_model_emb_dim(300) first)")
    return a


def _check_weights_depth(model: str, w, num_layers: int) -> None:
    """GIN / GIN-VN / GCN: the C call reads num_layers blocks of every per-layer tensor through a bare pointer, so a weight set of
    another depth (flowgnn_set_num_layers) is refused here, before it sees one.  The depth is read off the per-layer edge table,
    [L][13][D] with D the row length of the node table; a set without those two names is left to the C call as ever."""
    if model not in ("GIN", "GIN-VN", "GCN") or not hasattr(w, "keys") or not {"node_embedding_weight", "edge_embedding_weight"} <= set(w.keys()):
        return
    d = np.asarray(w["node_embedding_weight"]).size // 173
    have = np.asarray(w["edge_embedding_weight"]).size
    if d and have != int(num_layers) * 13 * d:
        raise ValueError(f"set_weights: edge_embedding_weight holds {have / (13 * d):g} layers of {d}-wide rows and the engine's depth is "
                         f"{int(num_layers)} (set_num_layers / flowgnn_set_num_layers)")


def option_value(v) -> float:
    """Option values are numbers; "f32" / "f16" (the *_mfma switches) read as 32 / 16."""
    if isinstance(v, str) and v in ("f32", "f16"):
        return 32.0 if v == "f32" else 16.0
    return float(v)


def embedding_dim(model: str) -> int:
    """Floats per graph of a model's graph embedding (flowgnn.h: flowgnn_embedding_dim); host code only, no GPU needed."""
    model = model.upper()
    if model not in _lib.MODEL_IDS:
        raise ValueError(f"unknown model {model}")
    return int(_lib.load().flowgnn_embedding_dim(_lib.MODEL_IDS[model]))


def laplacian_eigen_max_nodes() -> int:
    """The largest graph Engine.laplacian_eigen takes (flowgnn.h: flowgnn_laplacian_eigen_max_nodes); host code only, no GPU needed."""
    return int(_lib.load().flowgnn_laplacian_eigen_max_nodes())


def attention_shape(model: str):
    """(layers, heads) of a model's attention coefficients (flowgnn.h: flowgnn_attention_shape): (5, 4) for GAT, FlowGNNError with
    code 8 for the models that have none; host code only, no GPU needed."""
    model = model.upper()
    if model not in _lib.MODEL_IDS:
        raise ValueError(f"unknown model {model}")
    a, b = C.c_int(0), C.c_int(0)
    rc = int(_lib.load().flowgnn_attention_shape(_lib.MODEL_IDS[model], C.byref(a), C.byref(b)))
    if rc:
        raise FlowGNNError(rc, "flowgnn_attention_shape", f"{model} has no attention coefficients")
    return int(a.value), int(b.value)


def attention_mask(model: str, layers) -> int:
    """The layer mask of flowgnn_set_attention from an iterable of layer indices, "all", "last", or None / False (0: off)."""
    if layers is None or layers is False:
        return 0
    n_layers = 5  # (GAT; a model without attention is refused by the library with its own text)
    if isinstance(layers, str):
        if layers not in ("all", "last"):
            raise ValueError(f"attention layers: {layers!r} (an iterable of layer indices, 'all', 'last' or None)")
        return (1 << n_layers) - 1 if layers == "all" else 1 << (n_layers - 1)
    if layers is True:
        return 1 << (n_layers - 1)
    mask = 0
    for l in layers:
        if int(l) != l or not 0 <= int(l) < n_layers:
            raise ValueError(f"attention layer {l!r}: layers are 0..{n_layers - 1}")
        mask |= 1 << int(l)
    return mask


class Engine:
    """One engine = one GPU, one stream, one model's weights, one resident batch.
    `options`: {key: value} passed to flowgnn_set_option right after creation (e.g. {"gin_resident": 0})."""

    def __init__(self, model: str = "GIN", device: int = 0, options: Optional[Dict[str, float]] = None):
        self.lib = _lib.load()
        self.model = model.upper()
        if self.model not in _lib.MODEL_IDS:
            raise ValueError(f"unknown model {model}")
        self._h = C.c_void_p()
        self._check(self.lib.flowgnn_create(_lib.MODEL_IDS[self.model], device, C.byref(self._h)), "flowgnn_create")
        self.device = int(device)
        self._keep = []
        self.num_tasks = 1
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, key: str, value):
        """Run-time switch by name (flowgnn.h: flowgnn_set_option); call before set_batch."""
        self._check(self.lib.flowgnn_set_option(self._h, key.encode(), option_value(value)), f"flowgnn_set_option({key})")

    def get_option(self, key: str) -> float:
        v = C.c_double()
        self._check(self.lib.flowgnn_get_option(self._h, key.encode(), C.byref(v)), f"flowgnn_get_option({key})")
        return float(v.value)

    def _check(self, rc: int, where: str):
        if rc != 0:
            detail = ""
            if self._h:
                detail = (self.lib.flowgnn_last_error(self._h) or b"").decode(errors="replace")
            raise FlowGNNError(rc, where, detail)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.flowgnn_destroy(self._h)
            self._h = C.c_void_p()
        self._results_tensor = None  # (forward_device's output: released once the engine, and its stream, are gone)
        self._embeddings_tensor = None
        self._node_embeddings_tensor = None
        self._node_logits_tensor = None
        self._attention_tensors = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights
    def set_weights(self, w: Dict[str, np.ndarray]):
        """`w`: OrderedDict in the argument order of the model's <M>_compute_graphs entry point."""
        _check_weights_depth(self.model, w, self.num_layers)
        arrs = [_f32(v) for v in w.values()]
        ptrs = (_lib.p_float * len(arrs))(*[_pf(a) for a in arrs])
        self._check(self.lib.flowgnn_set_weights(self._h, len(arrs), ptrs), "flowgnn_set_weights")

    def load_weights_dir(self, directory: str, eps: bool = False, virtual_node: bool = False, attention_pooling: bool = False,
                         set2set: bool = False, set2set_steps: int = 2):
        """eps=True (GIN, GIN-VN): also read the directory's eps file and apply it (set_gin_eps); virtual_node=True: also read
        gin_ep1_virtualnode_dim100.bin and apply it (GIN: set_ogb_virtual_node), or gcn_ep1_virtualnode_dim100.bin on a GCN engine
        (set_gcn_virtual_node; at width 300 gcn_ep1_virtualnode_dim300.bin, through flowgnn_set_gcn_virtual_node_dim).  The C call itself does neither.  A GIN engine at width 300 (set_emb_dim) reads the dim300 set, its eps
        file and its virtual-node file (gin_ep1_virtualnode_dim300.bin, through flowgnn_set_ogb_virtual_node_dim) included.
        attention_pooling=True (GIN, GCN at width 300): also read gin_ep1_attnpool_dim300.bin / gcn_ep1_attnpool_dim300.bin and apply it
        (set_attention_pooling).
        set2set=True (GIN, GCN at width 300): also read gin_ep1_set2set_dim300.bin / gcn_ep1_set2set_dim300.bin and apply it with
        set2set_steps processing steps (set_set2set_pooling; OGB: 2).
        After set_num_layers the files are read at the engine's depth: the per-layer tensors, num_layers eps values, num_layers - 1
        updates of the virtual node; a file of another depth is refused."""
        self._check(self.lib.flowgnn_load_weights_dir(self._h, directory.encode()), "flowgnn_load_weights_dir")
        if eps:
            from .weights import load_gin_eps
            self.set_gin_eps(load_gin_eps(directory, emb_dim=self.emb_dim if self.model == "GIN" else 100, num_layers=self.num_layers))
        if virtual_node and self.model == "GCN":
            from .weights import load_gcn_virtual_node
            self.set_gcn_virtual_node(load_gcn_virtual_node(directory, emb_dim=self.emb_dim, num_layers=self.num_layers))
        elif virtual_node:
            from .weights import load_gin_virtual_node
            self.set_ogb_virtual_node(load_gin_virtual_node(directory, emb_dim=self.emb_dim, num_layers=self.num_layers))
        if attention_pooling:
            from .weights import load_attention_pooling
            self.set_attention_pooling(load_attention_pooling(directory, model=self.model, emb_dim=self.emb_dim))
        if set2set:
            from .weights import load_set2set
            self.set_set2set_pooling(load_set2set(directory, model=self.model, emb_dim=self.emb_dim), steps=set2set_steps)

    # ---- batch
    def set_job_totals(self, job_nodes: int = -1, job_edges: int = -1):
        """The next batches are shards of a job of this size (flowgnn.h: flowgnn_set_job_totals); (-1, -1): each batch is its own job."""
        self._check(self.lib.flowgnn_set_job_totals(self._h, int(job_nodes), int(job_edges)), "flowgnn_set_job_totals")

    def graph_tile_fill(self, nums_of_nodes, nums_of_edges) -> float:
        """Fill of this model's graph tiles for a graph list (flowgnn.h: flowgnn_graph_tile_fill); host code only."""
        nn, ne = _i32(nums_of_nodes), _i32(nums_of_edges)
        f = C.c_double()
        self._check(self.lib.flowgnn_graph_tile_fill(self._h, len(nn), _pi(nn), _pi(ne), C.byref(f)), "flowgnn_graph_tile_fill")
        return float(f.value)

    def batch_tiles(self):
        """(tiles in batch order, bin-packed tiles or 0) of the resident batch (flowgnn.h: flowgnn_batch_tiles)."""
        a, b = C.c_int(0), C.c_int(0)
        self._check(self.lib.flowgnn_batch_tiles(self._h, C.byref(a), C.byref(b)), "flowgnn_batch_tiles")
        return int(a.value), int(b.value)

    def set_job_tile_fill(self, fill: float = -1.0):
        """The next batches take the JOB's side of the resident kernels' fill threshold (flowgnn.h: flowgnn_set_job_tile_fill)."""
        self._check(self.lib.flowgnn_set_job_tile_fill(self._h, float(fill)), "flowgnn_set_job_tile_fill")

    def set_batch(self, batch: GraphBatch):
        nn, ne = _i32(batch.nums_of_nodes), _i32(batch.nums_of_edges)
        nf, el, ea = _i32(batch.node_feature), _i32(batch.edge_list), _i32(batch.edge_attr)
        eig = None if batch.node_eigen is None else _f32(batch.node_eigen)
        self._check(self.lib.flowgnn_set_batch(self._h, batch.num_graphs, _pi(nn), _pi(ne), _pi(nf), _pi(el), _pi(ea),
                                               _pf(eig)), "flowgnn_set_batch")
        self.num_graphs = batch.num_graphs
        self.total_nodes = batch.total_nodes
        self.total_edges = batch.total_edges

    def set_batch_device_ptrs(self, nums_of_nodes, nums_of_edges, layout: str, node_feature: int, edge_list: int,
                              edge_attr: int = 0, node_eigen: int = 0):
        """flowgnn_set_batch_device with raw DEVICE addresses (ints, 0 = NULL), for callers without torch.  Counts are host arrays;
        `layout` "pyg" (int64 x [N][9], edge_index [2][E] with batch-global ids, edge_attr [E][3]) or "reference" (int32, as
        set_batch takes them).  The arrays must be complete on the engine's launch stream (stream_handle()) and stay unchanged until
        the ingest has run there; validation errors surface at sync() / results()."""
        nn, ne = _i32(nums_of_nodes), _i32(nums_of_edges)
        if layout not in _lib.LAYOUT_IDS:
            raise ValueError(f"unknown layout {layout!r} (pyg / reference)")
        ptrs = [C.c_void_p(int(p)) if p else None for p in (node_feature, edge_list, edge_attr, node_eigen)]
        self._check(self.lib.flowgnn_set_batch_device(self._h, len(nn), _pi(nn), _pi(ne), _lib.LAYOUT_IDS[layout], *ptrs),
                    "flowgnn_set_batch_device")
        self.num_graphs = len(nn)
        self.total_nodes = int(nn.sum(dtype=np.int64))
        self.total_edges = int(ne.sum(dtype=np.int64))

    def stream_handle(self) -> int:
        """The hipStream_t the engine launches on (its own, or the one given to set_stream), as an int."""
        p = C.c_void_p()
        self._check(self.lib.flowgnn_stream(self._h, C.byref(p)), "flowgnn_stream")
        return int(p.value or 0)

    def _device_batch_args(self, x, edge_index, edge_attr, node_eigen, ptr, nums_of_edges):
        import torch
        dev = torch.device("cuda", self.device)
        if x.dtype == torch.int64 and edge_index.dtype == torch.int64:
            layout, n_e = "pyg", (edge_index.shape[1] if edge_index.dim() == 2 and edge_index.shape[0] == 2 else -1)
        elif x.dtype == torch.int32 and edge_index.dtype == torch.int32:
            layout, n_e = "reference", (edge_index.shape[0] if edge_index.dim() == 2 and edge_index.shape[1] == 2 else -1)
        else:
            raise TypeError("x / edge_index: both int64 (PyG layout) or both int32 (reference layout)")
        if n_e < 0:
            raise ValueError("edge_index: [2][E] in the PyG layout, [E][2] in the reference layout")
        need = [("x", x, x.dtype, (-1, 9)), ("edge_index", edge_index, x.dtype, None)]
        if edge_attr is not None:
            need.append(("edge_attr", edge_attr, x.dtype, (n_e, 3)))
        if node_eigen is not None:
            need.append(("node_eigen", node_eigen, torch.float32, (x.shape[0], 4)))
        for name, t, dtype, shape in need:
            if t.device != dev:
                raise ValueError(f"{name} is on {t.device}, the engine on {dev}")
            if t.dtype != dtype:
                raise TypeError(f"{name}: dtype {t.dtype}, expected {dtype}")
            if not t.is_contiguous():
                raise ValueError(f"{name} is not contiguous")
            if shape is not None and (t.dim() != 2 or t.shape[1] != shape[1] or (shape[0] >= 0 and t.shape[0] != shape[0])):
                raise ValueError(f"{name}: shape {tuple(t.shape)}, expected [{'N' if shape[0] < 0 else shape[0]}][{shape[1]}]")
        return (layout,) + self._graph_counts(edge_index, layout, n_e, ptr, nums_of_edges, n_rows=x.shape[0])

    def _graph_counts(self, edge_index, layout, n_e, ptr, nums_of_edges, n_rows=None):
        """(nums_of_nodes, nums_of_edges) as host arrays from `ptr` ([G + 1], any device; it must end at n_rows when that is given)
        and, when no edge counts are given (PyG layout only), from each edge's source id."""
        import torch
        if ptr is None:
            raise ValueError("ptr (the node pointer, [G + 1]) is required")
        ptr_h = ptr.detach().to("cpu", torch.int64).numpy() if isinstance(ptr, torch.Tensor) else np.asarray(ptr, dtype=np.int64)
        nn = np.diff(ptr_h)
        if ptr_h.size < 1 or ptr_h[0] != 0 or (n_rows is not None and ptr_h[-1] != n_rows):
            raise ValueError("ptr must run from 0 to N (the rows of x)")
        if nums_of_edges is None:
            if layout != "pyg":
                raise ValueError("the reference layout holds local ids: pass nums_of_edges")
            # each edge's graph from its source id, bucketed against ptr (the edges of a PyG Batch are grouped by graph)
            gid = torch.bucketize(edge_index[0], torch.as_tensor(ptr_h[1:], device=edge_index.device), right=True)
            ne = torch.bincount(gid, minlength=len(nn))[: len(nn)].cpu().numpy()
            if int(ne.sum()) != n_e:
                raise ValueError("edge_index[0] holds ids outside [0, N): pass nums_of_edges")
        else:
            ne = (nums_of_edges.detach().cpu().numpy() if isinstance(nums_of_edges, torch.Tensor) else np.asarray(nums_of_edges))
        return nn, ne

    def set_batch_device(self, x, edge_index, edge_attr=None, node_eigen=None, *, ptr, nums_of_edges=None):
        """A batch whose arrays are torch tensors on the engine's device (flowgnn.h: flowgnn_set_batch_device).  The layout follows
        the dtypes: int64 x [N][9] / edge_index [2][E] with batch-global ids / edge_attr [E][3] (a PyG Batch), or int32 x [N][9] /
        edge_list [E][2] with local ids / edge_attr [E][3] (the reference's).  node_eigen: float32 [N][4] (DGN).  Per-graph sizes:
        `ptr` (node pointer [G + 1], any device) and `nums_of_edges` ([G]; PyG layout: computed from edge_index[0] when omitted).
        The engine's stream is ordered after torch's current stream, and torch's current stream after the ingest, so the call needs
        no synchronisation and the caller may drop or overwrite the tensors at once."""
        import torch
        layout, nn, ne = self._device_batch_args(x, edge_index, edge_attr, node_eigen, ptr, nums_of_edges)
        cur = torch.cuda.current_stream(self.device)
        es = torch.cuda.ExternalStream(self.stream_handle(), device=torch.device("cuda", self.device))
        es.wait_stream(cur)
        self.set_batch_device_ptrs(nn, ne, layout, x.data_ptr(), edge_index.data_ptr(),
                                   edge_attr.data_ptr() if edge_attr is not None else 0,
                                   node_eigen.data_ptr() if node_eigen is not None else 0)
        # The caching allocator must not recycle the inputs before the ingest has read them: torch's current stream waits for it and
        # the inputs are recorded on THAT stream (whichever stream allocated them).  Not on the engine's own stream: torch records an
        # event on every recorded stream when a tensor is freed, and the engine's stream dies with the engine.
        cur.wait_stream(es)
        for t in (x, edge_index, edge_attr, node_eigen):
            if t is not None:
                t.record_stream(cur)

    def forward_device(self, x, edge_index, edge_attr=None, node_eigen=None, *, ptr, nums_of_edges=None, return_embeddings=False,
                       return_node_embeddings=False, return_node_logits=False, return_attention=None):
        """set_batch_device, then one forward into a new torch tensor on the device ([G], or [G][num_tasks]); torch's current stream
        waits for the engine's, the host does not.  Validation errors (and the range check that can repeat a pass on the exact
        kernels) are seen by sync(), which raises; without it the tensor of a refused batch holds whatever the kernels wrote.
        return_embeddings: (logits, embeddings), the graph embeddings ([G][embedding_dim]) in a new device tensor as well, written
        by the kernels themselves (flowgnn_set_embeddings_buffer); embeddings stay on for later runs (set_embeddings(False) ends it).
        return_node_embeddings: the node embeddings ([N][embedding_dim], in the order of the rows of x, i.e. of the PyG Batch's nodes)
        in a new device tensor, appended to the returned tuple; written by the kernels themselves
        (flowgnn_set_node_embeddings_buffer), and on for later runs until set_node_embeddings(False).
        return_node_logits: the per-node terms of the readout ([N], or [N][num_tasks], in the order of the rows of x) in a new device
        tensor, appended last; written by the kernels themselves (flowgnn_set_node_logits_buffer), on until set_node_logits(False).
        return_attention (GAT): what set_attention takes ("last", "all", layer indices); the pair (edge [n_sel][E][4] in the order of
        edge_index's columns, self [n_sel][N][4]) of new device tensors is appended after everything else; written by the kernels
        themselves (flowgnn_set_attention_buffers), on until set_attention(None)."""
        import torch
        dev = torch.device("cuda", self.device)
        cur = torch.cuda.current_stream(dev)
        G = (len(ptr) - 1) if not isinstance(ptr, torch.Tensor) else int(ptr.numel()) - 1
        out = torch.empty(G * self.num_tasks, dtype=torch.float32, device=dev)  # (before the engine's stream waits for torch's)
        emb = None
        if return_embeddings:
            emb = torch.empty((G, self.emb_dim), dtype=torch.float32, device=dev)
            self.set_embeddings(True)
        rows = None
        if return_node_embeddings:
            rows = torch.empty((int(x.shape[0]), self.emb_dim), dtype=torch.float32, device=dev)
            self.set_node_embeddings(True)
        terms = None
        if return_node_logits:
            n_rows = int(x.shape[0])
            terms = torch.empty((n_rows, self.num_tasks) if self.num_tasks > 1 else (n_rows,), dtype=torch.float32, device=dev)
            self.set_node_logits(True)
        attn = None
        if return_attention is not None and return_attention is not False:
            self.set_attention(return_attention)
            n_sel = bin(self._attn_mask).count("1")
            n_edges = int(edge_index.shape[1] if edge_index.dtype == torch.int64 else edge_index.shape[0])
            attn = (torch.empty((n_sel, n_edges, 4), dtype=torch.float32, device=dev),
                    torch.empty((n_sel, int(x.shape[0]), 4), dtype=torch.float32, device=dev))
        self.set_batch_device(x, edge_index, edge_attr, node_eigen, ptr=ptr, nums_of_edges=nums_of_edges)
        es = torch.cuda.ExternalStream(self.stream_handle(), device=dev)
        if G:
            self.set_results_buffer(out.data_ptr())
            self._results_tensor = out  # the engine writes there until the next set_batch: keep it alive
            if emb is not None:
                self.set_embeddings_buffer(emb.data_ptr())
                self._embeddings_tensor = emb
            if rows is not None:
                self.set_node_embeddings_buffer(rows.data_ptr())
                self._node_embeddings_tensor = rows
            if terms is not None:
                self.set_node_logits_buffer(terms.data_ptr())
                self._node_logits_tensor = terms
            if attn is not None:
                self.set_attention_buffers(attn[0].data_ptr(), attn[1].data_ptr())
                self._attention_tensors = attn
        self.run()
        cur.wait_stream(es)
        logits = out.view(G, self.num_tasks) if self.num_tasks > 1 else out
        ret = (logits,) + ((emb,) if return_embeddings else ()) + ((rows,) if return_node_embeddings else ()) + ((terms,) if return_node_logits else ())
        ret += (attn,) if attn is not None else ()
        return ret if len(ret) > 1 else logits

    # ---- DGN's Laplacian eigenvectors (flowgnn.h: flowgnn_laplacian_eigen)
    def laplacian_eigen(self, batch: GraphBatch) -> np.ndarray:
        """node_eigen, float32 [N][4], of a host batch, computed on the GPU: per graph the eigenvectors of the four smallest
        eigenvalues of its normalised Laplacian (graphpack.laplacian_eigen is the same definition on the CPU).  Graphs of up to
        laplacian_eigen_max_nodes() nodes; any model's engine will do, and its resident batch is left alone."""
        nn, ne, el = _i32(batch.nums_of_nodes), _i32(batch.nums_of_edges), _i32(batch.edge_list)
        out = np.empty((int(nn.sum(dtype=np.int64)), 4), dtype=np.float32)
        self._check(self.lib.flowgnn_laplacian_eigen(self._h, len(nn), _pi(nn), _pi(ne), _pi(el), _pf(out)), "flowgnn_laplacian_eigen")
        return out

    def laplacian_eigen_device_ptrs(self, nums_of_nodes, nums_of_edges, layout: str, edge_list: int, node_eigen: int):
        """flowgnn_laplacian_eigen_device with raw DEVICE addresses (ints), for callers without torch: counts are host arrays,
        `layout` as in set_batch_device_ptrs; asynchronous on the engine's launch stream (stream_handle())."""
        nn, ne = _i32(nums_of_nodes), _i32(nums_of_edges)
        if layout not in _lib.LAYOUT_IDS:
            raise ValueError(f"unknown layout {layout!r} (pyg / reference)")
        ptrs = [C.c_void_p(int(p)) if p else None for p in (edge_list, node_eigen)]
        self._check(self.lib.flowgnn_laplacian_eigen_device(self._h, len(nn), _pi(nn), _pi(ne), _lib.LAYOUT_IDS[layout], *ptrs),
                    "flowgnn_laplacian_eigen_device")

    def laplacian_eigen_device(self, edge_index, *, ptr, nums_of_edges=None):
        """node_eigen of a batch whose edges are a torch tensor on the engine's device, into a new float32 [N][4] tensor there:
        int64 edge_index [2][E] with batch-global ids (a PyG Batch) or int32 edge_list [E][2] with local ids; `ptr` and
        `nums_of_edges` as for set_batch_device.  Ordered against torch's streams the way set_batch_device is -- the engine's stream
        after torch's current one, torch's current one after the kernels -- so
        forward_device(x, ei, None, eng.laplacian_eigen_device(ei, ptr=ptr), ptr=ptr) needs no synchronisation."""
        import torch
        dev = torch.device("cuda", self.device)
        if edge_index.dtype == torch.int64 and edge_index.dim() == 2 and edge_index.shape[0] == 2:
            layout, n_e = "pyg", int(edge_index.shape[1])
        elif edge_index.dtype == torch.int32 and edge_index.dim() == 2 and edge_index.shape[1] == 2:
            layout, n_e = "reference", int(edge_index.shape[0])
        else:
            raise TypeError("edge_index: int64 [2][E] (PyG layout) or int32 [E][2] (reference layout)")
        if edge_index.device != dev:
            raise ValueError(f"edge_index is on {edge_index.device}, the engine on {dev}")
        if not edge_index.is_contiguous():
            raise ValueError("edge_index is not contiguous")
        nn, ne = self._graph_counts(edge_index, layout, n_e, ptr, nums_of_edges)
        cur = torch.cuda.current_stream(dev)
        out = torch.empty((int(nn.sum()), 4), dtype=torch.float32, device=dev)
        es = torch.cuda.ExternalStream(self.stream_handle(), device=dev)
        es.wait_stream(cur)
        self.laplacian_eigen_device_ptrs(nn, ne, layout, edge_index.data_ptr(), out.data_ptr())
        cur.wait_stream(es)  # (and the allocator may recycle edge_index only behind the kernels: see set_batch_device)
        edge_index.record_stream(cur)
        return out

    def run(self):
        self._check(self.lib.flowgnn_run(self._h), "flowgnn_run")

    def sync(self):
        self._check(self.lib.flowgnn_sync(self._h), "flowgnn_sync")

    def results(self) -> np.ndarray:
        out = np.empty(self.num_graphs * self.num_tasks, dtype=np.float32)
        self._check(self.lib.flowgnn_get_results(self._h, _pf(out)), "flowgnn_get_results")
        return out.reshape(self.num_graphs, self.num_tasks) if self.num_tasks > 1 else out

    def set_num_tasks(self, num_tasks: int):
        """NUM_TASK of the readout (GIN / GIN-VN / GCN): set before weights and batch; results become [G][num_tasks]."""
        self._check(self.lib.flowgnn_set_num_tasks(self._h, int(num_tasks)), "flowgnn_set_num_tasks")
        self.num_tasks = int(num_tasks)

    def set_num_layers(self, n: int, emb_dim: int = 300):
        """GIN's or GCN's depth at width 300, OGB's num_layer (flowgnn.h: flowgnn_set_num_layers): 2 .. 8, 5 by default; set behind the
        width and before weights and batch (both have to be set again after a change).  eps and the virtual node must be off while it
        changes: their tensors are a depth's."""
        self._check(self.lib.flowgnn_set_num_layers(self._h, int(emb_dim), int(n)), "flowgnn_set_num_layers")

    @property
    def num_layers(self) -> int:
        """The engine's depth (flowgnn.h: flowgnn_num_layers): 5 unless set_num_layers said otherwise."""
        return int(self.lib.flowgnn_num_layers(self._h))

    def set_emb_dim(self, emb_dim: int):
        """GIN's width (flowgnn.h: flowgnn_set_emb_dim): 100, the reference's, or 300, OGB's default; set before weights and batch
        (both have to be set again afterwards)."""
        self._check(self.lib.flowgnn_set_emb_dim(self._h, int(emb_dim)), "flowgnn_set_emb_dim")

    def set_model_emb_dim(self, emb_dim: int):
        """GIN's or GCN's width (flowgnn.h: flowgnn_set_model_emb_dim): on a GIN engine exactly set_emb_dim, on a GCN engine 100 or
        300 (OGB's default, gcn_ep1_dim300.weights.all.bin); set before weights and batch (both have to be set again afterwards)."""
        self._check(self.lib.flowgnn_set_model_emb_dim(self._h, int(emb_dim)), "flowgnn_set_model_emb_dim")

    @property
    def emb_dim(self) -> int:
        """The engine's width: what its embeddings, node embeddings and get_h rows are wide (flowgnn.h: flowgnn_emb_dim)."""
        return int(self.lib.flowgnn_emb_dim(self._h))

    def _device_ptrs(self, fn: str, count: int = 1):
        """`count` device addresses (0 = NULL) out of the C function `fn`(engine, void**, ...)."""
        ps = [C.c_void_p() for _ in range(count)]
        self._check(getattr(self.lib, fn)(self._h, *(C.byref(p) for p in ps)), fn)
        return tuple(int(p.value or 0) for p in ps)

    def _set_buffers(self, fn: str, *device_ptrs):
        """Device addresses into the C function `fn`(engine, void*, ...); None / 0 goes as NULL."""
        self._check(getattr(self.lib, fn)(self._h, *(C.c_void_p(p) if p else None for p in device_ptrs)), fn)

    def results_device_ptr(self) -> int:
        p = C.c_void_p()
        self._check(self.lib.flowgnn_results_device(self._h, C.byref(p)), "flowgnn_results_device")
        return int(p.value or 0)

    def set_results_buffer(self, device_ptr: int):
        self._check(self.lib.flowgnn_set_results_buffer(self._h, C.c_void_p(device_ptr)), "flowgnn_set_results_buffer")

    def forward(self, batch: GraphBatch, return_embeddings: bool = False, return_node_embeddings: bool = False,
                return_node_logits: bool = False, return_attention=None):
        """set_batch + run + results; return_embeddings: (logits, embeddings) -- embeddings stay on for later runs;
        return_node_embeddings: the node embeddings [N][embedding_dim] appended to the tuple (they stay on likewise);
        return_node_logits: the per-node readout terms [N] or [N][num_tasks] appended last (likewise);
        return_attention (GAT): what set_attention takes; the pair attention() returns is appended after everything else (likewise)."""
        want_attn = return_attention is not None and return_attention is not False
        if want_attn:
            self.set_attention(return_attention)
        if return_embeddings:
            self.set_embeddings(True)
        if return_node_embeddings:
            self.set_node_embeddings(True)
        if return_node_logits:
            self.set_node_logits(True)
        self.set_batch(batch)
        self.run()
        ret = (self.results(),) + ((self.embeddings(),) if return_embeddings else ()) + ((self.node_embeddings(),) if return_node_embeddings else ())
        ret += (self.node_logits(),) if return_node_logits else ()
        ret += (self.attention(),) if want_attn else ()
        return ret if len(ret) > 1 else ret[0]

    # ---- graph embeddings (flowgnn.h: flowgnn_set_embeddings)
    def set_embeddings(self, on: bool = True):
        """Runs enqueued after this also produce the per-graph pooled embeddings, the vector the readout head is applied to."""
        self._check(self.lib.flowgnn_set_embeddings(self._h, 1 if on else 0), "flowgnn_set_embeddings")

    def embeddings(self) -> np.ndarray:
        """[G][embedding_dim(model)] of the last run (synchronises); FLOWGNN_ERR_STATE if that run had embeddings off."""
        out = np.empty((self.num_graphs, self.emb_dim), dtype=np.float32)
        self._check(self.lib.flowgnn_get_embeddings(self._h, _pf(out)), "flowgnn_get_embeddings")
        return out

    def embeddings_device_ptr(self) -> int:
        return self._device_ptrs("flowgnn_embeddings_device")[0]

    def set_embeddings_buffer(self, device_ptr: Optional[int]):
        """Caller-owned device buffer of >= G * embedding_dim floats for the embeddings; None / 0 restores the engine's own."""
        self._set_buffers("flowgnn_set_embeddings_buffer", device_ptr)

    # ---- node embeddings (flowgnn.h: flowgnn_set_node_embeddings)
    def set_node_embeddings(self, on: bool = True):
        """Runs enqueued after this also store, per node and in the caller's node order, the row the readout pools."""
        self._check(self.lib.flowgnn_set_node_embeddings(self._h, 1 if on else 0), "flowgnn_set_node_embeddings")

    def node_embeddings(self) -> np.ndarray:
        """[N][embedding_dim(model)] of the last run (synchronises); FLOWGNN_ERR_STATE if that run had node embeddings off."""
        out = np.empty((self.total_nodes, self.emb_dim), dtype=np.float32)
        self._check(self.lib.flowgnn_get_node_embeddings(self._h, _pf(out)), "flowgnn_get_node_embeddings")
        return out

    def node_embeddings_device_ptr(self) -> int:
        return self._device_ptrs("flowgnn_node_embeddings_device")[0]

    def set_node_embeddings_buffer(self, device_ptr: Optional[int]):
        """Caller-owned device buffer of >= N * embedding_dim floats for the node embeddings; None / 0 restores the engine's own."""
        self._set_buffers("flowgnn_set_node_embeddings_buffer", device_ptr)

    # ---- node logits (flowgnn.h: flowgnn_set_node_logits; GIN, GIN-VN, GCN, GAT)
    def set_node_logits(self, on: bool = True):
        """Runs enqueued after this also store, per node and in the caller's node order, the node's term of the readout:
        r[v] . W[t] + b[t], whose mean over a graph's nodes is the graph's logit."""
        self._check(self.lib.flowgnn_set_node_logits(self._h, 1 if on else 0), "flowgnn_set_node_logits")

    def node_logits(self) -> np.ndarray:
        """[N], or [N][num_tasks], of the last run (synchronises); FLOWGNN_ERR_STATE if that run had node logits off."""
        out = np.empty((self.total_nodes, self.num_tasks) if self.num_tasks > 1 else (self.total_nodes,), dtype=np.float32)
        self._check(self.lib.flowgnn_get_node_logits(self._h, _pf(out)), "flowgnn_get_node_logits")
        return out

    def node_logits_device_ptr(self) -> int:
        return self._device_ptrs("flowgnn_node_logits_device")[0]

    def set_node_logits_buffer(self, device_ptr: Optional[int]):
        """Caller-owned device buffer of >= N * num_tasks floats for the node logits; None / 0 restores the engine's own."""
        self._set_buffers("flowgnn_set_node_logits_buffer", device_ptr)

    # ---- attention coefficients (flowgnn.h: flowgnn_set_attention; GAT)
    def set_attention(self, layers="last"):
        """Runs enqueued after this also store the attention coefficients of the selected layers: an iterable of layer indices,
        "all", "last" (the fifth layer: what explanation and edge pruning use), or None / False for off."""
        mask = attention_mask(self.model, layers)
        self._check(self.lib.flowgnn_set_attention(self._h, mask), "flowgnn_set_attention")
        self._attn_mask = mask

    def attention(self):
        """(edge [n_sel][E][4], self [n_sel][N][4]) of the last run (synchronises): per selected layer in ascending order, per edge
        of the batch as it was passed / per node (the implicit self edge), per head.  FLOWGNN_ERR_STATE if that run had it off."""
        n_sel = bin(getattr(self, "_attn_mask", 0)).count("1")
        edge = np.empty((n_sel, self.total_edges, 4), dtype=np.float32)
        own = np.empty((n_sel, self.total_nodes, 4), dtype=np.float32)
        self._check(self.lib.flowgnn_get_attention(self._h, _pf(edge), _pf(own)), "flowgnn_get_attention")
        return edge, own

    def attention_device_ptrs(self):
        """(edge, self) device addresses of the last run's attention coefficients (flowgnn.h: flowgnn_attention_device)."""
        return self._device_ptrs("flowgnn_attention_device", 2)

    def set_attention_buffers(self, edge_ptr: Optional[int], self_ptr: Optional[int]):
        """Caller-owned device buffers of >= n_sel * E * 4 and n_sel * N * 4 floats; None / 0 restores the engine's own (each)."""
        self._set_buffers("flowgnn_set_attention_buffers", edge_ptr, self_ptr)

    # ---- taps
    def set_numeric_mode(self, mode: str = "f32", emb_dim: Optional[int] = None):
        """"f32" (default), "q6.10": the bit patterns of the reference's own fixed-point format (ap_fixed<16,6>; DGN: ap_fixed<16,3>),
        or "f16" (GIN / GIN-VN): MLP operands rounded to f16, fp32 accumulation (flowgnn.h: FLOWGNN_NUMERIC_F16).
        emb_dim: the engine's width, which sends the call through flowgnn_set_numeric_mode_dim -- the way to "f16" on a GIN engine at
        set_emb_dim(300); without it the call is flowgnn_set_numeric_mode, which refuses every mode but "f32" at that width.
        A GCN engine takes the model form of the call, flowgnn_set_model_numeric_mode_dim, as set_jk_residual does: the way to "f16" for
        gcn and gcn-virtual at width 300 (stages 0..3 with one f16 rounding of each operand of the layer's product).
        A PNA engine takes the model form too: set_numeric_mode("f16", emb_dim=80) -- 80 is PNA's own width, FLOWGNN_EMB_DIM_PNA -- is
        the one way to PNA's "f16" (each operand of the layer's 320 -> 3 x 80 contraction rounded to f16 once, one MFMA per product);
        without emb_dim, or with 100, "f16" stays refused on PNA.
        A DGN engine with emb_dim (100, DGN's width) takes the call that names the model, flowgnn_set_model_numeric_mode:
        set_numeric_mode("f16", emb_dim=100) is the one way to DGN's "f16" (each operand of the matrix-pipe products -- both aggregates
        and the 200 -> 100 update -- rounded to f16 once, one MFMA per product); without emb_dim "f16" stays refused on DGN."""
        code = NUMERIC_MODES[mode]
        if emb_dim is None:
            self._check(self.lib.flowgnn_set_numeric_mode(self._h, code), "flowgnn_set_numeric_mode")
        elif self.model == "DGN":
            if int(emb_dim) != 100:
                raise ValueError(f"DGN's width is 100, not {emb_dim}")
            self._check(self.lib.flowgnn_set_model_numeric_mode(self._h, _lib.MODEL_IDS["DGN"], code), "flowgnn_set_model_numeric_mode")
        elif self.model == "GCN":
            self._check(self.lib.flowgnn_set_model_numeric_mode_dim(self._h, int(emb_dim), code), "flowgnn_set_model_numeric_mode_dim")
        elif self.model == "PNA":  # (emb_dim=80: the one way to PNA's "f16")
            self._check(self.lib.flowgnn_set_model_numeric_mode_dim(self._h, int(emb_dim), code), "flowgnn_set_model_numeric_mode_dim")
        else:
            self._check(self.lib.flowgnn_set_numeric_mode_dim(self._h, int(emb_dim), code), "flowgnn_set_numeric_mode_dim")

    def set_pooling(self, mode: str = "mean"):
        """The readout's pooling: "mean" (default, the reference's), "sum" or "max" (flowgnn.h: flowgnn_set_pooling; GIN, GIN-VN, GCN,
        GAT).  The engine's, across batches; `embeddings()` then returns the sum / the maximum, the vector the head is applied to."""
        self._check(self.lib.flowgnn_set_pooling(self._h, POOLING_MODES[mode]), "flowgnn_set_pooling")

    def pooling(self) -> str:
        code = int(self.lib.flowgnn_pooling(self._h))
        return next(k for k, v in POOLING_MODES.items() if v == code)

    def set_gin_eps(self, eps=None):
        """GIN / GIN-VN: apply a trained eps, five values, one per layer -- a[v] = (1 + eps[l]) h[v] + sum of messages (flowgnn.h:
        flowgnn_set_gin_eps).  None turns it off (the default: the reference has no eps).  The engine's, across batches and weight sets."""
        self._check(self.lib.flowgnn_set_gin_eps(self._h, _eps_arg(eps, self.num_layers)), "flowgnn_set_gin_eps")

    def gin_eps(self):
        """The five values as float32[5] (float32[num_layers] after set_num_layers), or None while eps is off (flowgnn.h: flowgnn_gin_eps)."""
        out = np.zeros(self.num_layers, np.float32)
        return out if int(self.lib.flowgnn_gin_eps(self._h, _pf(out))) == 1 else None

    def set_ogb_virtual_node(self, vn=None):
        """GIN: run OGB's virtual node (gnn_type='gin-virtual'; flowgnn.h: flowgnn_set_ogb_virtual_node).  `vn`: a dict with the keys
        vn_embedding [100], w1 [4][200][100], b1 [4][200], w2 [4][100][200], b2 [4][100] (BatchNorms folded:
        export.gin_virtual_node_from_ogb_state_dict); None turns it off.  The engine's, across batches and weight sets.
        300-wide tensors ([300], [4][600][300], ...: weights.gin_virtual_node_shapes(300)) go through the call that carries the width,
        flowgnn_set_ogb_virtual_node_dim, for an engine at set_emb_dim(300); 100-wide ones through the call that has none."""
        a = _ogb_vn_args(vn, num_layers=self.num_layers)
        if _ogb_vn_dim(a) == 100:  # (at width 300 that is the call's own refusal: it has no width argument)
            self._check(self.lib.flowgnn_set_ogb_virtual_node(self._h, *[_pf(x) for x in a]), "flowgnn_set_ogb_virtual_node")
        else:
            self._check(self.lib.flowgnn_set_ogb_virtual_node_dim(self._h, _ogb_vn_dim(a), *[_pf(x) for x in a]), "flowgnn_set_ogb_virtual_node_dim")

    def ogb_virtual_node(self) -> bool:
        """Whether OGB's virtual node is on (flowgnn.h: flowgnn_ogb_virtual_node)."""
        return int(self.lib.flowgnn_ogb_virtual_node(self._h)) == 1

    def set_gcn_virtual_node(self, vn=None):
        """GCN: run OGB's virtual node (gnn_type='gcn-virtual'; flowgnn.h: flowgnn_set_gcn_virtual_node).  `vn`: the dict of
        set_ogb_virtual_node (export.gcn_virtual_node_from_ogb_state_dict); None turns it off.  The engine's, across batches and
        weight sets.  300-wide tensors go through the call that carries the width, flowgnn_set_gcn_virtual_node_dim, for an engine at
        set_model_emb_dim(300) (on any other: ValueError); 100-wide ones through the call that has none."""
        a = _gcn_vn_args(vn, self.emb_dim, self.num_layers)
        if _ogb_vn_dim(a) == 100:  # (at width 300 that is the call's own refusal: it has no width argument)
            self._check(self.lib.flowgnn_set_gcn_virtual_node(self._h, *[_pf(x) for x in a]), "flowgnn_set_gcn_virtual_node")
        else:
            self._check(self.lib.flowgnn_set_gcn_virtual_node_dim(self._h, _ogb_vn_dim(a), *[_pf(x) for x in a]), "flowgnn_set_gcn_virtual_node_dim")

    def gcn_virtual_node(self) -> bool:
        """Whether GCN's virtual node is on (flowgnn.h: flowgnn_gcn_virtual_node)."""
        return int(self.lib.flowgnn_gcn_virtual_node(self._h)) == 1

    def set_attention_pooling(self, gate=None):
        """GIN, GCN at width 300: OGB's graph_pooling="attention" readout (flowgnn.h: flowgnn_set_attention_pooling).  `gate`: a dict
        with the keys w1 [600][300], b1 [600], w2 [600] (the gate's BatchNorm folded, its last bias dropped:
        export.attention_pooling_from_ogb_state_dict); the width is read off w1.  None turns it off.  The engine's, across batches and
        weight sets; `embeddings()` then returns the softmax-weighted sums, the vectors the head is applied to."""
        d, a = _attn_pool_args(gate)
        self._check(self.lib.flowgnn_set_attention_pooling(self._h, d, *[_pf(x) for x in a]), "flowgnn_set_attention_pooling")

    def attention_pooling(self) -> bool:
        """Whether the attention readout is on (flowgnn.h: flowgnn_attention_pooling)."""
        return int(self.lib.flowgnn_attention_pooling(self._h)) == 1

    def set_set2set_pooling(self, s2s=None, steps: int = 2):
        """GIN, GCN at width 300: OGB's graph_pooling="set2set" readout (flowgnn.h: flowgnn_set_set2set_pooling).  `s2s`: a dict with the
        keys of weights.SET2SET_KEYS (weights.load_set2set, weights.synth_set2set, export.set2set_from_ogb_state_dict); the width is
        read off w_hh and NUM_TASK off head_b.  steps: the processing steps, 1 .. 8 (OGB: 2).  None turns it off.  The engine's, across
        batches and weight sets; while it is on the model's own head is not read."""
        d, t, a = _s2s_args(s2s)
        self._check(self.lib.flowgnn_set_set2set_pooling(self._h, d, int(steps), t, *[_pf(x) for x in a]), "flowgnn_set_set2set_pooling")

    def set2set_pooling(self) -> int:
        """The set2set readout's processing steps, 0 when it is off (flowgnn.h: flowgnn_set2set_pooling)."""
        return int(self.lib.flowgnn_set2set_pooling(self._h))

    def set_jk_residual(self, jk: str = "last", residual: bool = False, emb_dim: int = 300):
        """GIN and GCN at width 300: OGB's GNN(JK=..., residual=...) (flowgnn.h: flowgnn_set_jk_residual, and for a GCN engine the model
        form of the call, flowgnn_set_model_jk_residual).  jk: "last" or "sum"; under "sum" the rows the readout pools, node embeddings
        and node logits are the sum of the encoder's rows and every layer's rows, while final_h() stays the last layer's output.
        Neither flag is in a state_dict: the caller passes what the model was trained with.  The engine's, across batches and weight
        sets; ("last", False) is the default state."""
        if self.model == "GCN":
            self._check(self.lib.flowgnn_set_model_jk_residual(self._h, int(emb_dim), _jk_code(jk), int(residual)), "flowgnn_set_model_jk_residual")
        else:
            self._check(self.lib.flowgnn_set_jk_residual(self._h, int(emb_dim), _jk_code(jk), int(residual)), "flowgnn_set_jk_residual")

    def jk_residual(self):
        """(jk, residual) as set_jk_residual takes them (flowgnn.h: flowgnn_jk_residual)."""
        jk, res = C.c_int(0), C.c_int(0)
        self.lib.flowgnn_jk_residual(self._h, C.byref(jk), C.byref(res))
        return JK_NAMES[jk.value], bool(res.value)

    def exact_reruns(self) -> int:
        """Forward passes repeated on the exact-fp32 kernels (flowgnn.h: flowgnn_exact_reruns)."""
        return int(self.lib.flowgnn_exact_reruns(self._h))

    def graph_replays(self) -> int:
        """Runs that were hipGraph replays of the recorded launch sequence (flowgnn.h: flowgnn_graph_replays)."""
        return int(self.lib.flowgnn_graph_replays(self._h))

    def csr(self):
        n, e = self.total_nodes, self.total_edges
        row_ptr = np.empty(n + 1, dtype=np.int32)
        src = np.empty(e, dtype=np.int32)
        eid = np.empty(e, dtype=np.int32)
        out_deg = np.empty(n, dtype=np.int32)
        self._check(self.lib.flowgnn_get_csr(self._h, _pi(row_ptr), _pi(src), _pi(eid), _pi(out_deg)), "flowgnn_get_csr")
        return row_ptr, src, eid, out_deg

    def final_h(self) -> np.ndarray:
        dim = C.c_int()
        self._check(self.lib.flowgnn_get_h(self._h, None, C.byref(dim)), "flowgnn_get_h")
        h = np.empty((self.total_nodes, dim.value), dtype=np.float32)
        self._check(self.lib.flowgnn_get_h(self._h, _pf(h), C.byref(dim)), "flowgnn_get_h")
        return h

    # ---- profiling
    def profile_enable(self, on: bool = True):
        self._check(self.lib.flowgnn_profile_enable(self._h, 1 if on else 0), "flowgnn_profile_enable")

    def profile_read(self) -> Dict[str, Dict[str, float]]:
        n = C.c_int()
        names = (C.c_char_p * 32)()
        ms = (C.c_double * 32)()
        cnt = (C.c_longlong * 32)()
        self._check(self.lib.flowgnn_profile_read(self._h, C.byref(n), names, ms, cnt), "flowgnn_profile_read")
        return {names[i].decode(): {"total_ms": ms[i], "launches": int(cnt[i])} for i in range(n.value)}

    def aggregation_only_ms(self, layer: int = 0, iters: int = 10) -> float:
        ms = C.c_float()
        self._check(self.lib.flowgnn_run_aggregation_only(self._h, layer, iters, C.byref(ms)),
                    "flowgnn_run_aggregation_only")
        return float(ms.value)


    def aggregate(self, layer: int = 0):
        """(rows read, aggregate written) by the standalone aggregation kernel of `layer` (flowgnn_get_aggregate)."""
        din, dagg = C.c_int(), C.c_int()
        self._check(self.lib.flowgnn_get_aggregate(self._h, layer, None, C.byref(din), None, C.byref(dagg)), "flowgnn_get_aggregate")
        h = np.empty((self.total_nodes, din.value), dtype=np.float32)
        a = np.empty((self.total_nodes, dagg.value), dtype=np.float32)
        self._check(self.lib.flowgnn_get_aggregate(self._h, layer, _pf(h), C.byref(din), _pf(a), C.byref(dagg)), "flowgnn_get_aggregate")
        return h, a

    def set_stream(self, stream_handle: Optional[int]):
        """Launch on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); None restores the engine's own."""
        if stream_handle is None:
            self._check(self.lib.flowgnn_set_stream(self._h, None, 0), "flowgnn_set_stream")
        else:
            self._check(self.lib.flowgnn_set_stream(self._h, C.c_void_p(stream_handle), 1), "flowgnn_set_stream")


class EngineGroup:
    """Several engines behind one handle (flowgnn.h: flowgnn_create_multi): the batch is cut into contiguous graph ranges
    balanced by sum(N + E), one engine + host thread per listed device; results come back in job order."""

    def __init__(self, model: str, devices, options: Optional[Dict[str, float]] = None):
        self.lib = _lib.load()
        self.model = model.upper()
        self.devices = [int(d) for d in devices]
        self._h = C.c_void_p()
        ids = _i32(self.devices)
        rc = self.lib.flowgnn_create_multi(_lib.MODEL_IDS[self.model], len(self.devices), _pi(ids), C.byref(self._h))
        if rc:
            raise FlowGNNError(rc, "flowgnn_create_multi")
        self.num_tasks = 1
        self.num_graphs = 0
        self.total_nodes = 0
        self.total_edges = 0
        for k, v in (options or {}).items():
            self._check(self.lib.flowgnn_group_set_option(self._h, k.encode(), option_value(v)), f"flowgnn_group_set_option({k})")

    def _check(self, rc: int, where: str):
        if rc != 0:
            raise FlowGNNError(rc, where, (self.lib.flowgnn_group_last_error(self._h) or b"").decode(errors="replace"))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.flowgnn_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_weights(self, w: Dict[str, np.ndarray]):
        _check_weights_depth(self.model, w, self.num_layers)
        arrs = [_f32(v) for v in w.values()]
        ptrs = (_lib.p_float * len(arrs))(*[_pf(a) for a in arrs])
        self._check(self.lib.flowgnn_group_set_weights(self._h, len(arrs), ptrs), "flowgnn_group_set_weights")

    def load_weights_dir(self, directory: str):
        self._check(self.lib.flowgnn_group_load_weights_dir(self._h, directory.encode()), "flowgnn_group_load_weights_dir")

    def set_num_tasks(self, num_tasks: int):
        self._check(self.lib.flowgnn_group_set_num_tasks(self._h, int(num_tasks)), "flowgnn_group_set_num_tasks")
        self.num_tasks = int(num_tasks)

    def set_emb_dim(self, emb_dim: int):
        """GIN's width on every member (flowgnn.h: flowgnn_group_set_emb_dim); weights and batch have to be set again afterwards."""
        self._check(self.lib.flowgnn_group_set_emb_dim(self._h, int(emb_dim)), "flowgnn_group_set_emb_dim")

    def set_model_emb_dim(self, emb_dim: int):
        """GIN's or GCN's width on every member (flowgnn.h: flowgnn_group_set_model_emb_dim)."""
        self._check(self.lib.flowgnn_group_set_model_emb_dim(self._h, int(emb_dim)), "flowgnn_group_set_model_emb_dim")

    def set_num_layers(self, n: int, emb_dim: int = 300):
        """Engine.set_num_layers on every member (flowgnn.h: flowgnn_group_set_num_layers); weights and batch have to be set again afterwards."""
        self._check(self.lib.flowgnn_group_set_num_layers(self._h, int(emb_dim), int(n)), "flowgnn_group_set_num_layers")

    @property
    def num_layers(self) -> int:
        """The members' depth (the first member answers, as for the width)."""
        return int(self.lib.flowgnn_num_layers(self.lib.flowgnn_group_engine(self._h, 0)))

    @property
    def emb_dim(self) -> int:
        """The members' width (they are one model with one setting: the first member answers)."""
        return int(self.lib.flowgnn_emb_dim(self.lib.flowgnn_group_engine(self._h, 0)))

    def set_numeric_mode(self, mode: str = "f32", emb_dim: Optional[int] = None):
        """Engine.set_numeric_mode on every member (flowgnn.h: flowgnn_group_set_numeric_mode; with emb_dim: ..._dim; GCN, and PNA
        with emb_dim=80: flowgnn_group_set_model_numeric_mode_dim; DGN with emb_dim=100: flowgnn_group_set_model_numeric_mode)."""
        if emb_dim is None:
            self._check(self.lib.flowgnn_group_set_numeric_mode(self._h, NUMERIC_MODES[mode]), "flowgnn_group_set_numeric_mode")
        elif self.model == "DGN":
            if int(emb_dim) != 100:
                raise ValueError(f"DGN's width is 100, not {emb_dim}")
            self._check(self.lib.flowgnn_group_set_model_numeric_mode(self._h, _lib.MODEL_IDS["DGN"], NUMERIC_MODES[mode]),
                        "flowgnn_group_set_model_numeric_mode")
        elif self.model == "GCN":
            self._check(self.lib.flowgnn_group_set_model_numeric_mode_dim(self._h, int(emb_dim), NUMERIC_MODES[mode]),
                        "flowgnn_group_set_model_numeric_mode_dim")
        elif self.model == "PNA":
            self._check(self.lib.flowgnn_group_set_model_numeric_mode_dim(self._h, int(emb_dim), NUMERIC_MODES[mode]),
                        "flowgnn_group_set_model_numeric_mode_dim")
        else:
            self._check(self.lib.flowgnn_group_set_numeric_mode_dim(self._h, int(emb_dim), NUMERIC_MODES[mode]), "flowgnn_group_set_numeric_mode_dim")

    def set_pooling(self, mode: str = "mean"):
        """Engine.set_pooling on every member (flowgnn.h: flowgnn_group_set_pooling)."""
        self._check(self.lib.flowgnn_group_set_pooling(self._h, POOLING_MODES[mode]), "flowgnn_group_set_pooling")

    def set_gin_eps(self, eps=None):
        """Engine.set_gin_eps on every member (flowgnn.h: flowgnn_group_set_gin_eps)."""
        self._check(self.lib.flowgnn_group_set_gin_eps(self._h, _eps_arg(eps, self.num_layers)), "flowgnn_group_set_gin_eps")

    def set_ogb_virtual_node(self, vn=None):
        """Engine.set_ogb_virtual_node on every member (flowgnn.h: flowgnn_group_set_ogb_virtual_node)."""
        a = _ogb_vn_args(vn, num_layers=self.num_layers)
        if _ogb_vn_dim(a) == 100:
            self._check(self.lib.flowgnn_group_set_ogb_virtual_node(self._h, *[_pf(x) for x in a]), "flowgnn_group_set_ogb_virtual_node")
        else:
            self._check(self.lib.flowgnn_group_set_ogb_virtual_node_dim(self._h, _ogb_vn_dim(a), *[_pf(x) for x in a]),
                        "flowgnn_group_set_ogb_virtual_node_dim")

    def set_gcn_virtual_node(self, vn=None):
        """Engine.set_gcn_virtual_node on every member (flowgnn.h: flowgnn_group_set_gcn_virtual_node)."""
        a = _gcn_vn_args(vn, self.emb_dim, self.num_layers)
        if _ogb_vn_dim(a) == 100:
            self._check(self.lib.flowgnn_group_set_gcn_virtual_node(self._h, *[_pf(x) for x in a]), "flowgnn_group_set_gcn_virtual_node")
        else:
            self._check(self.lib.flowgnn_group_set_gcn_virtual_node_dim(self._h, _ogb_vn_dim(a), *[_pf(x) for x in a]),
                        "flowgnn_group_set_gcn_virtual_node_dim")

    def set_attention_pooling(self, gate=None):
        """Engine.set_attention_pooling on every member (flowgnn.h: flowgnn_group_set_attention_pooling)."""
        d, a = _attn_pool_args(gate)
        self._check(self.lib.flowgnn_group_set_attention_pooling(self._h, d, *[_pf(x) for x in a]), "flowgnn_group_set_attention_pooling")

    def set_jk_residual(self, jk: str = "last", residual: bool = False, emb_dim: int = 300):
        """Engine.set_jk_residual on every member (flowgnn.h: flowgnn_group_set_jk_residual; GCN: flowgnn_group_set_model_jk_residual)."""
        if self.model == "GCN":
            self._check(self.lib.flowgnn_group_set_model_jk_residual(self._h, int(emb_dim), _jk_code(jk), int(residual)),
                        "flowgnn_group_set_model_jk_residual")
        else:
            self._check(self.lib.flowgnn_group_set_jk_residual(self._h, int(emb_dim), _jk_code(jk), int(residual)), "flowgnn_group_set_jk_residual")

    def set_set2set_pooling(self, s2s=None, steps: int = 2):
        """Engine.set_set2set_pooling on every member (flowgnn.h: flowgnn_group_set_set2set_pooling)."""
        d, t, a = _s2s_args(s2s)
        self._check(self.lib.flowgnn_group_set_set2set_pooling(self._h, d, int(steps), t, *[_pf(x) for x in a]), "flowgnn_group_set_set2set_pooling")

    def set_batch(self, batch: GraphBatch):
        nn, ne = _i32(batch.nums_of_nodes), _i32(batch.nums_of_edges)
        nf, el, ea = _i32(batch.node_feature), _i32(batch.edge_list), _i32(batch.edge_attr)
        eig = None if batch.node_eigen is None else _f32(batch.node_eigen)
        self._check(self.lib.flowgnn_group_set_batch(self._h, batch.num_graphs, _pi(nn), _pi(ne), _pi(nf), _pi(el), _pi(ea), _pf(eig)),
                    "flowgnn_group_set_batch")
        self.num_graphs = batch.num_graphs
        self.total_nodes = batch.total_nodes
        self.total_edges = batch.total_edges

    def shards(self):
        cuts = np.zeros(len(self.devices) + 1, dtype=np.int32)
        self._check(self.lib.flowgnn_group_shards(self._h, _pi(cuts)), "flowgnn_group_shards")
        return [(int(cuts[i]), int(cuts[i + 1])) for i in range(len(self.devices))]

    def run(self):
        self._check(self.lib.flowgnn_group_run(self._h), "flowgnn_group_run")

    def sync(self):
        self._check(self.lib.flowgnn_group_sync(self._h), "flowgnn_group_sync")

    def results(self) -> np.ndarray:
        out = np.empty(self.num_graphs * self.num_tasks, dtype=np.float32)
        self._check(self.lib.flowgnn_group_get_results(self._h, _pf(out)), "flowgnn_group_get_results")
        return out.reshape(self.num_graphs, self.num_tasks) if self.num_tasks > 1 else out

    def set_embeddings(self, on: bool = True):
        self._check(self.lib.flowgnn_group_set_embeddings(self._h, 1 if on else 0), "flowgnn_group_set_embeddings")

    def embeddings(self) -> np.ndarray:
        """[G][embedding_dim(model)] of the last run, in job order (flowgnn.h: flowgnn_group_get_embeddings)."""
        out = np.empty((self.num_graphs, self.emb_dim), dtype=np.float32)
        self._check(self.lib.flowgnn_group_get_embeddings(self._h, _pf(out)), "flowgnn_group_get_embeddings")
        return out

    def set_node_embeddings(self, on: bool = True):
        self._check(self.lib.flowgnn_group_set_node_embeddings(self._h, 1 if on else 0), "flowgnn_group_set_node_embeddings")

    def node_embeddings(self) -> np.ndarray:
        """[N][embedding_dim(model)] of the last run, in job order (flowgnn.h: flowgnn_group_get_node_embeddings)."""
        out = np.empty((self.total_nodes, self.emb_dim), dtype=np.float32)
        self._check(self.lib.flowgnn_group_get_node_embeddings(self._h, _pf(out)), "flowgnn_group_get_node_embeddings")
        return out

    def set_node_logits(self, on: bool = True):
        self._check(self.lib.flowgnn_group_set_node_logits(self._h, 1 if on else 0), "flowgnn_group_set_node_logits")

    def set_attention(self, layers="last"):
        mask = attention_mask(self.model, layers)
        self._check(self.lib.flowgnn_group_set_attention(self._h, mask), "flowgnn_group_set_attention")
        self._attn_mask = mask

    def attention(self):
        """(edge [n_sel][E][4], self [n_sel][N][4]) of the last run, in job order (flowgnn.h: flowgnn_group_get_attention)."""
        n_sel = bin(getattr(self, "_attn_mask", 0)).count("1")
        edge = np.empty((n_sel, self.total_edges, 4), dtype=np.float32)
        own = np.empty((n_sel, self.total_nodes, 4), dtype=np.float32)
        self._check(self.lib.flowgnn_group_get_attention(self._h, _pf(edge), _pf(own)), "flowgnn_group_get_attention")
        return edge, own

    def node_logits(self) -> np.ndarray:
        """[N], or [N][num_tasks], of the last run, in job order (flowgnn.h: flowgnn_group_get_node_logits)."""
        out = np.empty((self.total_nodes, self.num_tasks) if self.num_tasks > 1 else (self.total_nodes,), dtype=np.float32)
        self._check(self.lib.flowgnn_group_get_node_logits(self._h, _pf(out)), "flowgnn_group_get_node_logits")
        return out

    def forward(self, batch: GraphBatch) -> np.ndarray:
        self.set_batch(batch)
        self.run()
        return self.results()

    def compute(self, batch: GraphBatch, chunks_per_engine: int = 1) -> np.ndarray:
        """flowgnn_group_compute: the host batch cut into size x chunks_per_engine ranges, engine i taking ranges i, i + size, ...
        (set_batch, run, results) so that one engine's host -> device copies overlap the others' kernels.  The engines are left on
        their last range: run() / results() / shards() raise FLOWGNN_ERR_STATE until the next set_batch."""
        nn, ne = _i32(batch.nums_of_nodes), _i32(batch.nums_of_edges)
        nf, el, ea = _i32(batch.node_feature), _i32(batch.edge_list), _i32(batch.edge_attr)
        eig = None if batch.node_eigen is None else _f32(batch.node_eigen)
        out = np.empty(batch.num_graphs * self.num_tasks, dtype=np.float32)
        self._check(self.lib.flowgnn_group_compute(self._h, batch.num_graphs, _pi(nn), _pi(ne), _pi(nf), _pi(el), _pi(ea), _pf(eig), _pf(out),
                                                   int(chunks_per_engine)), "flowgnn_group_compute")
        return out.reshape(batch.num_graphs, self.num_tasks) if self.num_tasks > 1 else out


def shard_ranges_c(nums_of_nodes, nums_of_edges, parts: int):
    """flowgnn_shard_ranges (the C ABI's cut by cumulative node + edge count); pure host code, no GPU needed."""
    lib = _lib.load()
    nn, ne = _i32(nums_of_nodes), _i32(nums_of_edges)
    cuts = np.zeros(parts + 1, dtype=np.int32)
    rc = lib.flowgnn_shard_ranges(len(nn), _pi(nn), _pi(ne), parts, _pi(cuts))
    if rc:
        raise FlowGNNError(rc, "flowgnn_shard_ranges")
    return [(int(cuts[i]), int(cuts[i + 1])) for i in range(parts)]


def entry_set_devices(devices):
    """Devices of the <M>_compute_graphs entry points (flowgnn.h: flowgnn_entry_set_devices)."""
    ids = _i32(list(devices))
    rc = _lib.load().flowgnn_entry_set_devices(len(ids), _pi(ids))
    if rc:
        raise FlowGNNError(rc, "flowgnn_entry_set_devices")


def entry_set_pipeline(chunks_per_engine: int):
    """Ranges per engine of the entry points' host-array pipeline (flowgnn.h: flowgnn_entry_set_pipeline; 0 = by size, 1 = off)."""
    rc = _lib.load().flowgnn_entry_set_pipeline(int(chunks_per_engine))
    if rc:
        raise FlowGNNError(rc, "flowgnn_entry_set_pipeline")


def entry_set_option(model: str, key: str, value):
    rc = _lib.load().flowgnn_entry_set_option(_lib.MODEL_IDS[model.upper()], key.encode(), option_value(value))
    if rc:
        raise FlowGNNError(rc, f"flowgnn_entry_set_option({key})")


def entry_set_pooling(model: str, mode: str = "mean"):
    """The readout's pooling for the engines behind `model`'s <M>_compute_graphs symbols (flowgnn.h: flowgnn_entry_set_pooling)."""
    rc = _lib.load().flowgnn_entry_set_pooling(_lib.MODEL_IDS[model.upper()], POOLING_MODES[mode])
    if rc:
        raise FlowGNNError(rc, f"flowgnn_entry_set_pooling({mode})")


def entry_set_gin_eps(model: str, eps=None):
    """A trained eps for the engines behind `model`'s <M>_compute_graphs symbols, one vector for every weight set; None: off
    (flowgnn.h: flowgnn_entry_set_gin_eps)."""
    lib = _lib.load()
    rc = lib.flowgnn_entry_set_gin_eps(_lib.MODEL_IDS[model.upper()], _eps_arg(eps))
    if rc:
        raise FlowGNNError(rc, "flowgnn_entry_set_gin_eps", (lib.flowgnn_last_error(None) or b"").decode())


def compute_graphs(model: str, batch: GraphBatch, weight_sets, reload_weights=None, num_tasks: int = 1) -> np.ndarray:
    """Call the reference-compatible C symbol <M>_compute_graphs (e.g. GIN/src/dcl.h:75-94) with host
    arrays.  `weight_sets` is a list of weight dicts: the leading [S] dimension of every weight pointer,
    selected per graph by the running count of reload_weights (GIN/src/GIN_compute.cc:51-53)."""
    lib = _lib.load()
    model = model.upper()
    G = batch.num_graphs
    if reload_weights is None:
        reload_weights = np.zeros(G, dtype=np.int32)
        if G:
            reload_weights[0] = 1
    stacked = [np.ascontiguousarray(np.stack([np.asarray(ws[k], dtype=np.float32) for ws in weight_sets]))
               for k in weight_sets[0].keys()]  # [S, ...] per tensor (avg_deg: [S, 1] == float[S])
    out = np.zeros(G * num_tasks, dtype=np.float32)
    if num_tasks != 1 and model not in ("GIN", "GIN-VN", "GCN"):
        raise FlowGNNError(8, f"{model}_compute_graphs", "this model's readout is a single-task MLP head (NUM_TASK != 1 exists for GIN / GIN-VN / GCN)")
    nn, ne, rw = _i32(batch.nums_of_nodes), _i32(batch.nums_of_edges), _i32(reload_weights)
    nf, el, ea = _i32(batch.node_feature), _i32(batch.edge_list), _i32(batch.edge_attr)
    wp = [_pf(a) for a in stacked]
    if model in ("GIN", "GIN-VN"):
        if num_tasks == 1:
            rc = lib.GIN_compute_graphs(G, _pi(nn), _pi(ne), _pi(rw), _pf(out), _pi(nf), _pi(el), _pi(ea), *wp)
        else:  # NUM_TASK, a compile-time constant of the reference build, is an explicit argument here
            rc = lib.GIN_compute_graphs_mt(G, _pi(nn), _pi(ne), _pi(rw), _pf(out), _pi(nf), _pi(el), _pi(ea), *wp, num_tasks)
    elif model == "GCN":
        if num_tasks == 1:
            rc = lib.GCN_compute_graphs(G, _pi(nn), _pi(ne), _pi(rw), _pf(out), _pi(nf), _pi(el), _pi(ea), *wp)
        else:
            rc = lib.GCN_compute_graphs_mt(G, _pi(nn), _pi(ne), _pi(rw), _pf(out), _pi(nf), _pi(el), _pi(ea), *wp, num_tasks)
    elif model == "PNA":
        rc = lib.PNA_compute_graphs(G, _pi(nn), _pi(ne), _pi(rw), _pf(out), _pi(nf), _pi(el), *wp)
    elif model == "GAT":
        rc = lib.GAT_compute_graphs(G, _pi(nn), _pi(ne), _pi(rw), _pf(out), _pi(nf), _pi(el), *wp)
    elif model == "DGN":
        eig = _f32(batch.node_eigen)
        rc = lib.DGN_compute_graphs(G, _pi(nn), _pi(ne), _pi(rw), _pf(out), _pi(nf), _pf(eig), _pi(el), *wp)
    else:
        raise ValueError(model)
    if rc:
        raise FlowGNNError(rc, f"{model}_compute_graphs")
    return out.reshape(G, num_tasks) if num_tasks > 1 else out


def GIN_compute_graphs(batch: GraphBatch, weight_sets, reload_weights=None) -> np.ndarray:
    return compute_graphs("GIN", batch, weight_sets, reload_weights)


def GCN_compute_graphs(batch: GraphBatch, weight_sets, reload_weights=None) -> np.ndarray:
    return compute_graphs("GCN", batch, weight_sets, reload_weights)
