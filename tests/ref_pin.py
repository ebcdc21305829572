"""The reference's own kernel sources, compiled against oracle/hls_standin (make -C oracle ref) and called through ctypes: what
tests/test_reference_pin_*.py compare the oracle and the GPU with.  A plain helper module, not a conftest.

Form "f32": ap_fixed is one float, the reference's program runs in fp32; run() returns float32 logits.
Form "fx":  ap_fixed is a 16-bit two's-complement pattern under the operator rules listed in oracle/hls_standin/ap_fixed.h;
            run() returns the int16 patterns.  Weights (and DGN's eigenvectors) are quantised as the oracle's q_from_float does
            it and as ap_fixed's constructor from a float does: floor to the grid, keep the low 16 bits.

The reference keeps its state in globals: one call at a time, one library handle per (model, form).  GIN and GIN-VN have the
same kernel sources and the same entry point; they are two libraries all the same (-Wl,-Bsymbolic keeps each to itself)."""
import ctypes as C
import os
import subprocess

import numpy as np

from flowgnn_amd import graphpack as gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FLOWGNN_REFERENCE", "/root/reference")
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
MODELS = ("GIN", "GIN-VN", "GCN", "GAT", "PNA", "DGN")
FORMS = ("f32", "fx")
FRAC_BITS = {"GIN": 10, "GIN-VN": 10, "GCN": 10, "GAT": 10, "PNA": 10, "DGN": 13}
# the caps of each model's dcl.h (MAX_NODE, MAX_EDGE): the reference's arrays are that large and nothing checks an index
CAPS = {m: (500, 5500) for m in MODELS}
_ENTRY = {"GIN": "GIN_compute_graphs", "GIN-VN": "GIN_compute_graphs", "GCN": "GCN_compute_graphs", "GAT": "GAT_compute_graphs",
          "PNA": "PNA_compute_graphs", "DGN": "DGN_compute_graphs"}
_handles = {}
_built = False


def lib_path(model, form):
    return os.path.join(REF_DIR, f"libref_{model}_{form}.so")


def have_reference_tree():
    return os.path.isdir(os.path.join(REF, "GIN", "src"))


def available():
    """True when all twelve libraries are there, built first if the reference tree is."""
    global _built
    if have_reference_tree() and not _built:
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref", f"REF={REF}"])
        _built = True
    return all(os.path.exists(lib_path(m, f)) for m in MODELS for f in FORMS)


def _lib(model, form):
    key = (model, form)
    if key not in _handles:
        _handles[key] = C.CDLL(lib_path(model, form))
        getattr(_handles[key], _ENTRY[model]).restype = None
    return _handles[key]


def quantise(a, frac_bits):
    """float -> 16-bit pattern: floor(x 2^F), low 16 bits (oracle/q_oracle.c orc_q_from_float)."""
    q = np.floor(np.asarray(a, np.float32).astype(np.float64) * float(1 << frac_bits)).astype(np.int64)
    return np.ascontiguousarray((q & 0xFFFF).astype(np.uint16).view(np.int16))


def inside_caps(model, batch):
    n_cap, e_cap = CAPS[model]
    return bool((batch.nums_of_nodes <= n_cap).all() and (batch.nums_of_edges <= e_cap).all())


def arguments(model, form, batch, weight_sets, reload_weights=None):
    """The arrays <M>_compute_graphs takes after num_graphs, in its order; the fifth of them is the output."""
    G = batch.num_graphs
    if reload_weights is None:
        reload_weights = np.zeros(G, np.int32)
        if G:
            reload_weights[0] = 1
    if form == "f32":
        conv = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
        out = np.zeros(G, np.float32)
    else:
        conv = lambda a: quantise(a, FRAC_BITS[model])  # noqa: E731
        out = np.zeros(G, np.int16)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
    arrays = [i32(batch.nums_of_nodes), i32(batch.nums_of_edges), i32(reload_weights), out, i32(batch.node_feature)]
    if model == "DGN":
        arrays.append(conv(batch.node_eigen))
    arrays.append(i32(batch.edge_list))
    if model in ("GIN", "GIN-VN", "GCN"):
        arrays.append(i32(batch.edge_attr))
    arrays += [conv(np.stack([np.asarray(ws[k], np.float32) for ws in weight_sets])) for k in weight_sets[0].keys()]
    return arrays


def run(model, form, batch, weight_sets, reload_weights=None):
    """<M>_compute_graphs of the reference over a GraphBatch, all graphs in one call."""
    assert inside_caps(model, batch), "a graph beyond MAX_NODE / MAX_EDGE would write outside the reference's arrays"
    arrays = arguments(model, form, batch, weight_sets, reload_weights)
    getattr(_lib(model, form), _ENTRY[model])(C.c_int(batch.num_graphs), *[a.ctypes.data_as(C.c_void_p) for a in arrays])
    return arrays[3]


def dump_call(path, model, form, batch, weight_sets, reload_weights=None):
    """The call run() would make, as a file for oracle/hls_standin/replay.cc (the stand-alone sanitizer build)."""
    arrays = arguments(model, form, batch, weight_sets, reload_weights)
    with open(path, "wb") as f:
        f.write(np.array([batch.num_graphs, len(arrays)], np.int32).tobytes())
        for a in arrays:
            f.write(np.array([a.nbytes], np.int64).tobytes())
            f.write(a.tobytes())


def run_per_graph(model, form, batch, weight_set):
    """One call per graph: every offset the reference keeps across the graphs of a call is 0 (GAT without its offset quirk)."""
    outs = [run(model, form, batch.slice(g, g + 1), [weight_set]) for g in range(batch.num_graphs)]
    return np.concatenate(outs) if outs else np.zeros(0, np.float32 if form == "f32" else np.int16)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _atoms(rng, n):
    return np.stack([rng.integers(0, c, n) for c in (119, 4, 12, 12, 10, 6, 6, 2, 2)], 1).astype(np.int32)


def _bonds(rng, e):
    return np.stack([rng.integers(0, 5, e), rng.integers(0, 6, e), rng.integers(0, 2, e)], 1).astype(np.int32).reshape(e, 3)


def graph(rng, n, edges, eigen=False):
    edges = np.asarray(edges, np.int32).reshape(-1, 2)
    eig = rng.uniform(-0.5, 0.5, (n, 4)).astype(np.float32) if eigen else None
    return gp.GraphBatch(np.array([n], np.int32), np.array([len(edges)], np.int32), _atoms(rng, n), edges, _bonds(rng, len(edges)), eig)


def tiny_graphs(seed, eigen=False):
    """One node; one node with a self loop; three nodes and no edge; two nodes joined both ways; two nodes, one edge."""
    rng = np.random.default_rng(seed)
    return gp.concat_batches([graph(rng, 1, [], eigen), graph(rng, 1, [[0, 0]], eigen), graph(rng, 3, [], eigen),
                              graph(rng, 2, [[0, 1], [1, 0]], eigen), graph(rng, 2, [[1, 0]], eigen)])


def with_eigen(b, seed):
    rng = np.random.default_rng(seed)
    b.node_eigen = rng.uniform(-0.5, 0.5, (b.total_nodes, 4)).astype(np.float32)
    return b


def directed_variant(b):
    """Every sixth edge dropped, so that nodes without out-edges (and without in-edges) exist."""
    keep = np.ones(b.total_edges, bool)
    keep[1::6] = False
    eo = b.edge_offsets()
    ne = np.add.reduceat(keep.astype(np.int64), eo[:-1]).astype(np.int32)
    return gp.GraphBatch(b.nums_of_nodes, ne, b.node_feature, b.edge_list[keep], b.edge_attr[keep],
                         None if b.node_eigen is None else b.node_eigen)


def with_duplicates(b, seed):
    """Duplicate edges and self loops inside every seventh graph; forty copies of one edge in graph 5."""
    rng = np.random.default_rng(seed)
    eo = b.edge_offsets()
    for g in range(0, b.num_graphs, 7):
        e0, ne = int(eo[g]), int(eo[g + 1] - eo[g])
        if ne == 0:
            continue
        for _ in range(12):
            i, k = rng.integers(0, ne, 2)
            b.edge_list[e0 + i] = b.edge_list[e0 + k]
        v = int(rng.integers(0, b.nums_of_nodes[g]))
        b.edge_list[e0 + int(rng.integers(0, ne))] = [v, v]
    if b.num_graphs > 5 and eo[6] - eo[5] >= 40:
        b.edge_list[int(eo[5]):int(eo[5]) + 40] = b.edge_list[int(eo[5])]
    return b


def dataset_batch(model, num_graphs, seed):
    """The synthetic batch of the model's dataset shape: molhiv (GIN, GIN-VN, GAT), molpcba (GCN), hep10k (PNA, DGN)."""
    if model in ("PNA", "DGN"):
        return gp.synth_hep10k_batch(num_graphs, seed=seed, with_eigen=(model == "DGN"))
    b = gp.synth_molpcba_batch(num_graphs, seed=seed) if model == "GCN" else gp.synth_molhiv_batch(num_graphs, seed=seed)
    return gp.add_virtual_nodes(b) if model == "GIN-VN" else b


def capped_graph(model, seed):
    """One graph at both caps of the model's dcl.h, random endpoints (duplicates, self loops, rows of very different in-degree).
    GIN-VN: the virtual node and its 2 N edges are part of the graph the kernel sees, so the molecule under them is smaller."""
    n_cap, e_cap = CAPS[model]
    rng = np.random.default_rng(seed)
    if model == "GIN-VN":
        n = n_cap - 1
        b = graph(rng, n, rng.integers(0, n, (e_cap - 2 * n, 2)))
        b = gp.add_virtual_nodes(b)
        assert int(b.nums_of_nodes[0]) == n_cap and int(b.nums_of_edges[0]) == e_cap
        return b
    return graph(rng, n_cap, rng.integers(0, n_cap, (e_cap, 2)), eigen=(model == "DGN"))
