"""The width-300 family's shape cases, seeded random batches and instance table: what tests/test_wide_shapes_cpu.py proves conditions
on and tests/test_wide_shapes_gpu.py and scripts/dev/fuzz_wide.py run.  Nothing here knows what a GPU
returns, and nothing but engine() needs one.  A helper module, not a conftest: nothing is collected from it.

  graph / path / isolated / hub   the builders of tests/test_gin_wide_gpu.py (moved here; that file imports them).
  random_batch(seed, family)      rand_graph of scripts/dev/fuzz.py under the caps of CAPS[family]; a pure function of its arguments.
  INSTANCES                       kind x virtual node x (jk, residual), default numeric mode, and gin's eight again in f16 mode: 24.
  fixed_cases(instance)           the fixed shape families (a) .. (f) the default instances already pass, by name.
  weights_dir / tensors           the damped make_model(...) of ogb_jk_torch / ogb_gcn_jk_torch through export_weights, once per process.
  engine(instance)                the instance's engine, as the GPU test and the fuzzer build it.
  reference / operands            the float64 forward of the instance on a batch (f16=True for the f16 rows); its largest guarded operand.

Caps (why, and the maxima measured with them: tests/test_wide_shapes_cpu.py's docstring).  GCN normalises a neighbour sum by the
degrees, GIN does not: a GIN row's a grows with its in-degree in every layer, so the GIN families bound the in-degree, the graph size
(t of the virtual node's update is a sum over the graph's nodes) and the hub's leaf count; the tile-edge paths (in-degree 2) need none.
"""
import functools
import tempfile
from collections import namedtuple

import numpy as np

from flowgnn_amd import graphpack as gp

CARDS = (119, 4, 12, 12, 10, 6, 6, 2, 2)
EDGE_COUNTS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]  # every power-of-two row tile up to 256 at its edge and one past it
TILE_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)  # the random graphs' sizes at the 16-row and 128-row tiles' edges
GRAPH_COUNTS = (1, 15, 16, 17, 33)  # around the update's 16-graph column tile
SEEDS = (1, 2, 3)  # the suite's random batches; fuzz_wide.py takes any
RANGE_LIMIT = 3.0e4  # half the kernels' 6e4 threshold: the margin tests/test_jk_residual_cpu.py uses


# ---------------------------------------------------------------- shape builders
def graph(n, edges, seed):
    """One graph of n nodes with the directed edges [(src, dst)]; the edge attributes walk through all 60 (a0, a1, a2) codes."""
    rng = np.random.default_rng(seed)
    nf = np.stack([rng.integers(0, c, n) for c in CARDS], 1).astype(np.int32)
    el = np.asarray(edges, np.int32).reshape(-1, 2)
    code = (np.arange(len(el)) + seed) % 60
    ea = np.stack([code // 12, (code // 2) % 6, code % 2], 1).astype(np.int32)
    return gp.GraphBatch(np.array([n], np.int32), np.array([len(el)], np.int32), nf, el, ea)


def path(n, seed):
    fwd = [(i, i + 1) for i in range(n - 1)]
    return graph(n, fwd + [(b, a) for a, b in fwd], seed)


def isolated(n, seed):
    return graph(n, [], seed)


def hub(leaves, seed):
    """Node 0 has `leaves` in-edges and no out-edge: with edges back to the leaves the activations grow by `leaves` every two layers and
    leave the split's range at 300 leaves (the exact re-run would then compute the result, not the kernel under test)."""
    return graph(leaves + 1, [(i, 0) for i in range(1, leaves + 1)], seed)


def many(G, seed):
    """G small graphs (1 .. 5 nodes): tests/test_gin_wide_vn_gpu.py's."""
    return gp.concat_batches([path(1 + (i * 7 + seed) % 5, 1000 * seed + i) for i in range(G)])


def total_of(N, seed):
    """Paths whose node counts add up to N exactly (the last one takes what is left)."""
    sizes, k = [], 0
    while sum(sizes) < N:
        sizes.append(min((37, 5, 1, 64, 23, 2, 16)[k % 7], N - sum(sizes)))
        k += 1
    return gp.concat_batches([path(n, 10 * seed + i) for i, n in enumerate(sizes)])


# ---------------------------------------------------------------- the seeded generator
Caps = namedtuple("Caps", "max_nodes densities max_dups max_indeg hub_leaves")
# family -> Caps: nodes per graph (the fixed families' graphs too), the edges-per-node choices, duplicated edges per graph, in-degree
# (None: no cap), leaves of family (c)'s hub
DENSITIES = (0.0, 0.5, 1.0, 2.2, 4.0, 16.0)
CAPS = {"gcn": Caps(301, DENSITIES, None, None, 300),
        "gcn-virtual": Caps(129, DENSITIES, None, None, 100),
        "gin": Caps(301, DENSITIES[:4], 3, 6, 40),
        "gin-virtual": Caps(129, DENSITIES[:4], 3, 6, 40)}
RANDOM_MAX_NODES = {"gcn": 129, "gcn-virtual": 129, "gin": 33, "gin-virtual": 33}  # the random graphs' own cap
FAMILIES = tuple(CAPS)


def family_of(instance):
    return instance.kind + ("-virtual" if instance.vn else "")


def pieces(n, family):
    """n as the node counts of graphs within the family's cap: n itself, or 128-node graphs and a rest (the batch's rows stay where
    they were: what lies at a tile's edge still does)."""
    cap, out = CAPS[family].max_nodes, []
    while n > cap:
        out.append(min(cap, 128))
        n -= out[-1]
    return out + [n]


def rand_graph(rng, caps, max_nodes):
    """scripts/dev/fuzz.py's rand_graph under `caps`: a size from the tile edges (one time in six) or from 1 .. 59, a density, random
    endpoints (self loops and repeated pairs arise by chance; three times in ten some edges are overwritten with copies of one), all
    60 edge codes.  With an in-degree cap the edges beyond it are dropped, in order."""
    kind = rng.integers(0, 6)
    n = int(rng.choice(TILE_SIZES)) if kind == 0 else int(rng.integers(1, 60))
    n = min(n, max_nodes)
    dens = float(rng.choice(caps.densities))
    m = int(min(5500, max(0, round(n * dens + rng.integers(0, 3)))))
    el = rng.integers(0, n, (m, 2)).astype(np.int32)
    if m and rng.random() < 0.3:
        k = max(1, m // 10) if caps.max_dups is None else min(caps.max_dups, max(1, m // 10))
        el[rng.integers(0, m, k)] = el[rng.integers(0, m)]  # duplicates
    if caps.max_indeg is not None and m:
        seen = np.zeros(n, np.int64)
        keep = np.zeros(m, bool)
        for i, d in enumerate(el[:, 1]):
            seen[d] += 1
            keep[i] = seen[d] <= caps.max_indeg
        el = el[keep]
        m = len(el)
    nf = np.stack([rng.integers(0, c, n) for c in CARDS], 1).astype(np.int32)
    ea = np.stack([rng.integers(0, 5, m), rng.integers(0, 6, m), rng.integers(0, 2, m)], 1).astype(np.int32).reshape(m, 3)
    return gp.GraphBatch(np.array([n], np.int32), np.array([m], np.int32), nf, el.reshape(m, 2), ea)


def random_batch(seed, family):
    """1 .. 39 random graphs of `family` (a key of CAPS), tiny and larger ones mixed."""
    rng = np.random.default_rng(int(seed) * 100003 + FAMILIES.index(family))
    return gp.concat_batches([rand_graph(rng, CAPS[family], RANDOM_MAX_NODES[family]) for _ in range(int(rng.integers(1, 40)))])


def shard_cut(seed, batch):
    """The graph index the shard check cuts a random batch at (1 .. G - 1; 0 for a one-graph batch: one shard)."""
    G = batch.num_graphs
    return int(np.random.default_rng(7919 * int(seed) + 13).integers(1, G)) if G > 1 else 0


# ---------------------------------------------------------------- the instance table
Instance = namedtuple("Instance", "kind vn jk res f16")
SETTINGS = (("last", False), ("last", True), ("sum", False), ("sum", True))
INSTANCES = ([Instance(kind, vn, jk, res, False) for kind in ("gin", "gcn") for vn in (False, True) for jk, res in SETTINGS] +
             [Instance("gin", vn, jk, res, True) for vn in (False, True) for jk, res in SETTINGS])
READOUT_INSTANCES = [Instance("gin", False, "sum", True, False), Instance("gcn", False, "sum", True, False)]


def name_of(i):
    return f"{i.kind}{'-virtual' if i.vn else ''}-{i.jk}{'-res' if i.res else ''}{'-f16' if i.f16 else ''}"


IDS = [name_of(i) for i in INSTANCES]
_TMP = []  # the temporary directories, alive as long as the process is


def _module(kind):
    from tests import ogb_gcn_jk_torch, ogb_jk_torch
    return ogb_jk_torch if kind == "gin" else ogb_gcn_jk_torch


@functools.lru_cache(maxsize=None)
def weights_dir(kind, vn, jk, res):
    """The directory export_weights wrote for the damped model of (kind, vn, jk, res): written once per process (the f16 rows share
    the default mode's files)."""
    from flowgnn_amd import export
    model = _module(kind).make_model(vn, jk, res)
    tmp = tempfile.TemporaryDirectory(prefix=f"wide_{kind}{'_vn' if vn else ''}_{jk}{'_res' if res else ''}_")
    _TMP.append(tmp)
    kw = dict(virtual_node=True, virtual_node_dim=300) if vn else {}
    if kind == "gin":
        export.export_weights("GIN", model.state_dict(), tmp.name, keep_eps=True, **kw)
    else:
        export.export_weights("GCN", model.state_dict(), tmp.name, emb_dim=300, **kw)
    return tmp.name


@functools.lru_cache(maxsize=None)
def tensors(kind, vn, jk, res):
    """(w, vn tensors or None, eps or None) of weights_dir(...), as the forwards take them"""
    loaded = _module(kind).load(weights_dir(kind, vn, jk, res), vn)
    return loaded if kind == "gin" else (loaded[0], loaded[1], None)


def engine(i, pooling="mean"):
    """The width first, then the files, then the mode and the flags the model was trained with (tests/test_jk_residual_gpu.engine's and
    tests/test_gcn_jk_residual_gpu.engine's order); profiling on."""
    from flowgnn_amd import Engine
    d = weights_dir(i.kind, i.vn, i.jk, i.res)
    if i.kind == "gin":
        e = Engine("GIN", device=0)
        e.set_emb_dim(300)
        e.load_weights_dir(d, eps=True, virtual_node=i.vn)
    else:
        e = Engine("GCN", device=0)
        e.set_model_emb_dim(300)
        e.load_weights_dir(d, virtual_node=i.vn)
    if pooling != "mean":
        e.set_pooling(pooling)
    if i.f16:
        e.set_numeric_mode("f16", emb_dim=300)
    e.set_jk_residual(i.jk, i.res)
    assert e.jk_residual() == (i.jk, i.res)
    e.profile_enable(True)
    return e


def reference(instance, batch, pooling="mean", drop=None):
    """Ref(logits, rows = r, pooled, h5, scale, operands) of the instance on `batch`, float64 (the f16 rows: the f16 reference)."""
    i = instance
    w, vnt, eps = tensors(i.kind, i.vn, i.jk, i.res)
    if i.kind == "gin":
        return _module("gin").forward(batch, w, vnt, eps=eps, jk=i.jk, residual=i.res, pooling=pooling, f16=i.f16, drop=drop)
    return _module("gcn").forward(batch, w, vnt, jk=i.jk, residual=i.res, pooling=pooling, drop=drop)


def operands(instance, batch):
    """The largest value a range guard of the instance's fast path watches on `batch`, restated from the kernels: GIN (gw_layer_body /
    gw_step, gwf_*): per layer max |a| and the ReLU'd hidden units times pow2_scale(w1[l]), per update max |t| and the hidden units
    times pow2_scale(vn.w1[l]); GCN: x_1 .. x_4, t and the update's pre-scaled hidden units.  The guards compare with 6.0e4f."""
    return reference(instance, batch).operands


# ---------------------------------------------------------------- the fixed shape families
def fixed_cases(instance):
    """name -> batch builder, for this instance: (a) paths at every EDGE_COUNTS size, concatenated; (b) isolated nodes at the same
    sizes; (c) the gather test's batch -- one-node graphs around a hub and a 200-node path, where a destination's sources lie in another
    workgroup's 128-row tile -- with the hub's leaves as CAPS has them; (e) G small graphs, G around the update's 16-graph column tile,
    for the virtual-node rows; (f) total node counts of 128 k + 1, 128 k + 127 and 128 k."""
    fam = family_of(instance)
    leaves = CAPS[fam].hub_leaves
    sizes = [m for n in EDGE_COUNTS for m in pieces(n, fam)]
    long_path = pieces(200, fam)
    cases = {"a-paths": lambda: gp.concat_batches([path(n, 100 + i) for i, n in enumerate(sizes)]),
             "b-isolated": lambda: gp.concat_batches([isolated(n, 100 + i) for i, n in enumerate(sizes)]),
             "c-gather": lambda: gp.concat_batches([isolated(1, 1), hub(leaves, 2), isolated(1, 3), isolated(1, 4)] +
                                                   [path(n, 5 + 10 * i) for i, n in enumerate(long_path)] + [isolated(1, 6)])}
    if instance.vn:
        for G in GRAPH_COUNTS:
            cases[f"e-{G}-graphs"] = lambda G=G: many(G, G)
    for N in (257, 383, 256):
        cases[f"f-{N}-nodes"] = lambda N=N: total_of(N, N)
    return cases


@functools.lru_cache(maxsize=None)
def fixed_batch(family, name):
    return fixed_cases(Instance(family.split("-")[0], family.endswith("-virtual"), "last", False, False))[name]()


@functools.lru_cache(maxsize=None)
def random_case(seed, family):
    return random_batch(seed, family)


def cases_of(instance):
    """[(name, batch)] the GPU test runs for this instance: every fixed family, then the random batches of SEEDS (shared, unchanged)."""
    fam = family_of(instance)
    out = [(name, fixed_batch(fam, name)) for name in fixed_cases(instance)]
    return out + [(f"random-{s}", random_case(s, fam)) for s in SEEDS]


@functools.lru_cache(maxsize=None)
def cached_reference(instance, name, pooling="mean"):
    """reference(instance, the case `name` of cases_of(instance)), computed once and shared; callers leave it unchanged."""
    return reference(instance, dict(cases_of(instance))[name], pooling=pooling)
