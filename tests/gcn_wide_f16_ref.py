"""GCN and gcn-virtual at a width read off the weights in the f16 numeric mode (flowgnn.h: flowgnn_set_model_numeric_mode_dim; DESIGN.md
section 4.27), the reference side of tests/test_gcn_wide_f16_cpu.py and tests/test_gcn_wide_f16_gpu.py.  No GPU, and nothing here knows
what a GPU returns.

  forward        tests/ogb_gcn_jk_torch.forward's equations -- the engine's terms: x_l, h_{l+1}, vn_l, r and flowgnn.h's add order, the
                 update unrounded -- with the mode's two roundings in the products x_1 .. x_4 (x_0 is no matrix-pipe product at this
                 width: W_0 is applied to the node table on the host), through tests/f16_ref.rounder / pow2_scale: the operand a, what
                 stands behind the walk, the epilogue, the residual add and the virtual node's add, and the matrix after its
                 power-of-two scale, r(W s) / s.  `rnd` as tests/f16_ref has it: "rne" (the mode), "rtz", "none", or a dict per operand
                 point ("a", "w").  With nothing rounded it IS ogb_gcn_jk_torch.forward (tests/test_gcn_wide_f16_cpu.py checks that to
                 1e-9 x scale, and the plain cases against gcn_wide_ref.forward / gcn_wide_vn_ref.forward).
                 check=True: f16_ref._Exact on every fp32 sum of the mode -- the encoder (the projected table's nine rows and b_0),
                 the edge table, the walk, both epilogue FMAs, the residual and JK adds, the virtual node's add, t and the update's
                 products (where an update has weights), the four products with bias, the pools, the head -- and, for the operands of the
                 update (which the engine multiplies as split f16 pairs hi + lo), that each is such a pair exactly
                 (tests/gin_wide_f16_ref._split_bits).  Two figures are returned, each the largest log2 over its sums -- at most 24 and
                 every partial sum, in any order, is an fp32 value: `rows`, everything up to the rows r, and `pool`, the per-graph
                 sums of r, the head on them and the per-node terms.  The rows' figure is at most 24 in every case of the probe (19.1 .. 23.9) but the one with
                 the virtual node, the JK sum and the residual together (26.0: six terms that the residual doubles from layer to
                 layer, on the grid below); that case's rows are held to bound(), the others' to bits.  The
                 pool's is with the residual, the JK sum and the virtual node off (23.5); with one of them on the rows are larger on
                 the same 2^-19 grid (1 / 16 of a K16 node times the f16 spacing of a times BatchNorm's 1 / 2) and a graph's sum needs
                 24.5 (virtual node), 27.7 (JK sum), 29.2 (residual) and 33.3 bits (all three); no power-of-two scale of the weights
                 changes a ratio.  Those cases pool the mean, which is held to bound() in every case, so nothing is held to bits that
                 is not proven.
  probe_weights / probe_virtual_node / probe_batch     GIN's probe (tests/gin_wide_f16_ref.py) rebuilt for GCN: two non-zeros per row in
                 {1/4, 1/2} (W_1 .. W_4 in the `tight` form, W_0 as it is: the host applies it unrounded), dyadic biases, root and edge
                 rows, BatchNorm with var + eps = 1 and a weight in {1/2, 1} (1 in the last layer), so that the folded scale is a power of two; graphs whose
                 nodes all have degree 0, 3 or 15, so that dinv, 1 / (deg + 1) and every norm are powers of two.
  CASES, separation, NOT_SEPARATED      the probe's cases and what the references can tell apart among themselves.
  ACCURACY, TOL  the realistic-shape inputs and the tolerance ladder of the issue.
"""
import functools
from collections import OrderedDict, namedtuple

import numpy as np

from flowgnn_amd import export, graphpack as gp
from tests import f16_ref
from tests.f16_ref import _Exact, lsb_exp, pow2_scale, rounder
from tests.gin_wide_f16_ref import _split_bits

ND_OFF, ED_OFF = f16_ref.ND_OFF, f16_ref.ED_OFF
L = 5
WIDE = 300
POINTS = ("a", "w")  # the operand points the mode rounds
FACTOR = 100.0  # of the bound, as tests/f16_probe.py has it
BN_EPS = 2.0 ** -10  # the engine's (gcn_wide.hip: sqrt(var + 2^-10))

Out = namedtuple("Out", "logits rows pooled terms h5 scale")
Figures = namedtuple("Figures", "rows pool")  # forward(check=True): every sum up to the rows r | the pools, the head on them and on r


def forward(batch, w, vn=None, jk="last", residual=False, rnd="rne", check=False, pooling="mean", dtype=np.float64):
    """Out(logits [G] or [G][T], r [N][D] -- the rows the readout pools: h_5, or under JK sum the six-term sum --, pooled rows [G][D],
    per-node terms [N] or [N][T], h_5 [N][D], scale); with check=True a pair (Out, Figures).  vn: the five tensors of OGB's virtual node
    or None.  dtype=np.float32: every operation in fp32 (on an input whose figure is at most 24 that is the float64 result bit for bit)."""
    if pooling not in ("mean", "sum", "max") or jk not in ("last", "sum"):
        raise ValueError((pooling, jk))
    if isinstance(rnd, dict):
        if set(rnd) - set(POINTS):
            raise ValueError(rnd)
        r_a, r_w = (rounder(rnd.get(k, "rne")) for k in POINTS)
    else:
        r_a = r_w = rounder(rnd)
    ex, ex_pool = _Exact(), _Exact()
    c = lambda a: np.asarray(a, dtype=dtype)
    rr = lambda r, x: c(r(x))  # (the rounders return float64: an f16 value is one in either dtype)
    nemb, eemb = c(w["node_embedding_weight"]), c(w["edge_embedding_weight"])
    cw, cb, root = c(w["convs_weight"]), c(w["convs_bias"]), c(w["convs_root_emb_weight"])
    bnw, bnb, bnm, bnv = c(w["bn_weight"]), c(w["bn_bias"]), c(w["bn_mean"]), c(w["bn_var"])
    D = nemb.shape[-1]
    assert cw.shape == (L, D, D) and eemb.shape == (L, 13, D) and root.shape == (L, D), (cw.shape, eemb.shape, root.shape)
    pw, pb = c(w["graph_pred_weights"]).reshape(-1, D), c(w["graph_pred_bias"]).reshape(-1)
    N, G = batch.total_nodes, batch.num_graphs
    ge = batch.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    off = batch.node_offsets()
    st = off[:-1]
    gid = np.repeat(np.arange(G), batch.nums_of_nodes)
    seg = lambda rows: np.add.reduceat(rows, st, axis=0)  # (every graph has a node)
    seg_q = lambda rows: np.minimum.reduceat(lsb_exp(rows), st, axis=0)
    one = dtype(1.0)
    outdeg = np.bincount(u, minlength=N).astype(dtype)
    dinv = np.where(outdeg > 0, one / np.sqrt(outdeg + one), dtype(0.0))
    norm = dinv[u] * dinv[v]
    idp1 = one / (outdeg[:, None] + one)
    bn_scale = bnw / np.sqrt(bnv + dtype(BN_EPS))  # the folded form, as the engine applies it: one FMA
    bn_shift = bnb - bnm * bn_scale
    feat = batch.node_feature.astype(np.int64) + ND_OFF[None, :]
    h = nemb[feat].sum(axis=1, dtype=dtype)  # h_0
    big = [1.0, float(np.abs(h).max())]
    if vn is not None:
        E = c(vn["vn_embedding"]).reshape(-1)
        v1, c1, v2, c2 = c(vn["w1"]), c(vn["b1"]), c(vn["w2"]), c(vn["b2"])
        assert E.shape == (D,) and v1.shape == (L - 1, 2 * D, D) and v2.shape == (L - 1, D, 2 * D), (E.shape, v1.shape, v2.shape)
        vec = np.tile(E, (G, 1))
        x = h + vec[gid]
    else:
        x = h
    if check:  # x_0 = h_0 (+ E): the x_0 launch's ten rows (with either option on), and t_0's own sums
        terms = nemb[feat]
        bound, q = np.abs(terms).sum(axis=1), lsb_exp(terms).min(axis=1)
        if vn is not None:
            bound, q = bound + np.abs(E), np.minimum(q, lsb_exp(E))
        ex.sums(bound, q)
    r = None
    for l in range(L):
        if l == 0:  # the encoder on the projected table: sum_k (W_0 NodeEmb[row_k]) + b_0 (+ W_0 E), the projection in double on the host
            z = x @ cw[0].T + cb[0]
            if check:
                proj = nemb @ cw[0].T
                ex.matmul(nemb, cw[0])  # (the projected rows, and the folded bias, are fp32 values)
                pt = proj[feat]
                b0 = cb[0] + (E @ cw[0].T if vn is not None else 0.0)
                ex.sums(np.abs(b0), lsb_exp(b0))
                ex.sums(np.abs(pt).sum(axis=1) + np.abs(b0), np.minimum(lsb_exp(pt).min(axis=1), lsb_exp(b0)))
        else:
            s = pow2_scale(cw[l])
            Wl = rr(r_w, cw[l] * s) / s
            ar = rr(r_a, x)
            z = ar @ Wl.T + cb[l]
            if check:
                ex.matmul(ar, Wl, cb[l])
        eterms = eemb[l][batch.edge_attr.astype(np.int64) + ED_OFF[None, :]]
        ee = eterms.sum(axis=1, dtype=dtype)
        msg = np.maximum(z[u] + ee, 0.0)
        nm = norm[:, None] * msg
        m = np.zeros((N, D), dtype)
        np.add.at(m, v, nm)
        self_t = np.maximum(z + root[l], 0.0)
        inner = m + self_t * idp1
        pre = inner * bn_scale[l] + bn_shift[l]
        if check:
            ex.sums(np.abs(eterms).sum(axis=1), lsb_exp(eterms).min(axis=1))
            ex.sums(np.abs(z[u]) + np.abs(ee), np.minimum(lsb_exp(z[u]), lsb_exp(ee)))
            ex.sums(np.abs(z) + np.abs(root[l]), np.minimum(lsb_exp(z), lsb_exp(root[l])))
            ex.sums(np.abs(bn_shift[l]), lsb_exp(bn_shift[l]))
            am = np.zeros((N, D))
            np.add.at(am, v, np.abs(nm))
            qm = np.full((N, D), 10 ** 6)
            np.minimum.at(qm, v, lsb_exp(nm))
            ex.sums(am + np.abs(self_t * idp1), np.minimum(qm, lsb_exp(self_t * idp1)))  # the walk's FMAs and the first epilogue FMA
            ex.sums(np.abs(inner * bn_scale[l]) + np.abs(bn_shift[l]), np.minimum(lsb_exp(inner * bn_scale[l]), lsb_exp(bn_shift[l])))
        y = np.maximum(pre, 0.0) if l != L - 1 else pre
        h = y + x if residual else y
        if check and residual:
            ex.sums(np.abs(y) + np.abs(x), np.minimum(lsb_exp(y), lsb_exp(x)))
        big.extend([float(np.abs(x).max()), float(np.abs(z).max()), float(np.abs(m).max()) if m.size else 0.0, float(np.abs(pre).max()),
                    float(np.abs(h).max())])
        if vn is not None and l < L - 1:  # vn_{l+1} from x_l: the sum whatever the pooling is, the update unrounded
            t = seg(x) + vec
            uh = np.maximum(t @ v1[l].T + c1[l], 0.0)
            upd = np.maximum(uh @ v2[l].T + c2[l], 0.0)
            nvec = vec + upd if residual else upd
            if check and v1[l].any():  # (W1 = 0: t reaches no output -- 0 t is 0 whatever t's last bits are)
                ex.sums(seg(np.abs(x)) + np.abs(vec), np.minimum(seg_q(x), lsb_exp(vec)))
                ex.matmul(t, v1[l], c1[l])
                ex.matmul(uh, v2[l], c2[l])
                _split_bits(ex, t)
                _split_bits(ex, uh * pow2_scale(v1[l]))
            if check and residual:
                ex.sums(np.abs(vec) + np.abs(upd), np.minimum(lsb_exp(vec), lsb_exp(upd)))
            big.extend([float(np.abs(t).max()), float(uh.max()), float(nvec.max())])
            vec = nvec
            x_next = h + vec[gid]
            if check:
                ex.sums(np.abs(h) + np.abs(vec[gid]), np.minimum(lsb_exp(h), lsb_exp(vec[gid])))
        else:
            x_next = h
        if jk == "sum":
            prev = x if l == 0 else r
            r = prev + x_next  # (x_next of the last layer is h_5)
            if check:
                ex.sums(np.abs(prev) + np.abs(x_next), np.minimum(lsb_exp(prev), lsb_exp(x_next)))
        x = x_next
    if jk == "last":
        r = h
    big.append(float(np.abs(r).max()))
    if pooling == "max":
        pooled = np.maximum.reduceat(r, st, axis=0)
    else:
        pooled = seg(r)
        if check:
            ex_pool.sums(seg(np.abs(r)), seg_q(r))
        if pooling == "mean":
            pooled = pooled / c(batch.nums_of_nodes)[:, None]
    big.append(float(np.abs(pooled).max()))
    out = pooled @ pw.T + pb
    tv = r @ pw.T + pb
    if check:  # (a mean over a node count that is no power of two is rounded once, and the head then adds rounded values: those
        # graphs' logits are held to bound(), not to bits, and are left out here)
        n = np.asarray(batch.nums_of_nodes)
        dyadic = (n & (n - 1)) == 0 if pooling == "mean" else np.ones(G, bool)
        ex_pool.matmul(pooled[dyadic], pw, pb)
        ex_pool.matmul(r, pw, pb)
    single = pw.shape[0] == 1
    res = Out(out[:, 0] if single else out, r, pooled, tv[:, 0] if single else tv, h, max(big))
    return (res, Figures(ex.worst, ex_pool.worst)) if check else res


# ---------------------------------------------------------------- the probe's inputs
def probe_weights(emb_dim=WIDE, seed=5, num_tasks=1, tight=True):
    """tests/gin_wide_f16_ref.probe_weights for GCN.  The five matrices have two non-zeros per row in {1/4, 1/2}; W_1 .. W_4 -- the ones
    the mode rounds -- are multiplied by 1 - 2^-12 + 2^-20 (`tight`), so that rounded to nearest they ARE the few-bit values while
    rounded toward zero or unrounded they are not; W_0 is applied unrounded, on the host, and stays as it is.  Node rows, biases, root
    and BatchNorm's bias are positive and on a 2^-12 grid, edge rows of both signs and smaller than any bias, so a, which the mode
    rounds, stays at or above 1/4 and its f16 spacing at or above 2^-12.  BatchNorm: var = 1 - 2^-10 (var + eps = 1 with the engine's
    eps), mean 0, weight in {1/2, 1} (the last layer: 1): the folded scale is a power of two and the shift is the bias.  A head of four entries per task, 1, 1, 1/2 and 1/2 -- one sign, unlike GIN's
    probe: with the residual or the JK sum on a graph's sum of rows is not an fp32 value (the module docstring gives the bits), the
    pooled mean then carries fp32's own rounding, some 1e-7 of ITS size, and a head of both signs would subtract two such means and hold
    the difference to 1e-6 of the much smaller logit -- a test of cancellation, not of the mode.  With one sign the logit is the size
    of what it is made of, and one-sided errors (activations rounded toward zero) do not cancel in it either."""
    rng = np.random.default_rng(seed)
    D = emb_dim
    q = 2.0 ** -12
    f = lambda a: np.asarray(a, np.float32)

    def sparse(vals):
        m = np.zeros((D, D))
        for o in range(D):
            m[o, rng.choice(D, 2, replace=False)] = rng.choice(vals, 2)
        return m

    pw = np.zeros((num_tasks, D))
    for t in range(num_tasks):
        pw[t, rng.choice(D, 4, replace=False)] = [1.0, 1.0, 0.5, 0.5]
    t = (1.0 - 2.0 ** -12 + 2.0 ** -20) if tight else 1.0
    cw = np.stack([sparse([0.25, 0.5]) for _ in range(L)])
    cw[1:] *= t
    return {
        "node_embedding_weight": f(rng.integers(2 ** 8, 2 ** 9, (173, D)) * q),
        "edge_embedding_weight": f(rng.integers(-2 ** 6, 2 ** 6, (L, 13, D)) * q),
        "convs_weight": f(cw),
        "convs_bias": f(rng.integers(2 ** 10, 2 ** 11, (L, D)) * q),
        "convs_root_emb_weight": f(rng.integers(2 ** 8, 2 ** 9, (L, D)) * q),
        "bn_weight": f(np.concatenate([rng.choice([0.5, 1.0], (L - 1, D)), np.ones((1, D))])),  # (the last rows are pooled: one bit fewer)
        "bn_bias": f(rng.integers(2 ** 10, 2 ** 11, (L, D)) * q),
        "bn_mean": f(np.zeros((L, D))),
        "bn_var": f(np.full((L, D), 1.0 - BN_EPS)),
        "graph_pred_weights": f(pw),
        "graph_pred_bias": f(rng.integers(1, 2 ** 10, (num_tasks,)) * q),
    }


VN_LIVE_UPDATES = 1


def probe_virtual_node(emb_dim=WIDE, seed=9, live=VN_LIVE_UPDATES):
    """tests/gin_wide_f16_ref.probe_virtual_node, for the reason written there: the update is NOT rounded in this mode, so t carries the
    significant bits of a sum over a graph's rows and the next stage's sums carry them on.  Only the first `live` updates have weights
    (update 0: t_0 is a sum of encoder rows, on the 2^-12 grid); the others have W1 = W2 = 0 and their vector is relu(b2), the same for
    every graph.  The VN instances then add a vector that differs from graph to graph in stage 0 and one that does not in the other
    three, the partial rows are written by stages 0..2 as ever, and the update kernel multiplies operands that are exactly a split pair."""
    rng = np.random.default_rng(seed)
    D, H = emb_dim, 2 * emb_dim
    q = 2.0 ** -12
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)

    def single(rows, cols):
        m = np.zeros((rows, cols))
        m[np.arange(rows), rng.integers(0, cols, rows)] = 0.25
        return m

    w1 = np.stack([single(H, D) for _ in range(L - 1)])
    w2 = np.stack([single(D, H) for _ in range(L - 1)])
    w1[live:] = 0.0
    w2[live:] = 0.0
    return OrderedDict([
        ("vn_embedding", f(rng.integers(2 ** 8, 2 ** 9, (D,)) * q)),
        ("w1", f(w1)),
        ("b1", f(rng.integers(2 ** 9, 2 ** 10, (L - 1, H)) * q)),
        ("w2", f(w2)),
        ("b2", f(rng.integers(2 ** 9, 2 ** 10, (L - 1, D)) * q)),
    ])


CARDS = (119, 4, 12, 12, 10, 6, 6, 2, 2)


def _graph(n, pairs, seed):
    """n nodes, every undirected pair listed in both directions; random features, the edge codes walk through all 60"""
    rng = np.random.default_rng(seed)
    nf = np.stack([rng.integers(0, k, n) for k in CARDS], 1).astype(np.int32)
    el = np.asarray([(a, b) for a, b in pairs] + [(b, a) for a, b in pairs], np.int32).reshape(-1, 2)
    code = (np.arange(len(el)) + seed) % 60
    ea = np.stack([code // 12, (code // 2) % 6, code % 2], 1).astype(np.int32)
    return gp.GraphBatch(np.array([n], np.int32), np.array([len(el)], np.int32), nf, el, ea)


def complete(n, seed):
    return _graph(n, [(a, b) for a in range(n) for b in range(a + 1, n)], seed)


def prism(n, seed):
    """the cubic prism on n = 2 k nodes: two k-rings and the rungs between them"""
    k = n // 2
    assert n == 2 * k and k >= 3, n
    return _graph(n, [(i, (i + 1) % k) for i in range(k)] + [(k + i, k + (i + 1) % k) for i in range(k)] + [(i, k + i) for i in range(k)], seed)


def moebius(n, seed):
    """the Moebius ladder on n = 2 k nodes: an n-ring and its k diameters -- cubic"""
    k = n // 2
    assert n == 2 * k and k >= 3, n
    return _graph(n, [(i, (i + 1) % n) for i in range(n)] + [(i, i + k) for i in range(k)], seed)


def edgeless(n, seed):
    return _graph(n, [], seed)


@functools.lru_cache(maxsize=None)
def probe_batch():
    """60 graphs, 900 nodes, every node of degree 0, 3 or 15: one-node graphs, an edgeless four-node graph, K4, prisms, Moebius ladders
    and K16.  Eight workgroups of 128 rows, the last one ending inside a 16-row tile (900 = 7 x 128 + 4); graphs straddle 16-row
    tiles and workgroup boundaries (tests/test_gcn_wide_f16_cpu.py asserts each of these on the node offsets)."""
    gs, k = [edgeless(1, 1)], 2
    plan = ([("K16", 16)] * 3 + [("prism", 6), ("K4", 4), ("moebius", 8), ("prism", 10), ("one", 1), ("K16", 16), ("moebius", 12), ("prism", 14),
                                 ("K4", 4), ("K16", 16), ("prism", 20), ("moebius", 18), ("edgeless", 4), ("K16", 16), ("prism", 30)])
    sizes = 1
    while True:
        for kind, n in plan:
            if len(gs) == 59:
                break
            gs.append({"K16": complete, "K4": complete, "prism": prism, "moebius": moebius, "one": edgeless, "edgeless": edgeless}[kind](n, k))
            sizes += n
            k += 1
        if len(gs) == 59:
            break
    rest = 900 - sizes
    assert rest >= 6 and rest % 2 == 0, rest  # the last graph takes what is left: a prism
    gs.append(prism(rest, k))
    return gp.concat_batches(gs)


@functools.lru_cache(maxsize=None)
def weights_of(tasks=1, emb_dim=WIDE):
    return probe_weights(emb_dim, num_tasks=tasks)


@functools.lru_cache(maxsize=None)
def virtual_node_of(emb_dim=WIDE):
    return probe_virtual_node(emb_dim)


# ---------------------------------------------------------------- the probe's cases and what the references tell apart
Case = namedtuple("Case", "name fwd pooling tasks vn jk res device group")
EMB, ROWS, TERMS = "return_embeddings", "return_node_embeddings", "return_node_logits"
OUTPUT_OF = {EMB: "pooled", ROWS: "rows", TERMS: "terms"}


def case(name, fwd=(), pooling="mean", tasks=1, vn=False, jk="last", res=False, device=False, group=False):
    return Case(name, tuple(fwd), pooling, tasks, vn, jk, res, device, group)


CASES = [
    case("plain"),
    case("NUM_TASK 2", fwd=[EMB], tasks=2),
    case("sum", fwd=[EMB], pooling="sum"),
    case("max", fwd=[EMB], pooling="max"),
    case("graph embeddings", fwd=[EMB]),
    case("node embeddings", fwd=[ROWS]),
    case("node logits", fwd=[TERMS]),
    case("virtual node", fwd=[ROWS], vn=True),
    case("residual", fwd=[ROWS], res=True),
    case("JK sum", fwd=[ROWS], jk="sum"),
    case("virtual node, JK sum, residual", fwd=[ROWS], vn=True, jk="sum", res=True),
    case("device batch", fwd=[ROWS], device=True),
    case("group of two", fwd=[ROWS], group=True),
]
IDS = [c.name for c in CASES]
WRONG = {  # variant -> rnd of `forward`
    "rtz": {"a": "rtz"},                                # activations rounded toward zero
    "none": "none",                                     # the unrounded forward (what the f32 mode computes)
    "weights not rounded": {"w": "none"},
    "weights rounded toward zero": {"w": "rtz"},
    "activations not rounded": {"a": "none"},
}
CHECKED = ("rne", "rtz")  # the forwards whose fp32 sums must be exact (the others carry unrounded operands)


def outputs_of(c):
    return ("logits",) + tuple(OUTPUT_OF[k] for k in c.fwd)


@functools.lru_cache(maxsize=None)
def _reference(tasks, vn, jk, res, pooling, variant):
    rnd = "rne" if variant == "rne" else WRONG[variant]
    kw = dict(vn=virtual_node_of() if vn else None, jk=jk, residual=res, rnd=rnd, pooling=pooling)
    if variant in CHECKED:
        out, worst = forward(probe_batch(), weights_of(tasks), check=True, **kw)
    else:
        out, worst = forward(probe_batch(), weights_of(tasks), **kw), None
    for a in out[:5]:
        a.setflags(write=False)
    return out, worst


def references(c):
    """variant -> (Out, exactness figure or None): "rne" (the expected values) and every entry of WRONG"""
    return {v: _reference(c.tasks, c.vn, c.jk, c.res, c.pooling, v) for v in ("rne",) + tuple(WRONG)}


def rows_exact(c):
    """the rows of the case are held to bits: the figure of every sum up to them is at most 24 in both checked forwards"""
    refs = references(c)
    return all(refs[v][1].rows <= 24.0 for v in CHECKED)


def pool_exact(c):
    """... and so are its pooled sums or maxima, and the per-node terms' sums"""
    refs = references(c)
    return rows_exact(c) and all(refs[v][1].pool <= 24.0 for v in CHECKED)


ROWS_NOT_EXACT = ("virtual node, JK sum, residual",)  # what rows_exact answers, by name (tests/test_gcn_wide_f16_cpu.py holds it to that)
POOL_NOT_EXACT = ("virtual node", "residual", "JK sum", "virtual node, JK sum, residual")


def bound(want):
    return 1e-6 * (1.0 + np.abs(want))


def separated(got, other, want):
    """(the pair passes the probe's criterion, fraction of elements beyond FACTOR x the bound, median ratio to the bound)"""
    sep = np.abs(np.asarray(got, np.float64) - other) / bound(want)
    frac, med = float(np.mean(sep > FACTOR)), float(np.median(sep))
    return frac > 0.5 and med > FACTOR, frac, med


def separation(c, outputs=None):
    """(output, variant) -> (passes, fraction, median) of the references among themselves"""
    refs = references(c)
    want = refs["rne"][0]
    names = outputs_of(c) if outputs is None else outputs
    return {(o, v): separated(getattr(want, o), getattr(refs[v][0], o), getattr(want, o)) for o in names for v in WRONG}


TABLE_OUTPUTS = ("logits", "rows", "pooled")  # what NOT_SEPARATED is held to, in every case

# The pairs that do NOT separate, by name, with the fraction of elements the references reached (tests/test_gcn_wide_f16_cpu.py holds
# the list to the computed table in both directions over logits, rows and pooled rows of every case; every other pair is asserted on
# the GPU).  One kind of pair is listed, in every case and on all three outputs: the forward that rounds the weights and leaves a as
# it is.  GCN has one product per layer where GIN has two, a row of W has two entries of at most 1/2, and the walk that follows
# averages the round-to-nearest errors of a (both signs) over a node's neighbours with weights 1/4 or 1/16 -- the rows end up about ten
# bounds apart, not a hundred (0 .. 2 % of the elements beyond it, on every output).  That variant is told from the mode by the
# rows' BITS, which the GPU test asserts, not by this table.  Against activations rounded toward zero, the unrounded forward and both
# weight variants the logits, the rows and the pooled rows separate in every case.
NOT_SEPARATED = {
    ('plain', 'logits', 'activations not rounded'): 0.0,
    ('plain', 'rows', 'activations not rounded'): 0.01,
    ('plain', 'pooled', 'activations not rounded'): 0.01,
    ('NUM_TASK 2', 'logits', 'activations not rounded'): 0.0,
    ('NUM_TASK 2', 'rows', 'activations not rounded'): 0.01,
    ('NUM_TASK 2', 'pooled', 'activations not rounded'): 0.01,
    ('sum', 'logits', 'activations not rounded'): 0.0,
    ('sum', 'rows', 'activations not rounded'): 0.01,
    ('sum', 'pooled', 'activations not rounded'): 0.02,
    ('max', 'logits', 'activations not rounded'): 0.0,
    ('max', 'rows', 'activations not rounded'): 0.01,
    ('max', 'pooled', 'activations not rounded'): 0.02,
    ('graph embeddings', 'logits', 'activations not rounded'): 0.0,
    ('graph embeddings', 'rows', 'activations not rounded'): 0.01,
    ('graph embeddings', 'pooled', 'activations not rounded'): 0.01,
    ('node embeddings', 'logits', 'activations not rounded'): 0.0,
    ('node embeddings', 'rows', 'activations not rounded'): 0.01,
    ('node embeddings', 'pooled', 'activations not rounded'): 0.01,
    ('node logits', 'logits', 'activations not rounded'): 0.0,
    ('node logits', 'rows', 'activations not rounded'): 0.01,
    ('node logits', 'pooled', 'activations not rounded'): 0.01,
    ('virtual node', 'logits', 'activations not rounded'): 0.0,
    ('virtual node', 'rows', 'activations not rounded'): 0.02,
    ('virtual node', 'pooled', 'activations not rounded'): 0.01,
    ('residual', 'logits', 'activations not rounded'): 0.02,
    ('residual', 'rows', 'activations not rounded'): 0.01,
    ('residual', 'pooled', 'activations not rounded'): 0.01,
    ('JK sum', 'logits', 'activations not rounded'): 0.0,
    ('JK sum', 'rows', 'activations not rounded'): 0.0,
    ('JK sum', 'pooled', 'activations not rounded'): 0.0,
    ('virtual node, JK sum, residual', 'logits', 'activations not rounded'): 0.0,
    ('virtual node, JK sum, residual', 'rows', 'activations not rounded'): 0.0,
    ('virtual node, JK sum, residual', 'pooled', 'activations not rounded'): 0.0,
    ('device batch', 'logits', 'activations not rounded'): 0.0,
    ('device batch', 'rows', 'activations not rounded'): 0.01,
    ('device batch', 'pooled', 'activations not rounded'): 0.01,
    ('group of two', 'logits', 'activations not rounded'): 0.0,
    ('group of two', 'rows', 'activations not rounded'): 0.01,
    ('group of two', 'pooled', 'activations not rounded'): 0.01,
}

# ---------------------------------------------------------------- accuracy at a realistic shape
ACCURACY = ("synthetic weights", "synthetic weights, virtual node", "exported state_dict", "exported state_dict, virtual node")
LADDER = tuple(1e-4 * m * 10 ** k for k in range(4) for m in (1, 2, 5))  # 1e-4 x {1, 2, 5, 10, 20, 50, ..}


@functools.lru_cache(maxsize=None)
def accuracy_inputs(which):
    """(batch, w, vn or None): tests/gcn_wide_ref.sep_batch(0), 256 molpcba-shaped graphs, with gcn_wide_ref.sep_weights() and
    tests/gcn_wide_vn_ref.shapes_virtual_node(), or with the exported tensors of gcn_wide_ref.state_dict / gcn_wide_vn_ref.vn_state_dict"""
    from tests import gcn_wide_ref as R, gcn_wide_vn_ref as V
    b = R.sep_batch(0)
    vn = which.endswith("virtual node")
    if which.startswith("synthetic"):
        return b, R.sep_weights(), (V.shapes_virtual_node() if vn else None)
    sd = V.vn_state_dict(seed=4, vn_w1_scale=1.0 / 16) if vn else R.state_dict(seed=4)
    kw = dict(virtual_node=True, virtual_node_dim=WIDE) if vn else {}
    w = export.gcn_weights_from_ogb_state_dict(sd, emb_dim=WIDE, **kw)
    return b, w, (export.gcn_virtual_node_from_ogb_state_dict(sd, virtual_node_dim=WIDE) if vn else None)


def rule(x, ref, tol):
    """max |x - f64| / (tol (scale + |f64|)) on the logits: at most 1 passes"""
    return float((np.abs(np.asarray(x, np.float64).reshape(ref.logits.shape) - ref.logits) / (tol * (ref.scale + np.abs(ref.logits)))).max())


@functools.lru_cache(maxsize=None)
def accuracy_references(which):
    """(the float64 forward, the mode's restatement) on accuracy_inputs(which)"""
    b, w, vn = accuracy_inputs(which)
    f64, rne = forward(b, w, vn, rnd="none"), forward(b, w, vn)
    return f64, rne


def ladder_tol(which):
    """the smallest tol of LADDER that the restatement stays within half of"""
    f64, rne = accuracy_references(which)
    return next(t for t in LADDER if rule(rne.logits, f64, t) <= 0.5)


# What ladder_tol gives on each input (tests/test_gcn_wide_f16_cpu.py holds this to the measurement: the restatement is at 0.490, 0.029,
# 0.327 and 0.014 of 1e-4, so the first rung is within reach of its half in all four); the GPU test holds the kernel to it.
TOL = {"synthetic weights": 1e-4, "synthetic weights, virtual node": 1e-4, "exported state_dict": 1e-4,
       "exported state_dict, virtual node": 1e-4}
