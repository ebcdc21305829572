"""Float64 NumPy restatement of PNA in the f16 numeric mode (flowgnn.h: flowgnn_set_model_numeric_mode_dim at FLOWGNN_EMB_DIM_PNA;
kernels: flowgnn_amd/csrc/pna_f16.hip, pna_emb_f16.hip, pna_rows_f16.hip), for the tests of that mode.

The equations are tests/numpy_ref.pna_forward's, through its `dense` hook: the mode changes the layer's 320 -> 3 x 80 contraction and
nothing else,
    dense(x, W) = rnd(x) @ rnd(W s).T / s,      s = the layer's power-of-two scale (pna.hip: pna_pack_stream_layer),
x the node's aggregates [mean | min | max | std][80] as fp32 forms them (sentinels 31.9990234375 / -32 of rows without in-edges
included: the first rounds to 32), each rounded to f16 ONCE, to nearest even.  `rnd` picks the rounding: "rne" (the mode), "rtz"
(toward zero) or "none" (the plain model: the f32 mode); `skip` names one aggregator whose 80 operands stay unrounded -- the
restatements the probe must tell apart from the mode.

Also here: the probe (dyadic weights, a bipartite batch whose fp32 sums are exact -- tests/test_pna_f16_cpu.py proves which), the
fixed shape cases of the GPU test, and the tolerance table of the accuracy inputs (LADDER, TOL: computed by the CPU test)."""
from collections import OrderedDict, namedtuple

import numpy as np

from flowgnn_amd import graphpack as gp, weights
from flowgnn_amd.graphpack import GraphBatch
from tests import f16_ref as F, numpy_ref as N

AGGREGATORS = ("mean", "min", "max", "std")  # the reference's enum order: the column blocks of x
ROUNDINGS = ("rne", "rtz", "none")
D = 80
SENT_MAX, SENT_MIN = 31.9990234375, -32.0

Result = namedtuple("Result", "logits hs rows scale")


def dense_of(rnd="rne", skip=None):
    """the layer's contraction as numpy_ref.pna_forward calls it: x [N][320] (aggregator-major), W [3 * 80][320]"""
    r = F.rounder(rnd)

    def dense(x, W):
        s = F.pow2_scale(W)
        xr = np.array(r(x), np.float64)
        if skip is not None:
            a = AGGREGATORS.index(skip)
            xr[:, D * a:D * (a + 1)] = x[:, D * a:D * (a + 1)]
        return (xr @ r(W * s).T) / s

    return dense


def forward(batch, w, rnd="rne", skip=None):
    """-> Result(logits [G], hs [5][N][80], rows = h_4, scale = the largest activation, at least 1)"""
    assert rnd in ROUNDINGS and (skip is None or skip in AGGREGATORS)
    dense = None if (rnd == "none" and skip is None) else dense_of(rnd, skip)
    out, hs = N.pna_forward(batch, w, return_h=True, dense=dense)
    return Result(out, hs, hs[4], max(1.0, float(np.abs(hs).max())))


def rule(x, ref, tol):
    """tests/parity.py's rule against the float64 forward `ref` (a Result): max |x - f64| / (tol (scale + |f64|)) of logits or rows"""
    x = np.asarray(x, np.float64)
    want = ref.logits if x.ndim == 1 else ref.rows
    return float((np.abs(x.reshape(want.shape) - want) / (tol * (ref.scale + np.abs(want)))).max())


# ---------------------------------------------------------------- the ladder and the accuracy inputs
LADDER = tuple(1e-4 * m * 10 ** k for k in range(3) for m in (1, 2, 5))  # 1e-4 x {1, 2, 5, 10, 20, 50, 100, 200, 500}
ACCURACY_SEEDS = (3, 11)
ACCURACY = (("synth", "logits"), ("synth", "rows"), ("trained", "rows"))  # (weights, output): an accuracy input, on both seeds
# the smallest rung at which the "rne" restatement alone lies at <= 0.5 on both seeds (tests/test_pna_f16_cpu.py holds this table to
# the computation: 0.21 and 0.17 | 1.95 and 1.91 | 0.92 and 1.16 of the 1e-4 rule).  With the trained set the head saturates -- the
# logit is the same constant, 1.2289, in every mode -- so that set tests rows only.
TOL = {("synth", "logits"): 1e-4, ("synth", "rows"): 5e-4, ("trained", "rows"): 5e-4}


def accuracy_batch(seed):
    return gp.synth_hep10k_batch(24, seed=seed, with_eigen=False)


def trained_weights():
    """the trained PNA set the reference ships (tests/golden/ref_weights_pna*.npz, tests/golden/make_ref_weights.py)"""
    import os
    import sys
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if here not in sys.path:
        sys.path.insert(0, here)
    import make_ref_weights as mrw
    return OrderedDict(mrw.load("PNA"))


def accuracy_weights(wname):
    return weights.synth_pna_weights(7) if wname == "synth" else trained_weights()


def rung(ratio_at_1e4):
    """the smallest rung at which a restatement whose ratio of the 1e-4 rule is `ratio_at_1e4` lies at <= 0.5"""
    for t in LADDER:
        if ratio_at_1e4 * (1e-4 / t) <= 0.5:
            return t
    raise AssertionError(ratio_at_1e4)


# ---------------------------------------------------------------- the probe
# Every graph is bipartite: 32 SOURCES (no in-edge, out-edges only) and 12 SINKS (no out-edge) of in-degree 32, 4, 4, 2 x 4, 1 x 4 and 0
# -- every in-degree is in {0, 1, 2, 4, 32}, so 1 / indeg is a power of two -- and a sink's scalers are t = 0 and scale = 1 exactly
# (log(0 + 1) = 0).  A source's update never opens its ReLU except where the file says so (its aggregates are the sentinels, which
# the weights below turn into a large negative sum), so the sources keep h_0 in every layer and no irrational scaler reaches a sum.
#   features A = 0..15: h_0 = +-a_i + e on the 2^-10 grid, |h_0| < 1.5 (11 bits: squares and their pair sums are exact in fp32); the
#       sign is the node's (encoder feature 7).  A sink of in-degree 2 reads one source of either sign: its variance is the perfect
#       square ((x1 - x2) / 2)^2 and its std, on the 2^-11 grid in [1, 2), needs 12 bits: the f16 rounding moves every odd one.
#   features B = 16..79: h_0 = 3 + d on the 2^-12 grid (14 bits): mean, min and max all move under an f16 rounding (spacing 2^-9).
# Weights (dyadic, two significant bits after the layer's scale), per output o and scaler 0 and 2 (scaler 1 repeats scaler 0: t = 0
# on the sinks, so its products are never seen -- the accuracy test alone covers them):
#   B: W[max] = u, W[mean] = v, W[min] = -(u + v), u, v >= 0: the sum is u (max - min) + v (mean - min) >= 0, small where the
#      neighbours are close, while each rounding error is that of a value near 3;
#   A: W[max] = u', W[min] = -u', W[std] = -2 u': u' (range - 2 std) >= 0 (Popoviciu), exactly 0 at in-degree 2.
#   The std operand is exact only on A and only at in-degree 1 (0) and 2: std weights are zero on B in every layer (the B rows carry
#   14 bits, and the sum of their squares is not exact).  As the sources never change, the aggregates are those of layer 0 in every
#   layer, so std keeps its weights on A in layers 1..3 too.
#   Layer 3, outputs 0..7 (SENTINEL_OUT): W[min] = W[max] = 1 on eight A features and nothing else, in scaler 0 alone: on a row
#   without in-edges that is 8 (r(31.9990234375) - 32), which is 0 in the mode, -2^-7 unrounded and -2^-3 rounded toward zero: the
#   one place where a source's ReLU opens (bias 1/4), and what pins the sentinels' rounding.
PROBE_GRAPHS = 3
N_SRC, SINK_INDEG = 32, (32, 4, 4, 2, 2, 2, 2, 1, 1, 1, 1, 0)
N_PER = N_SRC + len(SINK_INDEG)
A_FEATS, SENTINEL_OUT = 16, 8
BOUND = 1e-6  # the probe's bound: |x - want| <= BOUND (1 + |want|)
SEPARATION = 100.0
VARIANTS = (("none", None), ("rtz", None), ("rne", "mean"), ("rne", "min"), ("rne", "max"), ("rne", "std"))


def variant_name(v):
    return v[0] if v[1] is None else "skip-" + v[1]


def probe_batch():
    rng = np.random.default_rng(20)
    feats, edges, nn, ne = [], [], [], []
    for _ in range(PROBE_GRAPHS):
        f = np.zeros((N_PER, 9), np.int32)
        f[:, 0] = rng.permutation(119)[:N_PER]
        f[:N_SRC, 7] = np.arange(N_SRC) % 2  # the sources' signs alternate
        f[N_SRC:, 7] = rng.integers(0, 2, N_PER - N_SRC)
        el = []
        for k, d in enumerate(SINK_INDEG):
            v = N_SRC + k
            if d == 32:
                src = np.arange(N_SRC)
            elif d == 2:  # one source of either sign
                src = np.array([2 * rng.integers(0, N_SRC // 2), 2 * rng.integers(0, N_SRC // 2) + 1])
            else:
                src = rng.permutation(N_SRC)[:d]
            el += [(int(u), v) for u in src]
        el = np.array(el, np.int32)[rng.permutation(len(el))]
        feats.append(f); edges.append(el); nn.append(N_PER); ne.append(len(el))
    el = np.concatenate(edges)
    return GraphBatch(np.array(nn, np.int32), np.array(ne, np.int32), np.concatenate(feats), el, np.zeros((len(el), 3), np.int32))


def probe_classes(b):
    """per node of the batch: in-degree, out-degree"""
    ge = b.global_edges()
    return np.bincount(ge[:, 1], minlength=b.total_nodes), np.bincount(ge[:, 0], minlength=b.total_nodes)


def probe_weights():
    rng = np.random.default_rng(21)
    w = weights.synth_pna_weights(7)
    for k in w:
        if k.startswith("graph_mlp"):
            w[k] = (np.asarray(w[k], np.float32) * np.float32(0.25)).astype(np.float32)
    T = np.zeros((173, D), np.float64)
    a = 1.0 + rng.integers(0, 400, A_FEATS) * 2.0 ** -10
    T[N.ND_OFF[7] + 0, :A_FEATS], T[N.ND_OFF[7] + 1, :A_FEATS] = a, -a
    T[:119, :A_FEATS] = rng.integers(-64, 65, (119, A_FEATS)) * 2.0 ** -10
    T[:119, A_FEATS:] = 3.0 + rng.integers(-128, 129, (119, D - A_FEATS)) * 2.0 ** -12
    cw = np.zeros((4, D, 3, 4, D), np.float64)  # [layer][out][scaler][aggregator][in]
    pick = lambda shape, p: rng.choice([0.5, 1.0], shape) * (rng.random(shape) < p)
    MEAN, MIN, MAX, STD = 0, 1, 2, 3
    for l in range(4):
        for s, p in ((0, 0.25), (2, 0.1)):
            u, v = pick((D, D - A_FEATS), p), pick((D, D - A_FEATS), p)
            cw[l, :, s, MAX, A_FEATS:], cw[l, :, s, MEAN, A_FEATS:], cw[l, :, s, MIN, A_FEATS:] = u, v, -(u + v)
            ua = pick((D, A_FEATS), 0.5)
            cw[l, :, s, MAX, :A_FEATS], cw[l, :, s, MIN, :A_FEATS], cw[l, :, s, STD, :A_FEATS] = ua, -ua, -2.0 * ua
        cw[l, :, 1] = cw[l, :, 0]
    cw[3, :SENTINEL_OUT] = 0.0
    cw[3, :SENTINEL_OUT, 0, MIN, :8] = 1.0
    cw[3, :SENTINEL_OUT, 0, MAX, :8] = 1.0
    cb = 0.25 + rng.integers(0, 1024, (4, D)) * 2.0 ** -13
    w["node_embedding_weight"] = T.astype(np.float32)
    w["node_conv_weights"] = cw.astype(np.float32)
    w["node_conv_bias"] = cb.astype(np.float32)
    w["avg_deg"] = np.array([weights.PNA_AVG_DEG], np.float32)
    return w


def _contraction_exact(ex, x, w):
    """x [N][K] @ w.T [K][M] in fp32: per (row, output) the finest bit among the terms whose weight is not zero, against sum |terms|"""
    lx, lw = F.lsb_exp(x), F.lsb_exp(w)
    bound = np.abs(x) @ np.abs(w).T
    q = np.empty(bound.shape)
    for o in range(w.shape[0]):
        nz = w[o] != 0
        q[:, o] = (lx[:, nz].min(axis=1) + lw[o, nz].min()) if nz.any() else 10 ** 6
    ex.sums(bound, q)
    return bound, q


def probe_check(b, w):
    """The "rne" forward of the probe with the bookkeeping of tests/f16_ref._Exact: -> (Result, exact [N] bool: the rows whose every
    fp32 sum is proven exact, worst log2(sum |terms| / quantum) over those sums (<= 24 passes), margin: the largest acc of a closed
    update of a row without in-edges).  It restates numpy_ref.pna_forward for this batch (the CPU test holds the two to the same bits)."""
    f64 = lambda a: np.asarray(a, np.float64)
    r = F.rounder("rne")
    ex = F._Exact()
    nemb, cw, cb = f64(w["node_embedding_weight"]), f64(w["node_conv_weights"]), f64(w["node_conv_bias"])
    indeg, outdeg = probe_classes(b)
    n = b.total_nodes
    ge = b.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    terms = nemb[b.node_feature.astype(np.int64) + N.ND_OFF[None, :]]
    ex.sums(np.abs(terms).sum(axis=1), F.lsb_exp(terms).min(axis=1))
    h = terms.sum(axis=1)
    sink, src = outdeg == 0, outdeg > 0
    assert (indeg[src] == 0).all() and np.isin(indeg, (0, 1, 2, 4, 32)).all()
    exact = src | (indeg <= 2)
    deg1 = np.maximum(indeg, 1)[:, None].astype(np.float64)
    hs, margin = [h], -np.inf
    for l in range(4):
        x = h[u]
        S, Q, Sa = np.zeros((n, D)), np.zeros((n, D)), np.zeros((n, D))
        np.add.at(S, v, x); np.add.at(Q, v, x * x); np.add.at(Sa, v, np.abs(x))
        mn, mx = np.full((n, D), SENT_MAX), np.full((n, D), SENT_MIN)
        np.minimum.at(mn, v, x); np.maximum.at(mx, v, x)
        qh = np.full((n, D), 10 ** 6, np.int64)
        np.minimum.at(qh, v, F.lsb_exp(x))
        ex.sums(Sa[exact], qh[exact])  # the walk's S
        mean = S / deg1
        var = np.maximum(Q / deg1 - mean * mean, 0.0)
        std = np.sqrt(var)
        # Q, mean^2 and the variance on A, where std carries weights, at in-degree 1 and 2: squares of 11-bit values, pair sums below 2^23 quanta
        two = exact & (indeg >= 1)
        xa = np.abs(x[:, :A_FEATS])
        assert (F.lsb_exp(x[:, :A_FEATS]) >= -10).all() and xa.max() < 1.5
        Qa = np.zeros((n, A_FEATS)); np.add.at(Qa, v, xa * xa)
        ex.sums(Qa[two], np.full(Qa[two].shape, -20))
        ex.sums((mean * mean)[two][:, :A_FEATS] + 2.0 ** -60, np.full(Qa[two].shape, -22))
        ex.sums(var[two][:, :A_FEATS], np.full(Qa[two].shape, -22))  # fma(Q, 1 / indeg, -mean^2) rounds once: its result is what must fit
        root = np.rint(std[two][:, :A_FEATS] * 2.0 ** 11)
        assert np.array_equal(root * root, var[two][:, :A_FEATS] * 2.0 ** 22)  # perfect squares: the root is exact
        assert (cw[l][:, :, 3, A_FEATS:] == 0).all()  # no std weight on B
        agg = np.stack([mean, mn, mx, std], axis=1).reshape(n, 4 * D)
        W = cw[l].transpose(1, 0, 2, 3).reshape(3 * D, 4 * D)
        s = F.pow2_scale(W)
        Ws, xr = r(W * s), r(agg)
        assert np.array_equal(Ws, W * s)  # the weights are on the f16 grid after the scale
        y = (xr @ Ws.T / s).reshape(n, 3, D)
        bound, q = _contraction_exact(ex, xr[exact], Ws)
        bound, q = bound.reshape(-1, 3, D) / s, q.reshape(-1, 3, D) - np.log2(s)
        logd = np.log(outdeg + 1.0)
        t = logd / f64(w["avg_deg"]).reshape(-1)[0]
        sc = np.where(logd == 0, 1.0, f64(w["avg_deg"]).reshape(-1)[0] / np.where(logd == 0, 1.0, logd))
        acc = cb[l] + y[:, 0] + t[:, None] * y[:, 1] + sc[:, None] * y[:, 2]
        # sinks: b + Y_0 + Y_2 (t = 0, scale = 1); sources: closed (acc far below 0: whatever fp32 makes of it, the ReLU returns 0)
        # but on SENTINEL_OUT in layer 3, where Y_1 = Y_2 = 0 and Y_0 is proven like a sink's
        # (the isolated sink's aggregates are the sentinels too: closed and opened like a source)
        empty = indeg == 0
        open_src = np.zeros((n, D), bool)
        if l == 3:
            open_src[empty, :SENTINEL_OUT] = True
            assert (y[empty][:, 1:, :SENTINEL_OUT] == 0).all()
        closed = empty[:, None] & ~open_src
        margin = max(margin, float(acc[closed].max()))
        sk = sink[exact]
        fb = np.abs(cb[l])[None, :] + bound[:, 0] + np.where(sk[:, None], bound[:, 2], 0.0)
        fq = np.minimum(np.minimum(F.lsb_exp(cb[l])[None, :], q[:, 0]), np.where(sk[:, None], q[:, 2], 10 ** 6))
        keep = ~closed[exact]
        ex.sums(fb[keep], fq[keep])
        hb, hq = np.abs(h[exact]) + fb, np.minimum(F.lsb_exp(h[exact]), fq)
        ex.sums(hb[keep], hq[keep])
        h = h + np.maximum(acc, 0.0)
        hs.append(h)
    hs = np.stack(hs)
    off = b.node_offsets()
    hg = np.add.reduceat(h, off[:-1], axis=0) / f64(b.nums_of_nodes)[:, None]
    o1 = np.maximum(hg @ f64(w["graph_mlp_1_weights"]).T + f64(w["graph_mlp_1_bias"]), 0.0)
    o2 = np.maximum(o1 @ f64(w["graph_mlp_2_weights"]).T + f64(w["graph_mlp_2_bias"]), 0.0)
    out = o2 @ f64(w["graph_mlp_3_weights"]).reshape(-1) + f64(w["graph_mlp_3_bias"]).reshape(-1)[0]
    return Result(out, hs, hs[4], max(1.0, float(np.abs(hs).max()))), exact, ex.worst, margin


def bound(x):
    return BOUND * (1.0 + np.abs(np.asarray(x, np.float64)))


def compared(b, v):
    """the values of h_4 [N][80] a variant is compared on: {name: mask}.  A rounding shows where its operand carries weights and bits:
    mean, min and max on the sinks with in-edges; std on the sinks of in-degree 2 (the exact ones) and above; the sentinels on the
    rows without in-edges at SENTINEL_OUT."""
    indeg, outdeg = probe_classes(b)
    m = np.zeros((b.total_nodes, D), bool)
    if v[1] == "std":
        m[indeg == 2] = True
        return {"rows": m}
    m[indeg >= 1] = True
    sets = {"rows": m}
    if v[1] is None:
        s = np.zeros_like(m)
        s[indeg == 0, :SENTINEL_OUT] = True
        sets["sentinels"] = s
    return sets


def separated(x, other, want, mask):
    """x [N][80] apart from `other` by more than SEPARATION x the bound (of `want`) on more than half of the masked values -> (ok, fraction)"""
    frac = float((np.abs(np.asarray(x, np.float64) - other)[mask] > SEPARATION * bound(want)[mask]).mean())
    return frac > 0.5, frac


# ---------------------------------------------------------------- the fixed shape cases of the GPU test
Case = namedtuple("Case", "name batch options slot claim")  # slot: the f16 slot that must have run; claim(batch): what the case says of itself
RESIDENT_SLOT, FUSED_SLOT, DENSE_SLOT = "pna_resident_f16", "pna_layer_fused_f16", "pna_dense_f16"
SPLIT_SLOTS = ("pna_resident", "pna_layer_fused", "pna_dense")  # the default mode's: none of them may run in the mode
TILE_ROWS, TILE_EDGES = 256, 4608  # pna.hip: PNA_FT_ROWS, PNA_FT_EDGES


def _graph(rng, n, k=4, hub=0):
    """n nodes, every node min(k, n - 1) in-edges from distinct other nodes; hub > 0: node 0 has exactly `hub` in-edges instead"""
    el = []
    for v in range(n):
        d = min(hub if (hub and v == 0) else k, n - 1)
        others = np.delete(np.arange(n), v)
        el += [(int(u), v) for u in rng.permutation(others)[:d]]
    el = np.array(el, np.int32).reshape(-1, 2)
    f = np.stack([rng.integers(0, c, n) for c in (119, 4, 12, 12, 10, 6, 6, 2, 2)], axis=1).astype(np.int32)
    return f, el[rng.permutation(len(el))] if len(el) else el


def _batch(graphs):
    nn = np.array([len(f) for f, _ in graphs], np.int32)
    ne = np.array([len(e) for _, e in graphs], np.int32)
    el = np.concatenate([e for _, e in graphs]) if ne.sum() else np.zeros((0, 2), np.int32)
    return GraphBatch(nn, ne, np.concatenate([f for f, _ in graphs]), el.astype(np.int32), np.zeros((len(el), 3), np.int32))


def _indeg(b):
    return np.bincount(b.global_edges()[:, 1], minlength=b.total_nodes)


def shape_cases():
    rng = np.random.default_rng(31)
    small = lambda m, n=12: [_graph(rng, n) for _ in range(m)]
    cases = []

    def add(name, graphs, options=None, slot=RESIDENT_SLOT, claim=lambda b: True):
        b = _batch(graphs)
        assert b.num_graphs <= 64
        cases.append(Case(name, b, options or {}, slot, claim))

    add("one-node-first-and-last", [_graph(rng, 1)] + small(5) + [_graph(rng, 1)],
        claim=lambda b: b.nums_of_nodes[0] == 1 and b.nums_of_nodes[-1] == 1 and b.nums_of_edges[0] == 0 and b.nums_of_edges[-1] == 0)
    add("edgeless-four-nodes", [_graph(rng, 4, k=0)] + small(3),
        claim=lambda b: b.nums_of_nodes[0] == 4 and b.nums_of_edges[0] == 0 and (_indeg(b)[:4] == 0).all())
    for n in (15, 16, 17, 255, 256):  # one graph = one tile of exactly n rows
        add(f"tile-of-{n}-rows", [_graph(rng, n, k=8)],
            claim=lambda b, n=n: b.num_graphs == 1 and b.total_nodes == n and b.total_edges <= TILE_EDGES)
    add("graph-across-the-wave-halves", [_graph(rng, 120, k=6), _graph(rng, 17, k=6)], options={"pna_binpack": 0},
        claim=lambda b: b.node_offsets()[1] == 120 and b.node_offsets()[2] == 137 and b.total_nodes <= TILE_ROWS)  # rows 120..136: waves 7 and 8
    for d in (16, 17, 40):  # the packed-word walk (16 in-edges in registers) against the LDS CSR tail
        add(f"hub-of-{d}-in-edges", [_graph(rng, d + 8, k=3, hub=d)] + small(2),
            claim=lambda b, d=d: _indeg(b)[0] == d and _indeg(b)[1:d + 8].max() <= 3)
    add("graph-of-300-nodes", small(3) + [_graph(rng, 300, k=4)] + small(2), slot=DENSE_SLOT,
        claim=lambda b: b.nums_of_nodes.max() == 300 > TILE_ROWS)  # fits no tile: the two-kernel layer
    # 70 nodes of 60 in-edges each: 4 200 in-edges, so no two of them share a tile of 4 608 and the tiles are 70 / 256 full: below 0.4
    add("graphs-of-70-nodes", [_graph(rng, 70, k=60) for _ in range(4)], slot=DENSE_SLOT,
        claim=lambda b: (b.nums_of_nodes == 70).all() and (2 * b.nums_of_edges > TILE_EDGES).all() and (b.nums_of_edges <= TILE_EDGES).all()
        and 70 / TILE_ROWS < 0.4)
    for bp in (1, 0):  # 32 graphs of 8 nodes fill a tile of 256 rows: the 33rd opens the next
        add(f"33-graphs-binpack-{bp}", [_graph(rng, 8, k=3) for _ in range(33)], options={"pna_binpack": bp},
            claim=lambda b: b.num_graphs == 33 and (b.nums_of_nodes == 8).all() and 32 * 8 == TILE_ROWS)
    add("tile-build-off", small(6, 20), options={"pna_tile_build": 0})
    return cases
