"""Float64 NumPy restatement of DGN in the f16 numeric mode (flowgnn.h: flowgnn_set_model_numeric_mode on a FLOWGNN_MODEL_DGN engine;
kernels: flowgnn_amd/csrc/dgn_f16.hip, dgn_emb_f16.hip, dgn_rows_f16.hip), for the tests of that mode.

The equations are tests/numpy_ref.dgn_forward's; the mode changes the operands of the matrix-pipe products and nothing else.  Per layer:
    x_u   = rnd(h[u])                                      each feature of a source row, once
    m1[v] = sum_{u->v} x_u                                  a1 = m1 / outdeg(v)   (x / 0 = 0)
    d_uv  = rnd((eig1[u] - eig1[v]) wscale_v)               wscale_v = 2^-floor(log2 abssum[v]) (exponent clamped at -100)
    pp[v] = sum_{u->v} x_u d_uv                             every copy of a duplicate edge is the same product
    a2    = |(pp - wsum[v] wscale_v h[v]) / (abssum[v] wscale_v)|      h[v] unrounded, wsum / abssum unrounded (abssum 0 -> 2^-13)
    acc   = b + (rnd(a1) @ rnd(W0 s).T + rnd(a2) @ rnd(W1 s).T) / s    s = the layer's power-of-two scale (dgn.hip: dgn_pack_fused_layer)
    h'    = h + relu(acc)
`rnd` picks the rounding: "rne" (the mode), "rtz" (toward zero) or "none" (the plain model: the f32 mode); `skip` names one operand
that stays unrounded -- "rows_m1" / "rows_m2" (the source rows as m1 / pp read them), "weight" (d_uv), "a1", "a2" -- the restatements
the probe must tell apart from the mode.

Also here: the probe (dyadic weights and eigenvectors, graphs of sources -> sinks -> drains whose fp32 sums are exact --
tests/test_dgn_f16_cpu.py proves which), the fixed shape cases of the GPU test, and the tolerance table of the accuracy inputs (LADDER,
TOL: computed by the CPU test)."""
from collections import OrderedDict, namedtuple

import numpy as np

from flowgnn_amd import graphpack as gp, weights
from flowgnn_amd.graphpack import GraphBatch
from tests import f16_ref as F, numpy_ref as N

ROUNDINGS = ("rne", "rtz", "none")
SKIPS = (None, "rows_m1", "rows_m2", "weight", "a1", "a2")
D = 100
K_EMB, K_W, K_B = ("embedding_h_atom_embedding_list_weights", "layers_posttrans_fully_connected_0_linear_weight",
                   "layers_posttrans_fully_connected_0_linear_bias")
HEAD = ("MLP_layer_FC_layers_0_weight", "MLP_layer_FC_layers_0_bias", "MLP_layer_FC_layers_1_weight", "MLP_layer_FC_layers_1_bias",
        "MLP_layer_FC_layers_2_weight", "MLP_layer_FC_layers_2_bias")

Result = namedtuple("Result", "logits hs rows scale")
f64 = lambda a: np.asarray(a, np.float64)


def row_scale(abssum):
    """wscale_v of dgn.hip: 2^-ae with abssum in [2^ae, 2^(ae+1)), ae clamped at -100 from below (abssum 0: 2^100)"""
    a = f64(abssum)
    ae = np.where(a > 0, np.floor(np.log2(np.where(a > 0, a, 1.0))), -127.0)
    return np.ldexp(1.0, -np.maximum(ae, -100.0).astype(np.int64))


def structure(batch):
    """what the row records hold, in float64 from the fp32 eigenvector column: u, v, we, wsum, abssum (0 kept), outdeg"""
    ge = batch.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    n = batch.total_nodes
    eig1 = f64(batch.node_eigen)[:, 1]
    we = eig1[u] - eig1[v]
    return u, v, we, np.bincount(v, weights=we, minlength=n), np.bincount(v, weights=np.abs(we), minlength=n), np.bincount(u, minlength=n).astype(np.float64)


def forward(batch, w, rnd="rne", skip=None, hook=None):
    """-> Result(logits [G], hs [5][N][100], rows = h_4, scale = the largest activation, at least 1).  hook(l, name, array): called with
    every intermediate of layer l (the probe's bookkeeping)."""
    assert rnd in ROUNDINGS and skip in SKIPS
    r = F.rounder(rnd)
    ro = lambda name, x: f64(x) if skip == name else r(x)
    emb, lw, lb = f64(w[K_EMB]), f64(w[K_W]), f64(w[K_B])
    n = batch.total_nodes
    u, v, we, wsum, abssum, outdeg = structure(batch)
    wscale = row_scale(abssum)
    abs_eps = np.where(abssum == 0, 2.0 ** -13, abssum)
    d = ro("weight", we * wscale[v])
    h = emb[np.arange(9)[None, :], batch.node_feature.astype(np.int64)].sum(axis=1)
    hs = [h]
    for l in range(4):
        m1, pp = np.zeros((n, D)), np.zeros((n, D))
        np.add.at(m1, v, ro("rows_m1", h)[u])
        np.add.at(pp, v, ro("rows_m2", h)[u] * d[:, None])
        a1 = np.where(outdeg[:, None] == 0, 0.0, m1 / np.maximum(outdeg, 1.0)[:, None])
        a2 = np.abs((pp - (wsum * wscale)[:, None] * h) / (abs_eps * wscale)[:, None])
        W = lw[l].reshape(D, 2, D)
        s = F.pow2_scale(lw[l])
        y = (ro("a1", a1) @ r(W[:, 0, :] * s).T + ro("a2", a2) @ r(W[:, 1, :] * s).T) / s
        acc = lb[l] + y
        if hook:
            for name, x in (("h", h), ("m1", m1), ("pp", pp), ("a1", a1), ("a2", a2), ("acc", acc)):
                hook(l, name, x)
        h = h + np.maximum(acc, 0.0)
        hs.append(h)
    hs = np.stack(hs)
    off = batch.node_offsets()
    hg = np.add.reduceat(h, off[:-1], axis=0) / f64(batch.nums_of_nodes)[:, None]
    o1 = np.maximum(hg @ f64(w[HEAD[0]]).T + f64(w[HEAD[1]]), 0.0)
    o2 = np.maximum(o1 @ f64(w[HEAD[2]]).T + f64(w[HEAD[3]]), 0.0)
    out = o2 @ f64(w[HEAD[4]]).reshape(-1) + f64(w[HEAD[5]]).reshape(-1)[0]
    return Result(out, hs, hs[4], max(1.0, float(np.abs(hs).max())))


def rule(x, ref, tol):
    """tests/parity.py's rule against the float64 forward `ref` (a Result): max |x - f64| / (tol (scale + |f64|)) of logits or rows"""
    x = f64(x)
    want = ref.logits if x.ndim == 1 else ref.rows
    return float((np.abs(x.reshape(want.shape) - want) / (tol * (ref.scale + np.abs(want)))).max())


# ---------------------------------------------------------------- the ladder and the accuracy inputs
LADDER = tuple(1e-4 * m * 10 ** k for k in range(3) for m in (1, 2, 5))  # 1e-4 x {1, 2, 5, 10, 20, 50, 100, 200, 500}
ACCURACY_SEEDS = (3, 11)
ACCURACY = (("synth", "logits"), ("synth", "rows"), ("trained", "logits"), ("trained", "rows"))  # (weights, output), on both seeds
# the smallest rung at which the "rne" restatement alone lies at <= 0.5 on both seeds (tests/test_dgn_f16_cpu.py holds this table to the
# computation and prints the ratios)
TOL = {("synth", "logits"): 1e-4, ("synth", "rows"): 5e-4, ("trained", "logits"): 1e-4, ("trained", "rows"): 5e-4}


def accuracy_batch(seed):
    return gp.synth_hep10k_batch(24, seed=seed)


def trained_weights():
    """the trained DGN set the reference ships (tests/golden/ref_weights_dgn.npz, tests/golden/make_ref_weights.py)"""
    import os
    import sys
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if here not in sys.path:
        sys.path.insert(0, here)
    import make_ref_weights as mrw
    return OrderedDict(mrw.load("DGN"))


def accuracy_weights(wname):
    return weights.synth_dgn_weights(7) if wname == "synth" else trained_weights()


def rung(ratio_at_1e4):
    """the smallest rung at which a restatement whose ratio of the 1e-4 rule is `ratio_at_1e4` lies at <= 0.5"""
    for t in LADDER:
        if ratio_at_1e4 * (1e-4 / t) <= 0.5:
            return t
    raise AssertionError(ratio_at_1e4)


# ---------------------------------------------------------------- the probe
# Every graph is 66 SOURCES -> 8 SINKS -> 4 DRAINS, one graph per tile (78 of 128 rows: fill 0.61).
#   sources  no in-edge: m1 = pp = 0, wsum = abssum = 0, so a1 = a2 = 0 and acc = b <= 0 (every bias is non-positive): they keep h_0, and
#            every layer sees the same aggregates.  64 of them come in 32 PAIRS (p, q) with eig1 = sign P (c + dl), sign P (1 - c - dl):
#            P = 2^-3, c a multiple of 1/16, dl = 3/8 of the f16 spacing of the smaller of c and 1 - c -- so a pair's |weights| add up to P
#            exactly, the rounding to nearest returns c and 1 - c (few bits: the products stay exact), the rounding toward zero moves
#            whichever member dl made smaller, and the unrounded weight keeps dl.  24 pairs are positive, 8 negative.  Two SINGLES carry
#            eig1 = +P and -P.
#   sinks    eig1 = 0, so w_uv = eig1[u].  In-degrees 1, 1 (a single each), 2, 2 (one pair), 4, 4 (two pairs), 32 (12 positive and 4
#            negative pairs, from both 32-source blocks) and 64 (every pair: the row crosses a block boundary): sum |w| is a power of
#            two and sum w is zero or a power of two with either sign, so wscale, 1 / abssum and wsum wscale are exact powers of two.
#            Out-degrees 1, 2 and 4 (edges to the drains): a1 = m1 / outdeg is exact.
#   drains   eig1 = 0 like their in-neighbours: every weight is 0, abssum = 0 (the 2^-13 branch), a2 = 0; out-degree 0, a1 = 0: they
#            keep h_0 too.  They exist to give the sinks an out-degree: a1 divides by the TARGET's out-degree.
# h_0 = +-(1 + k 2^-12), the two bits below f16's eleven mostly 11 (13 bits: "rne", "rtz" and "none" are three values on a majority), from the atom table alone (the other eight tables are
# zero).  Layer weights (W s) in {0, +-1/2, +-1} at density 0.05, biases -k 2^-8.  The second and third graph list their nodes in other
# orders (sinks and drains first; interleaved), so the sources sit at other rows of the tile.
PROBE_GRAPHS = 3
N_PAIRS, N_SRC, N_SINK, N_DRAIN = 32, 66, 8, 4
N_PER = N_SRC + N_SINK + N_DRAIN
H = 50  # features f and f + H are twins (below)
SINK_OUTDEG = (1, 2, 1, 2, 2, 4, 2, 4)
P_EIG = 2.0 ** -3
BOUND = 1e-6  # the probe's bound: |x - want| <= BOUND (1 + |want|)
SEPARATION = 100.0
SHARE = 0.5   # ... apart by more than SEPARATION x the bound on more than this share of the compared values
VARIANTS = (("none", None), ("rtz", None), ("rne", "rows_m1"), ("rne", "rows_m2"), ("rne", "weight"), ("rne", "a1"), ("rne", "a2"))
PROBE_OPTIONS = {"dgn_mfma_agg": 1}  # (122 edges on 78 nodes: by density the plan would pick the in-edge walk)


def variant_name(v):
    return v[0] if v[1] is None else "skip-" + v[1]


def _f16_spacing(c):
    return 2.0 ** (np.floor(np.log2(c)) - 10)


def probe_batch():
    rng = np.random.default_rng(40)
    feats, edges, eigs, nn, ne, roles = [], [], [], [], [], []
    for gi in range(PROBE_GRAPHS):
        # local roles: sources 0..65 (pair k = sources 2k, 2k + 1; singles 64, 65), sinks 66..73, drains 74..77
        eig = np.zeros(N_PER)
        c = rng.choice([3, 5, 6, 7, 9, 10, 11, 13], N_PAIRS) / 16.0  # (neither c nor 1 - c a power of two: dl stays inside one binade)
        sign = np.where(np.arange(N_PAIRS) < 24, 1.0, -1.0)[rng.permutation(N_PAIRS)]
        dl = 0.375 * _f16_spacing(np.minimum(c, 1 - c)) * rng.choice([-1.0, 1.0], N_PAIRS)
        eig[0:64:2], eig[1:64:2] = sign * P_EIG * (c + dl), sign * P_EIG * (1 - c - dl)
        eig[64], eig[65] = P_EIG, -P_EIG
        pos, neg = np.nonzero(sign > 0)[0], np.nonzero(sign < 0)[0]
        pairs = lambda ks: [int(x) for k in ks for x in (2 * k, 2 * k + 1)]
        sink_src = [[64], [65], pairs(rng.permutation(pos)[:1]), pairs(rng.permutation(neg)[:1]),
                    pairs(rng.permutation(pos)[:2]), pairs(list(rng.permutation(pos)[:1]) + list(rng.permutation(neg)[:1])),
                    pairs(list(rng.permutation(pos)[:12]) + list(rng.permutation(neg)[:4])), pairs(range(N_PAIRS))]
        el = [(u, N_SRC + k) for k, src in enumerate(sink_src) for u in src]
        for k, od in enumerate(SINK_OUTDEG):
            el += [(N_SRC + k, N_SRC + N_SINK + int(t)) for t in rng.permutation(N_DRAIN)[:od]]
        el = np.array(el, np.int64)
        role = np.array([0] * N_SRC + [1] * N_SINK + [2] * N_DRAIN)
        # the node order of the graph: as above, sinks and drains first, or shuffled
        order = (np.arange(N_PER), np.concatenate([np.arange(N_SRC, N_PER), np.arange(N_SRC)]), rng.permutation(N_PER))[gi % 3]
        place = np.empty(N_PER, np.int64)
        place[order] = np.arange(N_PER)  # local role index -> node id in the graph
        el = place[el][rng.permutation(len(el))]
        f = np.zeros((N_PER, 9), np.int32)
        f[:, 0] = rng.permutation(119)[:N_PER]
        e4 = np.zeros((N_PER, 4), np.float32)
        e4[place, 1] = eig.astype(np.float32)
        assert np.array_equal(f64(e4[place, 1]), eig)  # dyadic, few bits: fp32 holds them
        r = np.empty(N_PER, np.int64)
        r[place] = role
        feats.append(f); edges.append(el.astype(np.int32)); eigs.append(e4); nn.append(N_PER); ne.append(len(el)); roles.append(r)
    el = np.concatenate(edges)
    b = GraphBatch(np.array(nn, np.int32), np.array(ne, np.int32), np.concatenate(feats), el, np.zeros((len(el), 3), np.int32), np.concatenate(eigs))
    return b, np.concatenate(roles)


def probe_classes(b):
    """per node of the batch: in-degree, out-degree"""
    ge = b.global_edges()
    return np.bincount(ge[:, 1], minlength=b.total_nodes), np.bincount(ge[:, 0], minlength=b.total_nodes)


def probe_weights():
    rng = np.random.default_rng(41)
    w = weights.synth_dgn_weights(7)
    for k in HEAD:  # a head without cancellation: its fp32 sums stay within the bound of the float64 ones
        w[k] = (np.abs(np.asarray(w[k], np.float32)) * np.float32(0.25)).astype(np.float32)
    T = np.zeros((9, 119, D))
    # 13 significant bits; f16 drops the last two.  On 0.6 of the entries the twins end in 11 and 10 behind an odd kept part, so nearest
    # rounds both UP (10 is a tie: to even) and toward zero rounds both down: three different values.  On the others they end in two
    # different ones of 00, 01, 10, 11 behind an even kept part: the twins mostly round to different f16 values.
    up = rng.random((119, H)) < 0.6
    kept = (rng.integers(0, 2 ** 9 - 1, (119, H)) << 1) | up  # odd where both round up
    lo = np.where(up[..., None], rng.permuted(np.broadcast_to([3, 2], (119, H, 2)), axis=2),
                  rng.permuted(np.broadcast_to([0, 1, 2, 3], (119, H, 4)), axis=2)[..., :2])
    sg = rng.choice([-1.0, 1.0], (119, H))
    T[0, :, :H] = sg * (1.0 + ((kept << 2) | lo[..., 0]) * 2.0 ** -12)
    T[0, :, H:] = sg * (1.0 + ((kept << 2) | lo[..., 1]) * 2.0 ** -12)  # the twin: one to three units of 2^-12 away
    lw = np.zeros((4, D, 2, D))
    for l in range(4):
        half = rng.choice([0.5, 1.0], (H, 2, H)) * rng.choice([-1.0, 1.0], (H, 2, H)) * (rng.random((H, 2, H)) < 0.1)
        half[0, 0, 0] = 1.0  # the layer's largest entry: the scale is 1
        lw[l, :H, :, :H], lw[l, :H, :, H:] = half, -half
        lw[l, H:] = lw[l, :H]
    lb = np.tile(-rng.integers(0, 4, (4, H)) * 2.0 ** -12, (1, 2))
    w[K_EMB] = T.astype(np.float32)
    w[K_W] = lw.reshape(4, D, 2 * D).astype(np.float32)
    w[K_B] = lb.astype(np.float32)
    return w


def probe_check(b, w):
    """The "rne" forward of the probe with the bookkeeping of tests/f16_ref._Exact, per ROW: -> (Result, worst [N]: per row the largest
    log2(sum |terms| / quantum) over every fp32 sum the kernels form for it in the four layers -- <= 24: every partial sum, in any
    order, is a representable fp32 value).  The sums: the encoder's nine terms, m1, pp, fma(-wsum wscale, h, pp), the update's 200
    products with the bias, and h + relu(acc)."""
    r = F.rounder("rne")
    n = b.total_nodes
    u, v, we, wsum, abssum, outdeg = structure(b)
    wscale = row_scale(abssum)
    worst = np.full(n, -np.inf)

    kinds = {}

    def sums(bound, q, rows=None, kind=None):
        """per row (first axis): bound [N][..] = sum |terms|, q = the finest bit of any term"""
        bound, q = f64(bound), f64(q)
        bound, q = np.broadcast_arrays(bound.reshape(len(bound), -1), q.reshape(len(q), -1))
        ok = (bound > 0) & (q < 10 ** 5)
        ratio = np.where(ok, np.log2(np.where(ok, bound, 1.0)) - np.where(ok, q, 0.0), -np.inf).max(axis=1)
        idx = np.arange(n) if rows is None else rows
        np.maximum.at(worst, idx, ratio)
        if kind:
            kinds[kind] = max(kinds.get(kind, -np.inf), float(ratio.max()))

    emb, lw, lb = f64(w[K_EMB]), f64(w[K_W]), f64(w[K_B])
    terms = emb[np.arange(9)[None, :], b.node_feature.astype(np.int64)]
    sums(np.abs(terms).sum(axis=1), F.lsb_exp(terms).min(axis=1))
    # the row records: wsum and abssum as fp32 sums, and what is derived from them must be powers of two (or zero)
    qa = np.full(n, 10 ** 6, np.int64)
    np.minimum.at(qa, v, F.lsb_exp(we))
    sums(abssum[:, None], qa[:, None])
    pow2 = lambda x: (x == 0) | (np.abs(x) == 2.0 ** np.round(np.log2(np.where(x == 0, 1.0, np.abs(x)))))
    has_in = np.bincount(v, minlength=n) > 0  # (a row without in-edges multiplies 1 / outdeg by m1 = 0)
    assert pow2(abssum).all() and pow2(wsum).all() and pow2(outdeg[has_in]).all()
    d = r(we * wscale[v])
    state = {}

    def hook(l, name, x):
        state[name] = x
        if name != "acc":
            return
        h, m1, pp, a1, a2 = (state[k] for k in ("h", "m1", "pp", "a1", "a2"))
        xr = r(h)
        S, Sq = np.zeros((n, D)), np.full((n, D), 10 ** 6, np.int64)
        np.add.at(S, v, np.abs(xr[u])); np.minimum.at(Sq, v, F.lsb_exp(xr[u]))
        sums(S, Sq, kind='m1')  # m1
        t = xr[u] * d[:, None]
        S, Sq = np.zeros((n, D)), np.full((n, D), 10 ** 6, np.int64)
        np.add.at(S, v, np.abs(t)); np.minimum.at(Sq, v, F.lsb_exp(t))
        sums(S, Sq, kind='pp')  # pp
        ws = (wsum * wscale)[:, None] * h
        sums(np.abs(pp) + np.abs(ws), np.minimum(F.lsb_exp(pp), F.lsb_exp(ws)), kind='fma')  # the fma: its one rounding must be exact
        W = lw[l].reshape(D, 2, D)
        s = F.pow2_scale(lw[l])
        Ws = np.concatenate([W[:, 0, :], W[:, 1, :]], axis=1) * s  # [out][200]
        assert np.array_equal(r(Ws), Ws) and np.array_equal(Ws * 2, np.rint(Ws * 2))
        ar = np.concatenate([r(a1), r(a2)], axis=1)  # [N][200]
        la = F.lsb_exp(ar)
        bound = np.abs(ar) @ np.abs(Ws).T + np.abs(lb[l] * s)[None, :]
        q = np.empty((n, D))
        for o in range(D):
            nz = Ws[o] != 0
            q[:, o] = np.minimum((la[:, nz] + F.lsb_exp(Ws[o, nz])[None, :]).min(axis=1) if nz.any() else 10 ** 6, F.lsb_exp(lb[l, o] * s))
        sums(bound, q, kind='dense')  # the update's accumulator (scaled domain)
        relu = np.maximum(x, 0.0)
        sums(np.abs(h) + relu, np.minimum(F.lsb_exp(h), F.lsb_exp(relu)), kind='res')  # h + relu(acc)

    res = forward(b, w, "rne", hook=hook)
    probe_check.kinds = kinds
    return res, worst


def bound(x):
    return BOUND * (1.0 + np.abs(f64(x)))


def compared(b, roles, v):
    """the values of h_4 [N][100] a variant is compared on: the sinks' rows -- all of them, or, where a single in-edge makes the skipped
    rounding a no-op, those of in-degree 2 and more: a lone weight is +-1 after the row's scale, and with one source m1 = x_u and
    a1 = x_u / 2^k are f16 values already, so rounding the source row or a1 or neither gives the same a1"""
    indeg, _ = probe_classes(b)
    m = np.zeros((b.total_nodes, D), bool)
    m[(roles == 1) & (indeg >= (2 if v[1] in ("weight", "rows_m1", "a1") else 1))] = True
    return m


def separated(x, other, want, mask):
    """x [N][100] apart from `other` by more than SEPARATION x the bound (of `want`) on more than SHARE of the masked values -> (ok, fraction)"""
    frac = float((np.abs(f64(x) - other)[mask] > SEPARATION * bound(want)[mask]).mean())
    return frac > SHARE, frac


# ---------------------------------------------------------------- the fixed shape cases of the GPU test
Case = namedtuple("Case", "name batch options claim")  # claim(batch): what the case says of itself
RESIDENT_SLOT, LAYER_SLOT = "dgn_resident_f16", "dgn_layer_mfma_f16"
DEFAULT_SLOTS = ("dgn_resident", "dgn_layer_fused", "dgn_aggregate", "dgn_dense")  # the default mode's: none of them may run in the mode
TILE_ROWS, TILE_EDGES = 128, 2560  # dgn.hip: DGN_FT_ROWS, DGN_FT_EDGES


def _graph(rng, n, k=8, zero_eig_rows=(), no_in=()):
    """n nodes, every node min(k, n - 1) in-edges from distinct other nodes (none for the nodes of no_in); eig1 random on a unit vector,
    but equal (0) on zero_eig_rows AND their in-neighbours, so those rows' weights are all zero"""
    el = []
    for v in range(n):
        if v in no_in:
            continue
        others = np.delete(np.arange(n), v)
        el += [(int(u), v) for u in rng.permutation(others)[:min(k, n - 1)]]
    el = np.array(el, np.int32).reshape(-1, 2)
    f = np.stack([rng.integers(0, c, n) for c in (119, 4, 12, 12, 10, 6, 6, 2, 2)], axis=1).astype(np.int32)
    eig = rng.uniform(-1.0, 1.0, (n, 4))
    eig /= np.maximum(np.sqrt((eig ** 2).sum(axis=0, keepdims=True)), 1e-12)
    for v in zero_eig_rows:
        eig[v, 1] = 0.0
        eig[el[el[:, 1] == v, 0], 1] = 0.0
    return f, (el[rng.permutation(len(el))] if len(el) else el), eig.astype(np.float32)


def _batch(graphs):
    nn = np.array([len(g[0]) for g in graphs], np.int32)
    ne = np.array([len(g[1]) for g in graphs], np.int32)
    el = np.concatenate([g[1] for g in graphs]) if ne.sum() else np.zeros((0, 2), np.int32)
    return GraphBatch(nn, ne, np.concatenate([g[0] for g in graphs]), el.astype(np.int32), np.zeros((len(el), 3), np.int32),
                      np.concatenate([g[2] for g in graphs]))


def _indeg(b):
    return np.bincount(b.global_edges()[:, 1], minlength=b.total_nodes)


def _with_copies(g, mult):
    """the graph with the in-edges of node 0 listed `mult` times"""
    f, el, eig = g
    extra = el[el[:, 1] == 0]
    return f, np.concatenate([el] + [extra] * (mult - 1)), eig


def shape_cases():
    """Every case runs with dgn_mfma_agg = 1 and dgn_resident = 2 (small graphs are sparse jobs by the density rule) on the resident
    kernel; tiles fill to >= 0.4 or the case says otherwise."""
    rng = np.random.default_rng(51)
    small = lambda m, n=24: [_graph(rng, n) for _ in range(m)]
    base = {"dgn_mfma_agg": 1, "dgn_resident": 2}
    cases = []

    def add(name, graphs, options=None, claim=lambda b: True):
        b = _batch(graphs)
        cases.append(Case(name, b, dict(base, **(options or {})), claim))

    add("one-node-without-edges", [_graph(rng, 1)] + small(4) + [_graph(rng, 1)],
        claim=lambda b: b.nums_of_nodes[0] == 1 and b.nums_of_nodes[-1] == 1 and b.nums_of_edges[0] == 0 and b.nums_of_edges[-1] == 0)
    for n in (31, 32, 33, 128):  # block and tile edges; with three small graphs in front at 31..33 so the tile is full enough
        add(f"graph-of-{n}-nodes", [_graph(rng, n, k=12)] + (small(2) if n < 128 else []),
            claim=lambda b, n=n: b.nums_of_nodes[0] == n and b.nums_of_edges[0] <= TILE_EDGES)
    # 100 graphs of one or two nodes, 125 rows: they fit ONE tile, which then holds more graphs than a wave has lanes
    add("tile-of-100-tiny-graphs", [_graph(rng, 2 if i % 4 == 0 else 1, k=1) for i in range(100)], options={"dgn_binpack": 1},
        claim=lambda b: b.num_graphs == 100 > 63 and b.total_nodes == 125 <= TILE_ROWS)
    add("rows-without-in-edges", [_graph(rng, 30, no_in=(0, 7, 29))] + small(2),
        claim=lambda b: (_indeg(b)[[0, 7, 29]] == 0).all())
    add("rows-whose-weights-are-all-zero", [_graph(rng, 30, zero_eig_rows=(3,))] + small(2),
        claim=lambda b: _indeg(b)[3] > 0 and (np.abs(f64(b.node_eigen)[b.global_edges()[b.global_edges()[:, 1] == 3, 0], 1]) == 0).all()
        and b.node_eigen[3, 1] == 0)
    for mult in (2, 3):
        add(f"duplicate-edges-x{mult}", [_with_copies(_graph(rng, 30), mult)] + small(2),
            claim=lambda b, mult=mult: _indeg(b)[0] == 8 * mult)
    for bp in (1, 0):  # five graphs of 24 rows fill a tile of 128; the sixth opens the next
        add(f"six-graphs-binpack-{bp}", small(6), options={"dgn_binpack": bp}, claim=lambda b: b.num_graphs == 6 and b.total_nodes == 144)
    return cases
