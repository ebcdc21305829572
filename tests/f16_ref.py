"""Float64 NumPy restatement of GIN / GIN-VN in the f16 numeric mode (flowgnn.h: FLOWGNN_NUMERIC_F16), for the tests of that mode.

The same equations as tests/numpy_ref.py, with every operand of the node MLP's two linear layers rounded to f16 where the kernels
round it (gin_split.hip, single-product instances):
  * the aggregate a = h + sum_e relu(h[src] + e) (the first layer's input) and the ReLU'd hidden units (the second layer's input);
  * the weights, after the power-of-two scale the kernels apply per matrix (gin_split.hip: pow2_scale): r(W s) / s.  The hidden
    units are rounded in the scaled domain of the kernels as well: r(hid s1) / s1, s1 = the first linear layer's scale.
`fold` picks the readout rule of the path:
  * fold=True  -- the single-task graph-resident path: the last layer's second linear layer is folded into the readout,
                  logit = mean_v(r(hid_v s1) . r(u / s1)) + b2 . w + b,  u = W2^T w (rounded once);
  * fold=False -- every other path: h_5 = r(W2) r(hid) + b2, then the fp32 readout of h_5.
`rnd` picks the rounding: "rne" (the mode), "rtz" (round toward zero: what the probe must tell apart from it) or "none" (the
plain model: what the default f32 mode computes).

`eps`, `pooling` and `outputs` (gin_forward's docstring) restate the trained eps, the sum / max readouts and the further outputs of
the engine -- h_5 rows, the pooled vector, the per-node logit terms -- by their written definitions in flowgnn.h.

With check=True the function also proves that fp32 arithmetic would be EXACT on this input: for every sum it computes (encoder,
walk and the self term s_l h, both linear layers with their biases, readout dot products, the per-graph sums of the pool) the bound sum |terms| must stay
below 2^24 times the finest power of two every term is a multiple of -- then every partial sum, in any order, is representable in
fp32.  It returns the largest such ratio as log2 (<= 24 passes) besides the logits."""
import numpy as np

ND_OFF = np.array([0, 119, 123, 135, 147, 157, 163, 169, 171])
ED_OFF = np.array([0, 5, 11])


def pow2_scale(w):
    m = float(np.abs(w).max())
    if not (m > 0.0) or not np.isfinite(m):
        return 1.0
    return float(2.0 ** -np.floor(np.log2(m)))


def rtz16(x):
    """x rounded toward zero to f16 (saturating at the largest finite f16)."""
    x = np.asarray(x, np.float64)
    _, ex = np.frexp(x)
    e = np.maximum(ex - 1, -14)
    ulp = np.ldexp(1.0, e - 10)
    return np.clip(np.trunc(x / ulp) * ulp, -65504.0, 65504.0)


def rounder(rnd):
    if rnd == "rne":
        return lambda x: np.asarray(x, np.float64).astype(np.float16).astype(np.float64)
    if rnd == "rtz":
        return rtz16
    if rnd == "none":
        return lambda x: np.asarray(x, np.float64)
    raise ValueError(rnd)


def lsb_exp(x):
    """Per element: the exponent of the lowest set bit of x (a large number for 0: zeros constrain nothing)."""
    x = np.asarray(x, np.float64)
    m, ex = np.frexp(np.abs(x))
    mi = np.rint(m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    tz = np.where(mi > 0, np.log2(np.where(low > 0, low, 1)).astype(np.int64), 0)
    return np.where(x != 0, ex - 53 + tz, 10 ** 6)


class _Exact:
    """Largest log2(sum |terms| / quantum) over every sum the fp32 kernels compute (conservative: per-row bounds)."""

    def __init__(self):
        self.worst = -np.inf

    def sums(self, bound, quantum_exp):
        bound = np.asarray(bound, np.float64)
        q = np.asarray(quantum_exp, np.float64)
        ok = (bound > 0) & (q < 10 ** 5)
        if ok.any():
            self.worst = max(self.worst, float((np.log2(bound[ok]) - q[ok]).max()))

    def matmul(self, x, w, b=None):
        """x [N][K] @ w.T [K][M] + b [M]: row minima of the operands' lowest bits bound every term's from below"""
        qx = lsb_exp(x).min(axis=1)[:, None]
        qw = lsb_exp(w).min(axis=1)[None, :]
        q = qx + qw
        bound = np.abs(x) @ np.abs(w).T
        if b is not None:
            q = np.minimum(q, lsb_exp(b)[None, :])
            bound = bound + np.abs(b)[None, :]
        self.sums(bound, q)


def self_scale(eps):
    """s_l as the engine forms it, (float)(1.0f + eps[l]) (flowgnn.h: flowgnn_set_gin_eps), as float64; None (eps off): None."""
    if eps is None:
        return None
    return (np.float32(1.0) + np.asarray(eps, np.float32)).astype(np.float32).astype(np.float64)


OUTPUTS = ("logits", "rows", "pooled", "terms")
POINTS = ("a", "hid", "w", "u")  # the operand points the mode rounds


def pool(rows, batch, pooling):
    """[G][...]: the per-graph mean / sum / maximum of per-node values (flowgnn.h: flowgnn_set_pooling)."""
    st = batch.node_offsets()[:-1]
    if pooling == "max":
        return np.maximum.reduceat(rows, st, axis=0)
    s = np.add.reduceat(rows, st, axis=0)
    if pooling == "sum":
        return s
    if pooling != "mean":
        raise ValueError(pooling)
    return s / np.asarray(batch.nums_of_nodes, np.float64).reshape((-1,) + (1,) * (rows.ndim - 1))


def gin_forward(batch, w, fold=True, rnd="rne", check=False, eps=None, pooling="mean", outputs=None):
    """eps: five values or None -- the self term becomes s_l h with s_l = float32(1 + eps[l]), product and sum fp32 (flowgnn.h:
    flowgnn_set_gin_eps).  pooling: "mean" | "sum" | "max" (flowgnn.h: flowgnn_set_pooling; the maximum un-folds the readout, as
    NUM_TASK > 1 does: W . max is not a maximum of per-node scores).  outputs: None -- the logits, as ever; or names out of OUTPUTS --
    a dict of them:
      "rows"    h_5 [N][100], and "pooled" [G][100], the vector the head is applied to (the mean, sum or maximum of the rows): un-folded
                rule only -- the folded path never forms h_5, and asking it for either is an error;
      "terms"   the per-node logit terms (flowgnn.h: flowgnn_set_node_logits), [N] or [N][NUM_TASK]: rows . W + b un-folded,
                r(hid s1) . r(u / s1) + b2 . w + b folded; the mean of a graph's terms is its logit.
    The folded sum is the sum of the per-node terms less their constant, with no division: sum_v dots + n_g (b2 . w) + b.
    rnd may also be a dict {"a": .., "hid": .., "w": .., "u": ..} that names the rounding of each operand point alone -- the aggregate a,
    the hidden units, the MLP weights, the folded head u; a point left out is "rne" -- for references that are wrong in one respect only."""
    if pooling not in ("mean", "sum", "max"):
        raise ValueError(pooling)
    want = () if outputs is None else tuple(outputs)
    if any(o not in OUTPUTS for o in want):
        raise ValueError(want)
    if isinstance(rnd, dict):
        if set(rnd) - set(POINTS):
            raise ValueError(rnd)
        r_a, r_hid, r_w, r_u = (rounder(rnd.get(k, "rne")) for k in POINTS)
    else:
        r_a = r_hid = r_w = r_u = rounder(rnd)
    ex = _Exact()
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    nemb, eemb = f64(w["node_embedding_weight"]), f64(w["edge_embedding_weight"])
    w1, b1 = f64(w["node_mlp_1_weights"]), f64(w["node_mlp_1_bias"])
    w2, b2 = f64(w["node_mlp_2_weights"]), f64(w["node_mlp_2_bias"])
    pw, pb = f64(w["graph_pred_weights"]).reshape(-1, 100), f64(w["graph_pred_bias"]).reshape(-1)
    ntask = pw.shape[0]
    if ntask != 1 or pooling == "max":
        fold = False  # the folded readout is single-task, and a sum of per-node scores
    if fold and ("rows" in want or "pooled" in want):
        raise ValueError("the folded path forms neither h_5 nor its pooled vector")
    ss = self_scale(eps)
    done = lambda res: (res, ex.worst) if check else res
    N = batch.total_nodes
    ge = batch.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    terms = nemb[batch.node_feature.astype(np.int64) + ND_OFF[None, :]]  # [N][9][100]
    h = terms.sum(axis=1)
    if check:
        ex.sums(np.abs(terms).sum(axis=1), lsb_exp(terms).min(axis=1))
    off = batch.node_offsets()
    nn = f64(batch.nums_of_nodes)
    for l in range(5):
        eterms = eemb[l][batch.edge_attr.astype(np.int64) + ED_OFF[None, :]]
        ee = eterms.sum(axis=1)
        msg = np.maximum(h[u] + ee, 0.0)
        m = np.zeros((N, 100))
        np.add.at(m, v, msg)
        hs = h if ss is None else ss[l] * h  # the self term
        a = m + hs
        if check:
            ex.sums(np.abs(eterms).sum(axis=1), lsb_exp(eterms).min(axis=1))
            ex.sums(np.abs(h[u]) + np.abs(ee), np.minimum(lsb_exp(h[u]), lsb_exp(ee)))
            am = np.zeros((N, 100))
            np.add.at(am, v, np.abs(msg))
            qm = np.full((N, 100), 10 ** 6)
            np.minimum.at(qm, v, lsb_exp(msg))
            if ss is not None:
                ex.sums(np.abs(hs), lsb_exp(hs))  # the product s_l h is itself an fp32 value
            ex.sums(am + np.abs(hs), np.minimum(qm, lsb_exp(hs)))  # (the smaller quantum: s_l h may carry bits below h's)
        s1, s2 = pow2_scale(w1[l]), pow2_scale(w2[l])
        W1, W2 = r_w(w1[l] * s1) / s1, r_w(w2[l] * s2) / s2
        ar = r_a(a)
        pre = ar @ W1.T + b1[l]
        if check:
            ex.matmul(ar, W1, b1[l])
        hid = r_hid(np.maximum(pre, 0.0) * s1) / s1
        if l == 4 and fold:
            uu = r_u((w2[l].T @ pw[0]) / s1) * s1  # [200]: u rounded once (in the kernels' scaled domain)
            dots = hid @ uu
            c = float(b2[l] @ pw[0])
            if check:
                ex.matmul(hid, uu[None, :])
                ex.sums(np.add.reduceat(np.abs(dots), off[:-1]), np.minimum.reduceat(lsb_exp(dots), off[:-1]))
            if pooling == "sum":  # the sum of the per-node terms, no division: the constant b2 . w is a per-NODE term
                out = np.add.reduceat(dots, off[:-1]) + (nn * c + pb[0])
            else:
                out = np.add.reduceat(dots, off[:-1]) / batch.nums_of_nodes + c + pb[0]
            if outputs is None:
                return done(out)
            full = {"logits": out, "terms": dots + (c + pb[0])}
            return done({k: full[k] for k in want})
        hn = hid @ W2.T + b2[l]
        if check:
            ex.matmul(hid, W2, b2[l])
        h = np.maximum(hn, 0.0) if l != 4 else hn
    if outputs is None and pooling == "mean":  # (as it always was)
        if ntask == 1:
            dots = h @ pw[0]
            if check:
                ex.matmul(h, pw)
                ex.sums(np.add.reduceat(np.abs(dots), off[:-1]), np.minimum.reduceat(lsb_exp(dots), off[:-1]))
            out = np.add.reduceat(dots, off[:-1]) / batch.nums_of_nodes + pb[0]
        else:
            if check:
                ex.sums(np.add.reduceat(np.abs(h), off[:-1], axis=0), np.minimum.reduceat(lsb_exp(h), off[:-1], axis=0))
            pooled = np.add.reduceat(h, off[:-1], axis=0) / batch.nums_of_nodes[:, None]
            if check:
                ex.matmul(pooled, pw, pb)
            out = pooled @ pw.T + pb
        return done(out)
    # every other un-folded readout.  The logits in the order of the function's single-task mean where there is one (the pooled per-node
    # products), else the head of the pooled rows; the check covers the per-graph sums and the head products of that order, and of each
    # further output that is asked for: the pooled vector (sums of the rows, the head of the pooled rows) and the terms (the head of the rows).
    pooled = pool(h, batch, pooling)
    dots = h @ pw.T  # [N][ntask]
    by_dots = ntask == 1 and pooling != "max"
    if check:
        if by_dots:
            ex.matmul(h, pw)
            ex.sums(np.add.reduceat(np.abs(dots), off[:-1], axis=0), np.minimum.reduceat(lsb_exp(dots), off[:-1], axis=0))
        if not by_dots or "pooled" in want or "rows" in want:
            if pooling != "max":
                ex.sums(np.add.reduceat(np.abs(h), off[:-1], axis=0), np.minimum.reduceat(lsb_exp(h), off[:-1], axis=0))
            ex.matmul(pooled, pw, pb)
        if "terms" in want:
            ex.matmul(h, pw, pb)
    if by_dots:
        out = pool(dots[:, 0], batch, pooling) + pb[0]  # (the order of the function's single-task mean)
    else:
        out = pooled @ pw.T + pb
        if ntask == 1:
            out = out[:, 0]
    if outputs is None:
        return done(out)
    tv = dots + pb
    full = {"logits": out, "rows": h, "pooled": pooled, "terms": tv[:, 0] if ntask == 1 else tv}
    return done({k: full[k] for k in want})
