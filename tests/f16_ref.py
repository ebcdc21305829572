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

With check=True the function also proves that fp32 arithmetic would be EXACT on this input: for every sum it computes (encoder,
walk, both linear layers with their biases, readout dot products, the per-graph sums of the pool) the bound sum |terms| must stay
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


def gin_forward(batch, w, fold=True, rnd="rne", check=False):
    r = rounder(rnd)
    ex = _Exact()
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    nemb, eemb = f64(w["node_embedding_weight"]), f64(w["edge_embedding_weight"])
    w1, b1 = f64(w["node_mlp_1_weights"]), f64(w["node_mlp_1_bias"])
    w2, b2 = f64(w["node_mlp_2_weights"]), f64(w["node_mlp_2_bias"])
    pw, pb = f64(w["graph_pred_weights"]).reshape(-1, 100), f64(w["graph_pred_bias"]).reshape(-1)
    ntask = pw.shape[0]
    if ntask != 1:
        fold = False  # the folded readout is single-task
    N = batch.total_nodes
    ge = batch.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    terms = nemb[batch.node_feature.astype(np.int64) + ND_OFF[None, :]]  # [N][9][100]
    h = terms.sum(axis=1)
    if check:
        ex.sums(np.abs(terms).sum(axis=1), lsb_exp(terms).min(axis=1))
    off = batch.node_offsets()
    for l in range(5):
        eterms = eemb[l][batch.edge_attr.astype(np.int64) + ED_OFF[None, :]]
        ee = eterms.sum(axis=1)
        msg = np.maximum(h[u] + ee, 0.0)
        m = np.zeros((N, 100))
        np.add.at(m, v, msg)
        a = m + h
        if check:
            ex.sums(np.abs(eterms).sum(axis=1), lsb_exp(eterms).min(axis=1))
            ex.sums(np.abs(h[u]) + np.abs(ee), np.minimum(lsb_exp(h[u]), lsb_exp(ee)))
            am = np.zeros((N, 100))
            np.add.at(am, v, np.abs(msg))
            qm = np.full((N, 100), 10 ** 6)
            np.minimum.at(qm, v, lsb_exp(msg))
            ex.sums(am + np.abs(h), np.minimum(qm, lsb_exp(h)))
        s1, s2 = pow2_scale(w1[l]), pow2_scale(w2[l])
        W1, W2 = r(w1[l] * s1) / s1, r(w2[l] * s2) / s2
        ar = r(a)
        pre = ar @ W1.T + b1[l]
        if check:
            ex.matmul(ar, W1, b1[l])
        hid = r(np.maximum(pre, 0.0) * s1) / s1
        if l == 4 and fold:
            uu = r((w2[l].T @ pw[0]) / s1) * s1  # [200]: u rounded once (in the kernels' scaled domain)
            dots = hid @ uu
            c = float(b2[l] @ pw[0])
            if check:
                ex.matmul(hid, uu[None, :])
                ex.sums(np.add.reduceat(np.abs(dots), off[:-1]), np.minimum.reduceat(lsb_exp(dots), off[:-1]))
            out = np.add.reduceat(dots, off[:-1]) / batch.nums_of_nodes + c + pb[0]
            return (out, ex.worst) if check else out
        hn = hid @ W2.T + b2[l]
        if check:
            ex.matmul(hid, W2, b2[l])
        h = np.maximum(hn, 0.0) if l != 4 else hn
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
    return (out, ex.worst) if check else out
