"""The split-f16 dense products ("Common numerics") restated in NumPy, the wrong variants of them that hand-written
kernels produce, and the bound that separates the two -- the reference side of tests/test_split_accuracy_gpu.py; what it proves is
asserted without a GPU in tests/test_split_ref_cpu.py.

A `dense` callable of tests/numpy_ref.py's forwards is (a [N][K], W [O][K]) -> [N][O].  `SplitDense` is the kernels' product:
activations split as DS_SPLIT2 / GS_SPLIT2 do (hi = rtz_f16(a), lo = rtz_f16(a - hi), a in fp32), weights as the host packers do
(pack_dense100_split and its kin: W * 2^-ilogb(max |W|), hi = rne_f16, lo = rne_f16 of the remainder), hi.hi + hi.lo + lo.hi summed
in float64, un-scaled and rounded to fp32.  Its `Spec` names what is dropped and where; `VARIANTS` lists the wrong ones.

The bound, per model, input and returned output (`table`): with err(x) = max |x - f64| / unit,
    E_ok  = the largest err of the correct restatements (every operation in fp32 with an fp32 product; the three-product split),
    E_bad = the smallest err of the wrong variants,          B = sqrt(E_ok * E_bad),
unit = the float64 forward's largest activation (dense inputs included) for node rows, max(1, max |f64 output|) for pooled rows and
logits.  B comes from these references every time; nothing here knows what a GPU returns."""
import functools
from collections import namedtuple

import numpy as np

from flowgnn_amd import graphpack as gp, weights
from tests import numpy_ref

MODELS = ["GIN", "GIN-VN", "GCN", "GAT", "PNA", "DGN"]
# Two batch seeds per model: 3 and 11, except where one of them leaves an output short of MIN_RATIO and another seed does not (GIN-VN's
# max-pooled logits at seed 3: 38; DGN's logits at seed 3: 63).  Chosen on the references alone, like everything else here.
SEEDS = {"GIN": (3, 11), "GIN-VN": (5, 11), "GCN": (3, 11), "GAT": (3, 11), "PNA": (3, 11), "DGN": (5, 11)}
LINEAR_HEAD = ("GIN", "GIN-VN", "GCN", "GAT")  # one linear layer on the pooled rows: node logits, sum and max pooling exist (flowgnn.h)
MIN_RATIO = 64.0  # E_bad / E_ok: 8 x of room on each side of B
# ... except: GCN's logits reach 50-80 at every seed tried (3, 5, 7, 11, 13, 17).  A logit is a mean over the graph's nodes of a dot
# product over 100 columns, so a split defect's errors (random in sign from row to row and column to column) average out, while E_ok there
# is the fp32 rounding of the head itself, relative to the largest logit.  16 x (4 x of room on each side) is what is asked of them.
# ... and GAT's logits in the pre-scale case (`weights_of`), 37 x at seed 3 and 21 x at seed 11: GAT has no bias, its logits are far
# below the unit's floor of 1, and with lin_1 and skip_3 at 2^-10 the head's own fp32 rounding is a larger share of every defect.  What
# that case is there for -- a wrong scale, a wrong 1 / scale -- is off by a factor of two or more.
LOW_RATIO = {("GCN", "logits", "synth"): 16.0, ("GCN", "logits_sum", "synth"): 16.0, ("GAT", "logits", "prescale"): 16.0}

# The pre-scale case runs on the default outputs, at one seed: the model's first, except DGN (logits 64.9 x at seed 5, 78.7 x at seed 11:
# a summation order away from 64).
CASE_OUTPUTS = {"synth": None, "prescale": ("logits", "h", "rows", "emb")}
PRESCALE_SEED = {m: (11 if m == "DGN" else SEEDS[m][0]) for m in MODELS}


def min_ratio(model, output, case="synth"):
    return LOW_RATIO.get((model, output, case), MIN_RATIO)


def cases():
    """(model, seed, case) of every input that the tests run."""
    return [(m, seed, "synth") for m in MODELS for seed in SEEDS[m]] + [(m, PRESCALE_SEED[m], "prescale") for m in MODELS]


# ---------------------------------------------------------------- operands
def rtz_f16(x):
    """float32 -> the f16 value toward zero (v_cvt_pkrtz_f16_f32), as float32; subnormals kept.  Bit operations: NumPy's float16
    conversions are slow, and they round to nearest."""
    x = np.ascontiguousarray(x, np.float32)
    t = (x.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32)          # 11 significant bits, the rest cut
    sub = np.abs(x) < np.float32(2.0 ** -14)                                  # below the normal range: multiples of 2^-24
    t = np.where(sub, np.trunc(x * np.float32(2.0 ** 24)) * np.float32(2.0 ** -24), t)
    return np.clip(t, np.float32(-65504.0), np.float32(65504.0))


def split_act(a):
    """(hi, lo) of the activations in float64: the kernels see a in fp32; a - hi is exact in fp32 (v_fma_mix_f32)."""
    a32 = np.asarray(a, np.float32)
    hi = rtz_f16(a32)
    lo = rtz_f16(a32 - hi)
    return hi.astype(np.float64), lo.astype(np.float64)


def pow2_scale(W):
    """2^-ilogb(max |W|): max |W| * scale in [1, 2) (pack_dense100_split, pow2_scale of gin_split.hip)."""
    m = float(np.abs(np.asarray(W, np.float32)).max())
    return float(np.ldexp(1.0, -int(np.floor(np.log2(m))))) if m > 0.0 and np.isfinite(m) else 1.0


def split_weight(W):
    """(hi, lo, scale) in float64: v = W * scale in fp32 (exact), hi = (_Float16)v, lo = (_Float16)(v - (float)hi), both to nearest even."""
    sc = pow2_scale(W)
    v = np.asarray(W, np.float32) * np.float32(sc)
    hi = v.astype(np.float16).astype(np.float32)
    lo = (v - hi).astype(np.float16).astype(np.float32)
    return hi.astype(np.float64), lo.astype(np.float64), sc


def dense_fp32(a, W):
    """The fp32 product (the *_mfma: 32 kernels, and the all-fp32 restatement): fp32 operands, fp32 sums."""
    return np.asarray(a, np.float32) @ np.asarray(W, np.float32).T


# ---------------------------------------------------------------- the product and its wrong variants
# drop:  "" | "hl" (a_hi . w_lo) | "lh" (a_lo . w_hi) | "both" (the single product a_hi . w_hi)
# where: "all" | "kstep" (one K-step of 32, `kstep_columns`) | "tile" (output columns 48..63) | "last" (the calls of the model's last
#        layer) | "last_h" (GAT: the last layer that flowgnn_get_h's o_3 depends on -- layer 4 comes after it)
# tail:  what features 96..99 of a K = 100 block are: "fp32" (v_mfma_f32_16x16x4f32 on the unsplit operands: dense100_split_kernel,
#        dense200_res_relu_split_kernel, gin_layer_split_kernel's first linear layer, gcn.hip), "split" (three-product like the rest:
#        gin_resident_kernel packs the tail's three products into one f16 MFMA; dgn_resident / dgn_layer_fused pad K to 112 per block
#        and split all of it) or "single" (wrong: the tail as one f16 product)
# K = 64 (GAT), 200 as GIN's hidden units and 320 (PNA) have no fp32 tail in any kernel.
Spec = namedtuple("Spec", "name drop where tail")
OK_SPECS = [Spec("three-product split, fp32 K tail", "", "all", "fp32"), Spec("three-product split, split K tail", "", "all", "split")]
VARIANTS = [
    Spec("a_hi.w_lo dropped", "hl", "all", "fp32"),
    Spec("a_lo.w_hi dropped", "lh", "all", "fp32"),
    Spec("single product", "both", "all", "fp32"),
    Spec("a_lo.w_hi dropped in one K-step", "lh", "kstep", "fp32"),
    Spec("a_hi.w_lo dropped in one K-step", "hl", "kstep", "fp32"),
    Spec("a_hi.w_lo dropped for 16 output columns", "hl", "tile", "fp32"),
    Spec("a_lo.w_hi dropped for 16 output columns", "lh", "tile", "fp32"),
    Spec("K tail as a single f16 product", "", "all", "single"),
    Spec("a_hi.w_lo dropped in the last layer", "hl", "last", "fp32"),
    Spec("a_lo.w_hi dropped in the last layer", "lh", "last", "fp32"),
    Spec("a_hi.w_lo dropped in the last layer before o_3", "hl", "last_h", "fp32"),
    Spec("a_lo.w_hi dropped in the last layer before o_3", "lh", "last_h", "fp32"),
]
BIAS_VARIANT = "1 / scale applied before the bias"  # (not a product: `misplaced_unscale` below)
CALLS = {"GIN": 10, "GIN-VN": 10, "GCN": 5, "GAT": 9, "PNA": 4, "DGN": 4}      # dense calls of one forward
LAST_CALLS = {"GIN": (8, 9), "GIN-VN": (8, 9), "GCN": (4,), "GAT": (7, 8), "PNA": (3,), "DGN": (3,)}  # GAT: lin_4 is formed at the end of layer 3
LAST_H_CALLS = {"GAT": (5, 6)}  # lin_3 and skip_3


def applies(spec, model, output):
    """Whether a wrong variant can show in an output of a model at all."""
    if spec.tail == "single":
        return any(tail_columns(model, K).size for K in (100, 200))
    if spec.where == "last_h":
        return model == "GAT" and output == "h"
    if spec.where == "last":
        return not (model == "GAT" and output == "h")
    return True


def kstep_columns(model, K):
    """The 32 features of one K-step, in the order of numpy_ref's operand: the last whole step of 32 consecutive features (k = 64..95 at
    K = 100, 160..191 of GIN's hidden units, 32..63 for GAT) -- but feature-major where the kernels contract so: PNA's step 9 is
    features 72..79 of the four aggregators (pna_pack_stream_layer), DGN's step 5 features 80..95 of both blocks (dgn_pack_fused_layer)."""
    if model == "PNA":
        return np.concatenate([80 * a + np.arange(72, 80) for a in range(4)])
    if model == "DGN":
        return np.concatenate([np.arange(80, 96), np.arange(180, 196)])
    return np.arange(32 * (K // 32 - 1), 32 * (K // 32))


def tail_columns(model, K):
    """The features that a K = 100 block's fp32 tail MFMA contracts; DGN's K = 200 is two such blocks."""
    if K == 100 and model in ("GIN", "GIN-VN", "GCN"):
        return np.arange(96, 100)
    if K == 200 and model == "DGN":
        return np.concatenate([np.arange(96, 100), np.arange(196, 200)])
    return np.zeros(0, np.int64)


class SplitDense:
    """One forward's `dense`: counts its calls (for where = "last") and keeps every input it saw (for the activation scale)."""

    def __init__(self, model, spec, keep_inputs=False):
        self.model, self.spec, self.calls = model, spec, 0
        self.inputs = [] if keep_inputs else None

    def __call__(self, a, W):
        spec, call = self.spec, self.calls
        self.calls += 1
        a32, W32 = np.asarray(a, np.float32), np.asarray(W, np.float32)
        N, K = a32.shape
        O = W32.shape[0]
        a_hi, a_lo = split_act(a32)
        w_hi, w_lo, sc = split_weight(W32)
        tail = tail_columns(self.model, K)
        main = np.ones(K, bool)
        main[tail] = False
        if spec.tail == "split":
            main[:] = True
        # where the defect applies: a mask over (output, k)
        hit = np.zeros((O, K), bool)
        if spec.drop:
            if spec.where == "all":
                hit[:] = True
            elif spec.where == "kstep":
                hit[:, kstep_columns(self.model, K)] = True
            elif spec.where == "tile":
                hit[48:64, :] = True
            elif spec.where in ("last", "last_h"):
                hit[:] = call in (LAST_CALLS if spec.where == "last" else LAST_H_CALLS).get(self.model, ())
        hl = np.where(hit & (spec.drop in ("hl", "both")), 0.0, w_lo) * main[None, :]
        lh = np.where(hit & (spec.drop in ("lh", "both")), 0.0, w_hi) * main[None, :]
        acc = a_hi @ (w_hi * main[None, :]).T + a_hi @ hl.T + a_lo @ lh.T
        if tail.size and spec.tail != "split":
            if spec.tail == "fp32":  # exact products of the fp32 operands (the weights pre-scaled, exactly)
                acc += a32[:, tail].astype(np.float64) @ (W32[:, tail].astype(np.float64) * sc).T
            else:                    # "single"
                acc += a_hi[:, tail] @ w_hi[:, tail].T
        return (acc / sc).astype(np.float32)


class Recorder:
    """Wraps a dense callable (None: the float matmul): keeps inputs and outputs of every call."""

    def __init__(self, dense=None):
        self.dense, self.inputs, self.outputs = dense, [], []

    def __call__(self, a, W):
        out = a @ W.T if self.dense is None else self.dense(a, W)
        self.inputs.append(np.asarray(a))
        self.outputs.append(np.asarray(out))
        return out


# ---------------------------------------------------------------- 1 / scale before the bias
BIASED = {  # split matrix -> the bias its accumulators start from (pre-scaled by the matrix's power of two)
    "GIN": [("node_mlp_1_weights", "node_mlp_1_bias"), ("node_mlp_2_weights", "node_mlp_2_bias")],
    "GCN": [("convs_weight", "convs_bias")],
    "PNA": [("node_conv_weights", "node_conv_bias")],
    "DGN": [("layers_posttrans_fully_connected_0_linear_weight", "layers_posttrans_fully_connected_0_linear_bias")],
    "GAT": [],  # lin and skip have no bias: the defect cannot show
}
BIASED["GIN-VN"] = BIASED["GIN"]


def misplaced_unscale(model, w):
    """The weights with which the correct forward computes what a kernel would that multiplied by 1 / scale BEFORE adding its pre-scaled
    bias: out = (W a) + scale * b, i.e. every such bias times its matrix's power of two (per layer)."""
    out = type(w)(w)
    for wk, bk in BIASED[model]:
        W, b = np.asarray(w[wk], np.float32), np.asarray(w[bk], np.float32).copy()
        for l in range(W.shape[0]):
            b[l] = b[l] * np.float32(pow2_scale(W[l]))
        out[bk] = b
    return out


# ---------------------------------------------------------------- inputs (tests/test_split_accuracy_gpu.py runs the same ones)
def _one_node(model, seed):
    rng = np.random.default_rng(seed)
    nf = np.stack([rng.integers(0, c, 1) for c in (119, 4, 12, 12, 10, 6, 6, 2, 2)], 1).astype(np.int32)
    eig = np.array([[0, 0.25, 0, 0]], np.float32) if model == "DGN" else None
    return gp.GraphBatch(np.array([1], np.int32), np.array([0], np.int32), nf, np.zeros((0, 2), np.int32), np.zeros((0, 3), np.int32), eig)


def _two_nodes(model, seed):
    rng = np.random.default_rng(seed)
    nf = np.stack([rng.integers(0, c, 2) for c in (119, 4, 12, 12, 10, 6, 6, 2, 2)], 1).astype(np.int32)
    eig = np.array([[0, 0.5, 0, 0], [0, -0.5, 0, 0]], np.float32) if model == "DGN" else None
    return gp.GraphBatch(np.array([2], np.int32), np.array([2], np.int32), nf, np.array([[0, 1], [1, 0]], np.int32),
                         rng.integers(0, 2, (2, 3)).astype(np.int32), eig)


@functools.lru_cache(maxsize=None)
def batch_of(model, seed):
    """64 molhiv-shaped graphs (GIN, GIN-VN, GCN, GAT) or 24 hep10k-shaped ones (PNA, DGN: there PNA's std = sqrt(Q / n - mean^2) does
    not cancel), then a one-node graph without edges and a two-node graph; one more single node if the rows would end on a 16-row tile."""
    if model in ("PNA", "DGN"):
        main = gp.synth_hep10k_batch(24, seed=seed, with_eigen=model == "DGN")
    else:
        main = gp.synth_molhiv_batch(64, seed=seed)
    parts = [main, _one_node(model, seed + 100), _two_nodes(model, seed + 200)]
    vn = model == "GIN-VN"
    if (sum(p.total_nodes + (p.num_graphs if vn else 0) for p in parts)) % 16 == 0:
        parts.append(_one_node(model, seed + 300))
    b = gp.concat_batches(parts)
    b = gp.add_virtual_nodes(b) if vn else b  # (as tests/test_gin_eps.py puts the virtual node in)
    assert b.total_nodes % 16 != 0
    return b


def base(model):
    return model.replace("-VN", "").lower()


SPLIT_KEYS = {"GIN": ("node_mlp_1_weights", "node_mlp_2_weights"), "GCN": ("convs_weight",), "GAT": ("linear_proj_weights", "skip_proj_weights"),
              "PNA": ("node_conv_weights",), "DGN": ("layers_posttrans_fully_connected_0_linear_weight",)}
SPLIT_KEYS["GIN-VN"] = SPLIT_KEYS["GIN"]


# (small, just below, just above) layer per split matrix.  GAT has no bias anywhere, so a layer whose two matrices are both small would
# shrink every later activation below the outputs' unit: its lin is small in layer 1 (lin_0 is not a split product) and its skip in
# layer 3 -- each time the layer's other term carries the signal on.
PRESCALE_LAYERS = {"linear_proj_weights": (1, 2, 3), "skip_proj_weights": (3, 1, 2)}


@functools.lru_cache(maxsize=None)
def weights_of(model, case="synth"):
    """"synth": the seeded synthetic set (full 24-bit mantissas, nonzero biases).  "prescale": the same with, per split matrix, one layer (0) at
    2^-10 of its size, another's (1) largest magnitude one fp32 step BELOW a power of two and a third's (2) one step ABOVE it: three different scales, the two sides of the ilogb boundary, and a layer whose lo halves live among the f16 subnormals
    before the scale lifts them."""
    w = getattr(weights, f"synth_{base(model)}_weights")(seed=7)
    if case == "synth":
        return w
    assert case == "prescale"
    w = type(w)(w)
    for k in SPLIT_KEYS[model]:
        W = np.asarray(w[k], np.float32).copy()
        tiny, below, above = PRESCALE_LAYERS.get(k, (0, 1, 2))
        W[tiny] *= np.float32(2.0 ** -10)
        for l, up in ((below, False), (above, True)):
            m = float(np.abs(W[l]).max())
            p = 2.0 ** np.floor(np.log2(m))
            target = np.nextafter(np.float32(p), np.float32(2 * p if up else 0))
            W[l] = (W[l].astype(np.float64) * (float(target) / m)).astype(np.float32)
            i = np.unravel_index(np.abs(W[l]).argmax(), W[l].shape)
            W[l][i] = np.sign(W[l][i]) * target  # exactly the step beside the power of two, whatever the rescale rounded to
            assert float(np.abs(W[l]).max()) == float(target)
        w[k] = W
    return w


# ---------------------------------------------------------------- the outputs a kernel instance can return
def _head(model, w, x, dtype):
    c = lambda a: np.asarray(a, dtype=dtype)
    D = x.shape[1]
    out = x @ c(w["graph_pred_weights"]).reshape(-1, D).T + c(w["graph_pred_bias"]).reshape(-1)
    return out[:, 0]


def gcn_rows(b, w, x4, dtype=np.float64):
    """numpy_ref.gcn_forward's last stage (l = 4: no dense product in it) on x_4 -- the rows GCN's readout pools, which the forward
    does not return; `outputs` checks it against the forward's own logits every time."""
    c = lambda a: np.asarray(a, dtype=dtype)
    eemb, root = c(w["edge_embedding_weight"]), c(w["convs_root_emb_weight"])
    bnw, bnb, bnm, bnv = c(w["bn_weight"]), c(w["bn_bias"]), c(w["bn_mean"]), c(w["bn_var"])
    N, x, one = b.total_nodes, c(x4), dtype(1.0)
    ge = b.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    outdeg = np.bincount(u, minlength=N).astype(dtype)
    dinv = np.where(outdeg > 0, one / np.sqrt(outdeg + one), dtype(0.0))
    norm = dinv[u] * dinv[v]
    ee = eemb[4][b.edge_attr.astype(np.int64) + numpy_ref.ED_OFF[None, :]].sum(axis=1)
    m = np.zeros((N, 100), dtype)
    np.add.at(m, v, norm[:, None] * np.maximum(x[u] + ee, 0.0))
    t = m + np.maximum(x + root[4], 0.0) / (outdeg[:, None] + one)
    return (t - bnm[4]) / np.sqrt(bnv[4] + dtype(2.0 ** -10)) * bnw[4] + bnb[4]


def gat_rows(b, w, proj4, skip4, dtype=np.float64):
    """numpy_ref.gat_forward's l == 4 branch on the two dense products it is made of (recorded by `Recorder`): attention over
    proj4 = o_3 lin_4^T, plus skip4 = o_3 skip_4^T, mean over the heads -- the [N][16] rows GAT's readout pools."""
    c = lambda a: np.asarray(a, dtype=dtype)
    tgt, srcw = c(w["scoring_fn_target"]), c(w["scoring_fn_source"])
    N = b.total_nodes
    ge = b.global_edges()
    u = np.concatenate([np.arange(N), ge[:, 0]])
    v = np.concatenate([np.arange(N), ge[:, 1]])
    p3 = c(proj4).reshape(N, 16, 4)
    ssrc = np.einsum("ndh,hd->nh", p3, srcw[4]); stgt = np.einsum("ndh,hd->nh", p3, tgt[4])
    s = ssrc[v] + stgt[u]
    e = np.exp(np.where(s < 0, dtype(0.2) * s, s))
    den = np.zeros((N, 4), dtype); np.add.at(den, v, e)
    num = np.zeros((N, 16, 4), dtype); np.add.at(num, v, e[:, None, :] * p3[u])
    o = (num / den[:, None, :]).reshape(N, 64) + c(skip4)
    return o.reshape(N, 16, 4).mean(axis=2)


def outputs(model, b, w, dtype=np.float64, dense=None):
    """name -> array, everything a kernel instance of the model returns, from ONE numpy_ref forward with (dtype, dense):
    logits; h (flowgnn_get_h: GIN h_5, GCN x_4, GAT o_3, PNA / DGN h_4); rows (node embeddings: what the readout pools); emb (their
    per-graph mean); for the linear heads also emb_sum, emb_max, logits_sum, logits_max and node_logits.  Also "_acts": the largest
    magnitude among the dumped layers and the dense inputs."""
    rec = Recorder(dense)
    fwd = getattr(numpy_ref, f"{base(model)}_forward")
    kw = {"return_x": True} if model == "GCN" else {"return_h": True}
    logits, hs = fwd(b, w, dtype=dtype, dense=rec, **kw)
    if model == "GCN":
        h, rows = hs[4], gcn_rows(b, w, hs[4], dtype)
    elif model == "GAT":
        h, rows = hs[3], gat_rows(b, w, rec.outputs[7], rec.outputs[8], dtype)
    else:
        h = rows = hs[-1]
    assert len(rec.inputs) == CALLS[model]
    off = b.node_offsets()[:-1]
    nn = np.asarray(b.nums_of_nodes, dtype=dtype)[:, None]
    out = {"logits": logits, "h": h, "rows": rows, "emb": np.add.reduceat(rows, off, axis=0) / nn}
    if model in LINEAR_HEAD:
        out["emb_sum"] = np.add.reduceat(rows, off, axis=0)
        out["emb_max"] = np.maximum.reduceat(rows, off, axis=0)
        out["logits_sum"], out["logits_max"] = _head(model, w, out["emb_sum"], dtype), _head(model, w, out["emb_max"], dtype)
        out["node_logits"] = _head(model, w, rows, dtype)
        # the restated rows are the forward's: its logits follow from them (the same operations in another association)
        tol = 1e-11 if dtype is np.float64 else 1e-4
        assert np.abs(_head(model, w, out["emb"], dtype) - logits).max() <= tol * max(1.0, float(np.abs(logits).max()))
    out["_acts"] = max([1.0, float(np.abs(hs).max())] + [float(np.abs(a).max()) for a in rec.inputs])
    return out


NODE_OUTPUTS = ("h", "rows")  # unit = the activation scale; everything else: max(1, max |f64 output|)


def unit_of(name, ref):
    return ref["_acts"] if name in NODE_OUTPUTS else max(1.0, float(np.abs(ref[name]).max()))


def err(got, ref, name):
    """max |got - f64| / unit"""
    want = ref[name]
    return float(np.abs(np.asarray(got, np.float64).reshape(want.shape) - want).max()) / unit_of(name, ref)


Row = namedtuple("Row", "e_ok e_bad bound ok bad")  # ok / bad: name -> err, per restatement / wrong variant


@functools.lru_cache(maxsize=None)
def reference(model, seed, case="synth"):
    """The float64 forward's outputs at the input (model, seed, case): the target of every comparison."""
    return outputs(model, batch_of(model, seed), weights_of(model, case))


@functools.lru_cache(maxsize=None)
def restatements(model, seed, case="synth"):
    """(ok, bad, specs): name -> outputs of every correct restatement and of every wrong variant at the input."""
    b, w = batch_of(model, seed), weights_of(model, case)
    ref = reference(model, seed, case)
    ok = {"all fp32": outputs(model, b, w, np.float32, dense_fp32)}
    for spec in OK_SPECS:
        ok[spec.name] = outputs(model, b, w, dense=SplitDense(model, spec))
    specs = {spec.name: spec for spec in VARIANTS if any(applies(spec, model, o) for o in ref)}
    bad = {name: outputs(model, b, w, dense=SplitDense(model, spec)) for name, spec in specs.items()}
    if BIASED[model]:
        bad[BIAS_VARIANT] = outputs(model, b, misplaced_unscale(model, w), dense=SplitDense(model, OK_SPECS[0]))
    return ok, bad, specs


@functools.lru_cache(maxsize=None)
def table(model, seed, case="synth"):
    """output name -> Row, from the references alone."""
    ref = reference(model, seed, case)
    ok, bad, specs = restatements(model, seed, case)
    rows = {}
    for name in ref:
        if name.startswith("_") or (CASE_OUTPUTS[case] is not None and name not in CASE_OUTPUTS[case]):
            continue
        eo = {k: err(v[name], ref, name) for k, v in ok.items()}
        eb = {k: err(v[name], ref, name) for k, v in bad.items() if k not in specs or applies(specs[k], model, name)}
        e_ok, e_bad = max(eo.values()), min(eb.values())
        rows[name] = Row(e_ok, e_bad, float(np.sqrt(e_ok * e_bad)), eo, eb)
    return rows

