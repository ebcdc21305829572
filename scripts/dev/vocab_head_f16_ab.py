"""The vocabulary head's f16 numeric mode against its default form (flowgnn.h: flowgnn_set_vocab_head_numeric).
    usage: vocab_head_f16_ab.py [OUT.json]      (default: profiles/vocab_head_f16_ab.json; FLOWGNN_LIB: another build of the library)
P = 5 positions, V = 5002 entries, vocab_head_ab.py's synthetic batches of 4 096 and 2^16 graphs, one process, one engine, the
profile slots of flowgnn_profile_read, three warm runs and then ten measured, per launch.  Per size the default form (vocab_head +
vocab_head_fold) is measured, then the f16 form (vocab_head_f16 + vocab_head_fold), then the default form again: the two default
figures show the yardstick's spread, and the f16 form counts as faster only where it beats the faster of the two by more than that."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
if os.environ.get("FLOWGNN_LIB"):
    from flowgnn_amd import _lib as _L
    _L.LIB_PATH = os.path.abspath(os.environ["FLOWGNN_LIB"])
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

P, V, D, RUNS = 5, 5002, 300, 10
PEAK_F16_TFLOPS = 2516.0  # MI355X, dense f16 matrix pipe (profiles/limits.json's source)
rng = np.random.default_rng(1)
hw = (rng.uniform(-1, 1, (P, V, D)) / np.sqrt(D)).astype(np.float32)
hb = (rng.uniform(-1, 1, (P, V)) / np.sqrt(D)).astype(np.float32)


def batch_of(G):
    n = 1 + np.arange(G) % 5
    el = np.concatenate([np.stack([np.arange(k - 1), np.arange(1, k)], 1) for k in n if k > 1]).astype(np.int32)
    return gp.GraphBatch(n.astype(np.int32), (n - 1).astype(np.int32), np.zeros((int(n.sum()), 9), np.int32), el, np.zeros((len(el), 3), np.int32))


def per_launch(e, slots):
    for _ in range(3):
        e.run(); e.sync()
    a = e.profile_read()
    for _ in range(RUNS):
        e.run(); e.sync()
    b = e.profile_read()
    zero = {"launches": 0, "total_ms": 0.0}
    ran = lambda s: b.get(s, zero)["launches"] - a.get(s, zero)["launches"]  # (no fold where the plan has one slice: 0 ms)
    out = {s: (b[s]["total_ms"] - a.get(s, zero)["total_ms"]) / ran(s) if ran(s) else 0.0 for s in slots}
    out["sum"] = sum(out[s] for s in slots)
    return out


e = Engine("GIN", device=0)
e.set_emb_dim(300)
e.set_weights(weights.synth_gin_weights(seed=7, emb_dim=300))
e.set_vocab_head(hw, hb)
e.profile_enable(True)
res = {"positions": P, "vocab": V, "runs": RUNS}
for G in (4096, 1 << 16):
    e.set_batch(batch_of(G))
    r = {}
    for name, mode, slot in (("default_a", "f32", "vocab_head"), ("f16", "f16", "vocab_head_f16"), ("default_b", "f32", "vocab_head")):
        e.set_vocab_head_numeric(mode)
        r[name] = per_launch(e, [slot, "vocab_head_fold"])
    base = min(r["default_a"]["sum"], r["default_b"]["sum"])
    r["yardstick_spread"] = abs(r["default_a"]["sum"] - r["default_b"]["sum"]) / base
    r["default_over_f16"] = base / r["f16"]["sum"]
    r["f16_faster_beyond_spread"] = bool(r["f16"]["sum"] * (1.0 + r["yardstick_spread"]) < base)
    flops = 2.0 * G * P * (32 * ((V + 31) // 32)) * 320  # executed: one MFMA per product, K padded to 320, V to whole two-tile chunks
    r["f16_pipe_fraction"] = flops / (r["f16"]["vocab_head_f16"] * 1e-3) / (PEAK_F16_TFLOPS * 1e12)
    r["exact_reruns"] = e.exact_reruns()
    res[f"head_{G}"] = r
    print(json.dumps({G: r}), flush=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vocab_head_f16_ab.json")
json.dump(res, open(out, "w"), indent=1)
