"""code2's vocabulary head for GIN at width 300 (flowgnn.h: flowgnn_set_vocab_head): what the head costs per
launch.    usage: vocab_head_ab.py [OUT.json]      (default: profiles/vocab_head_ab.json)
P = 5 positions, V = 5002 entries, synthetic batches of 4 096 and 2^16 graphs, one process, the profile slots of
flowgnn_profile_read, three warm runs and then ten measured, per launch: vocab_head and vocab_head_fold; vocab_head_f32, the exact
form, forced by one pooled value of 1e5 (4 096 graphs only); and, on the same 4 096 graphs, the only route to the same logits
without the head: flowgnn_set_num_tasks(25010) and its pooled_head slot, which writes [G][25010] floats and leaves the argmax to the
caller.  At 2^16 graphs that result buffer alone would be 6.5 GB, so that row has no counterpart.  The head reads the pooled rows
only, so the graphs are small (paths of 1 .. 5 nodes): a code2-sized graph would change the layers' time, not the head's."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

P, V, D, RUNS = 5, 5002, 300, 10
PEAK_F16_TFLOPS = 2516.0  # MI355X, dense f16 matrix pipe (profiles/limits.json's source)
rng = np.random.default_rng(1)
hw = (rng.uniform(-1, 1, (P, V, D)) / np.sqrt(D)).astype(np.float32)
hb = (rng.uniform(-1, 1, (P, V)) / np.sqrt(D)).astype(np.float32)


def batch_of(G):
    n = 1 + np.arange(G) % 5
    el = np.concatenate([np.stack([np.arange(k - 1), np.arange(1, k)], 1) for k in n if k > 1]).astype(np.int32)
    e = (n - 1).astype(np.int32)
    return gp.GraphBatch(n.astype(np.int32), e, np.zeros((int(n.sum()), 9), np.int32), el, np.zeros((len(el), 3), np.int32))


def per_launch(e, batch, slots):
    e.set_batch(batch)
    for _ in range(3):
        e.run(); e.sync()
    a = e.profile_read()
    for _ in range(RUNS):
        e.run(); e.sync()
    b = e.profile_read()
    out = {}
    for s in slots:
        if s in b and b[s]["launches"] > a.get(s, {"launches": 0})["launches"]:
            out[s] = (b[s]["total_ms"] - a.get(s, {"total_ms": 0.0})["total_ms"]) / (b[s]["launches"] - a.get(s, {"launches": 0})["launches"])
    out["exact_reruns"] = e.exact_reruns()
    return out


def engine(w, head=True, tasks=1):
    e = Engine("GIN", device=0)
    e.set_emb_dim(300)
    e.set_num_tasks(tasks)
    e.set_weights(w)
    if head:
        e.set_vocab_head(hw, hb)
    e.profile_enable(True)
    return e


w = weights.synth_gin_weights(seed=7, emb_dim=300)
res = {"positions": P, "vocab": V}
for G in (4096, 1 << 16):
    r = per_launch(engine(w), batch_of(G), ["vocab_head", "vocab_head_fold", "pooled_head"])
    flops = 3 * 2.0 * G * P * (16 * ((V + 15) // 16)) * 320  # executed: three MFMAs per product, K padded to 320, V to whole tiles
    r["executed_tflop"] = flops / 1e12
    r["f16_pipe_fraction"] = flops / (r["vocab_head"] * 1e-3) / (PEAK_F16_TFLOPS * 1e12)
    res[f"head_{G}"] = r
    print(json.dumps({G: r}), flush=True)
big = dict(w)
b2 = np.array(big["node_mlp_2_bias"])
b2[-1, 7] = 1.0e5  # one pooled column beyond 6e4: the exact form
big["node_mlp_2_bias"] = b2
res["head_exact_4096"] = per_launch(engine(big), batch_of(4096), ["vocab_head_f32"])
wide = weights.synth_gin_weights(seed=7, emb_dim=300, num_tasks=P * V)
res["num_tasks_25010_4096"] = per_launch(engine(wide, head=False, tasks=P * V), batch_of(4096), ["pooled_head"])
res["num_tasks_25010_4096"]["result_bytes"] = 4096 * P * V * 4
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vocab_head_ab.json")
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
