"""code2's vocabulary head scoring given targets (flowgnn.h: flowgnn_set_vocab_targets): what the target's
logit, the rank and the log-sum-exp cost beside the argmax.    usage: vocab_score_ab.py [OUT.json]   (default: profiles/vocab_score_ab.json)
P = 5 positions, V = 5002 entries, synthetic batches of 4 096 and 2^16 graphs, one process and one engine, the profile slots of
flowgnn_profile_read, three warm runs and then ten measured, per launch: vocab_head + vocab_head_fold without targets, then
vocab_target + vocab_score + vocab_score_fold with seeded random targets on the same batch, and the pair once more (the two
variants alternate: head, score, head, score); ratio = the score sums' mean over the head sums' mean, and each variant's spread
between its two rounds is recorded beside it.  The head reads the pooled rows only, so the graphs are small (vocab_head_ab.py's paths of 1 .. 5 nodes)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

P, V, D, RUNS = 5, 5002, 300, 10
rng = np.random.default_rng(1)
hw = (rng.uniform(-1, 1, (P, V, D)) / np.sqrt(D)).astype(np.float32)
hb = (rng.uniform(-1, 1, (P, V)) / np.sqrt(D)).astype(np.float32)


def batch_of(G):
    n = 1 + np.arange(G) % 5
    el = np.concatenate([np.stack([np.arange(k - 1), np.arange(1, k)], 1) for k in n if k > 1]).astype(np.int32)
    e = (n - 1).astype(np.int32)
    return gp.GraphBatch(n.astype(np.int32), e, np.zeros((int(n.sum()), 9), np.int32), el, np.zeros((len(el), 3), np.int32))


def per_launch(e, slots):
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
    return out


e = Engine("GIN", device=0)
e.set_emb_dim(300)
e.set_weights(weights.synth_gin_weights(seed=7, emb_dim=300))
e.set_vocab_head(hw, hb)
e.profile_enable(True)
res = {"positions": P, "vocab": V}
for G in (4096, 1 << 16):
    e.set_batch(batch_of(G))
    t = rng.integers(-1, V, (G, P)).astype(np.int32)
    rounds = []
    for _ in range(2):
        e.set_vocab_targets(None)
        head = per_launch(e, ["vocab_head", "vocab_head_fold"])
        e.set_vocab_targets(t)
        rounds.append((head, per_launch(e, ["vocab_target", "vocab_score", "vocab_score_fold"])))
    hs, ss = [sum(h.values()) for h, _ in rounds], [sum(s.values()) for _, s in rounds]
    r = {"head": [h for h, _ in rounds], "score": [s for _, s in rounds], "head_ms": hs, "score_ms": ss, "exact_reruns": e.exact_reruns()}
    r["head_spread"], r["score_spread"] = abs(hs[0] - hs[1]) / min(hs), abs(ss[0] - ss[1]) / min(ss)
    r["ratio"] = sum(ss) / sum(hs)
    res[f"graphs_{G}"] = r
    print(json.dumps({G: r}), flush=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vocab_score_ab.json")
json.dump(res, open(out, "w"), indent=1)
