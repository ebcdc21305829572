"""The vocabulary head's top-k form (flowgnn.h: flowgnn_set_vocab_topk) against its argmax form, per launch.
usage: vocab_topk_ab.py [OUT.json]      (default: profiles/vocab_topk_ab.json)
scripts/dev/vocab_head_ab.py's protocol and inputs: P = 5, V = 5002, its batches of 4 096 and 2^16 graphs, one process and one engine
per batch, the profile slots of flowgnn_profile_read, three warm runs and then ten measured.  Per batch k = 0, 1, 8 and k = 0 once
more (the spread of the yardstick itself): vocab_head (+ vocab_head_fold) against vocab_topk (+ vocab_topk_fold).  Then, at 4 096
graphs and k = 8, the worst case for the lists: a bias that rises with the index by four times the largest |W pooled|, under which
every candidate of every lane is inserted."""
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
w = weights.synth_gin_weights(seed=7, emb_dim=300)


def batch_of(G):
    n = 1 + np.arange(G) % 5
    el = np.concatenate([np.stack([np.arange(k - 1), np.arange(1, k)], 1) for k in n if k > 1]).astype(np.int32)
    return gp.GraphBatch(n.astype(np.int32), (n - 1).astype(np.int32), np.zeros((int(n.sum()), 9), np.int32), el, np.zeros((len(el), 3), np.int32))


def per_launch(e, batch, slots):
    e.set_batch(batch)
    for _ in range(3):
        e.run(); e.sync()
    a = e.profile_read()
    for _ in range(RUNS):
        e.run(); e.sync()
    b = e.profile_read()
    none = {"launches": 0, "total_ms": 0.0}
    return {s: (b[s]["total_ms"] - a.get(s, none)["total_ms"]) / (b[s]["launches"] - a.get(s, none)["launches"])
            for s in slots if s in b and b[s]["launches"] > a.get(s, none)["launches"]}


def engine(w):
    e = Engine("GIN", device=0)
    e.set_emb_dim(300)
    e.set_weights(w)
    e.set_vocab_head(hw, hb)
    e.profile_enable(True)
    return e


SLOTS = ["vocab_head", "vocab_head_fold", "vocab_topk", "vocab_topk_fold"]
res = {"positions": P, "vocab": V}
for G in (4096, 1 << 16):
    e, batch = engine(w), batch_of(G)
    for name, k in (("k0", 0), ("k1", 1), ("k8", 8), ("k0_again", 0)):
        e.set_vocab_topk(k)
        r = per_launch(e, batch, SLOTS)
        r["total"] = sum(v for s, v in r.items() if s in SLOTS)
        res[f"{name}_{G}"] = r
        print(json.dumps({f"{name}_{G}": r}), flush=True)
    for name in ("k1", "k8"):
        res[f"{name}_{G}"]["ratio_to_k0"] = res[f"{name}_{G}"]["total"] / res[f"k0_{G}"]["total"]
    if G == 4096:
        pooled = e.forward(batch_of(5), return_embeddings=True)[1]  # the batch repeats these five graphs
        step = 4 * np.abs(np.einsum("pvd,gd->gpv", hw.astype(np.float64), pooled.astype(np.float64))).max()
        e.set_vocab_head(hw, np.tile((step * np.arange(V)).astype(np.float32), (P, 1)))
        e.set_vocab_topk(8)
        r = per_launch(e, batch, SLOTS)
        assert (e.topk()[0] == np.arange(V - 1, V - 9, -1)).all()
        r["total"] = sum(v for s, v in r.items() if s in SLOTS)
        r["ratio_to_k0"] = r["total"] / res["k0_4096"]["total"]
        res["k8_rising_bias_4096"] = r
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vocab_topk_ab.json")
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
