"""The f16 node MLP beside OGB's linear edge encoder against the default mode of the same layer (flowgnn.h:
flowgnn_set_edge_linear_numeric).    usage: gin_wide_el_f16_ab.py      (writes profiles/gin_wide_el_f16_ab.json)
The batch of gin_wide_el_ab.py: one synthetic ppa-shaped batch (256 graphs of 243 nodes and 2 270 random edges, seven float features
per edge).  One process, ONE engine, the two modes alternating round by round through the call; three warm rounds, then three
repeats of ten measured rounds.  A round is four runs of a mode (20 layer launches); its figure is the profile slot's device-event
time per launch (gin_wide_layer_el / gin_wide_layer_el_f16).  Per repeat the median of the ten rounds; the spread of a mode is the
distance between its largest and its smallest median.  The same again on the same nodes with no edges: what is left is not the
walk.  exact_reruns must stay 0.  The node MLP's second matrix is scaled down as in gin_wide_el_ab.py (in-degree 9)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

G, NODES, EDGES, F, WARM, ROUNDS, REPEATS, RUNS = 256, 243, 2270, 7, 3, 10, 3, 4
SLOT = {"f32": "gin_wide_layer_el", "f16": "gin_wide_layer_el_f16"}
rng = np.random.default_rng(1)


def one(edges):
    el = rng.integers(0, NODES, (edges, 2)).astype(np.int32)
    return gp.GraphBatch(np.array([NODES], np.int32), np.array([edges], np.int32), np.zeros((NODES, 9), np.int32), el, np.zeros((edges, 3), np.int32))


ppa = gp.concat_batches([one(EDGES) for _ in range(G)])
bare = gp.concat_batches([one(0) for _ in range(G)])
w = weights.synth_gin_weights(seed=7, emb_dim=300)
for k in ("node_mlp_2_weights", "node_mlp_2_bias"):
    w[k] = w[k] * np.float32(0.05)  # in-degree 9: keep the activations inside the f16 range
el = {"w": (0.05 * rng.uniform(-1, 1, (5, 300, F))).astype(np.float32), "b": (0.05 * rng.uniform(-1, 1, (5, 300))).astype(np.float32)}
ef = rng.standard_normal((ppa.total_edges, F)).astype(np.float32)


def round_of(e, mode):
    """four runs in `mode` -> ms per launch of the mode's slot"""
    e.set_edge_linear_numeric(mode)
    a = e.profile_read().get(SLOT[mode], {"total_ms": 0.0, "launches": 0})
    for _ in range(RUNS):
        e.run()
    e.sync()
    b = e.profile_read()[SLOT[mode]]
    return (b["total_ms"] - a["total_ms"]) / (b["launches"] - a["launches"])


def ab(batch, feats):
    e = Engine("GIN", device=0)
    e.set_emb_dim(300)
    e.set_weights(w)
    e.set_edge_linear(el["w"], el["b"])
    e.profile_enable(True)
    e.set_batch(batch)
    e.set_edge_features(feats)
    for _ in range(WARM):
        for mode in SLOT:
            round_of(e, mode)
    medians = {mode: [] for mode in SLOT}
    for _ in range(REPEATS):
        samples = {mode: [] for mode in SLOT}
        for _ in range(ROUNDS):
            for mode in SLOT:  # alternating: f32, f16, f32, ...
                samples[mode].append(round_of(e, mode))
        for mode in SLOT:
            medians[mode].append(float(np.median(samples[mode])))
    out = {mode: {"ms_per_launch": min(m), "medians": m, "spread": max(m) - min(m)} for mode, m in medians.items()}
    out["f16_over_f32"] = out["f16"]["ms_per_launch"] / out["f32"]["ms_per_launch"]
    out["gain_ms"] = out["f32"]["ms_per_launch"] - out["f16"]["ms_per_launch"]
    out["rule_2"] = bool(out["gain_ms"] > 2.0 * out["f32"]["spread"])  # faster by more than twice the default mode's spread
    out["exact_reruns"] = e.exact_reruns()
    e.close()
    return out


res = {"graphs": G, "nodes": ppa.total_nodes, "edges": ppa.total_edges, "edge_dim": F, "runs_per_round": RUNS, "rounds": ROUNDS, "repeats": REPEATS}
res["ppa"] = ab(ppa, ef)
print(json.dumps(res["ppa"]), flush=True)
res["no_edges"] = ab(bare, np.zeros((0, F), np.float32))
json.dump(res, open(os.path.join(ROOT, "profiles", "gin_wide_el_f16_ab.json"), "w"), indent=1)
print(json.dumps(res, indent=1))
