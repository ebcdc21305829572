"""GCN's f16 product beside OGB's linear edge encoder against the default mode of the same stage (flowgnn.h:
flowgnn_set_model_edge_linear_numeric).    usage: gcn_wide_el_f16_ab.py      (writes profiles/gcn_wide_el_f16_ab.json)
The batch of gcn_wide_el_ab.py: one synthetic ppa-shaped batch (256 graphs of 243 nodes and 2 270 random edges, seven float features
per edge).  One process, ONE engine, the two modes alternating round by round through the call; three warm rounds, then three
repeats of ten measured rounds.  A round is four runs of a mode; its figures are the profile slots' device-event times.  A pass has
four layer launches and the final stage, which has no product and keeps gcn_wide_layer_el in both modes: in the default mode the slot
holds all five, in the f16 mode the four layer launches are gcn_wide_layer_el_f16's and the slot holds the final stage alone.  So a
default round's layer launch is (the slot's time - the final stage's, taken from the f16 round beside it) / 16; the slot's raw
per-launch average over all twenty is recorded too.  Per repeat the median of the ten rounds; the spread of a mode is the distance
between its largest and its smallest median.  The same again on the same nodes with no edges: what is left is not the walk.
exact_reruns must stay 0."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

G, NODES, EDGES, F, WARM, ROUNDS, REPEATS, RUNS, LAYER_LAUNCHES = 256, 243, 2270, 7, 3, 10, 3, 4, 4
EL, EL16 = "gcn_wide_layer_el", "gcn_wide_layer_el_f16"
rng = np.random.default_rng(1)


def one(edges):
    el = rng.integers(0, NODES, (edges, 2)).astype(np.int32)
    return gp.GraphBatch(np.array([NODES], np.int32), np.array([edges], np.int32), np.zeros((NODES, 9), np.int32), el, np.zeros((edges, 3), np.int32))


ppa = gp.concat_batches([one(EDGES) for _ in range(G)])
bare = gp.concat_batches([one(0) for _ in range(G)])
w = weights.synth_gcn_weights(seed=7, emb_dim=300)
el = {"w": (0.05 * rng.uniform(-1, 1, (5, 300, F))).astype(np.float32), "b": (0.05 * rng.uniform(-1, 1, (5, 300))).astype(np.float32)}
ef = rng.standard_normal((ppa.total_edges, F)).astype(np.float32)


def round_of(e, mode):
    """four runs in `mode` -> {slot: (ms, launches)} gained by the two slots"""
    e.set_model_edge_linear_numeric(mode)
    zero = {"total_ms": 0.0, "launches": 0}
    a = e.profile_read()
    for _ in range(RUNS):
        e.run()
    e.sync()
    b = e.profile_read()
    return {s: (b.get(s, zero)["total_ms"] - a.get(s, zero)["total_ms"], b.get(s, zero)["launches"] - a.get(s, zero)["launches"]) for s in (EL, EL16)}


def ab(batch, feats):
    e = Engine("GCN", device=0)
    e.set_model_emb_dim(300)
    e.set_weights(w)
    e.set_model_edge_linear(el["w"], el["b"])
    e.profile_enable(True)
    e.set_batch(batch)
    e.set_edge_features(feats)
    for _ in range(WARM):
        for mode in ("f32", "f16"):
            round_of(e, mode)
    keys = ("f32", "f16", "f32_slot_raw", "final")
    medians = {k: [] for k in keys}
    for _ in range(REPEATS):
        samples = {k: [] for k in keys}
        for _ in range(ROUNDS):
            r32, r16 = round_of(e, "f32"), round_of(e, "f16")  # alternating: f32, f16, f32, ...
            assert r32[EL][1] == RUNS * (LAYER_LAUNCHES + 1) and r32[EL16][1] == 0 and r16[EL16][1] == RUNS * LAYER_LAUNCHES and r16[EL][1] == RUNS, (r32, r16)
            samples["f32"].append((r32[EL][0] - r16[EL][0]) / (RUNS * LAYER_LAUNCHES))
            samples["f16"].append(r16[EL16][0] / r16[EL16][1])
            samples["f32_slot_raw"].append(r32[EL][0] / r32[EL][1])
            samples["final"].append(r16[EL][0] / r16[EL][1])
        for k in keys:
            medians[k].append(float(np.median(samples[k])))
    out = {k: {"ms_per_launch": min(m), "medians": m, "spread": max(m) - min(m)} for k, m in medians.items()}
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
json.dump(res, open(os.path.join(ROOT, "profiles", "gcn_wide_el_f16_ab.json"), "w"), indent=1)
print(json.dumps(res, indent=1))
