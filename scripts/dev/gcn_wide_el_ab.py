"""OGB's linear edge encoder for GCN at width 300 (flowgnn.h: flowgnn_set_model_edge_linear): what the encoder
costs per stage launch.    usage: gcn_wide_el_ab.py      (writes profiles/gcn_wide_el_ab.json)
The batch and the method of gin_wide_el_ab.py: one synthetic ppa-shaped batch (G graphs of 243 nodes and 2 270 random edges, seven
float features per edge), one process, the profile slots of flowgnn_profile_read, three warm runs and then ten measured.  Per slot
the time per launch and per pass (a pass has five launches of a stage slot: four layers and the final stage, which has no product):
gcn_wide_layer_el; gcn_wide_layer on the same graphs with integer bond codes (the table path); both on the same nodes with no edges
(what is left is not the walk); and the exact path, gcn_wide_aggregate_el plus gcn_wide_layer_f32 (its dense launch), forced by one
feature of 1e5.  exact_reruns is reported and must be 0 in the fast rows."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

G, NODES, EDGES, F, RUNS = 256, 243, 2270, 7, 10
rng = np.random.default_rng(1)


def one(i, edges):
    el = rng.integers(0, NODES, (edges, 2)).astype(np.int32)
    ea = np.stack([rng.integers(0, 5, edges), rng.integers(0, 6, edges), rng.integers(0, 2, edges)], 1).astype(np.int32).reshape(edges, 3)
    return gp.GraphBatch(np.array([NODES], np.int32), np.array([edges], np.int32), np.zeros((NODES, 9), np.int32), el, ea)


ppa = gp.concat_batches([one(i, EDGES) for i in range(G)])
bare = gp.concat_batches([one(i, 0) for i in range(G)])
w = weights.synth_gcn_weights(seed=7, emb_dim=300)
el = {"w": (0.05 * rng.uniform(-1, 1, (5, 300, F))).astype(np.float32), "b": (0.05 * rng.uniform(-1, 1, (5, 300))).astype(np.float32)}
ef = rng.standard_normal((ppa.total_edges, F)).astype(np.float32)


def engine(on):
    e = Engine("GCN", device=0)
    e.set_model_emb_dim(300)
    e.set_weights(w)
    if on:
        e.set_model_edge_linear(el["w"], el["b"])
    e.profile_enable(True)
    return e


def measure(e, batch, feats, slots):
    e.set_batch(batch)
    if feats is not None:
        e.set_edge_features(feats)
    for _ in range(3):
        e.run(); e.sync()
    a = e.profile_read()
    for _ in range(RUNS):
        e.run(); e.sync()
    b = e.profile_read()
    out = {}
    for s in slots:
        n = b.get(s, {"launches": 0})["launches"] - a.get(s, {"launches": 0})["launches"]
        if n > 0:
            ms = b[s]["total_ms"] - a.get(s, {"total_ms": 0.0})["total_ms"]
            out[s] = {"per_launch_ms": ms / n, "per_pass_ms": ms / RUNS}
    out["exact_reruns"] = e.exact_reruns()
    return out


res = {"graphs": G, "nodes": ppa.total_nodes, "edges": ppa.total_edges, "edge_dim": F}
print(json.dumps(res), flush=True)
res["el"] = measure(engine(True), ppa, ef, ["gcn_wide_layer_el", "gcn_wide_aggregate_el"])
print(json.dumps(res["el"]), flush=True)
res["table"] = measure(engine(False), ppa, None, ["gcn_wide_layer"])
print(json.dumps(res["table"]), flush=True)
res["el_no_edges"] = measure(engine(True), bare, np.zeros((0, F), np.float32), ["gcn_wide_layer_el"])
res["table_no_edges"] = measure(engine(False), bare, None, ["gcn_wide_layer"])
big = ef.copy()
big[0, 0] = 1.0e5  # the exact path: the fp32 VALU form of the encoder and the fp32 dense launch
res["el_exact"] = measure(engine(True), ppa, big, ["gcn_wide_aggregate_el", "gcn_wide_layer_f32"])
json.dump(res, open(os.path.join(ROOT, "profiles", "gcn_wide_el_ab.json"), "w"), indent=1)
print(json.dumps(res, indent=1))
