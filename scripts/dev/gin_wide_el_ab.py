"""OGB's linear edge encoder for GIN at width 300 (flowgnn.h: flowgnn_set_edge_linear): what the encoder costs
per layer launch.    usage: gin_wide_el_ab.py      (writes profiles/gin_wide_el_ab.json)
One synthetic ppa-shaped batch (G graphs of 243 nodes and 2 270 random edges, seven float features per edge), one process, the
profile slots of flowgnn_profile_read, three warm runs and then ten measured, per launch: gin_wide_layer_el; gin_wide_layer on the
same graphs with integer bond codes (the table path); both on the same nodes with no edges (what is left is not the walk);
gin_wide_aggregate_el, the exact path's fp32 VALU form of the encoder, forced by one feature of 1e5; and gin_wide_layer on 4 096
molhiv-shaped graphs with the encoder off.  The node MLP's second matrix and the tables are scaled down so that the activations of
in-degree 9 stay inside the split kernels' range: exact_reruns is reported and must be 0 in the fast rows."""
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
w = weights.synth_gin_weights(seed=7, emb_dim=300)
for k in ("node_mlp_2_weights", "node_mlp_2_bias", "edge_embedding_weight"):
    w[k] = w[k] * np.float32(0.05)  # in-degree 9: keep the activations inside the split kernels' range
el = {"w": (0.05 * rng.uniform(-1, 1, (5, 300, F))).astype(np.float32), "b": (0.05 * rng.uniform(-1, 1, (5, 300))).astype(np.float32)}
ef = rng.standard_normal((ppa.total_edges, F)).astype(np.float32)


def engine(on):
    e = Engine("GIN", device=0)
    e.set_emb_dim(300)
    e.set_weights(w)
    if on:
        e.set_edge_linear(el["w"], el["b"])
    e.profile_enable(True)
    return e


def per_launch(e, batch, feats, slots):
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
        if s in b and b[s]["launches"] > a.get(s, {"launches": 0})["launches"]:
            out[s] = (b[s]["total_ms"] - a.get(s, {"total_ms": 0.0})["total_ms"]) / (b[s]["launches"] - a.get(s, {"launches": 0})["launches"])
    out["exact_reruns"] = e.exact_reruns()
    return out


res = {"graphs": G, "nodes": ppa.total_nodes, "edges": ppa.total_edges, "edge_dim": F}
print(json.dumps(res), flush=True)
res["el"] = per_launch(engine(True), ppa, ef, ["gin_wide_layer_el", "gin_wide_aggregate_el"])
print(json.dumps(res["el"]), flush=True)
res["table"] = per_launch(engine(False), ppa, None, ["gin_wide_layer"])
print(json.dumps(res["table"]), flush=True)
res["el_no_edges"] = per_launch(engine(True), bare, np.zeros((0, F), np.float32), ["gin_wide_layer_el"])
res["table_no_edges"] = per_launch(engine(False), bare, None, ["gin_wide_layer"])
big = ef.copy()
big[0, 0] = 1.0e5  # the exact path: the fp32 VALU form of the encoder
res["el_exact"] = per_launch(engine(True), ppa, big, ["gin_wide_aggregate_el", "gin_wide_layer_f32"])
mol = gp.synth_molhiv_batch(4096, seed=1)
res["molhiv_4096_off"] = per_launch(engine(False), mol, None, ["gin_wide_layer"])
res["molhiv_nodes"] = mol.total_nodes
json.dump(res, open(os.path.join(ROOT, "profiles", "gin_wide_el_ab.json"), "w"), indent=1)
print(json.dumps(res, indent=1))
