"""OGB's virtual node for GCN (flowgnn.h: flowgnn_set_gcn_virtual_node): what one step costs beside the paths it is built on.
usage: gcn_vn_ab.py OUT.json [--graphs N]
One batch of N = 2^16 molpcba-shaped graphs, five engines:
  (a)  the per-layer path (gcn_resident 0), virtual node off;
  (b)  the same kernels with the virtual node on, in the fused form (the path every batch takes then, by default);
  (c)  the virtual node on with gcn_unfused 1 (the in-place form), beside (c0), gcn_unfused 1 with it off;
  (d)  the default graph-resident path, off, for context.
A step's time is the device-event total of its kernels (profile_read) -- best of three medians of ten runs after two warm-up runs, as
scripts/dev/ogb_vn_ab.py does -- and for (b) the gcn_ogb_vn slot's own time per step (four launches), the map's, and (b - a) / a."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

ROUNDS, RUNS = 3, 10


def measure(b, options, vn):
    e = Engine("GCN", 0, options=options)
    e.set_weights(weights.synth_gcn_weights(seed=7))
    if vn is not None:
        e.set_gcn_virtual_node(vn)
    e.set_batch(b)
    e.profile_enable(True)
    read = lambda: {k: v["total_ms"] for k, v in e.profile_read().items()}

    def step():
        k0 = read()
        e.run()
        e.sync()
        k1 = read()
        return {k: k1[k] - k0.get(k, 0.0) for k in k1}
    for _ in range(2):
        step()
    rounds = [[step() for _ in range(RUNS)] for _ in range(ROUNDS)]
    reruns = e.exact_reruns()
    e.close()
    med = lambda key: [float(np.median([key(s) for s in r])) for r in rounds]
    total = med(lambda s: sum(s.values()))
    slots = sorted({k for r in rounds for s in r for k in s})
    best = int(np.argmin(total))
    return {"step_ms": min(total), "step_medians_ms": total, "exact_reruns": reruns,
            "slots_ms": {k: med(lambda s, k=k: s.get(k, 0.0))[best] for k in slots}}


def main():
    out_path = sys.argv[1]
    graphs = int(sys.argv[sys.argv.index("--graphs") + 1]) if "--graphs" in sys.argv else 1 << 16
    b = gp.synth_molpcba_batch(graphs, seed=1234)
    vn = weights.synth_gcn_virtual_node(seed=13, scale=0.05)  # (small: the run stays on the split-f16 kernels, as a trained model's does)
    configs = [("a_per_layer", {"gcn_resident": 0}, None), ("b_fused_with_virtual_node", {}, vn),
               ("c_in_place_with_virtual_node", {"gcn_unfused": 1}, vn), ("c0_unfused", {"gcn_unfused": 1}, None), ("d_resident", {}, None)]
    res = {"graphs": graphs, "nodes": b.total_nodes, "edges": b.total_edges, "rounds": ROUNDS, "runs": RUNS}
    for k, options, v in configs:
        res[k] = measure(b, options, v)
        print(f"{k}: {res[k]['step_ms']:.3f} ms (medians {['%.3f' % m for m in res[k]['step_medians_ms']]}), re-runs {res[k]['exact_reruns']}: {res[k]['slots_ms']}", flush=True)
    a, bb, c, c0, d = (res[k] for k, _, _ in configs)
    res["gcn_ogb_vn_ms_per_step"] = bb["slots_ms"].get("gcn_ogb_vn", 0.0)
    res["gcn_ogb_vn_map_ms_per_step"] = bb["slots_ms"].get("gcn_ogb_vn_map", 0.0)
    res["fused_layers_b_minus_a_ms"] = bb["slots_ms"].get("gcn_layer_fused", 0.0) - a["slots_ms"].get("gcn_layer_fused", 0.0)
    res["b_minus_a_over_a"] = (bb["step_ms"] - a["step_ms"]) / a["step_ms"]
    res["c_minus_c0_over_c0"] = (c["step_ms"] - c0["step_ms"]) / c0["step_ms"]
    res["d_minus_b_ms"] = d["step_ms"] - bb["step_ms"]
    print(f"gcn_ogb_vn: {res['gcn_ogb_vn_ms_per_step']:.3f} ms per step, map {res['gcn_ogb_vn_map_ms_per_step']:.3f}, fused layers "
          f"{res['fused_layers_b_minus_a_ms']:+.3f}; (b - a) / a = {res['b_minus_a_over_a']:.3f}; (c - c0) / c0 = {res['c_minus_c0_over_c0']:.3f}; "
          f"d - b = {res['d_minus_b_ms']:.3f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
