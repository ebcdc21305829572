"""OGB's virtual node for GIN (flowgnn.h: flowgnn_set_ogb_virtual_node): what one step costs beside the paths it is built on.
usage: ogb_vn_ab.py OUT.json [--graphs N]
One batch of N = 2^16 molhiv-shaped graphs, three engines:
  (a) the per-layer path (gin_resident 0), virtual node off;
  (b) the same with the virtual node on (the path every batch takes then);
  (c) the default graph-resident path, for context.
A step's time is the device-event total of its kernels (profile_read) -- best of three medians of ten runs after two warm-up runs, as
scripts/dev/eigen_ab.py does -- and for (b) the gin_ogb_vn slot's own time per step (five launches) and its share of the step."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

ROUNDS, RUNS = 3, 10


def measure(b, options, vn):
    e = Engine("GIN", 0, options=options)
    e.set_weights(weights.synth_gin_weights(seed=7))
    if vn is not None:
        e.set_ogb_virtual_node(vn)
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
    b = gp.synth_molhiv_batch(graphs, seed=1234)
    vn = weights.synth_gin_virtual_node(seed=11, scale=0.05)  # (small: the run stays on the split-f16 kernels, as a trained model's does)
    res = {"graphs": graphs, "nodes": b.total_nodes, "edges": b.total_edges, "rounds": ROUNDS, "runs": RUNS,
           "a_per_layer": measure(b, {"gin_resident": 0}, None),
           "b_per_layer_with_virtual_node": measure(b, {}, vn),
           "c_resident": measure(b, {}, None)}
    a, bb = res["a_per_layer"], res["b_per_layer_with_virtual_node"]
    slot = bb["slots_ms"].get("gin_ogb_vn", 0.0)
    res["gin_ogb_vn_ms_per_step"] = slot
    res["gin_ogb_vn_share_of_step"] = slot / bb["step_ms"]
    res["b_minus_a_over_a"] = (bb["step_ms"] - a["step_ms"]) / a["step_ms"]
    for k in ("a_per_layer", "b_per_layer_with_virtual_node", "c_resident"):
        print(f"{k}: {res[k]['step_ms']:.3f} ms (medians {['%.3f' % m for m in res[k]['step_medians_ms']]}), re-runs {res[k]['exact_reruns']}: {res[k]['slots_ms']}", flush=True)
    print(f"gin_ogb_vn: {slot:.3f} ms per step, {100 * res['gin_ogb_vn_share_of_step']:.1f} % of (b); (b - a) / a = {res['b_minus_a_over_a']:.3f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
