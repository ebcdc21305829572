"""OGB's gcn-virtual at width 300 (flowgnn.h: flowgnn_set_gcn_virtual_node_dim): what the virtual node adds to one step.
usage: gcn_wide_vn_ab.py OUT.json [--graphs N]
One batch of N = 2^16 molpcba-shaped graphs (the batch of scripts/dev/gcn_wide_ab.py), one width-300 engine measured twice:
  (a) the virtual node off -- the step of the commit before the call existed;
  (b) the virtual node on (gcn_wide.hip: b_0' in the encoder, gcn_wide_vn_t0, the add and the partial rows inside the layer launches,
      gcn_wide_vn_t, gcn_wide_vn_update).
A step's time is the device-event total of its kernels (profile_read) -- best of three medians of ten runs after two warm-up runs, as
scripts/dev/gin_wide_vn_ab.py does --, with the per-slot split of both.  The tensors are weights.synth_gcn_virtual_node(seed=13,
emb_dim=300) with the first linear layer scaled by 1 / 64, which keeps t and the update's hidden layer inside the split-f16 range on
this batch (exact_reruns is reported and must be 0: a re-run would time the fp32 form)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

ROUNDS, RUNS = 3, 10


def measure(e):
    read = lambda: {k: v["total_ms"] for k, v in e.profile_read().items()}

    def step():
        k0 = read()
        e.run()
        e.sync()
        k1 = read()
        return {k: k1[k] - k0.get(k, 0.0) for k in k1 if k1[k] - k0.get(k, 0.0) > 0.0}
    before = e.exact_reruns()
    for _ in range(2):
        step()
    rounds = [[step() for _ in range(RUNS)] for _ in range(ROUNDS)]
    med = lambda key: [float(np.median([key(s) for s in r])) for r in rounds]
    total = med(lambda s: sum(s.values()))
    slots = sorted({k for r in rounds for s in r for k in s})
    best = int(np.argmin(total))
    return {"step_ms": min(total), "step_medians_ms": total, "exact_reruns": e.exact_reruns() - before,
            "slots_ms": {k: med(lambda s, k=k: s.get(k, 0.0))[best] for k in slots}}


def main():
    out_path = sys.argv[1]
    graphs = int(sys.argv[sys.argv.index("--graphs") + 1]) if "--graphs" in sys.argv else 1 << 16
    b = gp.synth_molpcba_batch(graphs, seed=1234)
    vn = weights.synth_gcn_virtual_node(seed=13, emb_dim=300)
    vn["w1"] = vn["w1"] * np.float32(1.0 / 64)
    e = Engine("GCN", 0)
    e.set_model_emb_dim(300)
    e.set_weights(weights.synth_gcn_weights(seed=7, emb_dim=300))
    e.set_batch(b)
    e.profile_enable(True)
    res = {"graphs": graphs, "nodes": b.total_nodes, "edges": b.total_edges, "rounds": ROUNDS, "runs": RUNS}
    res["a_virtual_node_off"] = measure(e)
    e.set_gcn_virtual_node(vn)
    res["b_virtual_node_on"] = measure(e)
    e.close()
    a, bb = res["a_virtual_node_off"], res["b_virtual_node_on"]
    res["b_minus_a_ms"] = bb["step_ms"] - a["step_ms"]
    res["b_over_a"] = bb["step_ms"] / a["step_ms"]
    res["slot_difference_ms"] = {k: bb["slots_ms"].get(k, 0.0) - a["slots_ms"].get(k, 0.0) for k in sorted(set(a["slots_ms"]) | set(bb["slots_ms"]))}
    res["t0_over_atom_encoder"] = bb["slots_ms"].get("gcn_wide_vn_t0", 0.0) / bb["slots_ms"]["atom_encoder"]
    # three launches store (graphs + ceil(nodes / 16)) partial rows of 1 200 bytes each
    res["partial_row_bytes_per_step"] = 3 * (graphs + (b.total_nodes + 15) // 16) * 300 * 4
    for k in ("a_virtual_node_off", "b_virtual_node_on"):
        print(f"{k}: {res[k]['step_ms']:.3f} ms (medians {['%.3f' % m for m in res[k]['step_medians_ms']]}), re-runs {res[k]['exact_reruns']}: {res[k]['slots_ms']}", flush=True)
    print(f"(b) - (a) = {res['b_minus_a_ms']:.3f} ms, (b) / (a) = {res['b_over_a']:.3f}; per slot: {res['slot_difference_ms']}; "
          f"t_0 / atom_encoder = {res['t0_over_atom_encoder']:.2f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
