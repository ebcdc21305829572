"""OGB's attention readout at width 300 (flowgnn.h: flowgnn_set_attention_pooling): what it adds to one step.
usage: attn_pool_ab.py [OUT.json] [--graphs N]      (default OUT: profiles/attn_pool_ab.json)
One batch of N = 2^16 molhiv-shaped graphs, one width-300 GIN engine measured twice:
  (a) the mean readout (mean_pool_rows + pooled_head);
  (b) the attention readout (wide_attn.hip: attn_gate + attn_pool_rows in place of mean_pool_rows).
A step's time is the device-event total of its kernels (profile_read) -- best of three medians of ten runs after two warm-up runs, as
scripts/dev/gcn_wide_vn_ab.py does --, with the per-slot split of both.  The gate is weights.synth_attention_pooling(seed=11);
exact_reruns is reported and must be 0: a re-run would time the fp32 form."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

ROUNDS, RUNS = 3, 10


def measure(e):
    read = lambda: {k: (v["total_ms"], v["launches"]) for k, v in e.profile_read().items()}

    def step():
        k0 = read()
        e.run()
        e.sync()
        k1 = read()
        return {k: k1[k][0] - k0.get(k, (0.0, 0))[0] for k in k1 if k1[k][1] - k0.get(k, (0.0, 0))[1] > 0}
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
    args = [a for a in sys.argv[1:]]
    graphs = 1 << 16
    if "--graphs" in args:
        i = args.index("--graphs")
        graphs = int(args[i + 1])
        del args[i:i + 2]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "attn_pool_ab.json")
    b = gp.synth_molhiv_batch(graphs, seed=1234)
    e = Engine("GIN", 0)
    e.set_emb_dim(300)
    e.set_weights(weights.synth_gin_weights(seed=7, emb_dim=300))
    e.set_batch(b)
    e.profile_enable(True)
    res = {"graphs": graphs, "nodes": b.total_nodes, "edges": b.total_edges, "rounds": ROUNDS, "runs": RUNS}
    res["a_mean_readout"] = measure(e)
    e.set_attention_pooling(weights.synth_attention_pooling(seed=11))
    res["b_attention_readout"] = measure(e)
    e.close()
    a, bb = res["a_mean_readout"], res["b_attention_readout"]
    res["b_minus_a_ms"] = bb["step_ms"] - a["step_ms"]
    res["b_over_a"] = bb["step_ms"] / a["step_ms"]
    res["slot_difference_ms"] = {k: bb["slots_ms"].get(k, 0.0) - a["slots_ms"].get(k, 0.0) for k in sorted(set(a["slots_ms"]) | set(bb["slots_ms"]))}
    res["layer_launch_ms"] = bb["slots_ms"]["gin_wide_layer"] / 5
    res["gate_over_layer_launch"] = bb["slots_ms"]["attn_gate"] / res["layer_launch_ms"]
    for k in ("a_mean_readout", "b_attention_readout"):
        print(f"{k}: {res[k]['step_ms']:.3f} ms (medians {['%.3f' % m for m in res[k]['step_medians_ms']]}), re-runs {res[k]['exact_reruns']}: {res[k]['slots_ms']}", flush=True)
    print(f"(b) - (a) = {res['b_minus_a_ms']:.3f} ms, (b) / (a) = {res['b_over_a']:.3f}; per slot: {res['slot_difference_ms']}; "
          f"attn_gate / one gin_wide_layer launch = {res['gate_over_layer_launch']:.2f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
