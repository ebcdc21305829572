"""OGB's set2set readout at width 300 (flowgnn.h: flowgnn_set_set2set_pooling): what it adds to one step.
usage: set2set_ab.py [OUT.json] [--graphs N] [--steps S]      (default OUT: profiles/set2set_ab.json)
One batch of N = 2^16 molhiv-shaped graphs, one width-300 GIN engine under three readouts, alternating in one process:
  (a) the mean readout (mean_pool_rows + pooled_head);
  (b) the attention readout (wide_attn.hip: attn_gate + attn_pool_rows);
  (c) the set2set readout, S = 2 steps (wide_s2s.hip: s2s_lstm, s2s_dot_rows, s2s_pool_rows per step, then s2s_head).
A step's time is the device-event total of its kernels (profile_read): per readout the best of three medians of ten runs after two
warm-up runs, a round of each readout in turn, as scripts/dev/attn_pool_ab.py measures, with the per-slot split of each.  The tensors
are weights.synth_attention_pooling(seed=11) and weights.synth_set2set(seed=17); exact_reruns is reported and must be 0: a re-run
would time the fp32 form."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

ROUNDS, RUNS = 3, 10


def one_round(e):
    read = lambda: {k: (v["total_ms"], v["launches"]) for k, v in e.profile_read().items()}

    def step():
        k0 = read()
        e.run()
        e.sync()
        k1 = read()
        return {k: k1[k][0] - k0.get(k, (0.0, 0))[0] for k in k1 if k1[k][1] - k0.get(k, (0.0, 0))[1] > 0}
    for _ in range(2):
        step()
    return [step() for _ in range(RUNS)]


def summary(rounds, reruns):
    med = lambda key: [float(np.median([key(s) for s in r])) for r in rounds]
    total = med(lambda s: sum(s.values()))
    slots = sorted({k for r in rounds for s in r for k in s})
    best = int(np.argmin(total))
    return {"step_ms": min(total), "step_medians_ms": total, "spread_ms": max(total) - min(total), "exact_reruns": reruns,
            "slots_ms": {k: med(lambda s, k=k: s.get(k, 0.0))[best] for k in slots}}


def main():
    args = [a for a in sys.argv[1:]]
    graphs, steps = 1 << 16, 2
    for flag in ("--graphs", "--steps"):
        if flag in args:
            i = args.index(flag)
            if flag == "--graphs":
                graphs = int(args[i + 1])
            else:
                steps = int(args[i + 1])
            del args[i:i + 2]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "set2set_ab.json")
    b = gp.synth_molhiv_batch(graphs, seed=1234)
    gate, s2s = weights.synth_attention_pooling(seed=11), weights.synth_set2set(seed=17)
    e = Engine("GIN", 0)
    e.set_emb_dim(300)
    e.set_weights(weights.synth_gin_weights(seed=7, emb_dim=300))
    e.set_batch(b)
    e.profile_enable(True)
    states = {"a_mean_readout": lambda: None, "b_attention_readout": lambda: e.set_attention_pooling(gate),
              "c_set2set_readout": lambda: e.set_set2set_pooling(s2s, steps=steps)}
    rounds, reruns = {k: [] for k in states}, {k: 0 for k in states}
    for _ in range(ROUNDS):
        for k, turn_on in states.items():
            turn_on()
            before = e.exact_reruns()
            rounds[k].append(one_round(e))
            reruns[k] += e.exact_reruns() - before
            e.set_attention_pooling(None)
            e.set_set2set_pooling(None)
    e.close()
    res = {"graphs": graphs, "nodes": b.total_nodes, "edges": b.total_edges, "rounds": ROUNDS, "runs": RUNS, "set2set_steps": steps}
    for k in states:
        res[k] = summary(rounds[k], reruns[k])
    a, c = res["a_mean_readout"], res["c_set2set_readout"]
    res["c_minus_a_ms"] = c["step_ms"] - a["step_ms"]
    res["c_over_a"] = c["step_ms"] / a["step_ms"]
    res["b_minus_a_ms"] = res["b_attention_readout"]["step_ms"] - a["step_ms"]
    res["new_slots_ms"] = {k: v for k, v in c["slots_ms"].items() if k.startswith("s2s_")}
    for k in states:
        print(f"{k}: {res[k]['step_ms']:.3f} ms (medians {['%.3f' % m for m in res[k]['step_medians_ms']]}), re-runs {res[k]['exact_reruns']}: {res[k]['slots_ms']}", flush=True)
    print(f"(c) - (a) = {res['c_minus_a_ms']:.3f} ms, (c) / (a) = {res['c_over_a']:.3f}, (b) - (a) = {res['b_minus_a_ms']:.3f} ms; new slots: {res['new_slots_ms']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
