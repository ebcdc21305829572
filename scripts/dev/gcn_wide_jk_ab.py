"""OGB's JK="sum" and residual=True for GCN at width 300 (flowgnn.h: flowgnn_set_model_jk_residual): what the second row stream costs per step.
usage: gcn_wide_jk_ab.py [OUT.json] [--graphs N]      (default OUT: profiles/gcn_wide_jk_ab.json)
One batch of N = 2^16 molpcba-shaped graphs, one width-300 GCN engine, eight states alternating in one process: the settings
(last, off), (last, res), (sum, off), (sum, res), each without and with OGB's virtual node.  (last, off) runs the kernels of
gcn_wide.hip, the other three those of gcn_wide_jk.hip and one more encoder launch (slot gcn_wide_x0): the residual is one more read
AND one more write of [N][D] per stage (the pre-linear rows are stored for the next stage), the JK sum one more read and one more write.
A step's time is the device-event total of its kernels (profile_read): per state the best of three medians of ten runs after two
warm-up runs, a round of each state in turn, as scripts/dev/gin_wide_jk_ab.py measures, with the per-slot split of each.  The virtual
node is weights.synth_gcn_virtual_node(seed=13) with its first linear layer scaled by 1 / 64, which keeps the vector inside the
kernels' range under the residual as well (the synthetic tensors have no BatchNorm to do it); exact_reruns is reported and must be
0: a re-run would time the fp32 form."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

ROUNDS, RUNS = 3, 10
SETTINGS = (("last", False), ("last", True), ("sum", False), ("sum", True))
VN_W1_SCALE = 1.0 / 64


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
    graphs = 1 << 16
    if "--graphs" in args:
        i = args.index("--graphs")
        graphs = int(args[i + 1])
        del args[i:i + 2]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "gcn_wide_jk_ab.json")
    b = gp.synth_molpcba_batch(graphs, seed=1234)
    vn = weights.synth_gcn_virtual_node(seed=13, emb_dim=300)
    vn["w1"] = vn["w1"] * np.float32(VN_W1_SCALE)
    e = Engine("GCN", 0)
    e.set_model_emb_dim(300)
    e.set_weights(weights.synth_gcn_weights(seed=7, emb_dim=300))
    e.set_batch(b)
    e.profile_enable(True)
    states = [(use_vn, jk, res) for use_vn in (False, True) for jk, res in SETTINGS]
    name = lambda s: f"{'vn' if s[0] else 'plain'}_{s[1]}{'_res' if s[2] else ''}"
    rounds, reruns = {name(s): [] for s in states}, {name(s): 0 for s in states}
    for _ in range(ROUNDS):
        for s in states:
            use_vn, jk, res = s
            e.set_gcn_virtual_node(vn if use_vn else None)
            e.set_jk_residual(jk, res)
            before = e.exact_reruns()
            rounds[name(s)].append(one_round(e))
            reruns[name(s)] += e.exact_reruns() - before
    e.close()
    out = {"graphs": graphs, "nodes": b.total_nodes, "edges": b.total_edges, "rounds": ROUNDS, "runs": RUNS, "vn_w1_scale": VN_W1_SCALE}
    for s in states:
        out[name(s)] = summary(rounds[name(s)], reruns[name(s)])
    out["delta_ms"], out["ratio"] = {}, {}
    for s in states:
        base = out[name((s[0], "last", False))]["step_ms"]
        out["delta_ms"][name(s)] = out[name(s)]["step_ms"] - base
        out["ratio"][name(s)] = out[name(s)]["step_ms"] / base
        r = out[name(s)]
        print(f"{name(s)}: {r['step_ms']:.3f} ms (medians {['%.3f' % m for m in r['step_medians_ms']]}), {out['delta_ms'][name(s)]:+.3f} ms, "
              f"x {out['ratio'][name(s)]:.4f}, re-runs {r['exact_reruns']}: {r['slots_ms']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
