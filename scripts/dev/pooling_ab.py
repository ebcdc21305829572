"""Readout pooling (flowgnn.h: flowgnn_set_pooling): step time per model for the mean, the sum and the maximum, on ONE batch per model in
ONE process per commit, the modes alternating on one engine.
usage: pooling_ab.py PACKAGE_ROOT OUT.json [--merge PARENT.json] [--models GIN,GAT,..]
  PACKAGE_ROOT  the checkout whose flowgnn_amd (and built library) is measured: this one, or a scratch checkout of the parent commit
                (which has the mean alone).
  --merge       the OUT.json of a run of this script against the parent commit, same box, same session: its figures are added and
                the condition is evaluated (profiles/pooling_ab.json is such a merged file).
Per mode: three medians of 10 synchronised runs, of the device-event time of all kernels of a step (profile_read), of the model's
graph-resident slot alone, and of the wall clock.  Batches: 2^16 molhiv-shaped graphs (GIN, GIN-VN, GCN, GAT).
Condition (--merge): this commit's mean within the spread of the parent's own three medians of the mean (the default launches are the
parent's).  Beside it: sum / mean and max / mean of the step's kernels."""
import json
import os
import sys
import time

import numpy as np

ROUNDS, RUNS = 3, 10
GRAPHS = 1 << 16
MODELS = ["GIN", "GIN-VN", "GCN", "GAT"]


def measure(e, slot, runs=RUNS):
    total = lambda: sum(v["total_ms"] for v in e.profile_read().values())
    resident = lambda: e.profile_read().get(slot, {"total_ms": 0.0})["total_ms"]
    for _ in range(2):
        e.run()
    e.sync()
    kern, res, wall = [], [], []
    for _ in range(runs):
        k0, r0 = total(), resident()
        t0 = time.perf_counter()
        e.run()
        e.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(total() - k0)
        res.append(resident() - r0)
    return float(np.median(kern)), float(np.median(res)), float(np.median(wall))


def spread(xs):
    return (max(xs) - min(xs)) / float(np.median(xs))


def main():
    root, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
    merge = sys.argv[sys.argv.index("--merge") + 1] if "--merge" in sys.argv else None
    models = sys.argv[sys.argv.index("--models") + 1].split(",") if "--models" in sys.argv else MODELS
    sys.path.insert(0, root)
    from flowgnn_amd import Engine, graphpack as gp, weights
    has = hasattr(Engine, "set_pooling")
    res = {"package": "this commit" if has else "parent commit", "rounds": ROUNDS, "runs": RUNS, "models": {}}
    modes = ["mean", "sum", "max"] if has else ["mean"]
    for model in models:
        base = model.replace("-VN", "").lower()
        b = gp.synth_molhiv_batch(GRAPHS, seed=1234)
        if model == "GIN-VN":
            b = gp.add_virtual_nodes(b)
        e = Engine(model, 0)
        e.set_weights(getattr(weights, f"synth_{base}_weights")(seed=7))
        e.set_batch(b)
        e.profile_enable(True)
        select = (lambda m: e.set_pooling(m)) if has else (lambda m: None)
        med = {m: {"kernel_ms": [], "resident_ms": [], "wall_ms": []} for m in modes}
        for _ in range(ROUNDS):
            for m in modes:
                select(m)
                k, r, t = measure(e, base + "_resident")
                med[m]["kernel_ms"].append(k)
                med[m]["resident_ms"].append(r)
                med[m]["wall_ms"].append(t)
        names = {}
        for m in modes:
            select(m)
            before = {k: v["launches"] for k, v in e.profile_read().items()}
            e.run()
            e.sync()
            names[m] = sorted(k for k, v in e.profile_read().items() if v["launches"] > before.get(k, 0))
        e.close()
        res["models"][model] = {"graphs": GRAPHS, "nodes": int(b.total_nodes), "edges": int(b.total_edges), "medians": med, "kernels": names}
        for m in modes:
            print(f"{model:6s} {GRAPHS:7d} graphs  {m:5s} kernels {min(med[m]['kernel_ms']):8.3f} ms  resident slot {min(med[m]['resident_ms']):8.3f} ms"
                  f"  wall {min(med[m]['wall_ms']):8.3f} ms  (medians {['%.3f' % x for x in med[m]['kernel_ms']]})", flush=True)
    if merge:
        parent = json.load(open(merge))
        res["parent"] = parent["models"]
        checks = {}
        for model, r in res["models"].items():
            if model not in parent["models"] or "sum" not in r["medians"]:
                continue
            p = parent["models"][model]["medians"]["mean"]["kernel_ms"]
            best = lambda m: min(r["medians"][m]["kernel_ms"])
            sp = spread(p)
            checks[model] = {"parent_mean": min(p), "mean": best("mean"), "sum": best("sum"), "max": best("max"), "parent_mean_spread": sp,
                             "mean_within_spread_of_parent": best("mean") <= min(p) * (1.0 + sp), "sum_over_mean": best("sum") / best("mean"),
                             "max_over_mean": best("max") / best("mean")}
            print(model, json.dumps(checks[model]), flush=True)
        res["checks"] = checks
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
