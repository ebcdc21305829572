"""Graph embeddings off against on (flowgnn.h: flowgnn_set_embeddings) on ONE batch per model in ONE process, the settings alternating.
usage: embeddings_ab.py PACKAGE_ROOT OUT.json [--merge PARENT.json] [--models GIN,PNA,..]
  PACKAGE_ROOT  the checkout whose flowgnn_amd (and built library) is measured: this one, or a scratch checkout of the parent commit.
                A package without Engine.set_embeddings (the parent) is measured with embeddings off only.
  --merge       the OUT.json of a run of this script against the parent commit, same box, same session: its figures are added and
                the conditions of the speed check are evaluated (profiles/embeddings_ab.json is such a merged file).
Per model and setting: three medians of 10 synchronised runs, of the device-event time of all kernels of a step (profile_read) and
of the wall clock.  Batches: GIN 2^18 molhiv graphs (settings: off, on, and NUM_TASK = 2 -- the path that runs the same un-folded
resident instance, writes the h_5 rows to HBM and reads them back), PNA / DGN 2^16 hep10k graphs, GCN / GAT 2^16 molhiv graphs."""
import json
import os
import sys
import time

import numpy as np

ROUNDS, RUNS = 3, 10
SIZES = {"GIN": 1 << 18, "PNA": 1 << 16, "DGN": 1 << 16, "GCN": 1 << 16, "GAT": 1 << 16}


def measure(e, runs=RUNS):
    total = lambda: sum(v["total_ms"] for v in e.profile_read().values())
    for _ in range(2):
        e.run()
    e.sync()
    kern, wall = [], []
    for _ in range(runs):
        k0 = total()
        t0 = time.perf_counter()
        e.run()
        e.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(total() - k0)
    return float(np.median(kern)), float(np.median(wall))


def spread(xs):
    return (max(xs) - min(xs)) / float(np.median(xs))


def main():
    root, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
    merge = sys.argv[sys.argv.index("--merge") + 1] if "--merge" in sys.argv else None
    models = sys.argv[sys.argv.index("--models") + 1].split(",") if "--models" in sys.argv else list(SIZES)
    sys.path.insert(0, root)
    from flowgnn_amd import Engine, graphpack as gp, weights
    has_emb = hasattr(Engine, "set_embeddings")
    res = {"package": "this commit" if has_emb else "parent commit", "rounds": ROUNDS, "runs": RUNS, "models": {}}
    for model in models:
        G = SIZES[model]
        if model in ("PNA", "DGN"):
            b = gp.synth_hep10k_batch(G, seed=1234, with_eigen=model == "DGN")
        else:
            b = gp.synth_molhiv_batch(G, seed=1234)
        wfn = getattr(weights, f"synth_{model.lower()}_weights")
        engines = {}
        e = Engine(model, 0)
        e.set_weights(wfn(seed=7))
        e.set_batch(b)
        e.profile_enable(True)
        engines["off"] = e
        if model == "GIN":
            t2 = Engine(model, 0)
            t2.set_num_tasks(2)
            t2.set_weights(wfn(seed=7, num_tasks=2))
            t2.set_batch(b)
            t2.profile_enable(True)
            engines["num_task_2"] = t2
        settings = ["off"] + (["on"] if has_emb else []) + (["num_task_2"] if model == "GIN" else [])
        med = {s: {"kernel_ms": [], "wall_ms": []} for s in settings}
        for _ in range(ROUNDS):
            for s in settings:
                eng = engines["num_task_2"] if s == "num_task_2" else engines["off"]
                if has_emb and s != "num_task_2":
                    eng.set_embeddings(s == "on")
                k, t = measure(eng)
                med[s]["kernel_ms"].append(k)
                med[s]["wall_ms"].append(t)
        names = {}
        if has_emb:
            for s in ("off", "on"):
                e.set_embeddings(s == "on")
                before = {k: v["launches"] for k, v in e.profile_read().items()}
                e.run()
                e.sync()
                names[s] = sorted(k for k, v in e.profile_read().items() if v["launches"] > before.get(k, 0))
        for eng in engines.values():
            eng.close()
        res["models"][model] = {"graphs": G, "nodes": int(b.total_nodes), "edges": int(b.total_edges), "medians": med, "kernels": names}
        for s in settings:
            print(f"{model:4s} {G:7d} graphs  {s:10s} kernels {min(med[s]['kernel_ms']):8.3f} ms  wall {min(med[s]['wall_ms']):8.3f} ms"
                  f"  (medians {['%.3f' % x for x in med[s]['kernel_ms']]})", flush=True)
    if merge:
        parent = json.load(open(merge))
        res["parent"] = parent["models"]
        checks = {}
        for model, r in res["models"].items():
            if model not in parent["models"] or "on" not in r["medians"]:
                continue
            p = parent["models"][model]["medians"]
            t_on, t_off = min(r["medians"]["on"]["kernel_ms"]), min(r["medians"]["off"]["kernel_ms"])
            c = {"t_on": t_on, "t_off": t_off, "t_on_over_t_off": t_on / t_off, "t_parent_default": min(p["off"]["kernel_ms"]),
                 "parent_default_spread": spread(p["off"]["kernel_ms"]),
                 "off_within_parent_spread": t_off <= min(p["off"]["kernel_ms"]) * (1.0 + spread(p["off"]["kernel_ms"]))}
            if model == "GIN":
                s = spread(p["num_task_2"]["kernel_ms"])
                c.update(t_parent_T2=min(p["num_task_2"]["kernel_ms"]), s=s, t_this_T2=min(r["medians"]["num_task_2"]["kernel_ms"]),
                         condition="t_on <= t_parent_T2 * (1 + s)", holds=t_on <= min(p["num_task_2"]["kernel_ms"]) * (1.0 + s))
            elif model in ("PNA", "DGN"):
                s = c["parent_default_spread"]
                c.update(s=s, condition="t_on <= t_parent_default * (1 + s)", holds=t_on <= c["t_parent_default"] * (1.0 + s))
            else:
                c.update(condition="none: the per-layer detour is the documented open item")
            checks[model] = c
            print(model, json.dumps(c), flush=True)
        res["checks"] = checks
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
