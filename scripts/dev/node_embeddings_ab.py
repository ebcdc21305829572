"""Node embeddings off against on (flowgnn.h: flowgnn_set_node_embeddings), and the graph-resident path against the per-layer one, on
ONE batch per model in ONE process, the settings alternating.
usage: node_embeddings_ab.py PACKAGE_ROOT OUT.json [--merge PARENT.json] [--models GCN,PNA,..]
  PACKAGE_ROOT  the checkout whose flowgnn_amd (and built library) is measured: this one, or a scratch checkout of the parent commit.
  --merge       the OUT.json of a run of this script against the parent commit, same box, same session: its figures are added and
                the two conditions are evaluated (profiles/node_embeddings_ab.json is such a merged file).
Settings per model, two engines (default options; <model>_resident 0):
  parent commit   (a) default            (b) resident0        -- (b) is a lower bound on what the parent needs to leave the rows
                                                                 in HBM: its last stage is still folded
  this commit     (c) off = default      (d) on               resident0_on = the per-layer path with node embeddings on
Per setting: three medians of 10 synchronised runs, of the device-event time of all kernels of a step (profile_read) and of the wall
clock.  Batches: 2^16 graphs of the model's shape (molhiv: GIN, GIN-VN, GCN, GAT; hep10k: PNA, DGN).
Conditions (--merge): (c) within the spread of (a)'s own three medians; (d) <= (b) for GCN, PNA and DGN.  Beside (d) - (c): the stored
bytes N x dim x 4 over 6.29 TB/s, the HBM rate a float4 copy reaches on this GPU."""
import json
import os
import sys
import time

import numpy as np

ROUNDS, RUNS = 3, 10
GRAPHS = 1 << 16
MODELS = ["GIN", "GIN-VN", "GCN", "GAT", "PNA", "DGN"]
ON_CHIP = ("GCN", "PNA", "DGN")
HBM_BYTES_PER_MS = 6.29e9
DIM = {"GIN": 100, "GIN-VN": 100, "GCN": 100, "GAT": 16, "PNA": 80, "DGN": 100}


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
    models = sys.argv[sys.argv.index("--models") + 1].split(",") if "--models" in sys.argv else MODELS
    sys.path.insert(0, root)
    from flowgnn_amd import Engine, graphpack as gp, weights
    has = hasattr(Engine, "set_node_embeddings")
    res = {"package": "this commit" if has else "parent commit", "rounds": ROUNDS, "runs": RUNS, "models": {}}
    for model in models:
        base = model.replace("-VN", "").lower()
        if model in ("PNA", "DGN"):
            b = gp.synth_hep10k_batch(GRAPHS, seed=1234, with_eigen=model == "DGN")
        else:
            b = gp.synth_molhiv_batch(GRAPHS, seed=1234)
            if model == "GIN-VN":
                b = gp.add_virtual_nodes(b)
        w = getattr(weights, f"synth_{base}_weights")(seed=7)
        eng = {}
        for key, opts in (("default", {}), ("resident0", {f"{base}_resident": 0})):
            e = Engine(model, 0, options=opts)
            e.set_weights(w)
            e.set_batch(b)
            e.profile_enable(True)
            eng[key] = e
        # setting -> (engine, node embeddings on)
        settings = ({"off": ("default", False), "on": ("default", True), "resident0_on": ("resident0", True)} if has
                    else {"default": ("default", None), "resident0": ("resident0", None)})
        med = {s: {"kernel_ms": [], "wall_ms": []} for s in settings}
        for _ in range(ROUNDS):
            for s, (key, on) in settings.items():
                if on is not None:
                    eng[key].set_node_embeddings(on)
                k, t = measure(eng[key])
                med[s]["kernel_ms"].append(k)
                med[s]["wall_ms"].append(t)
        names = {}
        for s, (key, on) in settings.items():
            e = eng[key]
            if on is not None:
                e.set_node_embeddings(on)
            before = {k: v["launches"] for k, v in e.profile_read().items()}
            e.run()
            e.sync()
            names[s] = sorted(k for k, v in e.profile_read().items() if v["launches"] > before.get(k, 0))
        for e in eng.values():
            e.close()
        res["models"][model] = {"graphs": GRAPHS, "nodes": int(b.total_nodes), "edges": int(b.total_edges), "medians": med, "kernels": names,
                                "stored_bytes": int(b.total_nodes) * DIM[model] * 4}
        for s in settings:
            print(f"{model:6s} {GRAPHS:7d} graphs  {s:12s} kernels {min(med[s]['kernel_ms']):8.3f} ms  wall {min(med[s]['wall_ms']):8.3f} ms"
                  f"  (medians {['%.3f' % x for x in med[s]['kernel_ms']]})", flush=True)
    if merge:
        parent = json.load(open(merge))
        res["parent"] = parent["models"]
        checks = {}
        for model, r in res["models"].items():
            if model not in parent["models"] or "on" not in r["medians"]:
                continue
            p = parent["models"][model]["medians"]
            best = lambda m, s: min(m[s]["kernel_ms"])
            a, bb, c, d = best(p, "default"), best(p, "resident0"), best(r["medians"], "off"), best(r["medians"], "on")
            sp = spread(p["default"]["kernel_ms"])
            ck = {"a_parent_default": a, "b_parent_resident0": bb, "c_off": c, "d_on": d, "this_resident0_on": best(r["medians"], "resident0_on"),
                  "parent_default_spread": sp, "c_within_spread_of_a": c <= a * (1.0 + sp),
                  "d_minus_c_ms": d - c, "stored_bytes": r["stored_bytes"], "stored_bytes_over_hbm_rate_ms": r["stored_bytes"] / HBM_BYTES_PER_MS}
            if model in ON_CHIP:
                ck["d_le_b"] = d <= bb
            checks[model] = ck
            print(model, json.dumps(ck), flush=True)
        res["checks"] = checks
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
