"""Node logits (flowgnn.h: flowgnn_set_node_logits) against the only way the parent commit can deliver those values -- node embeddings on
plus a dot product on the caller's side -- on ONE batch per model in ONE process per commit, the settings alternating.
usage: node_logits_ab.py PACKAGE_ROOT OUT.json [--merge PARENT.json] [--models GIN,GAT,..]
  PACKAGE_ROOT  the checkout whose flowgnn_amd (and built library) is measured: this one, or a scratch checkout of the parent commit.
  --merge       the OUT.json of a run of this script against the parent commit, same box, same session: its figures are added and
                the two conditions are evaluated (profiles/node_logits_ab.json is such a merged file).
Settings per model, one engine, default options:
  parent commit   (a) default                      (b) node embeddings on
  this commit     (c) off = default                (d) node logits on            (and node embeddings on, for reference)
Per setting: three medians of 10 synchronised runs, of the device-event time of all kernels of a step (profile_read) and of the wall
clock.  Batches: 2^16 molhiv-shaped graphs (GIN, GIN-VN, GCN, GAT).
Conditions (--merge): (c) within the spread of (a)'s own three medians; (d) <= (b).  Beside (d) - (c): the stored bytes N x 4 over
6.29 TB/s, the HBM rate a float4 copy reaches on this GPU."""
import json
import os
import sys
import time

import numpy as np

ROUNDS, RUNS = 3, 10
GRAPHS = 1 << 16
MODELS = ["GIN", "GIN-VN", "GCN", "GAT"]
HBM_BYTES_PER_MS = 6.29e9


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
    has = hasattr(Engine, "set_node_logits")
    res = {"package": "this commit" if has else "parent commit", "rounds": ROUNDS, "runs": RUNS, "models": {}}
    # setting -> (node embeddings on, node logits on)
    settings = ({"off": (False, False), "node_logits": (False, True), "node_embeddings": (True, False)} if has
                else {"default": (False, None), "node_embeddings": (True, None)})
    for model in models:
        base = model.replace("-VN", "").lower()
        b = gp.synth_molhiv_batch(GRAPHS, seed=1234)
        if model == "GIN-VN":
            b = gp.add_virtual_nodes(b)
        e = Engine(model, 0)
        e.set_weights(getattr(weights, f"synth_{base}_weights")(seed=7))
        e.set_batch(b)
        e.profile_enable(True)

        def select(s):
            emb, nl = settings[s]
            e.set_node_embeddings(emb)
            if nl is not None:
                e.set_node_logits(nl)
        med = {s: {"kernel_ms": [], "wall_ms": []} for s in settings}
        for _ in range(ROUNDS):
            for s in settings:
                select(s)
                k, t = measure(e)
                med[s]["kernel_ms"].append(k)
                med[s]["wall_ms"].append(t)
        names = {}
        for s in settings:
            select(s)
            before = {k: v["launches"] for k, v in e.profile_read().items()}
            e.run()
            e.sync()
            names[s] = sorted(k for k, v in e.profile_read().items() if v["launches"] > before.get(k, 0))
        e.close()
        res["models"][model] = {"graphs": GRAPHS, "nodes": int(b.total_nodes), "edges": int(b.total_edges), "medians": med, "kernels": names,
                                "stored_bytes": int(b.total_nodes) * 4}
        for s in settings:
            print(f"{model:6s} {GRAPHS:7d} graphs  {s:16s} kernels {min(med[s]['kernel_ms']):8.3f} ms  wall {min(med[s]['wall_ms']):8.3f} ms"
                  f"  (medians {['%.3f' % x for x in med[s]['kernel_ms']]})", flush=True)
    if merge:
        parent = json.load(open(merge))
        res["parent"] = parent["models"]
        checks = {}
        for model, r in res["models"].items():
            if model not in parent["models"] or "node_logits" not in r["medians"]:
                continue
            p = parent["models"][model]["medians"]
            best = lambda m, s: min(m[s]["kernel_ms"])
            a, bb, c, d = best(p, "default"), best(p, "node_embeddings"), best(r["medians"], "off"), best(r["medians"], "node_logits")
            sp = spread(p["default"]["kernel_ms"])
            checks[model] = {"a_parent_default": a, "b_parent_node_embeddings": bb, "c_off": c, "d_node_logits": d,
                             "this_node_embeddings": best(r["medians"], "node_embeddings"), "parent_default_spread": sp,
                             "c_within_spread_of_a": c <= a * (1.0 + sp), "d_le_b": d <= bb, "d_minus_c_ms": d - c,
                             "stored_bytes": r["stored_bytes"], "stored_bytes_over_hbm_rate_ms": r["stored_bytes"] / HBM_BYTES_PER_MS}
            print(model, json.dumps(checks[model]), flush=True)
        res["checks"] = checks
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
