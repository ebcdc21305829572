"""Attention coefficients (flowgnn.h: flowgnn_set_attention): what the stores cost, on ONE batch in ONE process per commit, the settings
alternating.
usage: attention_ab.py PACKAGE_ROOT OUT.json [--merge PARENT.json]
  PACKAGE_ROOT  the checkout whose flowgnn_amd (and built library) is measured: this one, or a scratch checkout of the parent commit.
  --merge       the OUT.json of a run of this script against the parent commit, same box, same session: its figures are added
                (profiles/attention_ab.json is such a merged file).
Settings (GAT, 2^16 molhiv-shaped graphs, default options unless said):
  parent commit   (a) default
  this commit     (b) off = default   (c) mask 16 (the last layer)   (d) mask 31 (all five)
                  (e) gat_resident 0, off     (f) gat_resident 0, mask 16     (g) gat_resident 0, mask 31
Per setting: three medians of 10 synchronised runs, of the device-event time of all kernels of a step (profile_read) and of the wall
clock.  Beside the differences: the stored bytes, n_sel x (E + N) x 16, over 6.29 TB/s, the HBM rate a float4 copy reaches on this
GPU (the edge stores are scattered 16-byte writes, so that is a floor, not an estimate)."""
import json
import os
import sys
import time

import numpy as np

ROUNDS, RUNS = 3, 10
GRAPHS = 1 << 16
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


def main():
    root, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
    merge = sys.argv[sys.argv.index("--merge") + 1] if "--merge" in sys.argv else None
    sys.path.insert(0, root)
    from flowgnn_amd import Engine, graphpack as gp, weights
    has = hasattr(Engine, "set_attention")
    res = {"package": "this commit" if has else "parent commit", "rounds": ROUNDS, "runs": RUNS}
    # setting -> (engine, mask)
    settings = ({"off": ("resident", 0), "mask16": ("resident", 16), "mask31": ("resident", 31),
                 "per_layer_off": ("per_layer", 0), "per_layer_mask16": ("per_layer", 16), "per_layer_mask31": ("per_layer", 31)} if has
                else {"default": ("resident", None)})
    b = gp.synth_molhiv_batch(GRAPHS, seed=1234)
    w = weights.synth_gat_weights(seed=7)
    eng = {}
    for key, opts in (("resident", {}), ("per_layer", {"gat_resident": 0})):
        if not any(k == key for k, _ in settings.values()):
            continue
        e = Engine("GAT", 0, options=opts)
        e.set_weights(w)
        e.set_batch(b)
        e.profile_enable(True)
        eng[key] = e

    def select(s):
        e, mask = eng[settings[s][0]], settings[s][1]
        if mask is not None:
            e.set_attention([l for l in range(5) if (mask >> l) & 1] or None)
        return e
    med = {s: {"kernel_ms": [], "wall_ms": []} for s in settings}
    for _ in range(ROUNDS):
        for s in settings:
            k, t = measure(select(s))
            med[s]["kernel_ms"].append(k)
            med[s]["wall_ms"].append(t)
    names = {}
    for s in settings:
        e = select(s)
        before = {k: v["launches"] for k, v in e.profile_read().items()}
        e.run()
        e.sync()
        names[s] = sorted(k for k, v in e.profile_read().items() if v["launches"] > before.get(k, 0))
    for e in eng.values():
        e.close()
    res.update(graphs=GRAPHS, nodes=int(b.total_nodes), edges=int(b.total_edges), medians=med, kernels=names,
               stored_bytes_per_layer=(int(b.total_nodes) + int(b.total_edges)) * 16)
    for s in settings:
        print(f"GAT {GRAPHS:7d} graphs  {s:18s} kernels {min(med[s]['kernel_ms']):8.3f} ms  wall {min(med[s]['wall_ms']):8.3f} ms"
              f"  (medians {['%.3f' % x for x in med[s]['kernel_ms']]})", flush=True)
    if merge:
        parent = json.load(open(merge))
        res["parent"] = {k: parent[k] for k in ("medians", "kernels")}
        if has:
            best = lambda m, s: min(m[s]["kernel_ms"])
            pk = parent["medians"]["default"]["kernel_ms"]
            layer = res["stored_bytes_per_layer"] / HBM_BYTES_PER_MS
            res["summary"] = {"parent_default": min(pk), "parent_default_spread": (max(pk) - min(pk)) / float(np.median(pk)),
                              "off": best(med, "off"), "mask16": best(med, "mask16"), "mask31": best(med, "mask31"),
                              "per_layer_off": best(med, "per_layer_off"), "per_layer_mask16": best(med, "per_layer_mask16"),
                              "per_layer_mask31": best(med, "per_layer_mask31"),
                              "mask16_minus_off_ms": best(med, "mask16") - best(med, "off"),
                              "mask31_minus_off_ms": best(med, "mask31") - best(med, "off"),
                              "one_layer_bytes_over_hbm_rate_ms": layer, "five_layers_bytes_over_hbm_rate_ms": 5 * layer}
            print(json.dumps(res["summary"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
