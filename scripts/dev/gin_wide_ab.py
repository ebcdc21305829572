"""GIN at OGB's default width (flowgnn.h: flowgnn_set_emb_dim): what one step costs beside the 100-wide per-layer path.
usage: gin_wide_ab.py OUT.json [--graphs N]
One batch of N = 2^16 molhiv-shaped graphs, two engines:
  (a) width 100 on the per-layer path (gin_resident 0) -- measurable on the commit before this width existed;
  (b) width 300 (gin_wide.hip).
A step's time is the device-event total of its kernels (profile_read) -- best of three medians of ten runs after two warm-up runs, as
scripts/dev/ogb_vn_ab.py does --, with the per-slot split of (b) and the share of the f16 matrix pipe's 2.5 PFLOP/s that the layer
kernel's executed MFMA flops amount to (three f16 MFMAs per product over the PADDED sizes: 16-row node tiles, K 320 and 608, 608 hidden
and 304 output rows)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

ROUNDS, RUNS = 3, 10
F16_PEAK = 2.5e15


def measure(b, options, emb_dim):
    e = Engine("GIN", 0, options=options)
    if emb_dim != 100:
        e.set_emb_dim(emb_dim)
    e.set_weights(weights.synth_gin_weights(seed=7, emb_dim=emb_dim) if emb_dim != 100 else weights.synth_gin_weights(seed=7))
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


def executed_f16_flops(nodes, d):
    """Of the five layer launches of one step: 3 MFMAs per product, 2 flops per MAC, padded sizes."""
    ks1, ks2, t2 = (d + 31) // 32, (2 * d + 31) // 32, (d + 15) // 16
    cols = 16 * ((nodes + 15) // 16)
    macs = cols * (16 * 2 * ks2 * 32 * ks1 + 16 * t2 * 32 * ks2)
    return 5 * 3 * 2 * macs


def main():
    out_path = sys.argv[1]
    graphs = int(sys.argv[sys.argv.index("--graphs") + 1]) if "--graphs" in sys.argv else 1 << 16
    b = gp.synth_molhiv_batch(graphs, seed=1234)
    res = {"graphs": graphs, "nodes": b.total_nodes, "edges": b.total_edges, "rounds": ROUNDS, "runs": RUNS,
           "a_width_100_per_layer": measure(b, {"gin_resident": 0}, 100),
           "b_width_300": measure(b, {}, 300)}
    a, bb = res["a_width_100_per_layer"], res["b_width_300"]
    layer_ms = bb["slots_ms"].get("gin_wide_layer", 0.0)
    flops = executed_f16_flops(b.total_nodes, 300)
    res["b_over_a"] = bb["step_ms"] / a["step_ms"]
    res["gin_wide_layer_ms_per_step"] = layer_ms
    res["executed_f16_flops_per_step"] = flops
    res["f16_flop_fraction_of_2.5_PF"] = flops / (layer_ms * 1e-3) / F16_PEAK if layer_ms > 0 else None
    for k in ("a_width_100_per_layer", "b_width_300"):
        print(f"{k}: {res[k]['step_ms']:.3f} ms (medians {['%.3f' % m for m in res[k]['step_medians_ms']]}), re-runs {res[k]['exact_reruns']}: {res[k]['slots_ms']}", flush=True)
    print(f"(b) / (a) = {res['b_over_a']:.2f}; gin_wide_layer {layer_ms:.3f} ms per step, {flops:.3e} f16 flops executed, "
          f"{100 * (res['f16_flop_fraction_of_2.5_PF'] or 0):.1f} % of 2.5 PFLOP/s", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
