"""GCN at OGB's default width (flowgnn.h: flowgnn_set_model_emb_dim): what one step costs beside the 100-wide per-layer path.
usage: gcn_wide_ab.py OUT.json [--graphs N]
One batch of N = 2^16 molpcba-shaped graphs, two engines:
  (a) width 100 on the per-layer path (gcn_resident 0);
  (b) width 300 (gcn_wide.hip).
A step's time is the device-event total of its kernels (profile_read) -- best of three medians of ten runs after two warm-up runs, as
scripts/dev/gin_wide_ab.py does --, with the per-slot split, and for the five launches of (b)'s gcn_wide_layer slot:
  * the share of the f16 matrix pipe's 2.5 PFLOP/s that the four layer launches' executed MFMA flops amount to (three f16 MFMAs per
    product over the PADDED sizes: 16-row node tiles, K 320, 20 output tiles of which the last is all padding);
  * the share of the HBM's 8 TB/s that their algorithmic bytes amount to: every row read once and written once, the CSR arrays once
    (the walk's neighbour rows, E x D floats per launch, are reported beside it: whether they come from HBM or L2 is the cache's doing)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

ROUNDS, RUNS = 3, 10
F16_PEAK = 2.5e15
HBM_PEAK = 8.0e12
LAYER_SLOT = "gcn_wide_layer"


def measure(b, options, emb_dim):
    e = Engine("GCN", 0, options=options)
    if emb_dim != 100:
        e.set_model_emb_dim(emb_dim)
    e.set_weights(weights.synth_gcn_weights(seed=7, emb_dim=emb_dim))
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
    """Of the four layer launches of one step: 3 MFMAs per product, 2 flops per MAC, padded sizes."""
    ks, tiles = (d + 31) // 32, 2 * (((d + 15) // 16 + 1) // 2)  # whole chunks of two output tiles
    cols = 16 * ((nodes + 15) // 16)
    return 4 * 3 * 2 * cols * 16 * tiles * 32 * ks


def algorithmic_bytes(nodes, edges, d):
    """Of the five launches of the slot (four layers and the last stage): rows in, rows out, CSR entry (src, code, dinv) and row_ptr / out_deg."""
    return 5 * (2 * nodes * d * 4 + edges * 9 + nodes * 8)


def main():
    out_path = sys.argv[1]
    graphs = int(sys.argv[sys.argv.index("--graphs") + 1]) if "--graphs" in sys.argv else 1 << 16
    b = gp.synth_molpcba_batch(graphs, seed=1234)
    res = {"graphs": graphs, "nodes": b.total_nodes, "edges": b.total_edges, "rounds": ROUNDS, "runs": RUNS,
           "a_width_100_per_layer": measure(b, {"gcn_resident": 0}, 100),
           "b_width_300": measure(b, {}, 300)}
    a, bb = res["a_width_100_per_layer"], res["b_width_300"]
    layer_ms = bb["slots_ms"].get(LAYER_SLOT, 0.0)
    flops = executed_f16_flops(b.total_nodes, 300)
    nbytes = algorithmic_bytes(b.total_nodes, b.total_edges, 300)
    res["b_over_a"] = bb["step_ms"] / a["step_ms"]
    res["gcn_wide_layer_ms_per_step"] = layer_ms
    res["executed_f16_flops_per_step"] = flops
    res["algorithmic_bytes_per_step"] = nbytes
    res["gather_bytes_per_step"] = 5 * b.total_edges * 300 * 4
    # (the slot's five launches: four with the product; the fifth, without one, is a fifth of the bytes -- both shares use the slot's time)
    res["f16_flop_fraction_of_2.5_PF"] = flops / (layer_ms * 1e-3) / F16_PEAK if layer_ms > 0 else None
    res["hbm_fraction_of_8_TBs"] = nbytes / (layer_ms * 1e-3) / HBM_PEAK if layer_ms > 0 else None
    for k in ("a_width_100_per_layer", "b_width_300"):
        print(f"{k}: {res[k]['step_ms']:.3f} ms (medians {['%.3f' % m for m in res[k]['step_medians_ms']]}), re-runs {res[k]['exact_reruns']}: {res[k]['slots_ms']}", flush=True)
    print(f"(b) / (a) = {res['b_over_a']:.2f}; {LAYER_SLOT} {layer_ms:.3f} ms per step (five launches), {flops:.3e} f16 flops executed, "
          f"{100 * (res['f16_flop_fraction_of_2.5_PF'] or 0):.1f} % of 2.5 PFLOP/s; {nbytes:.3e} algorithmic bytes, "
          f"{100 * (res['hbm_fraction_of_8_TBs'] or 0):.1f} % of 8 TB/s", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
