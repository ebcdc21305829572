"""DGN, FLOWGNN_NUMERIC_F16 against the default mode (flowgnn.h: flowgnn_set_model_numeric_mode on a FLOWGNN_MODEL_DGN engine; DESIGN.md
section 4.29).
usage: dgn_f16_ab.py OUT.json [--graphs N ...] [--f32-only] [--parent-f32-ms N=MS ...]
scripts/dev/pna_f16_ab.py for DGN.  One process, per size one batch of hep10k-shaped graphs (2^16 and 2^15 by default: bench.py's
shape) and one engine; the two modes alternate -- f32, f16, f32, f16, f32, f16 -- so that both see the same clocks.  A step's time is
the device-event total of its kernels (profile_read): the median of ten runs after two warm-up runs per turn, best of a mode's three
turns.  The f32 medians' spread is reported: the f16 step has to be faster than the f32 step by more than twice that spread for the
ratio to mean anything.  The step is dgn_tile_build + the resident kernel (slot dgn_resident, or dgn_resident_f16 in the mode);
exact_reruns is reported and must be 0 (a re-run would time the fp32 form).
--parent-f32-ms N=MS: the f32 step this script measured on the parent commit's build at N graphs; the result then carries
f32_over_parent_f32, which should be 1 within the spread (the default kernels are the parent's code)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

TURNS, RUNS = 3, 10
F32_SLOT, F16_SLOT = "dgn_resident", "dgn_resident_f16"


def turn(e):
    """one turn of a mode: (median step, median per slot, launches per step and slot) of RUNS runs after two warm-up runs"""
    def step():
        k0 = e.profile_read()
        e.run()
        e.sync()
        k1 = e.profile_read()
        ms = {k: k1[k]["total_ms"] - k0.get(k, {"total_ms": 0.0})["total_ms"] for k in k1}
        n = {k: k1[k]["launches"] - k0.get(k, {"launches": 0})["launches"] for k in k1}
        return {k: v for k, v in ms.items() if n[k] > 0}, {k: v for k, v in n.items() if v > 0}
    for _ in range(2):
        step()
    steps = [step() for _ in range(RUNS)]
    slots = sorted({k for s, _ in steps for k in s})
    return (float(np.median([sum(s.values()) for s, _ in steps])), {k: float(np.median([s.get(k, 0.0) for s, _ in steps])) for k in slots},
            steps[-1][1])


def measure(e, modes):
    before = e.exact_reruns()
    turns = {m: [] for m in modes}
    for _ in range(TURNS):
        for mode in modes:
            if mode == "f16":
                e.set_numeric_mode("f16", emb_dim=100)
            else:
                e.set_numeric_mode("f32")
            turns[mode].append(turn(e))
    res = {"exact_reruns": e.exact_reruns() - before}
    for mode, t in turns.items():
        best = int(np.argmin([x[0] for x in t]))
        res[mode] = {"step_ms": t[best][0], "step_medians_ms": [x[0] for x in t], "slots_ms": t[best][1], "launches": t[best][2]}
    assert res["f32"]["launches"].get(F32_SLOT) == 1 and F16_SLOT not in res["f32"]["launches"], res["f32"]["launches"]
    m = res["f32"]["step_medians_ms"]
    res["f32_spread_ms"] = max(m) - min(m)
    if "f16" in res:
        assert res["f16"]["launches"].get(F16_SLOT) == 1 and F32_SLOT not in res["f16"]["launches"], res["f16"]["launches"]
        res["f16_over_f32"] = res["f16"]["step_ms"] / res["f32"]["step_ms"]
        res["resident_f16_over_f32"] = res["f16"]["slots_ms"][F16_SLOT] / res["f32"]["slots_ms"][F32_SLOT]
        res["faster_by_more_than_twice_the_spread"] = res["f32"]["step_ms"] - res["f16"]["step_ms"] > 2 * res["f32_spread_ms"]
    return res


def main():
    out_path = sys.argv[1]
    sizes = [int(sys.argv[i + 1]) for i, a in enumerate(sys.argv) if a == "--graphs"] or [1 << 16, 1 << 15]
    parent = dict((int(k), float(v)) for k, v in (sys.argv[i + 1].split("=") for i, a in enumerate(sys.argv) if a == "--parent-f32-ms"))
    modes = ("f32",) if "--f32-only" in sys.argv else ("f32", "f16")  # --f32-only: what a build without the mode can run (the parent's)
    res = {"turns": TURNS, "runs": RUNS, "sizes": {}}
    for graphs in sizes:
        b = gp.synth_hep10k_batch(graphs, seed=1234)
        e = Engine("DGN", 0)
        e.set_weights(weights.synth_dgn_weights(seed=7))
        e.set_batch(b)
        e.profile_enable(True)
        r = measure(e, modes)
        e.close()
        r.update(graphs=graphs, nodes=b.total_nodes, edges=b.total_edges)
        if graphs in parent:
            r["parent_f32_step_ms"] = parent[graphs]
            r["f32_over_parent_f32"] = r["f32"]["step_ms"] / parent[graphs]
        res["sizes"][str(graphs)] = r
        for mode in modes:
            print(f"{graphs} graphs, {mode}: {r[mode]['step_ms']:.3f} ms (medians {['%.3f' % m for m in r[mode]['step_medians_ms']]}): {r[mode]['slots_ms']}",
                  flush=True)
        if "f16" in modes:
            print(f"{graphs} graphs: f16 / f32 = {r['f16_over_f32']:.3f} (resident kernel {r['resident_f16_over_f32']:.3f}), f32 spread "
                  f"{r['f32_spread_ms']:.3f} ms, faster by more than twice the spread: {r['faster_by_more_than_twice_the_spread']}, "
                  f"re-runs {r['exact_reruns']}" + (f", f32 / parent's f32 = {r['f32_over_parent_f32']:.3f}" if graphs in parent else ""), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
