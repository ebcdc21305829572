"""GIN at width 300, FLOWGNN_NUMERIC_F16 against the default mode (flowgnn.h: flowgnn_set_numeric_mode_dim).
usage: gin_wide_f16_ab.py OUT.json [--graphs N]
One process, one batch of N = 2^16 molhiv-shaped graphs, one width-300 engine; the two modes alternate -- f32, f16, f32, f16, f32,
f16 -- so that both see the same clocks, first with the virtual node off, then with it on.  A step's time is the device-event total
of its kernels (profile_read): the median of ten runs after two warm-up runs per turn, best of a mode's three turns, as
scripts/dev/numeric_ab.py and gin_wide_vn_ab.py do; the layer slot of each mode (gin_wide_layer, gin_wide_layer_f16) per launch beside
it.  The f32 medians' spread is reported: the f16 step has to be faster than the f32 step by more than twice that spread for the ratio
to mean anything.  exact_reruns is reported and must be 0 (a re-run would time the fp32 form); the virtual node's tensors are
gin_wide_vn_ab.py's."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

TURNS, RUNS = 3, 10
SLOT = {"f32": "gin_wide_layer", "f16": "gin_wide_layer_f16"}


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


def measure(e):
    before = e.exact_reruns()
    turns = {"f32": [], "f16": []}
    for _ in range(TURNS):
        for mode in ("f32", "f16"):
            e.set_numeric_mode(mode, emb_dim=300)
            turns[mode].append(turn(e))
    res = {"exact_reruns": e.exact_reruns() - before}
    for mode, t in turns.items():
        best = int(np.argmin([x[0] for x in t]))
        slot_ms, launches = t[best][1], t[best][2]
        assert SLOT[mode] in slot_ms and SLOT["f16" if mode == "f32" else "f32"] not in slot_ms, (mode, slot_ms)
        res[mode] = {"step_ms": t[best][0], "step_medians_ms": [x[0] for x in t], "slots_ms": slot_ms, "launches": launches,
                     "layer_ms_per_launch": slot_ms[SLOT[mode]] / launches[SLOT[mode]]}
    m = res["f32"]["step_medians_ms"]
    res["f32_spread_ms"] = max(m) - min(m)
    res["f16_over_f32"] = res["f16"]["step_ms"] / res["f32"]["step_ms"]
    res["layer_f16_over_f32"] = res["f16"]["layer_ms_per_launch"] / res["f32"]["layer_ms_per_launch"]
    res["faster_by_more_than_twice_the_spread"] = res["f32"]["step_ms"] - res["f16"]["step_ms"] > 2 * res["f32_spread_ms"]
    return res


def main():
    out_path = sys.argv[1]
    graphs = int(sys.argv[sys.argv.index("--graphs") + 1]) if "--graphs" in sys.argv else 1 << 16
    b = gp.synth_molhiv_batch(graphs, seed=1234)
    vn = weights.synth_gin_virtual_node(seed=11, emb_dim=300)
    vn["w1"] = vn["w1"] * np.float32(1.0 / 64)
    e = Engine("GIN", 0)
    e.set_emb_dim(300)
    e.set_weights(weights.synth_gin_weights(seed=7, emb_dim=300))
    e.set_batch(b)
    e.profile_enable(True)
    res = {"graphs": graphs, "nodes": b.total_nodes, "edges": b.total_edges, "turns": TURNS, "runs": RUNS}
    res["virtual_node_off"] = measure(e)
    e.set_ogb_virtual_node(vn)
    res["virtual_node_on"] = measure(e)
    e.close()
    for k in ("virtual_node_off", "virtual_node_on"):
        r = res[k]
        for mode in ("f32", "f16"):
            print(f"{k}, {mode}: {r[mode]['step_ms']:.3f} ms (medians {['%.3f' % m for m in r[mode]['step_medians_ms']]}), "
                  f"{SLOT[mode]} {r[mode]['layer_ms_per_launch']:.3f} ms per launch: {r[mode]['slots_ms']}", flush=True)
        print(f"{k}: f16 / f32 = {r['f16_over_f32']:.3f} (layer launches {r['layer_f16_over_f32']:.3f}), f32 spread {r['f32_spread_ms']:.3f} ms, "
              f"faster by more than twice the spread: {r['faster_by_more_than_twice_the_spread']}, re-runs {r['exact_reruns']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
