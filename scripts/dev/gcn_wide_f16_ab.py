"""GCN at width 300, FLOWGNN_NUMERIC_F16 against the default mode (flowgnn.h: flowgnn_set_model_numeric_mode_dim).
usage: gcn_wide_f16_ab.py OUT.json [--graphs N]
scripts/dev/gin_wide_f16_ab.py for GCN.  One process, one batch of N = 2^16 molpcba-shaped graphs (the batch of scripts/dev/gcn_wide_ab.py),
one width-300 engine; the two modes alternate -- f32, f16, f32, f16, f32, f16 -- so that both see the same clocks, first with the
virtual node off, then with it on, then with JK sum and the residual on top of it.  A step's time is the device-event total of its
kernels (profile_read): the median of ten runs after two warm-up runs per turn, best of a mode's three turns.  The f32 medians' spread is
reported: the f16 step has to be faster than the f32 step by more than twice that spread for the ratio to mean anything.
The layer launches: the default mode has five under gcn_wide_layer (stages 0..3 and stage 4, which has no product); the f16 mode has
four under gcn_wide_layer_f16 and stage 4 under gcn_wide_layer.  Per launch the f16 slot is compared with the default mode's slot
less the f16 mode's stage 4 (the same kernel on the same rows), over four.  exact_reruns is reported and must be 0 (a re-run would time the
fp32 form); the virtual node's tensors are gcn_wide_vn_ab.py's."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402

TURNS, RUNS = 3, 10
F32_SLOT, F16_SLOT = "gcn_wide_layer", "gcn_wide_layer_f16"
STATES = (("virtual_node_off", False, "last", False), ("virtual_node_on", True, "last", False), ("virtual_node_jk_sum_residual", True, "sum", True))


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
        res[mode] = {"step_ms": t[best][0], "step_medians_ms": [x[0] for x in t], "slots_ms": slot_ms, "launches": launches}
    assert res["f32"]["launches"][F32_SLOT] == 5 and F16_SLOT not in res["f32"]["launches"], res["f32"]["launches"]
    assert res["f16"]["launches"][F16_SLOT] == 4 and res["f16"]["launches"][F32_SLOT] == 1, res["f16"]["launches"]
    final_ms = res["f16"]["slots_ms"][F32_SLOT]  # stage 4 alone
    res["f16"]["layer_ms_per_launch"] = res["f16"]["slots_ms"][F16_SLOT] / 4
    res["f32"]["layer_ms_per_launch"] = (res["f32"]["slots_ms"][F32_SLOT] - final_ms) / 4
    res["stage4_ms"] = final_ms
    m = res["f32"]["step_medians_ms"]
    res["f32_spread_ms"] = max(m) - min(m)
    res["f16_over_f32"] = res["f16"]["step_ms"] / res["f32"]["step_ms"]
    res["layer_f16_over_f32"] = res["f16"]["layer_ms_per_launch"] / res["f32"]["layer_ms_per_launch"]
    res["faster_by_more_than_twice_the_spread"] = res["f32"]["step_ms"] - res["f16"]["step_ms"] > 2 * res["f32_spread_ms"]
    return res


def main():
    out_path = sys.argv[1]
    graphs = int(sys.argv[sys.argv.index("--graphs") + 1]) if "--graphs" in sys.argv else 1 << 16
    b = gp.synth_molpcba_batch(graphs, seed=1234)
    vn = weights.synth_gcn_virtual_node(seed=13, emb_dim=300)
    vn["w1"] = vn["w1"] * np.float32(1.0 / 64)
    e = Engine("GCN", 0)
    e.set_model_emb_dim(300)
    e.set_weights(weights.synth_gcn_weights(seed=7, emb_dim=300))
    e.set_batch(b)
    e.profile_enable(True)
    res = {"graphs": graphs, "nodes": b.total_nodes, "edges": b.total_edges, "turns": TURNS, "runs": RUNS}
    for name, use_vn, jk, residual in STATES:
        e.set_gcn_virtual_node(vn if use_vn else None)
        e.set_jk_residual(jk, residual)
        res[name] = measure(e)
    e.close()
    for name, *_ in STATES:
        r = res[name]
        for mode in ("f32", "f16"):
            print(f"{name}, {mode}: {r[mode]['step_ms']:.3f} ms (medians {['%.3f' % m for m in r[mode]['step_medians_ms']]}), "
                  f"stages 0..3 {r[mode]['layer_ms_per_launch']:.3f} ms per launch: {r[mode]['slots_ms']}", flush=True)
        print(f"{name}: f16 / f32 = {r['f16_over_f32']:.3f} (layer launches {r['layer_f16_over_f32']:.3f}), f32 spread {r['f32_spread_ms']:.3f} ms, "
              f"faster by more than twice the spread: {r['faster_by_more_than_twice_the_spread']}, re-runs {r['exact_reruns']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
