"""f32 against f16 numeric mode (flowgnn.h: FLOWGNN_NUMERIC_F16) on ONE batch in ONE process, the modes alternating.
usage: numeric_ab.py [rounds]   -- GIN at 2^18 and 4 113 molhiv graphs, GIN-VN at 2^18: per mode the best of `rounds` medians of the
gin_resident kernel (device events) and of the whole launch sequence (synchronised wall clock), graphs/s, and max |logit - oracle|
on a 256-graph slice (the oracle is the fp32 C restatement: the f16 mode's rounding error shows there)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402
from oracle import oracle  # noqa: E402


def measure(e, mode, runs=10):
    e.set_numeric_mode(mode)
    for _ in range(3):
        e.run()
    e.sync()
    kern, wall = [], []
    for _ in range(runs):
        k0 = e.profile_read().get("gin_resident", {"total_ms": 0.0})["total_ms"]
        t0 = time.perf_counter()
        e.run()
        e.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(e.profile_read().get("gin_resident", {"total_ms": 0.0})["total_ms"] - k0)
    return float(np.median(kern)), float(np.median(wall))


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    oracle.load()
    w = weights.synth_gin_weights(seed=7)
    for model, graphs in (("GIN", 1 << 18), ("GIN", 4113), ("GIN-VN", 1 << 18)):
        b = gp.synth_molhiv_batch(graphs, seed=1234)
        if model == "GIN-VN":
            b = gp.add_virtual_nodes(b)
        e = Engine(model, 0)
        e.set_weights(w)
        e.set_batch(b)
        e.profile_enable(True)
        best = {m: (np.inf, np.inf) for m in ("f32", "f16")}
        for _ in range(rounds):
            for mode in ("f32", "f16"):
                k, t = measure(e, mode)
                best[mode] = (min(best[mode][0], k), min(best[mode][1], t))
        sl = b.slice(0, 256)
        want = oracle.gin_forward(sl, [w], nthreads=8)
        err = {}
        for mode in ("f32", "f16"):
            e.set_numeric_mode(mode)
            err[mode] = float(np.abs(e.forward(sl).astype(np.float64) - want).max())
        e.close()
        for mode in ("f32", "f16"):
            k, t = best[mode]
            print(f"{model:6s} {graphs:7d} graphs  {mode}: gin_resident {k:8.3f} ms  launch {t:8.3f} ms  {graphs / t * 1e-3:8.3f} M graphs/s"
                  f"  max|d| vs oracle (256 graphs) {err[mode]:.2e}", flush=True)
        print(f"{model:6s} {graphs:7d} graphs  f16 / f32: gin_resident {best['f16'][0] / best['f32'][0]:.3f}  launch {best['f16'][1] / best['f32'][1]:.3f}",
              flush=True)


if __name__ == "__main__":
    main()
