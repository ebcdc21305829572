"""Phase prices of dgn_resident_kernel and dgn_resident_f16_kernel on one box: the shipped library against TIMING variants of both
(csrc/dev/dgn_timing_variants.h: -DFLOWGNN_DEV -DDGNR_TIMING=<bits> on dgn.hip AND dgn_f16.hip; wrong results on purpose), DESIGN.md
section 4.29.
usage: dgn_f16_phases.py OUT.json GRAPHS BASE.so [BITS=VARIANT.so ...]
Each library in a process of its own; in it the two modes alternate three times on one batch of hep10k-shaped graphs, and a mode's
figure is the device-event median of ten runs of the resident kernel's slot, best of three.  A phase's price is base - variant."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, %r)
import flowgnn_amd._lib as L
L.LIB_PATH = sys.argv[2]
from flowgnn_amd import Engine, graphpack as gp, weights
b = gp.synth_hep10k_batch(int(sys.argv[1]), seed=1234)
e = Engine("DGN", 0)
e.set_weights(weights.synth_dgn_weights(7)); e.set_batch(b); e.profile_enable(True)
best = {}
for _ in range(3):
    for mode, slot in (("f32", "dgn_resident"), ("f16", "dgn_resident_f16")):
        e.set_numeric_mode(mode, emb_dim=100)
        ms = []
        for i in range(12):
            t0 = e.profile_read().get(slot, {"total_ms": 0.0})["total_ms"]
            e.run(); e.sync()
            if i >= 2: ms.append(e.profile_read()[slot]["total_ms"] - t0)
        best[mode] = min(best.get(mode, 1e9), float(np.median(ms)))
best["exact_reruns"] = e.exact_reruns()
print(json.dumps(best))
''' % ROOT


def main():
    out_path, graphs, base = sys.argv[1:4]
    libs = [("base", base)] + [tuple(a.split("=", 1)) for a in sys.argv[4:]]
    res = {"graphs": int(graphs), "variants": {}}
    for name, lib in libs:
        p = subprocess.run([sys.executable, "-c", CHILD, graphs, os.path.abspath(lib)], capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            print(name, "failed:", p.stderr.strip()[-400:], flush=True)
            sys.exit(1)  # (nothing more is started on the GPU after a failure)
        res["variants"][name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(name, res["variants"][name], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
