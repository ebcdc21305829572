"""Differential fuzz of one width-300 kernel instance: the seeded random batches of tests/wide_cases.py (graph sizes from the tile
edges and 1 .. 59, edgeless graphs, self loops, duplicate edges, all 60 edge codes, 1 .. 39 graphs) through the HIP path against the
float64 reference of tests/ogb_jk_torch.py / tests/ogb_gcn_jk_torch.py, plus two shards cut at a seeded graph index -- the generator,
the reference and the rule of tests/test_wide_shapes_gpu.py, for as many batches as asked.
usage: fuzz_wide.py INSTANCE COUNT SEED      (dev tool; INSTANCE: an id of tests.wide_cases.IDS, e.g. gcn-virtual-sum-res, or `all`)
Batch k of a run is random_batch(SEED * 1000 + k, family).  A batch whose largest guarded operand reaches 3e4 on the reference is
counted and not compared: the exact re-run would compute it, not the kernels under test.  Rule: |gpu - f64| <= 1e-4 (scale + |f64|) on
logits, graph embeddings, node embeddings and h_5; in f16 mode 2e-4 on the logits.  Prints FAIL ... seed ... iter ... with the batch's
shape and exits non-zero on the first miss."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tests import wide_cases as C  # noqa: E402
from tests.parity import err_ratio  # noqa: E402

F16_REL, REL = 2e-4, 1e-4  # tests/test_gin_wide_f16_gpu.py's and tests/parity.py's
OUTPUTS = ("logits", "pooled", "rows", "h5")


def outputs(e, b):
    logits, pooled, rows = (np.array(x) for x in e.forward(b, return_embeddings=True, return_node_embeddings=True))
    return logits, pooled, rows.reshape(b.total_nodes, 300), np.array(e.final_h()).reshape(b.total_nodes, 300)


def ratios(i, got, ref):
    """name -> err_ratio, for the outputs the rule is asserted on"""
    names = ("logits",) if i.f16 else OUTPUTS
    want = dict(logits=ref.logits, pooled=ref.pooled, rows=ref.rows, h5=ref.h5)
    return {n: (err_ratio(g, want[n], ref.scale, F16_REL if i.f16 else REL) if np.isfinite(g).all() else np.inf)
            for n, g in zip(OUTPUTS, got) if n in names}


def fuzz(i, count, seed0):
    fam, worst, skipped = C.family_of(i), 0.0, 0
    e = C.engine(i)
    try:
        for it in range(count):
            seed = seed0 * 1000 + it
            b = C.random_batch(seed, fam)
            ref = C.reference(i, b)
            if not ref.operands < C.RANGE_LIMIT:
                skipped += 1
                continue
            shape = f"graphs {b.num_graphs} nodes {b.total_nodes} edges {b.total_edges}"
            before = e.exact_reruns()
            whole = outputs(e, b)
            cut = C.shard_cut(seed, b)
            e.set_job_totals(b.total_nodes, b.total_edges)
            parts = [outputs(e, b.slice(lo, hi)) for lo, hi in ((0, cut), (cut, b.num_graphs)) if hi > lo]
            e.set_job_totals(-1, -1)
            joined = tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
            r, rs = ratios(i, whole, ref), ratios(i, joined, ref)
            same_bits = i.kind != "gin" or i.f16 or all(x.tobytes() == y.tobytes() for x, y in zip(whole, joined))
            reruns = e.exact_reruns() - before
            worst = max([worst] + list(r.values()) + list(rs.values()))
            if max(r.values()) > 1.0 or max(rs.values()) > 1.0 or not same_bits or reruns:
                print(f"FAIL {C.name_of(i)} seed {seed0} iter {it} (random_batch({seed}, {fam!r})): {shape} cut {cut} err_ratio {r} shards {rs} "
                      f"shards_same_bits {same_bits} exact_reruns {reruns} scale {ref.scale:.4g} operands {ref.operands:.4g}", flush=True)
                return 1
    finally:
        e.close()
    print(f"{C.name_of(i)}: {count - skipped} random batches ok ({skipped} out of range, not compared), worst err_ratio {worst:.4f}", flush=True)
    return 0


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    seed0 = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    todo = C.INSTANCES if which == "all" else [C.INSTANCES[C.IDS.index(which)]]
    for inst in todo:
        if fuzz(inst, count, seed0):
            sys.exit(1)
