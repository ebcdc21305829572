"""Laplacian eigenvectors on the GPU (flowgnn.h: flowgnn_laplacian_eigen_device) beside the two things they are worth comparing with:
  (a) graphpack.laplacian_eigen, the dense float64 eigh per graph on the CPU, with 16 worker processes of one BLAS thread each;
  (b) the DGN step (flowgnn_run) of the same batch, fed the GPU's eigenvectors.
usage: eigen_ab.py OUT.json [--graphs N] [--cpu-only]
Batches: N = 2^16 hep10k-shaped and N molhiv-shaped graphs, PyG layout on the device.  The GPU figures are device events on the
torch's current stream around the whole call (the engine's launch stream is ordered between them) -- host-side plan, its upload and the three kernels -- best of three medians of ten
calls after two warm-up calls; the DGN step is the device-event total of its kernels (profile_read), same scheme.  The CPU runs
first, before the process opens the GPU (the workers are forked).  --cpu-only: rehearsal of (a) without a device."""
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flowgnn_amd import graphpack as gp  # noqa: E402

ROUNDS, RUNS, WORKERS = 3, 10, 16
_BATCH = None


def _one_blas_thread():
    try:
        import threadpoolctl
        threadpoolctl.threadpool_limits(1)
    except ImportError:
        pass


def _cpu_part(rng):
    return gp.laplacian_eigen(_BATCH.slice(*rng))


def cpu_seconds(batch):
    """graphpack.laplacian_eigen over WORKERS forked processes, contiguous graph ranges; the pool is up before the clock starts."""
    global _BATCH
    _BATCH = batch
    cuts = np.linspace(0, batch.num_graphs, 8 * WORKERS + 1).astype(int)
    with ProcessPoolExecutor(WORKERS, initializer=_one_blas_thread) as pool:
        list(pool.map(_cpu_part, [(0, 1)] * WORKERS))
        t0 = time.perf_counter()
        parts = list(pool.map(_cpu_part, list(zip(cuts[:-1], cuts[1:]))))
        dt = time.perf_counter() - t0
    assert sum(p.shape[0] for p in parts) == batch.total_nodes
    return dt


def up_to(b, limit):
    """The graphs of b with at most `limit` nodes, as a batch."""
    keep = b.nums_of_nodes <= limit
    nm, em = np.repeat(keep, b.nums_of_nodes), np.repeat(keep, b.nums_of_edges)
    return gp.GraphBatch(b.nums_of_nodes[keep], b.nums_of_edges[keep], b.node_feature[nm], b.edge_list[em], b.edge_attr[em])


def best_of_medians(fn):
    meds = [float(np.median([fn() for _ in range(RUNS)])) for _ in range(ROUNDS)]
    return min(meds), meds


def main():
    out_path = sys.argv[1]
    graphs = int(sys.argv[sys.argv.index("--graphs") + 1]) if "--graphs" in sys.argv else 1 << 16
    cpu_only = "--cpu-only" in sys.argv
    batches = {"hep10k": gp.synth_hep10k_batch(graphs, seed=1234, with_eigen=False), "molhiv": gp.synth_molhiv_batch(graphs, seed=1234)}
    res = {"graphs": graphs, "rounds": ROUNDS, "runs": RUNS, "cpu_workers": WORKERS, "batches": {}}
    for name, b in batches.items():
        dt = cpu_seconds(b)
        res["batches"][name] = {"nodes": b.total_nodes, "edges": b.total_edges, "cpu_eigh_ms": dt * 1e3,
                                "classes": [int((b.nums_of_nodes <= 32).sum()), int(((b.nums_of_nodes > 32) & (b.nums_of_nodes <= 64)).sum()),
                                            int(((b.nums_of_nodes > 64) & (b.nums_of_nodes <= 128)).sum()), int((b.nums_of_nodes > 128).sum())]}
        print(f"{name}: {graphs} graphs, {b.total_nodes} nodes: CPU eigh, {WORKERS} processes: {dt * 1e3:.1f} ms", flush=True)
    if not cpu_only:
        import torch
        from flowgnn_amd import Engine, weights
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: nothing to measure (--cpu-only rehearses the CPU side)")
        e = Engine("DGN", 0)
        e.set_weights(weights.synth_dgn_weights(seed=7))
        limit = e.lib.flowgnn_laplacian_eigen_max_nodes()
        for name, b in batches.items():
            r = res["batches"][name]
            b = up_to(b, limit)  # (a molecule batch has a few graphs beyond 128 nodes: not the eigensolver's)
            r["graphs_measured"] = b.num_graphs
            d = b.to_pyg("cuda:0")
            ei, ptr, ne = d["edge_index"], b.node_offsets(), b.nums_of_edges
            def call():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call.out = e.laplacian_eigen_device(ei, ptr=ptr, nums_of_edges=ne)  # (the engine's stream after torch's, torch's after it)
                t1.record()
                t1.synchronize()
                return t0.elapsed_time(t1)
            for _ in range(2):
                call()
            r["gpu_call_ms"], r["gpu_call_medians_ms"] = best_of_medians(call)
            eig = call.out
            # what was timed is right: the residual of the first 256 graphs over the tests' bound 8 max(n, 8) 2^-24
            got, no, eo, worst = eig.cpu().numpy(), b.node_offsets(), b.edge_offsets(), 0.0
            for g in range(min(256, b.num_graphs)):
                n = int(b.nums_of_nodes[g])
                L = gp.normalized_laplacian(n, b.edge_list[eo[g]:eo[g + 1]])
                v = got[no[g]:no[g + 1], :min(4, n)].astype(np.float64)
                lam = np.einsum("ik,ij,jk->k", v, L, v) / (v * v).sum(axis=0)
                worst = max(worst, float(np.abs(L @ v - v * lam).max() / (8 * max(n, 8) * 2.0 ** -24)))
            r["worst_residual_over_bound_first_256"] = worst
            x = d["x"]
            e.set_batch_device(x, ei, None, eig, ptr=ptr, nums_of_edges=ne)
            e.profile_enable(True)
            total = lambda: sum(v["total_ms"] for v in e.profile_read().values())

            def step():
                k0 = total()
                e.run()
                e.sync()
                return total() - k0
            for _ in range(2):
                step()
            r["dgn_step_ms"], r["dgn_step_medians_ms"] = best_of_medians(step)
            e.profile_enable(False)
            r["gpu_over_cpu"] = r["cpu_eigh_ms"] * r["graphs_measured"] / graphs / r["gpu_call_ms"]
            print(f"{name}: GPU call {r['gpu_call_ms']:.3f} ms (medians {['%.3f' % m for m in r['gpu_call_medians_ms']]}), "
                  f"{r['graphs_measured'] / r['gpu_call_ms'] * 1e3:.0f} graphs/s, {r['gpu_over_cpu']:.1f} x the CPU; DGN step {r['dgn_step_ms']:.3f} ms", flush=True)
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
