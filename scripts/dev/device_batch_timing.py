"""flowgnn_set_batch (host arrays) against flowgnn_set_batch_device (PyG int64 / reference int32 arrays already on the GPU), GIN,
2^18 molhiv-shaped graphs by default.  Wall times with the profiler off, each call ending in flowgnn_sync, after warm-up (the median
of --reps calls); the end-to-end "batch on the device -> logits in a device tensor" rate (forward_device + one synchronisation);
the bytes the PyG ingest must move, from the shapes.  Prints one JSON line (and writes it to --json).

  --ingest-only: only PyG set_batch_device calls (for a `rocprofv3 --kernel-trace --stats` run of the ingest kernel, which is
                 named fg::ingest_pyg_kernel).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from flowgnn_amd import Engine, graphpack as gp, weights  # noqa: E402


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ingest-only", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()

    b = gp.synth_molhiv_batch(a.graphs, seed=1234)
    N, E, G = b.total_nodes, b.total_edges, b.num_graphs
    e = Engine("GIN", device=0)
    e.set_weights(weights.synth_gin_weights(seed=7))
    dev = torch.device("cuda", 0)
    d = b.to_pyg(dev)
    ref = {"x": torch.from_numpy(b.node_feature).to(dev), "edge_list": torch.from_numpy(b.edge_list).to(dev),
           "edge_attr": torch.from_numpy(b.edge_attr).to(dev)}
    nn, ne = b.nums_of_nodes, b.nums_of_edges
    torch.cuda.synchronize()

    def dev_pyg():
        e.set_batch_device_ptrs(nn, ne, "pyg", d["x"].data_ptr(), d["edge_index"].data_ptr(), d["edge_attr"].data_ptr())
        e.sync()

    def dev_ref():
        e.set_batch_device_ptrs(nn, ne, "reference", ref["x"].data_ptr(), ref["edge_list"].data_ptr(), ref["edge_attr"].data_ptr())
        e.sync()

    def host():
        e.set_batch(b)
        e.sync()

    if a.ingest_only:
        for _ in range(a.warmup + a.reps):
            dev_pyg()
        print(json.dumps({"ingest_only": True, "graphs": G, "calls": a.warmup + a.reps}))
        return

    for fn in (host, dev_pyg, dev_ref):
        for _ in range(a.warmup):
            fn()
    res = {"graphs": G, "nodes": N, "edges": E}
    res["set_batch_host_ms"] = median_ms(host, a.reps)
    res["set_batch_device_pyg_ms"] = median_ms(dev_pyg, a.reps)
    res["set_batch_device_reference_ms"] = median_ms(dev_ref, a.reps)
    res["set_batch_host_ms_again"] = median_ms(host, a.reps)  # (the spread of the box: host path measured twice, around the others)

    # the ingest kernel alone, by the engine's profiler (events around it; a separate pass, profiler off above)
    e.profile_enable(True)
    for _ in range(a.reps):
        dev_pyg()
    p = e.profile_read().get("ingest", {"total_ms": float("nan"), "launches": 1})
    e.profile_enable(False)
    res["ingest_event_ms"] = p["total_ms"] / max(p["launches"], 1)

    # end to end: PyG tensors on the device -> logits in a device tensor
    def e2e():
        e.forward_device(d["x"], d["edge_index"], d["edge_attr"], ptr=d["ptr"], nums_of_edges=ne)
        torch.cuda.synchronize()
    for _ in range(a.warmup):
        e2e()
    ms = median_ms(e2e, a.reps)
    res["forward_device_ms"] = ms
    res["forward_device_graphs_per_s"] = G / (ms * 1e-3)
    e.sync()
    out = e.forward_device(d["x"], d["edge_index"], d["edge_attr"], ptr=d["ptr"], nums_of_edges=ne)
    e.sync()
    res["forward_device_equals_host_path"] = bool(np.array_equal(out.cpu().numpy(), e.forward(b)))

    # what the PyG ingest must move: int64 in, int32 out
    rd = 8 * (N * 9 + 2 * E + 3 * E)
    wr = 4 * (N * 9 + 2 * E + 3 * E)
    res["ingest_bytes_read"] = rd
    res["ingest_bytes_written"] = wr
    res["ingest_min_ms_at_8TBps"] = (rd + wr) / 8e12 * 1e3
    res["ingest_event_TBps"] = (rd + wr) / (res["ingest_event_ms"] * 1e-3) / 1e12
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
