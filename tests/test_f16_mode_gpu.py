"""The f16 numeric mode of GIN / GIN-VN (flowgnn.h: FLOWGNN_NUMERIC_F16): MLP operands rounded to f16 (round to nearest even),
one MFMA per product, fp32 accumulation -- the single-product instances of gin_split.hip's kernels.

The parity rule of the other tests cannot tell this mode from fp32 (its error is below 1e-4 (scale + |x|)), so the first test
pins the arithmetic itself: on a weight set of few-bit dyadic values every fp32 sum of the mode is exact (tests/f16_ref.py proves
it for the input), so the GPU must reproduce the float64 restatement with f16 casts at the operand points up to the final
divisions and additions of the readout, and must NOT reproduce the restatement without rounding (what fp32 computes) or with
rounding toward zero."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, graphpack as gp, weights
from tests import f16_ref
from tests.parity import assert_close, oracle_scale

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")


def probe_weights(seed=5, num_tasks=1, tight=False):
    """Dyadic weights of few significant bits: all positive MLP weights in {1/4, 1/2} (two per row), embeddings and biases on a
    2^-12 grid with 9..11 significant bits, a readout head of four entries in {+-1, +-1/2}.  Activations then carry bits below
    their f16 ulp (the roundings matter) while every fp32 sum stays exact (checked per input by f16_ref).
    tight (tests/f16_probe.py): the MLP weights times 1 - 2^-12 + 2^-20 -- after the kernels' power-of-two scale each lies just above
    the midpoint below a power of two, so rounded to nearest it IS the few-bit value of the plain set (every sum stays exact), while
    rounded toward zero or left unrounded it is not: the rounding of the weights shows, and through W2 that of the folded u = W2^T w."""
    rng = np.random.default_rng(seed)
    q = 2.0 ** -12
    f = lambda a: np.asarray(a, np.float32)

    def sparse(rows, cols, vals):
        w = np.zeros((rows, cols))
        for o in range(rows):
            w[o, rng.choice(cols, 2, replace=False)] = rng.choice(vals, 2)
        return w

    pw = np.zeros((num_tasks, 100))
    for t in range(num_tasks):
        pw[t, rng.choice(100, 4, replace=False)] = [1.0, -1.0, 0.5, -0.5]
    t = (1.0 - 2.0 ** -12 + 2.0 ** -20) if tight else 1.0
    return {
        "node_embedding_weight": f(rng.integers(2 ** 8, 2 ** 9, (173, 100)) * q),
        "edge_embedding_weight": f(rng.integers(-2 ** 7, 2 ** 7, (5, 13, 100)) * q),
        "node_mlp_1_weights": f(np.stack([sparse(200, 100, [0.25, 0.5]) for _ in range(5)]) * t),
        "node_mlp_1_bias": f(rng.integers(2 ** 10, 2 ** 11, (5, 200)) * q),
        "node_mlp_2_weights": f(np.stack([sparse(100, 200, [0.25]) for _ in range(5)]) * t),
        "node_mlp_2_bias": f(rng.integers(2 ** 10, 2 ** 11, (5, 100)) * q),
        "graph_pred_weights": f(pw),
        "graph_pred_bias": f(rng.integers(1, 2 ** 10, (num_tasks,)) * q),
    }


def probe_batch(vn, extra=False):
    """Molecules whose node count (with GIN-VN's virtual node) is a power of two: the mean pool's division is then exact too.
    extra (tests/f16_probe.py): a one-node graph in front, one behind, and a four-node graph without edges (three nodes under its
    virtual node) in the middle -- 1, 2 and 4 are powers of two as well."""
    big = gp.synth_molhiv_batch(1500, seed=11)
    sizes = {7, 15} if vn else {8, 16}
    parts = [big.slice(g, g + 1) for g in range(big.num_graphs) if int(big.nums_of_nodes[g]) in sizes]
    if extra:
        lone = lambda n, seed: gp.GraphBatch(np.array([n], np.int32), np.array([0], np.int32), big.node_feature[seed:seed + n].copy(),
                                             np.zeros((0, 2), np.int32), np.zeros((0, 3), np.int32))
        half = len(parts) // 2
        parts = [lone(1, 3)] + parts[:half] + [lone(3 if vn else 4, 40)] + parts[half:] + [lone(1, 90)]
    b = gp.concat_batches(parts)
    return gp.add_virtual_nodes(b) if vn else b


PATHS = {  # name: (model, options, num_tasks, readout rule of f16_ref)
    "one_pass": ("GIN", {}, 1, True),
    "per_layer": ("GIN", {"gin_resident": 0}, 1, False),
    "multi_task_csr": ("GIN", {}, 2, False),
    "gin_vn": ("GIN-VN", {}, 1, True),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_exactness_probe(path):
    model, opts, tasks, fold = PATHS[path]
    w = probe_weights(num_tasks=tasks)
    b = probe_batch(model == "GIN-VN")
    want, worst = f16_ref.gin_forward(b, w, fold=fold, rnd="rne", check=True)
    assert worst <= 24.0, f"fp32 would round on this input (2^{worst:.1f} > 2^24): the probe proves nothing"
    rtz, worst_rtz = f16_ref.gin_forward(b, w, fold=fold, rnd="rtz", check=True)
    assert worst_rtz <= 24.0
    plain = f16_ref.gin_forward(b, w, fold=fold, rnd="none")
    e = Engine(model, device=0, options=opts)
    if tasks != 1:
        e.set_num_tasks(tasks)
    e.set_weights(w)
    e.set_numeric_mode("f16")
    got = e.forward(b)
    e.set_numeric_mode("f32")
    f32 = e.forward(b)
    assert e.exact_reruns() == 0
    e.close()
    got, f32 = got.reshape(want.shape).astype(np.float64), f32.reshape(want.shape).astype(np.float64)
    bound = 1e-6 * (1.0 + np.abs(want))  # the readout's fp32 division by a power of two is exact; its final additions are not
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / bound).max())
    for other, name in ((f32, "f32 mode"), (rtz, "round toward zero")):
        sep = np.abs(got - other) / bound
        assert np.mean(sep > 100.0) > 0.5 and np.median(sep) > 100.0, (name, float(np.median(sep)), float(np.mean(sep > 100)))
    # control: the default mode computes the unrounded model (its fp32 roundings are not exact on this input: 1e-5)
    assert (np.abs(f32 - plain) <= 1e-5 * (1.0 + np.abs(plain))).all(), float(np.abs(f32 - plain).max())


@pytest.fixture(scope="module")
def molhiv4113():
    return gp.synth_molhiv_batch(4113, seed=13)


@pytest.mark.parametrize("model", ["GIN", "GIN-VN"])
@pytest.mark.parametrize("trained", [False, True])
def test_accuracy_at_dataset_size(model, trained, molhiv4113, oracle):
    if trained:
        import sys
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import make_ref_weights as mrw
        w = mrw.load("GIN")
    else:
        w = weights.synth_gin_weights(seed=7)
    b = gp.add_virtual_nodes(molhiv4113) if model == "GIN-VN" else molhiv4113
    want, hd = oracle.gin_forward(b, [w], dump_h=True, nthreads=8)
    e = Engine(model, device=0)
    e.set_weights(w)
    f32 = e.forward(b)
    reruns32 = e.exact_reruns()
    e.set_numeric_mode("f16")
    got = e.forward(b)
    reruns16 = e.exact_reruns() - reruns32
    e.close()
    assert_close(got, want, scale=oracle_scale(hd), rel=2e-4, what=(model, trained))
    if reruns32:
        # an activation of this batch leaves the f16 range in the default mode already (trained weights on GIN-VN: the virtual nodes'
        # sums): the f16 mode takes the same documented fallback -- the batch is re-run on the fp32 kernels, f32-mode results
        assert reruns16 == reruns32 and np.array_equal(got, f32)
    else:
        assert reruns16 == 0
        assert float(np.abs(got.astype(np.float64) - f32).max()) > 1e-5  # the mode did change the arithmetic


def test_bit_identity(molhiv4113):
    w = weights.synth_gin_weights(seed=7)
    b = molhiv4113.slice(0, 1200)
    e = Engine("GIN", device=0)
    e.set_weights(w)
    e.set_numeric_mode("f16")
    full = e.forward(b)
    # a slice computed as a shard of the whole job: the same kernels, the same bits
    e.set_job_totals(b.total_nodes, b.total_edges)
    part = e.forward(b.slice(300, 900))
    e.set_job_totals()
    assert np.array_equal(part, full[300:900])
    # f16 -> f32 -> f16: each mode reproduces itself
    e.set_numeric_mode("f32")
    f32 = e.forward(b)
    e.set_numeric_mode("f16")
    assert np.array_equal(e.forward(b), full)
    e.set_numeric_mode("f32")
    assert np.array_equal(e.forward(b), f32) and not np.array_equal(f32, full)
    e.close()
    # the mode set before the weights: the same bits
    e2 = Engine("GIN", device=0)
    e2.set_numeric_mode("f16")
    e2.set_weights(w)
    assert np.array_equal(e2.forward(b), full)
    e2.close()
    # a two-member group on one device = one engine
    g = EngineGroup("GIN", [0, 0])
    g.set_weights(w)
    g.set_numeric_mode("f16")
    assert np.array_equal(g.forward(b), full)
    g.close()
    # launch-sequence replay = direct launches
    h = Engine("GIN", device=0, options={"hipgraph": 1})
    h.set_weights(w)
    h.set_numeric_mode("f16")
    h.set_batch(b)
    outs = []
    for _ in range(4):
        h.run()
        outs.append(h.results().copy())
    assert h.graph_replays() >= 1
    assert all(np.array_equal(o, full) for o in outs)
    h.close()


def test_range_fallback(oracle, gin_weights):
    b = gp.synth_molhiv_batch(200, seed=21)
    big = dict(gin_weights)
    big["node_embedding_weight"] = gin_weights["node_embedding_weight"] * np.float32(1e5)
    e = Engine("GIN", device=0)
    e.set_weights(big)
    e.set_numeric_mode("f16")
    got, want = e.forward(b), oracle.gin_forward(b, [big])
    assert e.exact_reruns() == 1
    assert np.isfinite(got).all()
    assert np.allclose(got, want, rtol=1e-4, atol=1e-4 * np.abs(want).max()), np.abs(got - want).max()
    e.close()


@pytest.mark.parametrize("model", ["GCN", "GAT", "PNA", "DGN"])
def test_other_models_refuse(model):
    e = Engine(model, device=0)
    with pytest.raises(FlowGNNError) as ei:
        e.set_numeric_mode("f16")
    assert ei.value.code == 8
    e.close()


def test_speed_guard():
    """f16 mode cuts the graph-resident kernel's matrix work to a third: it must show (device events, same process, same batch)."""
    b = gp.synth_molhiv_batch(1 << 16, seed=3)
    e = Engine("GIN", device=0)
    e.set_weights(weights.synth_gin_weights(seed=7))
    e.set_batch(b)
    e.profile_enable(True)

    def median_ms(mode, runs=7):
        e.set_numeric_mode(mode)
        e.run()
        e.results()
        ms = []
        for _ in range(runs):
            t0 = e.profile_read()["gin_resident"]["total_ms"]
            e.run()
            e.results()
            ms.append(e.profile_read()["gin_resident"]["total_ms"] - t0)
        return float(np.median(ms))

    best = {"f32": np.inf, "f16": np.inf}
    for _ in range(3):
        for mode in ("f32", "f16"):
            best[mode] = min(best[mode], median_ms(mode))
    e.close()
    assert best["f16"] <= 0.85 * best["f32"], best


def test_host_cli(tmp_path):
    w = weights.synth_gin_weights(seed=7)
    b = gp.synth_molhiv_batch(40, seed=3)
    gdir, wdir, out = tmp_path / "graphs", tmp_path / "weights", tmp_path / "HLS_output.txt"
    gp.write_pack(b, str(gdir))
    weights.SAVERS["GIN"](w, str(wdir))
    r = subprocess.run([HOST, "GIN", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--numeric", "f16", "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    e = Engine("GIN", device=0)
    e.set_weights(w)
    e.set_numeric_mode("f16")
    want = e.forward(b).astype(np.float64)
    e.set_numeric_mode("f32")
    f32 = e.forward(b).astype(np.float64)
    e.close()
    assert np.abs(got - want).max() <= 1e-8 + 1e-8 * np.abs(want).max()  # the file's 8 decimals
    assert np.abs(got - f32).max() > 1e-6
