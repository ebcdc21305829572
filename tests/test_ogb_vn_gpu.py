"""OGB's virtual node for GIN on the GPU (flowgnn.h: flowgnn_set_ogb_virtual_node; kernel: flowgnn_amd/csrc/gin_ogbvn.hip).

Expected values: the float64 forward of tests/ogb_vn_ref.py (with the five tensors zero it is tests/test_gin_eps.py's forward, which
reproduces tests/numpy_ref.py and the oracle; the oracle itself has no such model).  Tolerance: the project's rule and nothing else,
|gpu - want| <= rel (scale + |want|), rel = 1e-4 in f32 mode and 2e-4 in f16 mode (tests/test_gin_eps.py), scale = the largest
activation of the float64 forward, t and the virtual node's hidden vector included; node-embedding rows by the same rule.  Every
comparison prints its worst ratio to the bound.

The fixed input is tests/test_gin_eps.py's batch and weights (head x 8) with ogb_vn_ref.fixed_virtual_node(); tests/test_ogb_vn_cpu.py
shows that it moves more than a quarter of the logits by more than 10 x the bound under every wrong form of the definition."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, export, graphpack as gp, weights
from tests import ogb_vn_ref as R
from tests.parity import REL, assert_close, err_ratio
from tests.test_embeddings_gpu import launched
from tests.test_gin_eps import EPS, REL_F16, fixed_batch, fixed_weights, one_node
from tests.test_resident_limits_gpu import random_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
GPW = 16    # graphs per workgroup of gin_ogbvn_kernel (flowgnn_amd/csrc/gin_ogbvn.h: GIN_OGBVN_GPW)
BIG = 128   # a graph of more nodes is walked by the whole workgroup (GIN_OGBVN_BIG)
PER_SLOTS = {"gin_layer_fused", "gin_aggregate", "gin_mlp"}
SLOT = "gin_ogb_vn"
f64 = lambda a: np.asarray(a, dtype=np.float64)
rel_of = lambda numeric: REL_F16 if numeric == "f16" else REL


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


class Ref:
    def __init__(self, b, w, vn, eps=None, pooling="mean", num_tasks=1):
        self.b, self.w, self.vn, self.eps = b, w, vn, eps
        self.want, self.rows, self.scale = R.forward(b, w, vn, eps=eps, pooling=pooling, num_tasks=num_tasks)
        self.starts = b.node_offsets()[:-1]


@pytest.fixture(scope="module")
def ref():
    """eps on / off -> Ref on the fixed input, computed once and left unchanged"""
    out = {}

    def get(eps_on):
        if eps_on not in out:
            out[eps_on] = Ref(fixed_batch("GIN"), fixed_weights(), R.fixed_virtual_node(), EPS if eps_on else None)
        return out[eps_on]
    return get


def close(got, want, scale, rel, what):
    print(what, f"worst ratio to the bound {err_ratio(got, want, scale, rel):.3f}")
    assert_close(got, want, scale=scale, rel=rel, what=what)


def make(w, vn, eps=None, options=None, numeric=None, num_tasks=1, pooling=None):
    e = Engine("GIN", device=0, options=options or {})
    if num_tasks != 1:
        e.set_num_tasks(num_tasks)
    e.set_weights(w)
    if numeric:
        e.set_numeric_mode(numeric)
    if pooling:
        e.set_pooling(pooling)
    if eps is not None:
        e.set_gin_eps(eps)
    if vn is not None:
        e.set_ogb_virtual_node(vn)
    e.profile_enable(True)
    return e


def run_checked(r, what, rel=REL, expect_reruns=0, fwd=None, **kw):
    """One forward of r.b on a fresh engine: the virtual node's slot and the per-layer kernels ran, the resident one did not."""
    e = make(r.w, r.vn, r.eps, **kw)
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(r.b, **(fwd or {}))))
    reruns = e.exact_reruns()
    e.close()
    assert SLOT in names and names & PER_SLOTS and "gin_resident" not in names and "gin_tile_build" not in names, (what, names)
    if expect_reruns is not None:
        assert reruns == expect_reruns, (what, reruns)
    return res["got"]


# ---------------------------------------------------------------- 1. parity on the fixed input
@pytest.mark.parametrize("numeric", ["f32", "f16"])
@pytest.mark.parametrize("eps_on", [False, True])
def test_parity_on_the_fixed_input(eps_on, numeric, ref):
    r = ref(eps_on)
    e = make(r.w, r.vn, r.eps, numeric=numeric)
    assert e.ogb_virtual_node() is True
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(r.b)))
    reruns = e.exact_reruns()
    prof = e.profile_read()
    e.close()
    assert SLOT in names and names & PER_SLOTS and "gin_resident" not in names, names
    assert prof[SLOT]["launches"] == 5  # one per layer, the last one included
    assert reruns == 0
    close(res["got"], r.want, r.scale, rel_of(numeric), ("fixed input, eps", eps_on, numeric))


# ---------------------------------------------------------------- 2. shapes where the kernel can go wrong
def tiny_next_to_large():
    sizes = [(1, 0), (2, 2), (3, 4), (4, 6), (5, 8), (300, 640), (2048, 4400), (BIG, 270), (BIG + 1, 270)]
    gs = [one_node(5) if n == 1 else random_graph(n, e, seed=60 + n % 17) for n, e in sizes]
    return gp.concat_batches(gs[:3] + [gs[6]] + gs[3:6] + gs[7:])  # the 2 048-node graph in the middle of a workgroup's run


SHAPES = [(f"G = {g}", lambda g=g: gp.synth_molhiv_batch(g, seed=30 + g)) for g in (1, GPW - 1, GPW, GPW + 1, 2 * GPW + 1)]
SHAPES += [("one-node edgeless graphs only", lambda: gp.concat_batches([one_node(s) for s in range(GPW + 3)])),
           ("1..5 nodes next to 300 and 2 048", tiny_next_to_large),
           ("2 000 ragged molhiv-shaped graphs", lambda: gp.synth_molhiv_batch(2000, seed=21))]


@pytest.mark.parametrize("name,batch", SHAPES, ids=[n for n, _ in SHAPES])
def test_shapes(name, batch):
    r = Ref(batch(), fixed_weights(), R.fixed_virtual_node(), EPS)
    # (a 2 048-node graph's t is a sum of 2 048 rows: such a batch may leave the f16 split's range and take the exact re-run -- either
    # way the virtual node must have been applied, which the comparison shows)
    logits, rows = run_checked(r, name, expect_reruns=None if r.scale >= 6.0e4 else 0, fwd={"return_node_embeddings": True})
    close(rows, r.rows, r.scale, REL, (name, "node-embedding rows"))
    close(logits, r.want, r.scale, REL, (name, "logits"))


# ---------------------------------------------------------------- 3. every other configuration computes with it
OTHER = [("graph embeddings", dict(fwd={"return_embeddings": True})),
         ("node embeddings", dict(fwd={"return_node_embeddings": True})),
         ("node logits", dict(fwd={"return_node_logits": True})),
         ("pooling sum", dict(pooling="sum")),
         ("pooling max", dict(pooling="max")),
         ("NUM_TASK 2", dict(num_tasks=2)),
         ("gin_resident 0", dict(options={"gin_resident": 0})),
         ("gin_mfma 32", dict(options={"gin_mfma": 32})),
         ("gin_unfused 1", dict(options={"gin_unfused": 1}, eps_on=False))]


@pytest.mark.parametrize("name,cfg", OTHER, ids=[n for n, _ in OTHER])
def test_other_configurations_compute_with_it(name, cfg, ref):
    tasks, pooling, fwd = cfg.get("num_tasks", 1), cfg.get("pooling"), cfg.get("fwd", {})
    eps_on = cfg.get("eps_on", True)
    if tasks != 1 or pooling:
        r = Ref(fixed_batch("GIN"), fixed_weights(tasks), R.fixed_virtual_node(), EPS, pooling=pooling or "mean", num_tasks=tasks)
    else:
        r = ref(eps_on)
    got = run_checked(r, name, fwd=fwd, options=cfg.get("options"), num_tasks=tasks, pooling=pooling)
    got = got if isinstance(got, tuple) else (got,)
    close(got[0], r.want, r.scale, REL, (name, "logits"))
    if fwd.get("return_embeddings"):
        close(got[1], np.add.reduceat(r.rows, r.starts, axis=0) / f64(r.b.nums_of_nodes)[:, None], r.scale, REL, (name, "embeddings"))
    if fwd.get("return_node_embeddings"):
        close(got[1], r.rows, r.scale, REL, (name, "node-embedding rows"))
    if fwd.get("return_node_logits"):
        W, pb = f64(r.w["graph_pred_weights"]).reshape(-1, 100), f64(r.w["graph_pred_bias"]).reshape(-1)
        close(got[1], (r.rows @ W.T + pb)[:, 0], r.scale, REL, (name, "node logits"))


def test_range_rerun_keeps_the_virtual_node(gin_weights):
    """Operands beyond the f16 split's range: the pass is repeated on the exact kernels from the encoder on, virtual node included."""
    b = gp.synth_molhiv_batch(200, seed=21)
    big = dict(gin_weights)
    big["node_embedding_weight"] = gin_weights["node_embedding_weight"] * np.float32(1e5)
    r = Ref(b, big, R.fixed_virtual_node(), EPS)
    logits, rows = run_checked(r, "range re-run", expect_reruns=1, fwd={"return_node_embeddings": True})
    close(rows, r.rows, r.scale, REL, "range re-run, node-embedding rows")
    close(logits, r.want, r.scale, REL, "range re-run, logits")


def test_device_batches_and_group_give_the_same_bits(ref):
    r = ref(True)
    e = make(r.w, r.vn, r.eps)
    want = e.forward(r.b)
    close(want, r.want, r.scale, REL, "one engine")
    try:
        pytest.importorskip("torch")
        from tests.test_device_batch_gpu import device_args
        for layout in ("pyg", "reference"):
            args, kw = device_args(r.b, layout, "GIN")
            got = e.forward_device(*args, **kw)
            e.sync()
            assert np.array_equal(got.cpu().numpy(), want), layout
    finally:
        e.close()
    g = EngineGroup("GIN", [0, 0])
    g.set_weights(r.w)
    g.set_gin_eps(EPS)
    g.set_ogb_virtual_node(r.vn)
    got = g.forward(r.b)
    g.set_ogb_virtual_node(None)
    off = g.forward(r.b)
    g.close()
    assert np.array_equal(got, want)  # each graph's bits do not depend on where the group cuts the batch
    assert not np.array_equal(off, want)


def test_host_cli(tmp_path):
    sd = R.vn_state_dict()
    b = gp.synth_molhiv_batch(40, seed=3)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    export.export_weights("GIN", sd, str(wdir), keep_eps=True, virtual_node=True)
    w, eps, vn = weights.load_gin_weights(str(wdir)), weights.load_gin_eps(str(wdir)), weights.load_gin_virtual_node(str(wdir))
    outs = {}
    for flags in (("--eps", "--ogb-vn"), ("--eps",)):
        out = tmp_path / f"HLS_output_{len(flags)}.txt"
        p = subprocess.run([HOST, "GIN", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--out", str(out)] + list(flags),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        outs[flags] = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    with_vn, without = Ref(b, w, vn, eps), Ref(b, w, R.zero_virtual_node(), eps)
    close(outs[("--eps", "--ogb-vn")], with_vn.want, with_vn.scale, REL, "host --eps --ogb-vn")
    close(outs[("--eps", "--ogb-vn")], R.ogb_vn_forward(sd, b), with_vn.scale, REL, "host --eps --ogb-vn against the state_dict's own forward")
    close(outs[("--eps",)], without.want, without.scale, REL, "host --eps")
    assert err_ratio(outs[("--eps",)], with_vn.want, with_vn.scale, REL) > 10.0  # the two are different models at this tolerance
    e = Engine("GIN", device=0)  # ... and the Python wrapper's route to the same files
    e.load_weights_dir(str(wdir), eps=True, virtual_node=True)
    assert e.ogb_virtual_node() is True
    got = e.forward(b)
    e.close()
    close(got, with_vn.want, with_vn.scale, REL, "load_weights_dir(eps=True, virtual_node=True)")


# ---------------------------------------------------------------- 4. plumbing apart from arithmetic
@pytest.mark.parametrize("numeric", ["f32", "f16"])
def test_zero_tensors_give_the_per_layer_bits(numeric):
    """x + 0 == x and relu(0) == 0: five zero tensors against the same engine with gin_resident 0 and the virtual node off."""
    b, w = fixed_batch("GIN"), fixed_weights()
    plain = make(w, None, EPS, options={"gin_resident": 0}, numeric=numeric)
    want = plain.forward(b)
    assert plain.ogb_virtual_node() is False
    plain.close()
    e = make(w, R.zero_virtual_node(), EPS, numeric=numeric)
    names = launched(e, lambda: e.forward(b))
    got = e.results().copy()
    on = e.ogb_virtual_node()
    e.close()
    assert on is True and SLOT in names and "gin_resident" not in names  # on is a state, not a value
    assert np.array_equal(got, want), float(np.abs(got - want).max())


# ---------------------------------------------------------------- 5. off means off
def test_off_means_off(ref):
    r = ref(False)
    fresh = make(r.w, None)
    names_fresh = launched(fresh, lambda: fresh.forward(r.b))
    want = fresh.results().copy()
    fresh.close()
    assert "gin_resident" in names_fresh and SLOT not in names_fresh
    e = make(r.w, None)
    e.set_batch(r.b)
    res = {}
    n0 = launched(e, lambda: (e.run(), res.update(first=e.results().copy())))
    e.set_ogb_virtual_node(r.vn)  # changed between runs on a resident batch
    n1 = launched(e, lambda: (e.run(), res.update(on=e.results().copy())))
    e.set_weights(r.w)            # it holds across flowgnn_set_weights ...
    e.set_batch(r.b)              # ... and across batches
    assert e.ogb_virtual_node() is True
    n1b = launched(e, lambda: (e.run(), res.update(on_again=e.results().copy())))
    e.set_ogb_virtual_node(None)
    assert e.ogb_virtual_node() is False
    n2 = launched(e, lambda: (e.run(), res.update(off=e.results().copy())))
    e.close()
    assert np.array_equal(res["first"], want) and np.array_equal(res["off"], want)
    assert n0 == names_fresh and n2 == names_fresh, (n0, n2, names_fresh)
    assert SLOT in n1 and SLOT in n1b and "gin_resident" not in n1 and "gin_resident" not in n1b, (n1, n1b)
    close(res["on"], r.want, r.scale, REL, "set on a resident batch")
    assert np.array_equal(res["on_again"], res["on"]) and not np.array_equal(res["on"], want)


# ---------------------------------------------------------------- 6. order independence
def test_a_permuted_batch_gives_each_graph_the_same_bits(ref):
    r = ref(True)
    big = gp.concat_batches([r.b, random_graph(BIG + 70, 420, seed=3), random_graph(BIG + 1, 300, seed=4)])
    G = big.num_graphs
    perm = np.random.default_rng(5).permutation(G)
    shuffled = gp.concat_batches([big.slice(int(i), int(i) + 1) for i in perm])
    e = make(r.w, r.vn, r.eps)
    a_logits, a_rows = e.forward(big, return_node_embeddings=True)
    a_logits, a_rows = a_logits.copy(), a_rows.copy()
    b_logits, b_rows = e.forward(shuffled, return_node_embeddings=True)
    part = e.forward(big.slice(7, 7 + GPW + 2), return_node_embeddings=True)  # a slice: other workgroup slots, other neighbours
    e.close()
    assert np.array_equal(b_logits, a_logits[perm])
    off, soff = big.node_offsets(), shuffled.node_offsets()
    for k, i in enumerate(perm):
        assert np.array_equal(b_rows[soff[k]:soff[k + 1]], a_rows[off[i]:off[i + 1]]), (k, i)
    assert np.array_equal(part[0], a_logits[7:7 + GPW + 2]) and np.array_equal(part[1], a_rows[off[7]:off[7 + GPW + 2]])


# ---------------------------------------------------------------- 7. refusals, and a recorded launch sequence is dropped
def refused(fn, code=8):
    with pytest.raises(FlowGNNError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_refusals(ref):
    r = ref(False)
    for model in ("GIN-VN", "GCN"):
        g = Engine(model, device=0)
        assert "GIN" in refused(lambda: g.set_ogb_virtual_node(r.vn))
        assert g.ogb_virtual_node() is False
        g.close()
    e = make(r.w, None)
    bad = dict(r.vn)
    bad["w2"] = r.vn["w2"].copy()
    bad["w2"][3, 99, 199] = np.nan
    assert "finite" in refused(lambda: e.set_ogb_virtual_node(bad), code=1)
    bad["w2"][3, 99, 199] = np.inf
    assert "finite" in refused(lambda: e.set_ogb_virtual_node(bad), code=1)
    p = [r.vn[k].ctypes.data_as(e.lib.flowgnn_set_ogb_virtual_node.argtypes[1]) for k in r.vn]
    assert e.lib.flowgnn_set_ogb_virtual_node(e._h, p[0], p[1], None, p[3], p[4]) == 1  # some but not all
    assert e.lib.flowgnn_set_ogb_virtual_node(e._h, None, None, None, None, p[4]) == 1
    assert e.ogb_virtual_node() is False
    # the fixed-point mode, in both orders
    e.set_numeric_mode("q6.10")
    assert "fixed-point" in refused(lambda: e.set_ogb_virtual_node(r.vn))
    e.set_ogb_virtual_node(None)  # off is always accepted
    e.set_numeric_mode("f32")
    e.set_ogb_virtual_node(r.vn)
    assert "virtual node" in refused(lambda: e.set_numeric_mode("q6.10"))
    e.set_numeric_mode("f16")
    e.set_numeric_mode("f32")
    # the stand-alone aggregation kernel does not add it
    e.forward(r.b)
    assert "virtual node" in refused(lambda: e.aggregation_only_ms(0, 1))
    assert "virtual node" in refused(lambda: e.aggregate(0))
    e.set_ogb_virtual_node(None)
    assert e.aggregation_only_ms(0, 1) > 0.0
    e.close()
    v = EngineGroup("GIN-VN", [0, 0])
    refused(lambda: v.set_ogb_virtual_node(r.vn))
    v.close()


def test_hipgraph_replay_is_dropped(ref):
    r = ref(False)
    want = make(r.w, r.vn)
    expected = want.forward(r.b)
    want.close()
    h = Engine("GIN", device=0, options={"hipgraph": 1})
    h.set_weights(r.w)
    h.set_batch(r.b)
    for _ in range(3):
        h.run()
    plain = h.results().copy()
    assert h.graph_replays() >= 1
    h.set_ogb_virtual_node(r.vn)
    h.run()
    first = h.results().copy()
    before = h.graph_replays()
    outs = []
    for _ in range(3):
        h.run()
        outs.append(h.results().copy())
    assert h.graph_replays() > before  # the new sequence (five more launches) is recorded and replayed in its turn
    h.close()
    assert np.array_equal(first, expected) and not np.array_equal(first, plain)
    assert all(np.array_equal(o, expected) for o in outs)
    close(first, r.want, r.scale, REL, "hipgraph, the run after set_ogb_virtual_node")
