"""OGB's virtual node for GCN on the GPU (flowgnn.h: flowgnn_set_gcn_virtual_node; kernels: the VN instance of gcn_layer_fused_kernel
in flowgnn_amd/csrc/gcn.hip, gcn_ogbvn.hip, and gin_ogbvn.hip for the configurations that do not fuse).

Expected values: the float64 forward of tests/gcn_vn_ref.py (with the five tensors zero it is tests/numpy_ref.gcn_forward; the oracle
has no such model).  Tolerance: the project's rule and nothing else, |gpu - want| <= REL (scale + |want|), REL = 1e-4, scale = the
largest activation of the float64 forward, t and the virtual node's hidden vector included; rows by the same rule.  Every comparison
prints its worst ratio to the bound.

The fixed input is gcn_vn_ref.fixed_batch / fixed_weights / fixed_virtual_node; tests/test_gcn_vn_cpu.py shows that it moves at least
half of the logits by more than 10 x the bound under every wrong form of the definition."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, export, graphpack as gp, weights
from tests import gcn_vn_ref as R
from tests.parity import REL, assert_close, err_ratio
from tests.test_embeddings_gpu import launched
from tests.test_gin_eps import one_node
from tests.test_resident_limits_gpu import random_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
FUSED_SLOT, IN_PLACE_SLOT = "gcn_ogb_vn", "gin_ogb_vn"
f64 = lambda a: np.asarray(a, dtype=np.float64)


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
    def __init__(self, b, w, vn, pooling="mean", num_tasks=1):
        self.b, self.w, self.vn = b, w, vn
        self.want, self.rows, self.scale, self.x4 = R.forward(b, w, vn, pooling=pooling, num_tasks=num_tasks, return_x4=True)
        self.starts = b.node_offsets()[:-1]


@pytest.fixture(scope="module")
def ref():
    """the fixed input's reference, computed once and left unchanged"""
    return Ref(R.fixed_batch(), R.fixed_weights(), R.fixed_virtual_node())


def close(got, want, scale, what):
    print(what, f"worst ratio to the bound {err_ratio(got, want, scale, REL):.3f}")
    assert_close(got, want, scale=scale, rel=REL, what=what)


def make(w, vn, options=None, num_tasks=1, pooling=None):
    e = Engine("GCN", device=0, options=options or {})
    if num_tasks != 1:
        e.set_num_tasks(num_tasks)
    e.set_weights(w)
    if pooling:
        e.set_pooling(pooling)
    if vn is not None:
        e.set_gcn_virtual_node(vn)
    e.profile_enable(True)
    return e


def run_checked(r, what, slot=FUSED_SLOT, expect_reruns=0, fwd=None, **kw):
    """One forward of r.b on a fresh engine: the virtual node's slot ran, the resident kernel did not."""
    e = make(r.w, r.vn, **kw)
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(r.b, **(fwd or {}))))
    reruns = e.exact_reruns()
    e.close()
    assert slot in names and "gcn_resident" not in names and "gcn_tile_build" not in names, (what, names)
    assert reruns == expect_reruns, (what, reruns)
    return res["got"]


# ---------------------------------------------------------------- 1. parity on the fixed input, and the profile slots
def test_parity_on_the_fixed_input(ref):
    r = ref
    e = make(r.w, r.vn)
    assert e.gcn_virtual_node() is True and e.ogb_virtual_node() is False
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(r.b)))
    prof = e.profile_read()
    x4 = e.final_h()
    logits2, rows = e.forward(r.b, return_node_embeddings=True)
    reruns = e.exact_reruns()
    e.close()
    assert "gcn_resident" not in names and IN_PLACE_SLOT not in names, names
    assert prof[FUSED_SLOT]["launches"] == 4 and prof["gcn_layer_fused"]["launches"] == 5 and prof["gcn_encoder_dense"]["launches"] == 1, prof
    assert reruns == 0
    close(res["got"], r.want, r.scale, "fixed input, logits")
    close(x4, r.x4, r.scale, "fixed input, x_4 (flowgnn_get_h), vn_4 inside")
    close(rows, r.rows, r.scale, "fixed input, node-embedding rows")
    close(logits2, r.want, r.scale, "fixed input, logits beside the rows")


def test_fused_against_in_place_and_their_profile_slots(ref):
    r = ref
    got = {}
    for name, options, slot, count in (("fused", {}, FUSED_SLOT, 4), ("in place", {"gcn_unfused": 1}, IN_PLACE_SLOT, 5)):
        e = make(r.w, r.vn, options=options)
        names = launched(e, lambda: got.update({name: e.forward(r.b)}))
        prof = e.profile_read()
        e.close()
        assert prof[slot]["launches"] == count and "gcn_resident" not in names, (name, prof)
        assert (FUSED_SLOT if slot == IN_PLACE_SLOT else IN_PLACE_SLOT) not in names, (name, names)
        close(got[name], r.want, r.scale, (name, "logits"))
    print("fused vs in place, worst ratio to the bound", err_ratio(got["fused"], f64(got["in place"]), r.scale, REL))


# ---------------------------------------------------------------- 2. shapes where the tile logic can go wrong
def no_edges():
    b = gp.concat_batches([random_graph(n, n + 2, seed=70 + n) for n in (2, 15, 16, 17, 33, 5)] + [one_node(4)])  # ... their edges dropped
    return gp.GraphBatch(b.nums_of_nodes, np.zeros_like(b.nums_of_edges), b.node_feature, np.zeros((0, 2), np.int32), np.zeros((0, 3), np.int32))


SHAPES = [("G = 1, one node", lambda: one_node(5), IN_PLACE_SLOT),  # (no edge: the in-place form)
          ("sixteen one-node graphs and one edge", lambda: gp.concat_batches([one_node(s) for s in range(16)] + [random_graph(2, 2, seed=9)]), FUSED_SLOT),
          ("15, 16, 17, 33 nodes in a row", lambda: gp.concat_batches([random_graph(n, 2 * n, seed=50 + n) for n in (15, 16, 17, 33)]), FUSED_SLOT),
          ("1..5 nodes next to 128, 129, 300",
           lambda: gp.concat_batches([one_node(5)] + [random_graph(n, 2 * n, seed=60 + n % 17) for n in (2, 128, 3, 129, 4, 300, 5)]), FUSED_SLOT),
          ("the last graph ends mid-tile", lambda: gp.concat_batches([random_graph(n, 2 * n, seed=80 + n) for n in (16, 16, 7)]), FUSED_SLOT),
          ("no edge at all", no_edges, IN_PLACE_SLOT),
          ("more than 65 536 nodes, ragged", lambda: gp.synth_molhiv_batch(3000, seed=21), FUSED_SLOT)]


@pytest.mark.parametrize("name,batch,slot", SHAPES, ids=[n for n, _, _ in SHAPES])
def test_shapes(name, batch, slot):
    b = batch()
    if "65 536" in name:
        assert b.total_nodes > 65536, b.total_nodes  # 512 workgroups x 8 waves x 16 nodes: some wave takes a second tile
    r = Ref(b, R.fixed_weights(), R.fixed_virtual_node())
    assert r.scale < 6.0e4
    logits = run_checked(r, name, slot=slot)
    close(logits, r.want, r.scale, (name, "logits"))
    logits, rows = run_checked(r, name, slot=slot, fwd={"return_node_embeddings": True})
    close(rows, r.rows, r.scale, (name, "node-embedding rows"))
    close(logits, r.want, r.scale, (name, "logits beside the rows"))


# ---------------------------------------------------------------- 3. every other configuration computes with it
OTHER = [("graph embeddings", dict(fwd={"return_embeddings": True})),
         ("node embeddings", dict(fwd={"return_node_embeddings": True})),
         ("node logits", dict(fwd={"return_node_logits": True})),
         ("pooling sum", dict(pooling="sum")),
         ("pooling max", dict(pooling="max")),
         ("NUM_TASK 2", dict(num_tasks=2)),
         ("gcn_mfma 32", dict(options={"gcn_mfma": 32}, slot=IN_PLACE_SLOT)),
         ("gcn_resident 0", dict(options={"gcn_resident": 0}))]


@pytest.mark.parametrize("name,cfg", OTHER, ids=[n for n, _ in OTHER])
def test_other_configurations_compute_with_it(name, cfg, ref):
    tasks, pooling, fwd = cfg.get("num_tasks", 1), cfg.get("pooling"), cfg.get("fwd", {})
    if tasks != 1 or pooling:
        r = Ref(R.fixed_batch(), R.fixed_weights(tasks), R.fixed_virtual_node(), pooling=pooling or "mean", num_tasks=tasks)
    else:
        r = ref
    got = run_checked(r, name, slot=cfg.get("slot", FUSED_SLOT), fwd=fwd, options=cfg.get("options"), num_tasks=tasks, pooling=pooling)
    got = got if isinstance(got, tuple) else (got,)
    close(got[0], r.want, r.scale, (name, "logits"))
    if fwd.get("return_embeddings"):
        close(got[1], np.add.reduceat(r.rows, r.starts, axis=0) / f64(r.b.nums_of_nodes)[:, None], r.scale, (name, "embeddings"))
    if fwd.get("return_node_embeddings"):
        close(got[1], r.rows, r.scale, (name, "node-embedding rows"))
    if fwd.get("return_node_logits"):
        W, pb = f64(r.w["graph_pred_weights"]).reshape(-1, 100), f64(r.w["graph_pred_bias"]).reshape(-1)
        close(got[1], (r.rows @ W.T + pb)[:, 0], r.scale, (name, "node logits"))


def test_range_rerun_keeps_the_virtual_node():
    """x_1 = h_1 + vn_1 leaves the f16 split's range in the registers of the fused kernel's VN instance while every h stays small
    (gcn_vn_ref.range_virtual_node; tests/test_gcn_vn_cpu.py checks the reference): the flag trips there, and the pass is repeated on
    the exact kernels from the encoder on, in the in-place form.  The component is positive -- a negative one cannot be made: vn_l
    is behind a ReLU for l >= 1 and E never reaches those registers -- so this pins that the VN instance tracks the range of the
    SUM, not of relu(a) alone; the |.| beside it guards a sign that no tensors produce."""
    r = Ref(R.fixed_batch(), R.fixed_weights(), R.range_virtual_node())
    assert r.scale > 6.0e4
    e = make(r.w, r.vn)
    names = launched(e, lambda: e.forward(r.b, return_node_embeddings=True))
    logits, rows, reruns = e.results().copy(), e.node_embeddings(), e.exact_reruns()
    e.close()
    assert reruns == 1 and FUSED_SLOT in names and IN_PLACE_SLOT in names, (reruns, names)
    close(rows, r.rows, r.scale, "range re-run, node-embedding rows")
    close(logits, r.want, r.scale, "range re-run, logits")


# ---------------------------------------------------------------- 4. bit-identical
def test_two_runs_and_device_batches_give_the_same_bits(ref):
    r = ref
    e = make(r.w, r.vn)
    want = e.forward(r.b).copy()
    again = e.forward(r.b).copy()
    assert np.array_equal(again, want)
    close(want, r.want, r.scale, "one engine")
    try:
        pytest.importorskip("torch")
        from tests.test_device_batch_gpu import device_args
        for layout in ("pyg", "reference"):
            args, kw = device_args(r.b, layout, "GCN")
            got = e.forward_device(*args, **kw)
            e.sync()
            assert np.array_equal(got.cpu().numpy(), want), layout
    finally:
        e.close()


def test_zero_tensors_give_the_per_layer_bits(ref):
    """b_0 + W_0 0 == b_0 in double, a + 0 == a for a >= 0, relu(b) of zero biases == 0: five zero tensors against gcn_resident 0 with
    the virtual node off, bit for bit -- the arithmetic allows it."""
    b, w = ref.b, ref.w
    plain = make(w, None, options={"gcn_resident": 0})
    want = plain.forward(b).copy()
    assert plain.gcn_virtual_node() is False
    plain.close()
    e = make(w, R.zero_virtual_node())
    names = launched(e, lambda: e.forward(b))
    got = e.results().copy()
    on = e.gcn_virtual_node()
    e.close()
    assert on is True and FUSED_SLOT in names and "gcn_resident" not in names  # on is a state, not a value
    assert np.array_equal(got, want), float(np.abs(got - want).max())


def test_off_means_off(ref):
    r = ref
    fresh = make(r.w, None)
    names_fresh = launched(fresh, lambda: fresh.forward(r.b))
    want = fresh.results().copy()
    fresh.close()
    assert "gcn_resident" in names_fresh and FUSED_SLOT not in names_fresh and IN_PLACE_SLOT not in names_fresh
    e = make(r.w, None)
    e.set_batch(r.b)
    res = {}
    n0 = launched(e, lambda: (e.run(), res.update(first=e.results().copy())))
    e.set_gcn_virtual_node(r.vn)  # changed between runs on a resident batch
    n1 = launched(e, lambda: (e.run(), res.update(on=e.results().copy())))
    e.set_weights(r.w)            # it holds across flowgnn_set_weights ...
    e.set_batch(r.b)              # ... and across batches
    assert e.gcn_virtual_node() is True
    n1b = launched(e, lambda: (e.run(), res.update(on_again=e.results().copy())))
    e.set_gcn_virtual_node(None)
    assert e.gcn_virtual_node() is False
    n2 = launched(e, lambda: (e.run(), res.update(off=e.results().copy())))
    e.close()
    assert np.array_equal(res["first"], want) and np.array_equal(res["off"], want)
    assert n0 == names_fresh and n2 == names_fresh, (n0, n2, names_fresh)
    assert FUSED_SLOT in n1 and FUSED_SLOT in n1b and "gcn_resident" not in n1 and "gcn_resident" not in n1b, (n1, n1b)
    close(res["on"], r.want, r.scale, "set on a resident batch")
    assert np.array_equal(res["on_again"], res["on"]) and not np.array_equal(res["on"], want)


# ---------------------------------------------------------------- 5. within the bound only: the partial rows are cut at the batch's tiles
def test_a_permuted_batch_a_slice_and_a_group_agree_within_the_bound(ref):
    r = ref
    G = r.b.num_graphs
    perm = np.random.default_rng(5).permutation(G)
    shuffled = gp.concat_batches([r.b.slice(int(i), int(i) + 1) for i in perm])
    e = make(r.w, r.vn)
    b_logits = e.forward(shuffled).copy()
    part = e.forward(r.b.slice(7, 7 + 40)).copy()
    e.close()
    close(b_logits, r.want[perm], r.scale, "a permuted batch, per graph")
    close(part, r.want[7:7 + 40], r.scale, "a slice")
    g = EngineGroup("GCN", [0, 0])
    g.set_weights(r.w)
    g.set_gcn_virtual_node(r.vn)
    got = g.forward(r.b).copy()
    g.set_gcn_virtual_node(None)
    off = g.forward(r.b).copy()
    g.close()
    close(got, r.want, r.scale, "EngineGroup(GCN, [0, 0])")
    assert err_ratio(off, r.want, r.scale, REL) > 10.0


# ---------------------------------------------------------------- 6. files and the command-line host
def test_host_cli_and_load_weights_dir(tmp_path):
    sd = R.vn_state_dict()
    b = gp.synth_molhiv_batch(40, seed=3)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    export.export_weights("GCN", sd, str(wdir), virtual_node=True)
    w, vn = weights.load_gcn_weights(str(wdir)), weights.load_gcn_virtual_node(str(wdir))
    outs = {}
    for flags in (("--ogb-vn",), ()):
        out = tmp_path / f"HLS_output_{len(flags)}.txt"
        p = subprocess.run([HOST, "GCN", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--out", str(out)] + list(flags),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        outs[flags] = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    with_vn, without = Ref(b, w, vn), Ref(b, w, R.zero_virtual_node())
    close(outs[("--ogb-vn",)], with_vn.want, with_vn.scale, "host GCN --ogb-vn")
    close(outs[("--ogb-vn",)], R.ogb_vn_forward(sd, b), with_vn.scale, "host GCN --ogb-vn against the state_dict's own forward")
    close(outs[()], without.want, without.scale, "host GCN")
    assert err_ratio(outs[()], with_vn.want, with_vn.scale, REL) > 10.0  # the two are different models at this tolerance
    e = Engine("GCN", device=0)  # ... and the Python wrapper's route to the same files
    e.load_weights_dir(str(wdir), virtual_node=True)
    assert e.gcn_virtual_node() is True
    got = e.forward(b)
    e.close()
    close(got, with_vn.want, with_vn.scale, "load_weights_dir(virtual_node=True)")


# ---------------------------------------------------------------- 7. refusals, and a recorded launch sequence is dropped
def refused(fn, code=8):
    with pytest.raises(FlowGNNError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_refusals(ref):
    r = ref
    for model in ("GIN", "GIN-VN", "PNA", "DGN", "GAT"):
        g = Engine(model, device=0)
        assert "GCN" in refused(lambda: g.set_gcn_virtual_node(r.vn))
        assert g.gcn_virtual_node() is False
        g.close()
    e = make(r.w, None)
    assert "GIN" in refused(lambda: e.set_ogb_virtual_node(r.vn))  # GIN's call on a GCN engine stays refused
    bad = dict(r.vn)
    bad["w2"] = r.vn["w2"].copy()
    bad["w2"][3, 99, 199] = np.nan
    assert "finite" in refused(lambda: e.set_gcn_virtual_node(bad), code=1)
    bad["w2"][3, 99, 199] = np.inf
    assert "finite" in refused(lambda: e.set_gcn_virtual_node(bad), code=1)
    p = [r.vn[k].ctypes.data_as(e.lib.flowgnn_set_gcn_virtual_node.argtypes[1]) for k in r.vn]
    assert e.lib.flowgnn_set_gcn_virtual_node(e._h, p[0], p[1], None, p[3], p[4]) == 1  # some but not all
    assert e.lib.flowgnn_set_gcn_virtual_node(e._h, None, None, None, None, p[4]) == 1
    assert e.gcn_virtual_node() is False
    # the fixed-point mode, in both orders
    e.set_numeric_mode("q6.10")
    assert "fixed-point" in refused(lambda: e.set_gcn_virtual_node(r.vn))
    e.set_gcn_virtual_node(None)  # off is always accepted
    e.set_numeric_mode("f32")
    e.set_gcn_virtual_node(r.vn)
    assert "virtual node" in refused(lambda: e.set_numeric_mode("q6.10"))
    # the stand-alone aggregation kernel does not add it
    e.forward(r.b)
    assert "virtual node" in refused(lambda: e.aggregation_only_ms(0, 1))
    assert "virtual node" in refused(lambda: e.aggregate(0))
    e.set_gcn_virtual_node(None)
    assert e.aggregation_only_ms(0, 1) > 0.0
    e.close()
    v = EngineGroup("GIN", [0, 0])
    refused(lambda: v.set_gcn_virtual_node(r.vn))
    v.close()


def test_hipgraph_replay_is_dropped(ref):
    r = ref
    want = make(r.w, r.vn)
    expected = want.forward(r.b).copy()
    want.close()
    h = Engine("GCN", device=0, options={"hipgraph": 1})
    h.set_weights(r.w)
    h.set_batch(r.b)
    for _ in range(3):
        h.run()
    plain = h.results().copy()
    assert h.graph_replays() >= 1
    h.set_gcn_virtual_node(r.vn)
    h.run()
    first = h.results().copy()
    before = h.graph_replays()
    outs = []
    for _ in range(3):
        h.run()
        outs.append(h.results().copy())
    assert h.graph_replays() > before  # the new sequence is recorded and replayed in its turn
    h.close()
    assert np.array_equal(first, expected) and not np.array_equal(first, plain)
    assert all(np.array_equal(o, expected) for o in outs)
    close(first, r.want, r.scale, "hipgraph, the run after set_gcn_virtual_node")
