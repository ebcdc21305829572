"""OGB's gcn-virtual at width 300 on the GPU (flowgnn.h: flowgnn_set_gcn_virtual_node_dim; kernels: flowgnn_amd/csrc/gcn_wide.hip,
DESIGN.md section 4.19).

Expected values: the float64 forward of tests/gcn_wide_vn_ref.py (at width 100 it is tests/gcn_vn_ref.py's, with zero tensors
tests/gcn_wide_ref.py's: tests/test_gcn_wide_vn_cpu.py).  Tolerance: the project's rule and nothing else, |gpu - want| <= REL (scale +
|want|), REL = 1e-4, scale = the float64 forward's largest activation, t and the update's hidden vector included (tests/parity.py);
the split-accuracy case uses B = sqrt(E_ok * E_bad) of tests/golden/gcn_wide_vn_sep.json, which comes from the references alone.
Every comparison prints its worst ratio to the bound.

Tensors: weights.synth_gcn_weights(seed=7, emb_dim=300) with gcn_wide_vn_ref.shapes_virtual_node() -- the synthetic tensors with the
first linear layer scaled by 1 / 16 (1 / 64 where a graph has hundreds of nodes) -- wherever the split-f16 kernels are what is under
test: at the synthetic scales themselves the vector explodes over four updates and every pass would be repeated in fp32.  Each such test
asserts the range on the reference (`in_range`) and `exact_reruns == 0` on the engine.  Every test here fails on a library without
flowgnn_set_gcn_virtual_node_dim."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, export, graphpack as gp, weights
from tests import gcn_wide_ref as R, gcn_wide_vn_ref as V
from tests.parity import REL, assert_close, err_ratio
from tests.test_embeddings_gpu import launched
from tests.test_gcn_wide_gpu import NARROW_SLOTS, graph, isolated, path

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
LAYER, EXACT, T0, T, UPDATE = "gcn_wide_layer", "gcn_wide_layer_f32", "gcn_wide_vn_t0", "gcn_wide_vn_t", "gcn_wide_vn_update"
BIG_GRAPHS_W1 = 1.0 / 64  # t grows with the node count: for graphs of hundreds of nodes the first linear layer is scaled down once more


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def close(got, want, scale, what, rel=REL):
    print(what, f"worst ratio to the bound {err_ratio(got, want, scale, rel):.3f}")
    assert_close(got, want, scale=scale, rel=rel, what=what)


def in_range(ref):
    """From the reference alone: no operand of a split kernel (xin_1 .. xin_4, t, the update's pre-scaled hidden values) comes within a
    factor of two of its threshold, so no pass is repeated in fp32 and the kernels under test compute the result."""
    return ref.operands < 6.0e4 / 2


@pytest.fixture(scope="module")
def w300():
    return weights.synth_gcn_weights(seed=7, emb_dim=300)


@pytest.fixture(scope="module")
def vn300():
    return V.shapes_virtual_node()


def make(w, vn, num_tasks=1, pooling=None, options=None):
    e = Engine("GCN", device=0, options=options or {})
    e.set_model_emb_dim(300)
    if num_tasks != 1:
        e.set_num_tasks(num_tasks)
    e.set_weights(w)
    if pooling:
        e.set_pooling(pooling)
    if vn is not None:
        e.set_gcn_virtual_node(vn)
    e.profile_enable(True)
    return e


def run(e, b, expect_reruns=0, **fwd):
    """One forward with the virtual node on: the t_0 and update slots ran, no 100-wide kernel did, and the exact form ran exactly when
    a re-run is expected."""
    res = {}
    before = e.exact_reruns()
    names = launched(e, lambda: res.update(got=e.forward(b, **fwd)))
    assert {LAYER, T0, T, UPDATE} <= names and not names & (NARROW_SLOTS | {"gin_ogb_vn", "gcn_ogb_vn", "gcn_ogb_vn_map"}), names
    assert e.exact_reruns() - before == expect_reruns, (e.exact_reruns(), before)
    assert (EXACT in names) == (expect_reruns > 0), names
    got = res["got"]
    return tuple(np.array(x) for x in got) if isinstance(got, tuple) else np.array(got)


# ---------------------------------------------------------------- 1. the fixed input
def test_fixed_input_logits_rows_and_node_embeddings():
    """The input of tests/test_gcn_wide_vn_cpu.py, which tells every wrong form of the virtual node from the definition by more than ten
    times this bound."""
    b, w, vn = V.fixed_batch(), V.fixed_weights(), V.fixed_virtual_node()
    ref = V.forward(b, w, vn)
    assert in_range(ref)
    e = make(w, vn)
    assert e.gcn_virtual_node() is True
    logits = run(e, b)
    rows = e.final_h()  # flowgnn_get_h: pre_4 at this width
    logits2, emb_rows = run(e, b, return_node_embeddings=True)
    e.close()
    assert rows.shape == (b.total_nodes, 300)
    close(rows, ref.rows, ref.scale, ("fixed input", "pre_4 rows"))
    close(emb_rows, ref.rows, ref.scale, ("fixed input", "node embeddings"))
    close(logits, ref.logits, ref.scale, ("fixed input", "logits"))
    close(logits2, ref.logits, ref.scale, ("fixed input", "logits with node embeddings on"))


# ---------------------------------------------------------------- 2. shapes where the tile and graph bookkeeping can go wrong
def hub_in_only(n, seed):
    """Node 0 has n - 1 in-edges and no out-edge; its sources have an out-edge and no in-edge."""
    return graph(n, [(i, 0) for i in range(1, n)], seed)


SHAPES = {"one node": (lambda: isolated(1, 3), 1.0 / 16),
          "sixteen one-node graphs in one tile": (lambda: gp.concat_batches([isolated(1, 50 + i) for i in range(16)]), 1.0 / 16)}
for _n in (15, 16, 17, 33):
    SHAPES[f"{_n} nodes in a row"] = ((lambda n=_n: path(n, 100 + n)), 1.0 / 16)
# graphs of 1 .. 5 nodes next to ones that straddle a wave's 16-node tile and a workgroup's 128 rows; the last graph ends mid-tile
SHAPES["small graphs next to 128, 129 and 300 nodes"] = (lambda: gp.concat_batches(
    [path(n, 200 + i) for i, n in enumerate((1, 2, 128, 3, 129, 4, 5, 1, 300, 2, 3))]), BIG_GRAPHS_W1)
SHAPES["a last graph ending mid-tile"] = (lambda: gp.concat_batches([path(16, 1), path(16, 2), path(7, 3)]), 1.0 / 16)
SHAPES["a batch without an edge"] = (lambda: gp.concat_batches([isolated(n, 60 + n) for n in (1, 3, 16, 17, 2)]), 1.0 / 16)
SHAPES["a hub with in-edges only"] = (lambda: gp.concat_batches([isolated(1, 1), hub_in_only(41, 2), path(5, 3)]), 1.0 / 16)
SHAPES["ragged, tens of thousands of nodes"] = (lambda: gp.synth_molpcba_batch(800, seed=21), 1.0 / 16)


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name, w300):
    build, w1_scale = SHAPES[name]
    b, vn = build(), V.shapes_virtual_node(w1_scale=w1_scale)
    ref = V.forward(b, w300, vn)
    assert in_range(ref), ref.operands
    e = make(w300, vn)
    logits, rows = run(e, b, return_node_embeddings=True)
    e.close()
    close(rows, ref.rows, ref.scale, (name, "rows"))
    close(logits, ref.logits, ref.scale, (name, "logits"))


# ---------------------------------------------------------------- 3. other configurations
@pytest.fixture(scope="module")
def small():
    return gp.concat_batches([gp.synth_molpcba_batch(60, seed=13), isolated(1, 7), path(2, 8)])


CONFIGS = [("graph embeddings", dict(fwd=dict(return_embeddings=True))), ("node embeddings", dict(fwd=dict(return_node_embeddings=True))),
           ("node logits", dict(fwd=dict(return_node_logits=True))), ("sum pooling", dict(pooling="sum")), ("max pooling", dict(pooling="max")),
           ("NUM_TASK 2", dict(num_tasks=2))]


@pytest.mark.parametrize("name,cfg", CONFIGS, ids=[n for n, _ in CONFIGS])
def test_configurations(name, cfg, small, vn300):
    tasks, pooling, fwd = cfg.get("num_tasks", 1), cfg.get("pooling"), cfg.get("fwd", {})
    w = weights.synth_gcn_weights(seed=7, num_tasks=tasks, emb_dim=300)
    ref = V.forward(small, w, vn300, pooling=pooling or "mean", num_tasks=tasks)  # (the update pools by sum whatever the readout does)
    assert in_range(ref)
    e = make(w, vn300, num_tasks=tasks, pooling=pooling)
    got = run(e, small, **fwd)
    e.close()
    got = got if isinstance(got, tuple) else (got,)
    assert got[0].shape == ((small.num_graphs, tasks) if tasks > 1 else (small.num_graphs,))
    close(got[0], ref.logits, ref.scale, (name, "logits"))
    if fwd.get("return_embeddings"):
        close(got[1], ref.pooled, ref.scale, (name, "graph embeddings"))
    if fwd.get("return_node_embeddings"):
        close(got[1], ref.rows, ref.scale, (name, "node embeddings"))
    if fwd.get("return_node_logits"):
        close(got[1], V.node_logits(w, ref.rows), ref.scale, (name, "node logits"))


# ---------------------------------------------------------------- 4. range and the exact re-run
def test_range_rerun(small, w300):
    """gcn_vn_ref.range_virtual_node at 300: one component of vn_1 is 7e4, so xin_1 leaves the f16 split's range in the registers of
    the layer kernel's VN instance; the pass is repeated once in fp32 and lands within the bound."""
    vn = V.range_virtual_node()
    ref = V.forward(small, w300, vn)
    assert ref.operands > 6.6e4 and R.max_a(small, w300) < 6.0e4 / 2  # (the rows themselves are as small as without it)
    e = make(w300, vn)
    logits, rows = run(e, small, expect_reruns=1, return_node_embeddings=True)
    assert e.exact_reruns() == 1
    e.close()
    close(rows, ref.rows, ref.scale, "range re-run, rows")
    close(logits, ref.logits, ref.scale, "range re-run, logits")


# ---------------------------------------------------------------- 5. bit identity
def test_two_runs_zero_tensors_and_off_again(small, w300, vn300):
    never = Engine("GCN", device=0)
    never.set_model_emb_dim(300)
    never.set_weights(w300)
    want_logits, want_rows = [np.array(x) for x in never.forward(small, return_node_embeddings=True)]
    never.close()
    e = make(w300, V.zero_virtual_node())
    zero_logits, zero_rows = run(e, small, return_node_embeddings=True)
    assert e.gcn_virtual_node() is True  # on is a state, not a value
    e.set_gcn_virtual_node(vn300)
    on_logits, on_rows = run(e, small, return_node_embeddings=True)
    again_logits, again_rows = run(e, small, return_node_embeddings=True)
    e.set_gcn_virtual_node(None)
    assert e.gcn_virtual_node() is False
    names = launched(e, lambda: e.forward(small, return_node_embeddings=True))
    off_logits, off_rows = e.results().copy(), e.node_embeddings().copy()
    e.close()
    assert not names & {T0, T, UPDATE} and LAYER in names, names
    assert np.array_equal(again_logits, on_logits) and np.array_equal(again_rows, on_rows)  # two runs of a batch
    assert np.array_equal(zero_logits, want_logits) and np.array_equal(zero_rows, want_rows)
    assert np.array_equal(off_logits, want_logits) and np.array_equal(off_rows, want_rows)
    assert not np.array_equal(on_logits, want_logits)


@pytest.fixture(scope="module")
def one_engine(small, w300, vn300):
    """(logits, graph embeddings) of one engine on the host batch."""
    ref = V.forward(small, w300, vn300)
    assert in_range(ref)
    e = make(w300, vn300)
    want, want_emb = run(e, small, return_embeddings=True)
    e.close()
    close(want, ref.logits, ref.scale, "one engine")
    return ref, want, want_emb


def test_device_batches_give_the_same_bits(small, w300, vn300, one_engine):
    """The partial rows are cut at the batch's tiles, and the batch is the same batch in either input form."""
    pytest.importorskip("torch")
    from tests.test_device_batch_gpu import device_args
    ref, want, want_emb = one_engine
    e = make(w300, vn300)
    try:
        for layout in ("pyg", "reference"):
            args, kw = device_args(small, layout, "GCN")
            got, emb, rows = e.forward_device(*args, return_embeddings=True, return_node_embeddings=True, **kw)
            e.sync()
            assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(emb.cpu().numpy(), want_emb), layout
            close(rows.cpu().numpy(), ref.rows, ref.scale, (layout, "rows"))
        assert e.exact_reruns() == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 6. within the bound only: the partial rows are cut at batch-relative tiles
def test_group_within_the_bound(small, w300, vn300, one_engine):
    ref, want, _ = one_engine
    g = EngineGroup("GCN", [0, 0])
    g.set_model_emb_dim(300)
    g.set_weights(w300)
    g.set_gcn_virtual_node(vn300)
    got = g.forward(small).copy()
    g.set_gcn_virtual_node(None)
    off = g.forward(small).copy()
    g.close()
    close(got, ref.logits, ref.scale, "EngineGroup [0, 0]")
    assert err_ratio(off, ref.logits, ref.scale, REL) > 10.0  # (off is another model at this tolerance)


def test_permuted_batch_and_slice_within_the_bound(w300):
    big = gp.concat_batches([gp.synth_molpcba_batch(60, seed=17), hub_in_only(40, 9), path(200, 10), isolated(3, 11)])
    vn = V.shapes_virtual_node(w1_scale=BIG_GRAPHS_W1)
    G = big.num_graphs
    perm = np.random.default_rng(5).permutation(G)
    shuffled = gp.concat_batches([big.slice(int(i), int(i) + 1) for i in perm])
    part = big.slice(7, 40)
    refs = [V.forward(x, w300, vn) for x in (big, shuffled, part)]
    assert all(in_range(r) for r in refs)
    e = make(w300, vn)
    for x, r, what in zip((big, shuffled, part), refs, ("the batch", "permuted", "a slice")):
        logits, rows = run(e, x, return_node_embeddings=True)
        close(rows, r.rows, r.scale, (what, "rows"))
        close(logits, r.logits, r.scale, (what, "logits"))
    e.close()
    assert np.allclose(refs[1].logits, refs[0].logits[perm], rtol=1e-12, atol=1e-12)  # (the reference itself does not see the order)


# ---------------------------------------------------------------- 7. split accuracy
@pytest.mark.parametrize("seed", V.SEEDS)
def test_split_accuracy(seed):
    """err <= B = sqrt(E_ok * E_bad) for rows and logits with the virtual node on and the restatement applied to the update's eight
    products as well: closer to float64 than every wrong variant of the three-product split, by the margin the references leave."""
    from tests import split_ref
    b, w, vn, ref, t = R.sep_batch(seed), R.sep_weights(), V.sep_virtual_node(), V.reference(seed), V.golden()[str(seed)]
    assert in_range(ref)
    e = make(w, vn)
    logits, rows = run(e, b, return_node_embeddings=True)
    e.close()
    for name, got in (("rows", rows), ("logits", logits)):
        err = V.err(got, ref, name)
        print(f"seed {seed} {name}: err {err:.3e}  E_ok {t[name]['e_ok']:.3e}  B {t[name]['bound']:.3e}  E_bad {t[name]['e_bad']:.3e}  "
              f"ratio {t[name]['ratio']:.1f}")
        assert t[name]["ratio"] >= split_ref.min_ratio("GCN", name), (name, t[name])  # (a condition on the references)
        assert err <= t[name]["bound"], (name, err, t[name]["bound"])


# ---------------------------------------------------------------- 8. the exported checkpoint through the host CLI
def test_host_cli_runs_an_exported_300_wide_gcn_virtual_checkpoint(tmp_path):
    sd = V.vn_state_dict(seed=4, vn_w1_scale=1.0 / 16)  # (in the split kernels' range: asserted below, on the references and on the engine)
    b = gp.synth_molpcba_batch(40, seed=3)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    export.export_weights("GCN", sd, str(wdir), virtual_node=True, emb_dim=300, virtual_node_dim=300)
    assert sorted(os.listdir(wdir)) == sorted([weights.gcn_file(300), weights.gcn_virtual_node_file(300)])
    out = tmp_path / "HLS_output.txt"
    p = subprocess.run([HOST, "GCN", "--emb-dim", "300", "--ogb-vn", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1",
                        "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    w, vn = weights.load_gcn_weights(str(wdir), emb_dim=300), weights.load_gcn_virtual_node(str(wdir), emb_dim=300)
    ref, without = V.forward(b, w, vn), R.forward(b, w)
    assert in_range(ref)  # the exported checkpoint runs on the split-f16 kernels, not on the fp32 re-run
    want = V.ogb_forward(sd, b)
    close(got, ref.logits, ref.scale, "host GCN --emb-dim 300 --ogb-vn, against the files' float64 forward")
    close(got, want, ref.scale, "host GCN --emb-dim 300 --ogb-vn, against the state_dict's own forward")
    assert err_ratio(without.logits, ref.logits, ref.scale, REL) > 10.0  # (without the flag it is another model at this tolerance)
    e = Engine("GCN", device=0)  # ... and the Python wrapper's route to the same files
    e.set_model_emb_dim(300)
    e.load_weights_dir(str(wdir), virtual_node=True)
    assert e.gcn_virtual_node() is True
    e.profile_enable(True)
    got = run(e, b)  # (no exact re-run: the same files, the same kernels as the CLI's run)
    e.close()
    close(got, want, ref.scale, "load_weights_dir(virtual_node=True) at width 300")


# ---------------------------------------------------------------- 9. a recorded launch sequence is dropped
def test_the_run_after_a_hipgraph_drop(small, w300, vn300):
    ref = V.forward(small, w300, vn300)
    plain_engine = make(w300, vn300)
    expected = plain_engine.forward(small).copy()
    plain_engine.close()
    h = Engine("GCN", device=0, options={"hipgraph": 1})
    h.set_model_emb_dim(300)
    h.set_weights(w300)
    h.set_batch(small)
    for _ in range(3):
        h.run()
    plain = h.results().copy()
    assert h.graph_replays() >= 1
    h.set_gcn_virtual_node(vn300)
    h.run()
    first = h.results().copy()
    before = h.graph_replays()
    outs = []
    for _ in range(3):
        h.run()
        outs.append(h.results().copy())
    assert h.graph_replays() > before  # the new sequence is recorded and replayed in its turn
    h.set_gcn_virtual_node(None)
    h.run()
    off = h.results().copy()
    h.close()
    assert np.array_equal(first, expected) and not np.array_equal(first, plain) and np.array_equal(off, plain)
    assert all(np.array_equal(o, expected) for o in outs)
    close(first, ref.logits, ref.scale, "hipgraph, the run after set_gcn_virtual_node")
