"""OGB's gin-virtual at width 300 on the GPU (flowgnn.h: flowgnn_set_ogb_virtual_node_dim; kernels: flowgnn_amd/csrc/gin_wide.hip,
DESIGN.md section 4.17).

Expected values: the float64 forward of tests/gin_wide_vn_ref.py (at width 100 it is tests/ogb_vn_ref.py's, with zero tensors
tests/gin_wide_ref.py's: tests/test_gin_wide_vn_cpu.py).  Tolerance: the project's rule and nothing else, |gpu - want| <= REL (scale +
|want|), REL = 1e-4, scale = the float64 forward's largest activation, t and the virtual node's hidden vector included
(tests/parity.py); the split-accuracy case uses B = sqrt(E_ok * E_bad) of gin_wide_vn_ref.table, which comes from the references
alone.  Every comparison prints its worst ratio to the bound.

Tensors: weights.synth_gin_weights(seed=7, emb_dim=300) with gin_wide_vn_ref.shapes_virtual_node() -- weights.synth_gin_virtual_node(
seed=11, emb_dim=300) with its first linear layer scaled by 1 / 16 -- wherever the split-f16 kernels are what is under test: at the
synthetic scales themselves the float64 forward passes 6e4 after four updates (tests/test_gin_wide_vn_cpu.py shows it), every pass is
repeated in fp32, and the kernels under test would compute nothing.  test_the_synthetic_scales_take_the_exact_rerun runs the unscaled
tensors for what they do exercise.  Every test here fails on a library without flowgnn_set_ogb_virtual_node_dim."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, export, graphpack as gp, weights
from tests import gin_wide_ref as W, gin_wide_vn_ref as V, split_ref
from tests.parity import REL, assert_close, err_ratio
from tests.test_embeddings_gpu import launched
from tests.test_gin_wide_gpu import hub, isolated, path

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
LAYER, EXACT, POOL, UPDATE = "gin_wide_layer", "gin_wide_layer_f32", "gin_wide_vn_pool", "gin_wide_vn_update"
EPS = np.asarray(W.TRAINED_EPS, np.float32)


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


def in_range(b, w, vn, **kw):
    """From the reference alone: no operand of a split kernel comes within a factor of two of its threshold, so no pass is repeated in
    fp32 and the kernels under test compute the result."""
    node, upd = V.split_operands(b, w, vn, **kw)
    return max(node, upd) < 6.0e4 / 2


@pytest.fixture(scope="module")
def w300():
    return weights.synth_gin_weights(seed=7, emb_dim=300)


@pytest.fixture(scope="module")
def vn300():
    return V.shapes_virtual_node()


def make(w, vn, eps=None, num_tasks=1, pooling=None, options=None):
    e = Engine("GIN", device=0, options=options or {})
    e.set_emb_dim(300)
    if num_tasks != 1:
        e.set_num_tasks(num_tasks)
    e.set_weights(w)
    if pooling:
        e.set_pooling(pooling)
    if eps is not None:
        e.set_gin_eps(eps)
    if vn is not None:
        e.set_ogb_virtual_node(vn)
    e.profile_enable(True)
    return e


def run(e, b, expect_reruns=0, **fwd):
    """One forward with the virtual node on: the pool and update slots ran, no 100-wide kernel did."""
    res = {}
    before = e.exact_reruns()
    names = launched(e, lambda: res.update(got=e.forward(b, **fwd)))
    assert {LAYER, POOL, UPDATE} <= names and not names & {"gin_resident", "gin_layer_fused", "gin_aggregate", "gin_mlp", "gin_ogb_vn"}, names
    assert e.exact_reruns() - before == expect_reruns, (e.exact_reruns(), before)
    assert (EXACT in names) == (expect_reruns > 0), names
    return res["got"]


# ---------------------------------------------------------------- 1. the fixed input
@pytest.mark.parametrize("eps_on", [False, True], ids=["eps off", "eps on"])
def test_fixed_input_logits_and_rows(eps_on, w300):
    """The input of tests/test_gin_wide_vn_cpu.py, which tells every wrong form of the virtual node from the definition by more than ten
    times this bound."""
    b, vn, eps = V.fixed_batch(), V.fixed_virtual_node(), (EPS if eps_on else None)
    ref = V.forward(b, w300, vn, eps=eps)
    assert in_range(b, w300, vn, eps=eps)
    e = make(w300, vn, eps=eps)
    logits = run(e, b)
    rows = e.final_h()  # flowgnn_get_h: h_5
    e.close()
    assert rows.shape == (b.total_nodes, 300)
    close(rows, ref.rows, ref.scale, ("fixed input", "rows"))
    close(logits, ref.logits, ref.scale, ("fixed input", "logits"))


# ---------------------------------------------------------------- 2. shapes where the new code can go wrong
def many(G, seed):
    """G small graphs (1 .. 5 nodes)."""
    return gp.concat_batches([path(1 + (i * 7 + seed) % 5, 1000 * seed + i) for i in range(G)])


BIG_GRAPHS_W1 = 1.0 / 64  # t grows with the node count: for graphs of hundreds of nodes the first linear layer is scaled down once more
# (tests/gin_wide_vn_ref.shapes_virtual_node; at 1 / 16 the update's hidden layer passes 6e4 for a 300-node graph, on the float64 forward's evidence)
SHAPES = {f"{G} graphs": ((lambda G=G: many(G, G)), 1.0 / 16) for G in (1, 15, 16, 17, 33)}  # the update's 16-graph column tile
SHAPES["one-node graphs only"] = (lambda: gp.concat_batches([isolated(1, 50 + i) for i in range(150)]), 1.0 / 16)  # 16 graphs in one row tile's epilogue
SHAPES["graphs across the tile and workgroup boundaries"] = (lambda: gp.concat_batches(
    [path(n, 200 + n) for n in (1, 2, 127, 3, 128, 4, 5, 129, 1, 300, 2)]), BIG_GRAPHS_W1)  # (a graph across the 16-row tile and the 128-row workgroup)
SHAPES["2 000 ragged graphs"] = (lambda: gp.synth_molhiv_batch(2000, seed=21), 1.0 / 16)


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name, w300):
    build, w1_scale = SHAPES[name]
    b, vn = build(), V.shapes_virtual_node(w1_scale=w1_scale)
    ref = V.forward(b, w300, vn, eps=EPS)
    assert in_range(b, w300, vn, eps=EPS)
    e = make(w300, vn, eps=EPS)
    logits, rows = run(e, b, return_node_embeddings=True)
    e.close()
    close(rows, ref.rows, ref.scale, (name, "rows"))
    close(logits, ref.logits, ref.scale, (name, "logits"))


# ---------------------------------------------------------------- 3. other configurations
@pytest.fixture(scope="module")
def small():
    return gp.concat_batches([gp.synth_molhiv_batch(200, seed=13), isolated(1, 7), path(2, 8)])


CONFIGS = [("graph embeddings", dict(fwd=dict(return_embeddings=True))), ("node embeddings", dict(fwd=dict(return_node_embeddings=True))),
           ("node logits", dict(fwd=dict(return_node_logits=True))), ("sum pooling", dict(pooling="sum")), ("max pooling", dict(pooling="max")),
           ("NUM_TASK 2", dict(num_tasks=2)),
           ("eps, sum pooling, embeddings, NUM_TASK 2", dict(eps=EPS, pooling="sum", num_tasks=2, fwd=dict(return_embeddings=True)))]


@pytest.mark.parametrize("name,cfg", CONFIGS, ids=[n for n, _ in CONFIGS])
def test_configurations(name, cfg, small, vn300):
    tasks, pooling, eps, fwd = cfg.get("num_tasks", 1), cfg.get("pooling"), cfg.get("eps"), cfg.get("fwd", {})
    w = weights.synth_gin_weights(seed=7, num_tasks=tasks, emb_dim=300)
    ref = V.forward(small, w, vn300, eps=eps, pooling=pooling or "mean", num_tasks=tasks)  # (the update pools by sum whatever the readout does)
    assert in_range(small, w, vn300, eps=eps)
    e = make(w, vn300, eps=eps, num_tasks=tasks, pooling=pooling)
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
def test_range_rerun_from_the_update_alone(small, w300, vn300):
    """The first update's b1 scaled until its hidden layer passes 6e4 while its second matrix is scaled down by as much, so that vn_1 and
    with it the node MLP stay where they were: one exact re-run, raised by the update kernel alone, and the result within the bound."""
    vn = {k: np.asarray(v, np.float32).copy() for k, v in vn300.items()}
    top = float(vn["b1"][0].max())
    k = np.float32(7.5e4 / top)
    vn["b1"][0] *= k
    vn["w2"][0] /= k
    ref = V.forward(small, w300, vn)
    rec = split_ref.Recorder()
    V.forward(small, w300, vn, dense=rec)  # the node MLP's own operands: a and the hidden values, layer by layer
    node_max = max(float(np.abs(a).max()) for a in rec.inputs)
    s1 = max(split_ref.pow2_scale(M) for M in np.asarray(w300["node_mlp_1_weights"]))
    assert s1 * node_max < 6.0e4 / 4 and ref.scale > 6.6e4, (node_max, ref.scale)
    e = make(w300, vn)
    logits, rows = run(e, small, expect_reruns=1, return_node_embeddings=True)
    assert e.exact_reruns() == 1
    e.close()
    close(rows, ref.rows, ref.scale, "range re-run, rows")
    close(logits, ref.logits, ref.scale, "range re-run, logits")


def test_the_synthetic_scales_take_the_exact_rerun(small, w300):
    """weights.synth_gin_virtual_node(seed=11, emb_dim=300) as it is: t passes 6e4, the pass is repeated in fp32 (pool, two dense launches
    on G rows, the adds in the encoder and behind the dense kernel) and lands within the bound."""
    vn = weights.synth_gin_virtual_node(seed=11, emb_dim=300)
    ref = V.forward(small, w300, vn, eps=EPS)
    assert ref.scale > 6.6e4
    e = make(w300, vn, eps=EPS)
    logits, rows = run(e, small, expect_reruns=1, return_node_embeddings=True)
    e.close()
    close(rows, ref.rows, ref.scale, "synthetic scales, rows")
    close(logits, ref.logits, ref.scale, "synthetic scales, logits")


# ---------------------------------------------------------------- 5. bit identity
def test_zero_tensors_and_off_again_give_the_bits_of_an_engine_that_never_had_it(small, w300, vn300):
    never = Engine("GIN", device=0)
    never.set_emb_dim(300)
    never.set_weights(w300)
    never.set_gin_eps(EPS)
    want_logits, want_rows = [x.copy() for x in never.forward(small, return_node_embeddings=True)]
    never.close()
    e = make(w300, V.zero_virtual_node(), eps=EPS)
    zero_logits, zero_rows = [x.copy() for x in run(e, small, return_node_embeddings=True)]
    assert e.ogb_virtual_node() is True  # on is a state, not a value
    e.set_ogb_virtual_node(vn300)
    on_logits = run(e, small, return_node_embeddings=True)[0].copy()
    e.set_ogb_virtual_node(None)
    names = launched(e, lambda: e.forward(small, return_node_embeddings=True))
    off_logits, off_rows = e.results().copy(), e.node_embeddings().copy()
    e.close()
    assert not names & {POOL, UPDATE} and LAYER in names, names
    assert np.array_equal(zero_logits, want_logits) and np.array_equal(zero_rows, want_rows)
    assert np.array_equal(off_logits, want_logits) and np.array_equal(off_rows, want_rows)
    assert not np.array_equal(on_logits, want_logits)


@pytest.fixture(scope="module")
def one_engine(small, w300, vn300):
    """(logits, graph embeddings) of one engine on the host batch: what the device batches and the group have to reproduce bit for bit."""
    ref = V.forward(small, w300, vn300, eps=EPS)
    e = make(w300, vn300, eps=EPS)
    want, want_emb = [x.copy() for x in run(e, small, return_embeddings=True)]
    e.close()
    close(want, ref.logits, ref.scale, "one engine")
    return want, want_emb


def test_device_batches_give_the_same_bits(small, w300, vn300, one_engine):
    pytest.importorskip("torch")
    from tests.test_device_batch_gpu import device_args
    want, want_emb = one_engine
    ref = V.forward(small, w300, vn300, eps=EPS)
    e = make(w300, vn300, eps=EPS)
    try:
        for layout in ("pyg", "reference"):
            args, kw = device_args(small, layout, "GIN")
            got, emb, rows = e.forward_device(*args, return_embeddings=True, return_node_embeddings=True, **kw)
            e.sync()
            assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(emb.cpu().numpy(), want_emb), layout
            close(rows.cpu().numpy(), ref.rows, ref.scale, (layout, "rows"))
    finally:
        e.close()


def test_group_gives_the_same_bits(small, w300, vn300, one_engine):
    want, want_emb = one_engine
    g = EngineGroup("GIN", [0, 0])
    g.set_emb_dim(300)
    g.set_weights(w300)
    g.set_gin_eps(EPS)
    g.set_ogb_virtual_node(vn300)
    g.set_embeddings(True)
    got = g.forward(small)
    emb = g.embeddings()
    g.set_ogb_virtual_node(None)
    off = g.forward(small)
    g.close()
    assert np.array_equal(got, want) and np.array_equal(emb, want_emb)  # a graph's bits do not depend on where the group cuts the batch
    assert not np.array_equal(off, want)


def test_permuted_batch_and_slice_give_each_graph_the_same_bits(w300):
    big = gp.concat_batches([gp.synth_molhiv_batch(120, seed=17), hub(40, 9), path(200, 10), isolated(3, 11)])
    vn300 = V.shapes_virtual_node(w1_scale=BIG_GRAPHS_W1)
    assert in_range(big, w300, vn300, eps=EPS)
    G = big.num_graphs
    perm = np.random.default_rng(5).permutation(G)
    shuffled = gp.concat_batches([big.slice(int(i), int(i) + 1) for i in perm])
    e = make(w300, vn300, eps=EPS)
    a_logits, a_rows = [x.copy() for x in run(e, big, return_node_embeddings=True)]
    b_logits, b_rows = [x.copy() for x in run(e, shuffled, return_node_embeddings=True)]
    part = run(e, big.slice(7, 60), return_node_embeddings=True)
    e.close()
    assert np.array_equal(b_logits, a_logits[perm])
    off, soff = big.node_offsets(), shuffled.node_offsets()
    for k, i in enumerate(perm):
        assert np.array_equal(b_rows[soff[k]:soff[k + 1]], a_rows[off[i]:off[i + 1]]), (k, i)
    assert np.array_equal(part[0], a_logits[7:60]) and np.array_equal(part[1], a_rows[off[7]:off[60]])


# ---------------------------------------------------------------- 6. split accuracy
@pytest.mark.parametrize("seed", V.SEEDS)
def test_split_accuracy(seed):
    """err <= B = sqrt(E_ok * E_bad) for rows and logits with the virtual node on and the restatement applied to the update's two
    products as well: closer to float64 than every wrong variant of the three-product split, by the margin the references leave."""
    # (the table: the fixture tests/golden/gin_wide_vn_sep.json, which tests/test_gin_wide_vn_cpu.py checks against a recomputation)
    b, w, vn, ref, t = W.sep_batch(seed), W.sep_weights(), V.sep_virtual_node(), V.reference(seed), V.golden_table(seed)
    assert in_range(b, w, vn)
    e = make(w, vn)
    logits, rows = run(e, b, return_node_embeddings=True)
    e.close()
    for name, got in (("rows", rows), ("logits", logits)):
        err = V.err(got, ref, name)
        print(f"seed {seed} {name}: err {err:.3e}  E_ok {t[name].e_ok:.3e}  B {t[name].bound:.3e}  E_bad {t[name].e_bad:.3e}  "
              f"ratio {t[name].e_bad / t[name].e_ok:.1f}")
        assert t[name].e_bad / t[name].e_ok >= V.MIN_RATIO, (name, t[name].e_ok, t[name].e_bad)  # (a condition on the references)
        assert err <= t[name].bound, (name, err, t[name].bound)


# ---------------------------------------------------------------- 7. the exported checkpoint through the host CLI
def test_host_cli_runs_an_exported_300_wide_gin_virtual_checkpoint(tmp_path):
    sd = V.vn_state_dict(seed=3, vn_w1_scale=1.0 / 16)  # (in the split kernels' range: asserted below, on the references and on the engine)
    b = gp.synth_molhiv_batch(40, seed=3)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    export.export_weights("GIN", sd, str(wdir), keep_eps=True, virtual_node=True, virtual_node_dim=300)
    out = tmp_path / "HLS_output.txt"
    p = subprocess.run([HOST, "GIN", "--emb-dim", "300", "--eps", "--ogb-vn", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1",
                        "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    w, eps = weights.load_gin_weights(str(wdir), emb_dim=300), weights.load_gin_eps(str(wdir), emb_dim=300)
    vn = weights.load_gin_virtual_node(str(wdir), emb_dim=300)
    assert in_range(b, w, vn, eps=eps)  # the exported checkpoint runs on the split-f16 kernels, not on the fp32 re-run
    ref, without = V.forward(b, w, vn, eps=eps), W.forward(b, w, eps=eps)
    want = V.ogb_forward(sd, b)
    close(got, ref.logits, ref.scale, "host GIN --emb-dim 300 --eps --ogb-vn, against the files' float64 forward")
    close(got, want, ref.scale, "host GIN --emb-dim 300 --eps --ogb-vn, against the state_dict's own forward")
    assert err_ratio(without.logits, ref.logits, ref.scale, REL) > 10.0  # (without the flag it is another model at this tolerance)
    e = Engine("GIN", device=0)  # ... and the Python wrapper's route to the same files
    e.set_emb_dim(300)
    e.load_weights_dir(str(wdir), eps=True, virtual_node=True)
    assert e.ogb_virtual_node() is True
    e.profile_enable(True)
    got = run(e, b)  # (no exact re-run: the same files, the same kernels as the CLI's run)
    e.close()
    close(got, want, ref.scale, "load_weights_dir(eps=True, virtual_node=True) at width 300")


# ---------------------------------------------------------------- 8. a recorded launch sequence is dropped
def test_the_run_after_a_hipgraph_drop(small, w300, vn300):
    ref = V.forward(small, w300, vn300)
    plain_engine = make(w300, vn300)
    expected = plain_engine.forward(small).copy()
    plain_engine.close()
    h = Engine("GIN", device=0, options={"hipgraph": 1})
    h.set_emb_dim(300)
    h.set_weights(w300)
    h.set_batch(small)
    for _ in range(3):
        h.run()
    plain = h.results().copy()
    assert h.graph_replays() >= 1
    h.set_ogb_virtual_node(vn300)
    h.run()
    first = h.results().copy()
    before = h.graph_replays()
    outs = []
    for _ in range(3):
        h.run()
        outs.append(h.results().copy())
    assert h.graph_replays() > before  # the new sequence is recorded and replayed in its turn
    h.set_ogb_virtual_node(None)
    h.run()
    off = h.results().copy()
    h.close()
    assert np.array_equal(first, expected) and not np.array_equal(first, plain) and np.array_equal(off, plain)
    assert all(np.array_equal(o, expected) for o in outs)
    close(first, ref.logits, ref.scale, "hipgraph, the run after set_ogb_virtual_node")
