"""GIN at OGB's default width on the GPU (flowgnn.h: flowgnn_set_emb_dim; kernels: flowgnn_amd/csrc/gin_wide.hip).

Expected values: the float64 forward of tests/gin_wide_ref.py (at width 100 it is tests/numpy_ref.py's, tests/test_gin_wide_cpu.py).
Tolerance: the project's rule and nothing else, |gpu - want| <= REL (scale + |want|), REL = 1e-4, scale = the float64 forward's largest
activation (tests/parity.py); the split-accuracy case uses B = sqrt(E_ok * E_bad) of tests/gin_wide_ref.table, which comes from the
references alone.  Every comparison prints its worst ratio to the bound.  Every test here fails on a library without
flowgnn_set_emb_dim."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, export, graphpack as gp, weights
from tests import gin_wide_ref as R, split_ref
from tests.parity import REL, assert_close, err_ratio
from tests.test_embeddings_gpu import launched
from tests.wide_cases import CARDS, EDGE_COUNTS, graph, hub, isolated, path  # noqa: F401  (the builders live there; others import them from here)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
WIDE_SLOT = "gin_wide_layer"
EXACT_SLOT = "gin_wide_layer_f32"
EPS = np.asarray(R.TRAINED_EPS, np.float32)
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


def in_range(ref, w):
    """From the reference alone: no operand of the split kernel can reach its threshold (it sees |a| and the hidden values times the
    first matrix's power-of-two pre-scale; ref.scale bounds both)."""
    return max(split_ref.pow2_scale(W) for W in np.asarray(w["node_mlp_1_weights"])) * ref.scale < 6.0e4


def close(got, want, scale, what, rel=REL):
    print(what, f"worst ratio to the bound {err_ratio(got, want, scale, rel):.3f}")
    assert_close(got, want, scale=scale, rel=rel, what=what)


@pytest.fixture(scope="module")
def w300():
    return weights.synth_gin_weights(seed=7, emb_dim=300)


def make(w, eps=None, num_tasks=1, pooling=None, options=None):
    e = Engine("GIN", device=0, options=options or {})
    e.set_emb_dim(300)
    if num_tasks != 1:
        e.set_num_tasks(num_tasks)
    e.set_weights(w)
    if pooling:
        e.set_pooling(pooling)
    if eps is not None:
        e.set_gin_eps(eps)
    e.profile_enable(True)
    return e


def run(e, b, expect_reruns=0, **fwd):
    """One forward: the wide layer's slot ran five times, no 100-wide kernel did."""
    res = {}
    before = e.exact_reruns()
    names = launched(e, lambda: res.update(got=e.forward(b, **fwd)))
    assert WIDE_SLOT in names and not names & {"gin_resident", "gin_tile_build", "gin_layer_fused", "gin_aggregate", "gin_mlp"}, names
    assert e.exact_reruns() - before == expect_reruns, (e.exact_reruns(), before)
    assert (EXACT_SLOT in names) == (expect_reruns > 0), names
    return res["got"]


# ---------------------------------------------------------------- 1. tile edges
@pytest.mark.parametrize("kind", ["paths", "isolated"])
def test_tile_edges_rows_and_logits(kind, w300):
    mk = path if kind == "paths" else isolated
    b = gp.concat_batches([mk(n, 100 + n) for n in EDGE_COUNTS])
    ref = R.forward(b, w300)
    e = make(w300)
    logits = run(e, b)
    rows = e.final_h()
    e.close()
    assert rows.shape == (b.total_nodes, 300) and e.lib.flowgnn_embedding_dim(0) == 100
    close(rows, ref.rows, ref.scale, (kind, "rows"))
    close(logits, ref.logits, ref.scale, (kind, "logits"))


# ---------------------------------------------------------------- 2. gather
def test_gather_hub_all_edge_codes_and_rows_in_other_tiles(w300):
    """A hub of 300 in-edges next to one-node graphs; all 60 edge codes; a 200-node path, where a destination's sources lie in another
    workgroup's 128-row tile (rows 127 | 128 of the path, whatever the tile's offset)."""
    b = gp.concat_batches([isolated(1, 1), hub(300, 2), isolated(1, 3), isolated(1, 4), path(200, 5), isolated(1, 6)])
    codes = (b.edge_attr[:, 0] * 6 + b.edge_attr[:, 1]) * 2 + b.edge_attr[:, 2]
    assert len(np.unique(codes)) == 60
    indeg = np.bincount(b.global_edges()[:, 1], minlength=b.total_nodes)
    assert indeg.max() == 300
    ref = R.forward(b, w300)
    assert in_range(ref, w300), ref.scale
    e = make(w300)
    logits, rows = run(e, b, return_node_embeddings=True)
    e.close()
    close(rows, ref.rows, ref.scale, "gather, rows")
    close(logits, ref.logits, ref.scale, "gather, logits")


# ---------------------------------------------------------------- 3. ragged
@pytest.fixture(scope="module")
def ragged(w300):
    b = gp.synth_molhiv_batch(2000, seed=21)
    return b, R.forward(b, w300)


def test_ragged_logits_rows_and_graph_embeddings(ragged, w300):
    b, ref = ragged
    e = make(w300)
    logits, emb, rows = run(e, b, return_embeddings=True, return_node_embeddings=True)
    e.close()
    assert emb.shape == (2000, 300) and rows.shape == (b.total_nodes, 300)
    close(rows, ref.rows, ref.scale, "ragged, rows")
    close(emb, ref.pooled, ref.scale, "ragged, graph embeddings")
    close(logits, ref.logits, ref.scale, "ragged, logits")


# ---------------------------------------------------------------- 4. configurations
@pytest.fixture(scope="module")
def small():
    return gp.concat_batches([gp.synth_molhiv_batch(200, seed=13), isolated(1, 7), path(2, 8)])


CONFIGS = [("eps on", dict(eps=EPS)), ("sum pooling", dict(pooling="sum")), ("max pooling", dict(pooling="max")),
           ("NUM_TASK 128", dict(num_tasks=128)), ("node logits", dict(fwd=dict(return_node_logits=True))),
           ("node logits, NUM_TASK 3", dict(num_tasks=3, fwd=dict(return_node_logits=True))),
           ("node embeddings", dict(fwd=dict(return_node_embeddings=True))),
           ("eps, sum pooling, embeddings, NUM_TASK 128", dict(eps=EPS, pooling="sum", num_tasks=128, fwd=dict(return_embeddings=True)))]


@pytest.mark.parametrize("name,cfg", CONFIGS, ids=[n for n, _ in CONFIGS])
def test_configurations(name, cfg, small):
    tasks, pooling, eps, fwd = cfg.get("num_tasks", 1), cfg.get("pooling"), cfg.get("eps"), cfg.get("fwd", {})
    w = weights.synth_gin_weights(seed=7, num_tasks=tasks, emb_dim=300)
    ref = R.forward(small, w, eps=eps, pooling=pooling or "mean", num_tasks=tasks)
    e = make(w, eps=eps, num_tasks=tasks, pooling=pooling)
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
        close(got[1], R.node_logits(w, ref.rows), ref.scale, (name, "node logits"))


def test_eps_of_five_zeros_is_eps_off_bit_for_bit(small, w300):
    e = make(w300)
    off_logits, off_rows = run(e, small, return_node_embeddings=True)
    off_logits, off_rows = off_logits.copy(), off_rows.copy()
    e.set_gin_eps(np.zeros(5, np.float32))
    on_logits, on_rows = run(e, small, return_node_embeddings=True)
    e.set_gin_eps(EPS)
    other = run(e, small, return_node_embeddings=True)[0]
    e.close()
    assert np.array_equal(on_logits, off_logits) and np.array_equal(on_rows, off_rows)
    assert not np.array_equal(other, off_logits)


# ---------------------------------------------------------------- 5. split accuracy
@pytest.mark.parametrize("seed", R.SEEDS)
def test_split_accuracy(seed):
    """err <= B = sqrt(E_ok * E_bad) for rows and logits on the batches of the CPU separation test: closer to float64 than every wrong
    variant of the three-product split, by the margin the references leave."""
    b, w, ref, t = R.sep_batch(seed), R.sep_weights(), R.reference(seed), R.table(seed)
    e = make(w)
    logits, rows = run(e, b, return_node_embeddings=True)
    e.close()
    for name, got in (("rows", rows), ("logits", logits)):
        err = R.err(got, ref, name)
        print(f"seed {seed} {name}: err {err:.3e}  E_ok {t[name].e_ok:.3e}  B {t[name].bound:.3e}  E_bad {t[name].e_bad:.3e}")
        assert err <= t[name].bound, (name, err, t[name].bound)


# ---------------------------------------------------------------- 6. range and the exact re-run
def hid_max(b, w, layer):
    """The float64 forward's largest hidden value of one layer."""
    rec = split_ref.Recorder()
    R.forward(b, w, dense=rec)
    return float(np.maximum(rec.outputs[2 * layer] + f64(w["node_mlp_1_bias"])[layer], 0.0).max())


def test_range_flag_and_exact_rerun(small, w300):
    """The last layer's b1 scaled until its hidden layer exceeds 6.6e4 on some row: one exact re-run, the result within the bound; the
    same weights scaled back until the (pre-scaled) hidden layer stays below the kernel's threshold: none."""
    layer = 4
    s1 = split_ref.pow2_scale(w300["node_mlp_1_weights"][layer])  # the kernel sees s1 * hid (the weights' power-of-two pre-scale)
    top = float(np.asarray(w300["node_mlp_1_bias"])[layer].max())

    def scaled(target):
        w = dict(w300)
        b1 = np.asarray(w300["node_mlp_1_bias"], np.float32).copy()
        b1[layer] *= np.float32(target / top)
        w["node_mlp_1_bias"] = b1
        return w

    above, below = scaled(7.5e4), scaled(2.0e4 / s1)
    assert hid_max(small, above, layer) > 6.6e4 and s1 * hid_max(small, below, layer) < 5.0e4 and s1 >= 1.0
    ref = R.forward(small, above)
    e = make(above)
    logits, rows = run(e, small, expect_reruns=1, return_node_embeddings=True)
    close(rows, ref.rows, ref.scale, "range re-run, rows")
    close(logits, ref.logits, ref.scale, "range re-run, logits")
    e.set_weights(below)
    ref = R.forward(small, below)
    logits = run(e, small, expect_reruns=0)
    e.close()
    close(logits, ref.logits, ref.scale, "below the threshold, logits")


# ---------------------------------------------------------------- 7. bit identity
def test_permuted_batch_and_slice_give_each_graph_the_same_bits(w300):
    big = gp.concat_batches([gp.synth_molhiv_batch(120, seed=17), hub(40, 9), path(200, 10), isolated(3, 11)])
    G = big.num_graphs
    perm = np.random.default_rng(5).permutation(G)
    shuffled = gp.concat_batches([big.slice(int(i), int(i) + 1) for i in perm])
    e = make(w300)
    a_logits, a_rows = [x.copy() for x in run(e, big, return_node_embeddings=True)]
    b_logits, b_rows = [x.copy() for x in run(e, shuffled, return_node_embeddings=True)]
    part = run(e, big.slice(7, 60), return_node_embeddings=True)
    e.close()
    assert np.array_equal(b_logits, a_logits[perm])
    off, soff = big.node_offsets(), shuffled.node_offsets()
    for k, i in enumerate(perm):
        assert np.array_equal(b_rows[soff[k]:soff[k + 1]], a_rows[off[i]:off[i + 1]]), (k, i)
    assert np.array_equal(part[0], a_logits[7:60]) and np.array_equal(part[1], a_rows[off[7]:off[60]])


def test_device_batches_and_group_give_the_same_bits(small, w300):
    ref = R.forward(small, w300)
    e = make(w300)
    want, want_emb = [x.copy() for x in run(e, small, return_embeddings=True)]
    close(want, ref.logits, ref.scale, "one engine")
    try:
        pytest.importorskip("torch")
        from tests.test_device_batch_gpu import device_args
        for layout in ("pyg", "reference"):
            args, kw = device_args(small, layout, "GIN")
            got, emb, rows = e.forward_device(*args, return_embeddings=True, return_node_embeddings=True, **kw)
            e.sync()
            assert emb.shape == (small.num_graphs, 300) and rows.shape == (small.total_nodes, 300)
            assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(emb.cpu().numpy(), want_emb), layout
    finally:
        e.close()
    g = EngineGroup("GIN", [0, 0])
    g.set_emb_dim(300)
    g.set_weights(w300)
    g.set_embeddings(True)
    got = g.forward(small)
    emb = g.embeddings()
    g.close()
    assert emb.shape == (small.num_graphs, 300)
    assert np.array_equal(got, want) and np.array_equal(emb, want_emb)


def test_back_at_width_100_the_engine_is_what_it_was(small, gin_weights):
    fresh = Engine("GIN", device=0)
    fresh.set_weights(gin_weights)
    fresh.profile_enable(True)
    names_fresh = launched(fresh, lambda: fresh.forward(small))
    want = fresh.results().copy()
    fresh.close()
    assert "gin_resident" in names_fresh
    e = make(weights.synth_gin_weights(seed=7, emb_dim=300))
    run(e, small)
    e.set_emb_dim(100)
    assert e.emb_dim == 100
    e.set_weights(gin_weights)
    names = launched(e, lambda: e.forward(small))
    got = e.results().copy()
    e.close()
    assert names == names_fresh and "gin_resident" in names and WIDE_SLOT not in names, (names, names_fresh)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- 8. the exported checkpoint through the host CLI
def test_host_cli_runs_an_exported_300_wide_checkpoint(tmp_path):
    sd = R.state_dict(seed=3)
    b = gp.synth_molhiv_batch(40, seed=3)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    export.export_weights("GIN", sd, str(wdir), keep_eps=True)
    out = tmp_path / "HLS_output.txt"
    p = subprocess.run([HOST, "GIN", "--emb-dim", "300", "--eps", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    w, eps = weights.load_gin_weights(str(wdir), emb_dim=300), weights.load_gin_eps(str(wdir), emb_dim=300)
    ref = R.forward(b, w, eps=eps)
    want = R.ogb_forward(sd, b)
    close(got, ref.logits, ref.scale, "host GIN --emb-dim 300 --eps, against the files' float64 forward")
    close(got, want, ref.scale, "host GIN --emb-dim 300 --eps, against the state_dict's own forward")
    e = Engine("GIN", device=0)  # ... and the Python wrapper's route to the same files
    e.set_emb_dim(300)
    e.load_weights_dir(str(wdir), eps=True)
    got = e.forward(b)
    e.close()
    close(got, want, ref.scale, "load_weights_dir(eps=True) at width 300")
