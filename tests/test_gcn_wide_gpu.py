"""GCN at OGB's default width on the GPU (flowgnn.h: flowgnn_set_model_emb_dim; kernels: flowgnn_amd/csrc/gcn_wide.hip).

Expected values: the float64 forward of tests/gcn_wide_ref.py (at width 100 it is tests/numpy_ref.py's, tests/test_gcn_wide_cpu.py).
Tolerance: the project's rule and nothing else, |gpu - want| <= REL (scale + |want|), REL = 1e-4, scale = the float64 forward's largest
activation (tests/parity.py); the split-accuracy case uses B = sqrt(E_ok * E_bad) of tests/golden/gcn_wide_sep.json, which comes from the
references alone (tests/test_gcn_wide_cpu.py recomputes it).  Every comparison prints its worst ratio to the bound.  Every test here
fails on a library without flowgnn_set_model_emb_dim."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, embedding_dim, export, graphpack as gp, weights
from tests import gcn_wide_ref as R
from tests.parity import REL, assert_close, err_ratio
from tests.test_embeddings_gpu import launched

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
WIDE_SLOT = "gcn_wide_layer"
EXACT_SLOT = "gcn_wide_layer_f32"
NARROW_SLOTS = {"gcn_resident", "gcn_tile_build", "gcn_encoder_projected", "gcn_layer_fused", "gcn_aggregate", "gcn_dense", "gcn_encoder_dense",
                "mean_pool_linear"}
MODEL_SLOTS = {"edge_scalar", "atom_encoder", WIDE_SLOT, EXACT_SLOT, "mean_pool_rows", "pooled_head", "node_logits"}  # what GcnWideModel launches
TILE = 128  # rows of a workgroup of gcw_layer_kernel (GW_ROWS); a wave's tile is 16
EDGE_COUNTS = [1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
CARDS = (119, 4, 12, 12, 10, 6, 6, 2, 2)


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def graph(n, edges, seed):
    """One graph of n nodes with the directed edges [(src, dst)]; the edge attributes walk through all 60 (a0, a1, a2) codes."""
    rng = np.random.default_rng(seed)
    nf = np.stack([rng.integers(0, c, n) for c in CARDS], 1).astype(np.int32)
    el = np.asarray(edges, np.int32).reshape(-1, 2)
    code = (np.arange(len(el)) + seed) % 60
    ea = np.stack([code // 12, (code // 2) % 6, code % 2], 1).astype(np.int32)
    return gp.GraphBatch(np.array([n], np.int32), np.array([len(el)], np.int32), nf, el, ea)


def path(n, seed):
    fwd = [(i, i + 1) for i in range(n - 1)]
    return graph(n, fwd + [(b, a) for a, b in fwd], seed)


def isolated(n, seed):
    return graph(n, [], seed)


def close(got, want, scale, what, rel=REL):
    print(what, f"worst ratio to the bound {err_ratio(got, want, scale, rel):.3f}")
    assert_close(got, want, scale=scale, rel=rel, what=what)


@pytest.fixture(scope="module")
def w300():
    return weights.synth_gcn_weights(seed=7, emb_dim=300)


def make(w, num_tasks=1, pooling=None):
    e = Engine("GCN", device=0)
    e.set_model_emb_dim(300)
    if num_tasks != 1:
        e.set_num_tasks(num_tasks)
    e.set_weights(w)
    if pooling:
        e.set_pooling(pooling)
    e.profile_enable(True)
    return e


@pytest.fixture(scope="module")
def eng(w300):
    """One engine at width 300 with the synthetic weights, mean pooling, NUM_TASK 1, shared by the tests that change none of that."""
    e = make(w300)
    yield e
    e.close()


def run(e, b, expect_reruns=0, **fwd):
    """One forward: the wide layer's slot ran, no 100-wide kernel did, and the exact form ran exactly when a re-run is expected."""
    res = {}
    before = e.exact_reruns()
    names = launched(e, lambda: res.update(got=e.forward(b, **fwd)))
    assert WIDE_SLOT in names and not names & NARROW_SLOTS, names
    assert {"atom_encoder", "mean_pool_rows", "pooled_head"} <= names and not {n for n in names if n.startswith("gcn_")} - MODEL_SLOTS, names
    assert e.exact_reruns() - before == expect_reruns, (e.exact_reruns(), before)
    assert (EXACT_SLOT in names) == (expect_reruns > 0), names
    got = res["got"]
    return tuple(np.array(x) for x in got) if isinstance(got, tuple) else np.array(got)


# ---------------------------------------------------------------- 1. tile edges
@pytest.mark.parametrize("kind", ["paths", "isolated"])
def test_tile_edges_rows_and_logits(kind, eng, w300):
    """A single path of n nodes, and n one-node graphs (out-degree 0: dinv 0, 1 / (deg + 1) = 1), at every tile's edge and one past it."""
    for n in EDGE_COUNTS:
        b = path(n, 100 + n) if kind == "paths" else gp.concat_batches([isolated(1, 1000 * n + i) for i in range(n)])
        assert b.total_nodes == n and b.num_graphs == (1 if kind == "paths" else n)
        ref = R.forward(b, w300)
        logits = run(eng, b)
        rows = eng.final_h()
        assert rows.shape == (n, 300) and eng.emb_dim == 300 and embedding_dim("GCN") == 100
        close(rows, ref.rows, ref.scale, (kind, n, "rows"))
        close(logits, ref.logits, ref.scale, (kind, n, "logits"))


# ---------------------------------------------------------------- 2. degree edge cases and the gather
def test_degree_edge_cases(eng, w300):
    """Node 0 of the first graph has 40 in-edges and no out-edge: dinv is 0 and every message it receives carries norm 0, while its
    sources have out-edges and no in-edge.  The second graph is the reverse: node 0 has 40 out-edges and no in-edge, and its targets have
    in-edges and no out-edge."""
    sink = graph(41, [(i, 0) for i in range(1, 41)], 2)
    source = graph(41, [(0, i) for i in range(1, 41)], 3)
    b = gp.concat_batches([isolated(1, 1), sink, source, isolated(1, 4)])
    ge = b.global_edges()
    outdeg, indeg = np.bincount(ge[:, 0], minlength=b.total_nodes), np.bincount(ge[:, 1], minlength=b.total_nodes)
    assert ((indeg > 0) & (outdeg == 0)).sum() == 41 and ((outdeg > 0) & (indeg == 0)).sum() == 41
    ref = R.forward(b, w300)
    logits, rows = run(eng, b, return_node_embeddings=True)
    close(rows, ref.rows, ref.scale, "degree edge cases, rows")
    close(logits, ref.logits, ref.scale, "degree edge cases, logits")


def test_gather_hub_all_edge_codes_and_rows_in_other_tiles(eng, w300):
    """The batch's first graph has 200 rows: workgroup tiles 0..127 and 128..199.  Its hub is row 100 (wave tile 96..111) with 95
    in-edges, of all 60 edge codes: from rows 130..189 (another workgroup's tile), rows 0..29 (other waves' tiles) and rows 101..105
    (its own wave tile; they have zero in-edges), more than any other row of its tile has; its out-edges go to rows 190..195."""
    hub_row = 100
    srcs = list(range(130, 190)) + list(range(0, 30)) + list(range(101, 106))
    g = graph(200, [(s, hub_row) for s in srcs] + [(hub_row, t) for t in range(190, 196)], 2)
    b = gp.concat_batches([g, isolated(1, 3), path(200, 5), isolated(1, 6)])
    codes = (b.edge_attr[:, 0] * 6 + b.edge_attr[:, 1]) * 2 + b.edge_attr[:, 2]
    ge = b.global_edges()
    assert len(np.unique(codes[ge[:, 1] == hub_row])) == 60
    indeg = np.bincount(ge[:, 1], minlength=b.total_nodes)
    assert indeg[hub_row] == 95 and indeg[96:112].sum() == 95 and indeg.max() == 95
    ref = R.forward(b, w300)
    assert R.max_a(b, w300) < 6.0e4
    logits, rows = run(eng, b, return_node_embeddings=True)
    close(rows, ref.rows, ref.scale, "gather, rows")
    close(logits, ref.logits, ref.scale, "gather, logits")


# ---------------------------------------------------------------- 3. ragged
def test_ragged_logits_rows_and_graph_embeddings(eng, w300):
    """Graphs of 1 to 200 nodes, one-node graphs between large ones."""
    sizes = [200, 1, 150, 1, 1, 97, 3, 64, 1, 33, 200, 2, 17, 1, 128, 5, 1, 16, 15, 1, 129, 48]
    b = gp.concat_batches([path(n, 300 + i) for i, n in enumerate(sizes)] + [gp.synth_molpcba_batch(40, seed=21)])
    assert b.nums_of_nodes.min() == 1 and b.nums_of_nodes.max() == 200
    ref = R.forward(b, w300)
    logits, emb, rows = run(eng, b, return_embeddings=True, return_node_embeddings=True)
    assert emb.shape == (b.num_graphs, 300) and rows.shape == (b.total_nodes, 300)
    close(rows, ref.rows, ref.scale, "ragged, rows")
    close(emb, ref.pooled, ref.scale, "ragged, graph embeddings")
    close(logits, ref.logits, ref.scale, "ragged, logits")


# ---------------------------------------------------------------- 4. configurations
@pytest.fixture(scope="module")
def small():
    return gp.synth_molpcba_batch(24, seed=13)


CONFIGS = [("NUM_TASK 3", dict(num_tasks=3)), ("sum pooling", dict(pooling="sum")), ("max pooling", dict(pooling="max")),
           ("embeddings, node embeddings and node logits", dict(fwd=dict(return_embeddings=True, return_node_embeddings=True, return_node_logits=True))),
           ("all three, NUM_TASK 3", dict(num_tasks=3, fwd=dict(return_embeddings=True, return_node_embeddings=True, return_node_logits=True)))]


@pytest.mark.parametrize("name,cfg", CONFIGS, ids=[n for n, _ in CONFIGS])
def test_configurations(name, cfg, small):
    tasks, pooling, fwd = cfg.get("num_tasks", 1), cfg.get("pooling"), cfg.get("fwd", {})
    w = weights.synth_gcn_weights(seed=7, num_tasks=tasks, emb_dim=300)
    ref = R.forward(small, w, pooling=pooling or "mean", num_tasks=tasks)
    e = make(w, num_tasks=tasks, pooling=pooling)
    got = run(e, small, **fwd)
    e.close()
    got = got if isinstance(got, tuple) else (got,)
    assert got[0].shape == ((small.num_graphs, tasks) if tasks > 1 else (small.num_graphs,))
    close(got[0], ref.logits, ref.scale, (name, "logits"))
    if fwd:
        emb, rows, nlog = got[1], got[2], got[3]
        assert emb.shape == (small.num_graphs, 300) and rows.shape == (small.total_nodes, 300)
        close(emb, ref.pooled, ref.scale, (name, "graph embeddings"))
        close(rows, ref.rows, ref.scale, (name, "node embeddings"))
        close(nlog, R.node_logits(w, ref.rows), ref.scale, (name, "node logits"))


def test_get_h_is_the_rows_the_readout_pools(eng, small, w300):
    ref = R.forward(small, w300)
    run(eng, small)
    rows = eng.final_h()
    assert rows.shape == (small.total_nodes, 300)
    close(rows, ref.rows, ref.scale, "flowgnn_get_h")
    run(eng, small, return_node_embeddings=True)  # (the last stage then writes the caller's buffer: get_h still answers)
    again = eng.final_h()
    assert np.array_equal(again, rows)


# ---------------------------------------------------------------- 5. split accuracy
@pytest.mark.parametrize("seed", R.SEEDS)
def test_split_accuracy(seed, eng):
    """err <= B = sqrt(E_ok * E_bad) for rows and logits on the batches of the CPU separation test: closer to float64 than every wrong
    variant of the three-product split, by the margin the references leave."""
    b, ref, t = R.sep_batch(seed), R.reference(seed), R.golden()[str(seed)]
    logits, rows = run(eng, b, return_node_embeddings=True)
    for name, got in (("rows", rows), ("logits", logits)):
        err = R.err(got, ref, name)
        print(f"seed {seed} {name}: err {err:.3e}  E_ok {t[name]['e_ok']:.3e}  B {t[name]['bound']:.3e}  E_bad {t[name]['e_bad']:.3e}")
        assert err <= t[name]["bound"], (name, err, t[name]["bound"])


# ---------------------------------------------------------------- 6. range and the exact re-run
def test_range_flag_and_exact_rerun(small, w300):
    """BatchNorm 0 scaled (weight and bias alike, so pre_0 scales with them) until some a_1 = relu(pre_0) passes 6e4: one exact re-run,
    the result within the same bound; the unscaled set: none.  Both facts are checked on the reference first."""
    base = R.max_a(small, w300)
    factor = np.float32(8.0e4 / R.max_a_per_layer(small, w300)[0])  # a_1 = relu(pre_0) is what the scaled BatchNorm moves
    above = dict(w300)
    for k in ("bn_weight", "bn_bias"):
        a = np.asarray(w300[k], np.float32).copy()
        a[0] *= factor
        above[k] = a
    assert base < 6.0e4 and R.max_a(small, above) > 6.6e4, (base, R.max_a(small, above))
    ref = R.forward(small, above)
    e = make(above)
    logits, rows = run(e, small, expect_reruns=1, return_node_embeddings=True)
    assert e.exact_reruns() == 1
    close(rows, ref.rows, ref.scale, "range re-run, rows")
    close(logits, ref.logits, ref.scale, "range re-run, logits")
    e.set_weights(w300)
    ref = R.forward(small, w300)
    logits = run(e, small, expect_reruns=0)
    assert e.exact_reruns() == 1
    e.close()
    close(logits, ref.logits, ref.scale, "the unscaled set, logits")


# ---------------------------------------------------------------- 7. bit identity
def test_permuted_batch_slice_and_second_run_give_each_graph_the_same_bits(eng):
    sink = graph(41, [(i, 0) for i in range(1, 41)], 9)
    big = gp.concat_batches([gp.synth_molpcba_batch(120, seed=17), sink, path(200, 10), isolated(1, 11), isolated(1, 12)])
    G = big.num_graphs
    perm = np.random.default_rng(5).permutation(G)
    shuffled = gp.concat_batches([big.slice(int(i), int(i) + 1) for i in perm])
    a_logits, a_rows = run(eng, big, return_node_embeddings=True)
    again_logits, again_rows = run(eng, big, return_node_embeddings=True)
    assert np.array_equal(again_logits, a_logits) and np.array_equal(again_rows, a_rows)  # two runs are identical
    b_logits, b_rows = run(eng, shuffled, return_node_embeddings=True)
    part = run(eng, big.slice(7, 60), return_node_embeddings=True)
    assert np.array_equal(b_logits, a_logits[perm])
    off, soff = big.node_offsets(), shuffled.node_offsets()
    for k, i in enumerate(perm):
        assert np.array_equal(b_rows[soff[k]:soff[k + 1]], a_rows[off[i]:off[i + 1]]), (k, i)
    assert np.array_equal(part[0], a_logits[7:60]) and np.array_equal(part[1], a_rows[off[7]:off[60]])


def test_device_batches_and_group_give_the_same_bits(small, w300, eng):
    ref = R.forward(small, w300)
    want, want_emb = run(eng, small, return_embeddings=True)
    close(want, ref.logits, ref.scale, "one engine")
    pytest.importorskip("torch")
    from tests.test_device_batch_gpu import device_args
    for layout in ("pyg", "reference"):
        args, kw = device_args(small, layout, "GCN")
        got, emb, rows = eng.forward_device(*args, return_embeddings=True, return_node_embeddings=True, **kw)
        eng.sync()
        assert emb.shape == (small.num_graphs, 300) and rows.shape == (small.total_nodes, 300)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(emb.cpu().numpy(), want_emb), layout
    g = EngineGroup("GCN", [0, 0])
    g.set_model_emb_dim(300)
    assert g.emb_dim == 300
    g.set_weights(w300)
    g.set_embeddings(True)
    got = g.forward(small)
    emb = g.embeddings()
    g.close()
    assert emb.shape == (small.num_graphs, 300)
    assert np.array_equal(got, want) and np.array_equal(emb, want_emb)


def test_back_at_width_100_the_engine_is_what_it_was(small, w300):
    w100 = weights.synth_gcn_weights(seed=7)
    fresh = Engine("GCN", device=0)
    fresh.set_weights(w100)
    fresh.profile_enable(True)
    names_fresh = launched(fresh, lambda: fresh.forward(small))
    want = fresh.results().copy()
    fresh.close()
    assert "gcn_resident" in names_fresh
    e = make(w300)
    run(e, small)
    e.set_model_emb_dim(100)
    assert e.emb_dim == 100
    e.set_weights(w100)
    names = launched(e, lambda: e.forward(small))
    got = e.results().copy()
    e.close()
    assert names == names_fresh and WIDE_SLOT not in names, (names, names_fresh)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- 8. the exported checkpoint through the host CLI
def test_host_cli_runs_an_exported_300_wide_checkpoint(tmp_path):
    sd = R.state_dict(seed=4)
    b = gp.synth_molpcba_batch(40, seed=3)
    gdir, wdir = tmp_path / "graphs", tmp_path / "weights"
    gp.write_pack(b, str(gdir))
    export.export_weights("GCN", sd, str(wdir), emb_dim=300)
    assert os.listdir(wdir) == [weights.gcn_file(300)]
    out = tmp_path / "HLS_output.txt"
    cmd = [HOST, "GCN", "--emb-dim", "300", "--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--out", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    ref = R.forward(b, weights.load_gcn_weights(str(wdir), emb_dim=300))
    want = R.ogb_forward(sd, b)
    close(got, ref.logits, ref.scale, "host GCN --emb-dim 300, against the files' float64 forward")
    close(got, want, ref.scale, "host GCN --emb-dim 300, against the state_dict's own forward")
    e = Engine("GCN", device=0)  # ... and the Python wrapper's route to the same file
    e.set_model_emb_dim(300)
    e.load_weights_dir(str(wdir))
    got = e.forward(b)
    e.close()
    close(got, want, ref.scale, "load_weights_dir at width 300")
    p = subprocess.run(cmd + ["--ogb-vn"], capture_output=True, text=True, timeout=300)  # gcn-virtual has no 300-wide form
    assert p.returncode != 0 and "--ogb-vn" in p.stderr and "300" in p.stderr and "flowgnn_set_gcn_virtual_node" in p.stderr, p.stdout + p.stderr
