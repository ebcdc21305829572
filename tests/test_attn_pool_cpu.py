"""OGB's attention readout without a GPU (tests/attn_pool_ref.py): what the references alone establish, so that
tests/test_attn_pool_gpu.py can rely on it.

Input: the width-300 synthetic GIN weights of tests/gin_wide_ref.sep_weights(), the gate weights.synth_attention_pooling(seed=11), 64
molhiv-shaped graphs at batch seeds 5 and 7, and the rows of the float64 forward cast to float32 (what an engine hands its readout).
  1. every semantic wrong form of the readout is at least 50 x the project's 1e-4 rule away from the definition;
  2. the split-f16 table of the readout alone: E_bad / E_ok >= 16 (split_ref.LOW_RATIO's value) for `pooled` and `logits`;
  3. the exporter: torch model -> attention_pooling_from_ogb_state_dict -> float64 readout equals the torch model to 1e-9;
  4. the file round trip keeps the bits."""
import functools

import numpy as np
import pytest

from flowgnn_amd import export, graphpack as gp, weights
from tests import attn_pool_ref as A, gin_wide_ref as W

SEEDS = (5, 7)
GRAPHS = 64
MIN_SEMANTIC = 50 * 1e-4  # in units of max(max |rows|, max |s|)
MIN_RATIO = 16.0          # split_ref.LOW_RATIO's value


@functools.lru_cache(maxsize=None)
def case(seed):
    """(batch, rows float32, gate, pw, pb) of one batch seed."""
    b, w = gp.synth_molhiv_batch(GRAPHS, seed=seed), W.sep_weights()
    rows = W.forward(b, w).rows.astype(np.float32)
    return b, rows, weights.synth_attention_pooling(seed=11), np.asarray(w["graph_pred_weights"]), np.asarray(w["graph_pred_bias"])


def test_synth_gate_is_what_the_header_says():
    g = weights.synth_attention_pooling(seed=11)
    rng = np.random.default_rng(11)
    w1 = (rng.standard_normal((600, 300)) / np.sqrt(300)).astype(np.float32)
    b1 = (0.5 * rng.standard_normal(600)).astype(np.float32)
    w2 = (8.0 * rng.standard_normal(600) / np.sqrt(600)).astype(np.float32)
    assert list(g) == ["w1", "b1", "w2"] and all(v.dtype == np.float32 for v in g.values())
    assert np.array_equal(g["w1"], w1) and np.array_equal(g["b1"], b1) and np.array_equal(g["w2"], w2)


@pytest.mark.parametrize("seed", SEEDS)
def test_one_node_graphs_and_alpha(seed):
    """The definition's own corners: alpha sums to one per graph (pooled of constant rows is that constant), and a one-node graph's
    pooled row is its row."""
    b, rows, gate, pw, pb = case(seed)
    off = b.node_offsets()
    r = np.concatenate([rows[: off[3]], rows[:1], rows[5:6], rows[7:8]])  # three graphs, then three one-node graphs
    single = gp.GraphBatch(np.array([1, 1, 1], np.int32), np.zeros(3, np.int32), b.node_feature[:3], np.zeros((0, 2), np.int32), np.zeros((0, 3), np.int32))
    bb = gp.concat_batches([b.slice(0, 3), single])
    pooled, _, _ = A.readout(r, bb, gate, pw, pb)
    assert np.array_equal(pooled[3:], r[off[3]:].astype(np.float64))
    const = np.ones_like(rows) * np.float32(0.75)
    const[:, 0] = rows[:, 0]  # (the gates differ from node to node, the other columns are constant)
    pooled, _, _ = A.readout(const, b, gate, pw, pb)
    assert np.abs(pooled[:, 1:] - 0.75).max() < 1e-12


@pytest.mark.parametrize("seed", SEEDS)
def test_semantic_variants_are_far_from_the_definition(seed):
    b, rows, gate, pw, pb = case(seed)
    stats = {}
    pooled, _, s = A.readout(rows, b, gate, pw, pb, stats=stats)
    unit = max(float(np.abs(rows).max()), float(np.abs(s).max()))
    off = b.node_offsets()
    spread = np.mean([s[off[g]:off[g + 1]].max() - s[off[g]:off[g + 1]].min() for g in range(b.num_graphs)])
    seg = np.repeat(np.arange(b.num_graphs), np.diff(off))
    e = np.exp(s - np.maximum.reduceat(s, off[:-1])[seg])
    top = np.mean(1.0 / np.add.reduceat(e, off[:-1]))
    print(f"seed {seed}: unit {unit:.3f}, mean gate spread within a graph {spread:.2f}, mean largest alpha {top:.2f}")
    for k in A.WRONG:
        bad, _, _ = A.readout(rows, b, gate, pw, pb, **{k: True})
        d = A.err(bad, pooled, unit) / 1e-4
        print(f"seed {seed}: {A.WRONG_NAMES[k]:32s} {d:10.0f} x 1e-4 units")
        assert d >= 50, (k, d)


@pytest.mark.parametrize("seed", SEEDS)
def test_split_table(seed):
    b, rows, gate, pw, pb = case(seed)
    t = A.table(rows, b, gate, pw, pb)
    for name in A.OUTPUTS:
        r = t[name]
        closest = min(r.bad, key=r.bad.get)
        print(f"seed {seed} {name}: E_ok {r.e_ok:.3e}  B {r.bound:.3e}  E_bad {r.e_bad:.3e}  ratio {r.e_bad / r.e_ok:.1f}  closest: {closest}")
        assert r.e_bad / r.e_ok >= MIN_RATIO, (name, r.e_ok, r.e_bad)


# ---------------------------------------------------------------- the exporter
@pytest.fixture(scope="module")
def torch_model():
    pytest.importorskip("torch")
    return A.attention_model("gin", False, emb_dim=300)


def test_exporter_equals_the_torch_model(torch_model):
    from tests import ogb_torch as T
    sd = torch_model.state_dict()
    assert {"pool.gate_nn.0.weight", "pool.gate_nn.0.bias", "pool.gate_nn.1.running_mean", "pool.gate_nn.1.running_var",
            "pool.gate_nn.3.weight", "pool.gate_nn.3.bias"} <= set(sd)
    bn = torch_model.pool.gate_nn[1]
    assert float(bn.running_mean.abs().max()) > 0.1 and float((bn.running_var - 1).abs().max()) > 0.1  # non-trivial statistics
    b = T.gin_batch()
    want, _, _ = T.run(torch_model, b)
    real = export._checked
    try:  # the exporter's own functions with the float32 cast taken out (tests/gin_wide_ref.exported_unrounded)
        export._checked = lambda w, spec, shape_of: {k: np.asarray(w[k], np.float64).reshape(tuple(shape_of(k, v))) for k, v in spec.items()}
        gate = export.attention_pooling_from_ogb_state_dict(sd)
    finally:
        export._checked = real
    assert set(gate) == {"w1", "b1", "w2"}  # pool.gate_nn.3.bias is dropped
    pw, pb = sd["graph_pred_linear.weight"].numpy(), sd["graph_pred_linear.bias"].numpy()
    pooled, logits, _ = A.readout(want.rows, b, gate, pw, pb)
    assert np.abs(pooled - want.pooled).max() <= 1e-9 * np.abs(want.pooled).max()
    assert np.abs(logits - want.logits).max() <= 1e-9 * max(1.0, np.abs(want.logits).max())
    # ... and omitting the fold is detected: the unfolded W1, b1 give another result
    raw = dict(gate, w1=sd["pool.gate_nn.0.weight"].numpy(), b1=sd["pool.gate_nn.0.bias"].numpy())
    unfolded, _, _ = A.readout(want.rows, b, raw, pw, pb)
    assert np.abs(unfolded - want.pooled).max() > 1e-3 * np.abs(want.pooled).max()
    # ... and the float32 tensors the engine gets are the float64 ones rounded
    g32 = export.attention_pooling_from_ogb_state_dict(sd)
    assert all(g32[k].dtype == np.float32 and np.array_equal(g32[k], gate[k].astype(np.float32)) for k in gate)


def test_exporter_refusals(torch_model, tmp_path):
    sd = torch_model.state_dict()
    plain = {k: v for k, v in sd.items() if not k.startswith("pool.gate_nn")}
    with pytest.raises(export.ExportError, match="pool.gate_nn.0.weight"):
        export.attention_pooling_from_ogb_state_dict(plain)
    with pytest.raises(export.ExportError, match="300"):
        export.attention_pooling_from_ogb_state_dict(sd, emb_dim=100)
    short = dict(sd)
    short["pool.gate_nn.3.weight"] = sd["pool.gate_nn.3.weight"][:, :599]
    with pytest.raises(export.ExportError, match="pool.gate_nn.3.weight"):
        export.attention_pooling_from_ogb_state_dict(short)
    # export_weights: without the keyword an attention checkpoint is refused; with it a plain one is, before any file is written
    with pytest.raises(export.ExportError, match="attention"):
        export.export_weights("GIN", sd, str(tmp_path / "a"), keep_eps=True)
    with pytest.raises(export.ExportError, match="pool.gate_nn"):
        export.export_weights("GIN", plain, str(tmp_path / "b"), keep_eps=True, attention_pooling=True)
    assert not (tmp_path / "a").exists() and not (tmp_path / "b").exists()
    with pytest.raises(export.ExportError, match="attention_pooling"):
        export.export_weights("GIN-VN", sd, str(tmp_path / "c"), attention_pooling=True)


def test_export_weights_writes_the_file(torch_model, tmp_path):
    sd = torch_model.state_dict()
    export.export_weights("GIN", sd, str(tmp_path), keep_eps=True, attention_pooling=True)
    path = tmp_path / "gin_ep1_attnpool_dim300.bin"
    assert path.stat().st_size == 4 * 181200
    got = weights.load_attention_pooling(str(tmp_path), model="GIN")
    want = export.attention_pooling_from_ogb_state_dict(sd)
    assert all(np.array_equal(got[k], want[k]) for k in want)


# ---------------------------------------------------------------- files
@pytest.mark.parametrize("model", ["GIN", "GCN"])
def test_file_round_trip(model, tmp_path):
    gate = weights.synth_attention_pooling(seed=11)
    weights.save_attention_pooling(gate, str(tmp_path), model=model)
    name = {"GIN": "gin_ep1_attnpool_dim300.bin", "GCN": "gcn_ep1_attnpool_dim300.bin"}[model]
    raw = np.fromfile(tmp_path / name, dtype="<f4")
    assert raw.size == 181200
    assert np.array_equal(raw.view(np.uint32), np.concatenate([gate[k].ravel() for k in ("w1", "b1", "w2")]).view(np.uint32))
    back = weights.load_attention_pooling(str(tmp_path), model=model)
    assert list(back) == ["w1", "b1", "w2"]
    assert all(np.array_equal(back[k].view(np.uint32), gate[k].view(np.uint32)) and back[k].shape == gate[k].shape for k in gate)
    with open(tmp_path / name, "r+b") as f:
        f.truncate(4 * 181199)
    with pytest.raises(IOError):
        weights.load_attention_pooling(str(tmp_path), model=model)
    with pytest.raises(ValueError):
        weights.save_attention_pooling(dict(gate, w1=gate["w1"][:, :100]), str(tmp_path), model=model)
    with pytest.raises(ValueError):
        weights.attention_pooling_file("PNA")
