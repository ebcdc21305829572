"""GCN at OGB's default width without a GPU (flowgnn.h: flowgnn_set_model_emb_dim): the float64 reference that
tests/test_gcn_wide_gpu.py compares against, the weight file at width 300, the exporter, and the separation of the split-f16 product
from its wrong variants on the references alone."""
import json
import os

import numpy as np
import pytest

from flowgnn_amd import export, graphpack as gp, weights
from tests import gcn_wide_ref as R, numpy_ref, split_ref
from tests.test_export import ogb_state_dict


def test_forward_at_width_100_is_numpy_refs():
    b = gp.concat_batches([gp.synth_molpcba_batch(24, seed=5), gp.synth_molhiv_batch(8, seed=6)])
    for tasks in (1, 3):
        w = weights.synth_gcn_weights(seed=7, num_tasks=tasks)
        want = numpy_ref.gcn_forward(b, w)
        got = R.forward(b, w, num_tasks=tasks)
        assert got.logits.shape == want.shape and np.abs(got.logits - want).max() <= 1e-12
        assert got.rows.shape == (b.total_nodes, 100) and got.pooled.shape == (b.num_graphs, 100)
        assert got.scale >= max(1.0, float(np.abs(got.rows).max()))
    # ... and the rows are the ones split_ref restates from x_4 (numpy_ref returns no rows)
    w = weights.synth_gcn_weights(seed=7)
    _, xs = numpy_ref.gcn_forward(b, w, return_x=True)
    assert np.abs(R.forward(b, w).rows - split_ref.gcn_rows(b, w, xs[4])).max() <= 1e-12


def test_forward_uses_dense_for_four_products():
    b = gp.synth_molpcba_batch(4, seed=5)
    rec = split_ref.Recorder()
    R.forward(b, weights.synth_gcn_weights(seed=7, emb_dim=300), dense=rec)
    assert len(rec.inputs) == 4 and all(a.shape == (b.total_nodes, 300) for a in rec.inputs)


def test_widths_names_and_shapes():
    assert weights.GCN_EMB_DIMS == (100, 300)
    assert weights.gcn_file(100) == weights.GCN_FILE and weights.gcn_file(300) == "gcn_ep1_dim300.weights.all.bin"
    assert weights.gcn_shapes(100) == weights.GCN_SHAPES
    assert weights.gcn_shapes(300)["convs_weight"] == (5, 300, 300) and weights.gcn_shapes(300)["graph_pred_bias"] == (1,)
    for bad in (0, 200):
        with pytest.raises(ValueError):
            weights.gcn_file(bad)
    a, b = weights.synth_gcn_weights(seed=7), weights.synth_gcn_weights(seed=7, emb_dim=100)
    assert all(np.array_equal(a[k], b[k]) for k in a)  # at 100 the values are what they always were
    w = weights.synth_gcn_weights(seed=7, emb_dim=300)
    assert {k: v.shape for k, v in w.items()} == dict(weights.gcn_shapes(300))
    ratio = float(np.std(w["convs_weight"]) / np.std(a["convs_weight"]))
    assert abs(ratio - np.sqrt(100.0 / 300.0)) < 0.02, ratio


@pytest.mark.parametrize("tasks", [1, 3])
def test_file_round_trip_size_and_offsets_at_300(tmp_path, tasks):
    D = 300
    w = weights.synth_gcn_weights(seed=9, num_tasks=tasks, emb_dim=D)
    weights.save_gcn_weights(w, str(tmp_path))
    assert os.listdir(tmp_path) == ["gcn_ep1_dim300.weights.all.bin"]
    back = weights.load_gcn_weights(str(tmp_path), num_tasks=tasks, emb_dim=D)
    assert list(back) == list(w) and all(np.array_equal(back[k], w[k]) for k in w)
    layer, bn0 = D * D + 15 * D, 173 * D + 5 * (D * D + 15 * D)
    head = bn0 + 5 * (4 * D + 1)
    flat = np.fromfile(tmp_path / "gcn_ep1_dim300.weights.all.bin", dtype="<f4")
    assert flat.size == head + (D + 1) * tasks and os.path.getsize(tmp_path / "gcn_ep1_dim300.weights.all.bin") == 4 * flat.size
    assert np.array_equal(flat[:173 * D], w["node_embedding_weight"].ravel())
    for l in (0, 2, 4):
        base = 173 * D + l * layer
        assert np.array_equal(flat[base:base + D * D], w["convs_weight"][l].ravel())
        assert np.array_equal(flat[base + D * D:base + D * D + D], w["convs_bias"][l])
        assert np.array_equal(flat[base + D * D + D:base + D * D + 2 * D], w["convs_root_emb_weight"][l])
        assert np.array_equal(flat[base + D * D + 2 * D:base + layer], w["edge_embedding_weight"][l].ravel())
        bn = bn0 + l * (4 * D + 1)
        for i, k in enumerate(("bn_weight", "bn_bias", "bn_mean", "bn_var")):
            assert np.array_equal(flat[bn + i * D:bn + (i + 1) * D], w[k][l])
        assert flat[bn + 4 * D] == 0.0  # the skipped counter
    assert np.array_equal(flat[head:head + D * tasks], w["graph_pred_weights"].ravel())
    assert np.array_equal(flat[head + D * tasks:], w["graph_pred_bias"])
    with pytest.raises(ValueError, match="300.*100|100.*300"):
        weights.save_gcn_weights(w, str(tmp_path), emb_dim=100)


def test_the_four_offsets_at_100_are_todays():
    off = weights._gcn_offsets(1, 100)
    assert off[("convs_weight", 0)] == 17300 and off[("convs_weight", 1)] - off[("convs_weight", 0)] == 11500
    assert off[("bn_weight", 0)] == 74800 and off[("graph_pred_weights", None)] == 76805 and off[("graph_pred_bias", None)] == 76905
    assert weights._gcn_offsets(1) == off


def test_exporter_at_300_agrees_with_ogbs_forward(tmp_path):
    sd = R.state_dict(seed=4, tasks=3)
    b = gp.synth_molpcba_batch(24, seed=10)
    want = R.ogb_forward(sd, b)
    w = export.export_weights("GCN", sd, str(tmp_path), multi_task=True, emb_dim=300)
    assert os.listdir(tmp_path) == ["gcn_ep1_dim300.weights.all.bin"]
    back = weights.load_gcn_weights(str(tmp_path), num_tasks=3, emb_dim=300)
    assert all(np.array_equal(back[k], w[k]) for k in w)
    got = R.forward(b, back, num_tasks=3).logits
    assert np.allclose(got, want, rtol=1e-4, atol=2e-5), np.abs(got - want).max()  # float32 files vs float64 source
    same = export.gcn_weights_from_ogb_state_dict(sd, multi_task=True, emb_dim=300)
    assert all(np.array_equal(same[k], w[k]) for k in w)


def test_exporter_refusals():
    wide, narrow = R.state_dict(seed=4), ogb_state_dict("gcn", 4)
    with pytest.raises(export.ExportError, match="does not fit"):  # without the keyword: refused as it always was
        export.gcn_weights_from_ogb_state_dict(wide)
    with pytest.raises(export.ExportError, match="100 wide and emb_dim is 300"):
        export.gcn_weights_from_ogb_state_dict(narrow, emb_dim=300)
    with pytest.raises(export.ExportError, match="100.*300"):
        export.gcn_weights_from_ogb_state_dict(narrow, emb_dim=200)
    vn = R.state_dict(seed=4, virtual_node=True)
    with pytest.raises(export.ExportError, match="gcn-virtual"):
        export.gcn_weights_from_ogb_state_dict(vn, emb_dim=300)
    with pytest.raises(export.ExportError, match="emb_dim 300.*100 only"):
        export.gcn_weights_from_ogb_state_dict(vn, emb_dim=300, virtual_node=True)
    with pytest.raises(export.ExportError, match="emb_dim 300.*100 only"):
        export.export_weights("GCN", vn, "/nonexistent-directory", virtual_node=True, emb_dim=300)
    with pytest.raises(export.ExportError, match="GCN's keyword"):
        export.export_weights("GIN", narrow, "/nonexistent-directory", emb_dim=300)
    assert export.gcn_weights_from_ogb_state_dict(narrow, emb_dim=100)["convs_weight"].shape == (5, 100, 100)


# ---------------------------------------------------------------- the separation table
def test_the_seed_list_is_the_smallest_seeds():
    assert R.SEEDS == (0, 1) and sorted(R.SEEDS_TRIED) == [0, 1]  # seeds 0 and 1 reach both ratios: nothing else was tried
    assert R.sep_batch(0).num_graphs == 256
    assert [s.name for s in R.variants()] == [s.name for s in split_ref.VARIANTS if "K tail" not in s.name and "o_3" not in s.name]


@pytest.mark.parametrize("seed", R.SEEDS)
def test_split_product_is_separated_from_its_wrong_variants(seed):
    """E_bad / E_ok >= split_ref.min_ratio("GCN", output) for rows (64) and logits (16) at width 300, on the references alone;
    B = sqrt(E_ok * E_bad) is the bound of tests/test_gcn_wide_gpu.py's split-accuracy case, and the committed table is this one."""
    t = R.table(seed)
    gold = R.golden()[str(seed)]
    for name in R.SEP_OUTPUTS:
        row = t[name]
        ratio = row.e_bad / row.e_ok
        print(f"seed {seed} {name}: E_ok {row.e_ok:.3e}  B {row.bound:.3e}  E_bad {row.e_bad:.3e}  ratio {ratio:.1f}  closest: {min(row.bad, key=row.bad.get)}")
        assert ratio >= split_ref.min_ratio("GCN", name), (name, ratio, row.ok, row.bad)
        assert abs(ratio - R.SEEDS_TRIED[seed][0 if name == "rows" else 1]) < 0.06
        for k in ("e_ok", "e_bad", "bound"):
            assert abs(gold[name][k] - getattr(row, k)) <= 1e-6 * getattr(row, k), (name, k, gold[name][k], getattr(row, k))
    # every wrong variant is wrong: "last layer" reaches the fourth product (the count starts at 1), the bias variant changes b_1..b_4 only
    assert all(v > t["rows"].e_ok for v in t["rows"].bad.values())
    w = R.sep_weights()
    mis = R.misplaced_unscale(w)
    assert np.array_equal(mis["convs_bias"][0], w["convs_bias"][0]) and not np.array_equal(mis["convs_bias"][1], w["convs_bias"][1])


def test_golden_file_holds_the_two_seeds():
    with open(R.GOLDEN) as f:
        g = json.load(f)
    assert sorted(g) == [str(s) for s in R.SEEDS]
    for seed in g:
        assert sorted(g[seed]) == sorted(R.SEP_OUTPUTS)
