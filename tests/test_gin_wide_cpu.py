"""GIN at OGB's default width (flowgnn.h: flowgnn_set_emb_dim), everything that needs no GPU: the float64 reference of
tests/gin_wide_ref.py against tests/numpy_ref.py, the exporter and the weight files at width 300, the unchanged default of
weights.synth_gin_weights, and the separation of the split-f16 product from its wrong variants that tests/test_gin_wide_gpu.py's
bound rests on."""
import hashlib
import os

import numpy as np
import pytest

from flowgnn_amd import export, graphpack as gp, weights
from tests import gin_wide_ref as R, numpy_ref, split_ref
from tests.test_export import ogb_state_dict

# SHA-256 of the eight arrays of weights.synth_gin_weights() end to end, computed on the commit before `emb_dim` existed
SYNTH_DEFAULT_SHA256 = "083fba48a4fccf176af76f68f10d243fc359159dbdcb172fa471d7da905bc345"
DIM300_FILES = ["gin_ep1_nd_embed_dim300.bin", "gin_ep1_ed_embed_dim300.bin", "gin_ep1_mlp_1_weights_dim300.bin", "gin_ep1_mlp_1_bias_dim300.bin",
                "gin_ep1_mlp_2_weights_dim300.bin", "gin_ep1_mlp_2_bias_dim300.bin", "gin_ep1_pred_weights_dim300.bin", "gin_ep1_pred_bias_dim300.bin"]
WIDE_SHAPES = [(173, 300), (5, 13, 300), (5, 600, 300), (5, 600), (5, 300, 600), (5, 300)]


def test_at_width_100_it_is_numpy_ref():
    b = gp.synth_molhiv_batch(64, seed=3)
    w = weights.synth_gin_weights(seed=7)
    want, hs = numpy_ref.gin_forward(b, w, return_h=True)
    got = R.forward(b, w)
    assert np.abs(got.logits - want).max() <= 1e-12 and np.abs(got.rows - hs[-1]).max() <= 1e-12
    got0 = R.forward(b, w, eps=np.zeros(5, np.float32))
    assert np.array_equal(got0.logits, got.logits)
    w3 = weights.synth_gin_weights(seed=7, num_tasks=3)
    assert np.abs(R.forward(b, w3, num_tasks=3).logits - numpy_ref.gin_forward(b, w3)).max() <= 1e-12


@pytest.mark.parametrize("tasks", [1, 128])
def test_exported_300_wide_tensors_reproduce_the_unfolded_state_dict_forward(tasks):
    """Both BatchNorms folded, eps kept, graph_pred_linear mapped: the float64 forward of the exporter's folded tensors (before the
    float32 cast) against OGB's own forward with nothing folded, within 1e-9; then the float32 tensors at float32's precision."""
    sd = R.state_dict(seed=3, tasks=tasks)
    b = gp.synth_molhiv_batch(24, seed=9)
    want = R.ogb_forward(sd, b)
    assert want.shape == ((24, 128) if tasks == 128 else (24,))
    w64, eps64 = R.exported_unrounded(sd, multi_task=tasks > 1)
    got = R.forward(b, w64, eps=eps64, eps_f64=True, num_tasks=tasks).logits
    assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), np.abs(got - want).max()
    w32 = export.gin_weights_from_ogb_state_dict(sd, keep_eps=True, multi_task=tasks > 1)
    assert [w32[k].shape for k in list(w32)[:6]] == WIDE_SHAPES and w32["graph_pred_weights"].shape == (tasks, 300)
    assert all(a.dtype == np.float32 for a in w32.values())
    got32 = R.forward(b, w32, eps=export.gin_eps_from_ogb_state_dict(sd), num_tasks=tasks).logits
    assert np.allclose(got32, want, rtol=1e-4, atol=2e-5), np.abs(got32 - want).max()


def test_export_writes_the_dim300_set_and_it_round_trips(tmp_path):
    sd = R.state_dict(seed=4)
    w = export.export_weights("GIN", sd, str(tmp_path), keep_eps=True)
    assert sorted(os.listdir(tmp_path)) == sorted(DIM300_FILES + ["gin_ep1_eps_dim300.bin"])
    assert os.path.getsize(tmp_path / "gin_ep1_mlp_1_weights_dim300.bin") == 5 * 600 * 300 * 4
    back = weights.load_gin_weights(str(tmp_path), emb_dim=300)
    assert list(back) == list(w) and all(np.array_equal(back[k], w[k]) for k in w)
    assert np.array_equal(weights.load_gin_eps(str(tmp_path), emb_dim=300), np.asarray(R.TRAINED_EPS, np.float32))


def test_save_and_load_name_the_files_by_the_width(tmp_path):
    w = weights.synth_gin_weights(seed=5, num_tasks=3, emb_dim=300)
    weights.save_gin_weights(w, str(tmp_path / "a"))  # the width from the arrays
    weights.save_gin_weights(w, str(tmp_path / "b"), emb_dim=300, eps=[0.1, 0.2, 0.3, 0.4, 0.5])
    for d in ("a", "b"):
        assert sorted(os.listdir(tmp_path / d)) == sorted(DIM300_FILES + ["gin_ep1_eps_dim300.bin"])
        back = weights.load_gin_weights(str(tmp_path / d), num_tasks=3, emb_dim=300)
        assert all(np.array_equal(back[k], w[k]) for k in w)
    assert [f for f, _ in weights.gin_files(300).values()] == DIM300_FILES
    w100 = weights.synth_gin_weights(seed=5)
    weights.save_gin_weights(w100, str(tmp_path / "c"))
    assert sorted(os.listdir(tmp_path / "c")) == sorted([f for f, _ in weights.GIN_FILES.values()] + ["gin_ep1_eps_dim100.bin"])
    with pytest.raises(ValueError):
        weights.gin_files(200)


def test_the_default_synthetic_weights_are_the_parents():
    w = weights.synth_gin_weights()
    assert hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in w.values())).hexdigest() == SYNTH_DEFAULT_SHA256
    assert all(np.array_equal(a, b) for a, b in zip(w.values(), weights.synth_gin_weights(seed=7, num_tasks=1, emb_dim=100).values()))
    w3 = weights.synth_gin_weights(seed=7, emb_dim=300)
    assert [w3[k].shape for k in list(w3)[:6]] == WIDE_SHAPES


@pytest.mark.parametrize("width", [200, 301])
def test_other_widths_are_refused_naming_both(width):
    with pytest.raises(export.ExportError, match="100.*300"):
        export.gin_weights_from_ogb_state_dict(R.state_dict(seed=3, width=width, eps=None))


def test_a_300_wide_gin_virtual_is_refused_even_when_asked_for():
    sd = R.state_dict(seed=3, virtual_node=True)
    for vn in (False, True):
        with pytest.raises(export.ExportError, match="100-wide"):
            export.gin_weights_from_ogb_state_dict(sd, keep_eps=True, virtual_node=vn)
    with pytest.raises(export.ExportError, match="100-wide"):
        export.export_weights("GIN", sd, "/tmp/unused", keep_eps=True, virtual_node=True)


def test_gcn_at_300_fails_as_it_did():
    sd = ogb_state_dict("gcn", 4)
    wide = {k: np.tile(v, [3 if n == 100 else 1 for n in np.shape(v)]) for k, v in sd.items()}  # every axis of 100 becomes 300
    assert wide["gnn_node.convs.0.linear.weight"].shape == (300, 300)
    with pytest.raises(export.ExportError, match="does not fit"):
        export.gcn_weights_from_ogb_state_dict(wide)


@pytest.mark.parametrize("seed", R.SEEDS)
def test_split_product_is_separated_from_its_wrong_variants(seed):
    """E_bad / E_ok >= split_ref.MIN_RATIO for logits and rows at width 300, on the references alone; B = sqrt(E_ok * E_bad) is the
    bound of tests/test_gin_wide_gpu.py's split-accuracy case."""
    t = R.table(seed)
    for name in R.SEP_OUTPUTS:
        row = t[name]
        print(f"seed {seed} {name}: E_ok {row.e_ok:.3e} E_bad {row.e_bad:.3e} ratio {row.e_bad / row.e_ok:.1f} B {row.bound:.3e} "
              f"closest: {min(row.bad, key=row.bad.get)}")
        assert row.e_ok > 0 and row.e_bad / row.e_ok >= split_ref.MIN_RATIO, (name, row.e_ok, row.e_bad, row.bad)
        assert row.e_ok < row.bound < row.e_bad
    assert len(R.variants()) == len(split_ref.VARIANTS) - 3
    # the entries left out cannot show at this width: the reference computes the correct product for them
    b = gp.synth_molhiv_batch(4, seed=seed)
    w = R.sep_weights()
    ok = R.forward(b, w, dense=split_ref.SplitDense("GIN", split_ref.OK_SPECS[0]))
    for spec in split_ref.VARIANTS:
        if spec.tail == "single":
            assert np.array_equal(R.forward(b, w, dense=split_ref.SplitDense("GIN", spec)).rows, ok.rows)
