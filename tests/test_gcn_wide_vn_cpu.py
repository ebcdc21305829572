"""OGB's gcn-virtual at width 300 without a GPU (flowgnn.h: flowgnn_set_gcn_virtual_node_dim): the reference
forward of tests/gcn_wide_vn_ref.py against the two it generalises, the exporter's virtual_node_dim keyword against OGB's own forward,
the dim300 file, the refusals, the header, the condition on the fixed input -- that it tells every wrong form of the virtual node from
the definition -- and the fixture of the split-accuracy table.  The self-checks of the reference forward hold on any tree, as they
must; every other test here fails on a tree without the width-carrying call."""
import json
import os
import re

import numpy as np
import pytest

from flowgnn_amd import export, graphpack as gp, weights
from flowgnn_amd.export import ExportError
from tests import gcn_vn_ref, gcn_wide_ref as R, gcn_wide_vn_ref as V, split_ref
from tests.parity import REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("variant", [None] + V.VARIANTS)
def test_at_width_100_the_forward_is_gcn_vn_refs(variant):
    b = gp.synth_molhiv_batch(24, seed=5)
    w, vn = weights.synth_gcn_weights(seed=7), gcn_vn_ref.fixed_virtual_node()
    for pooling in ("mean", "sum", "max"):
        want = gcn_vn_ref.forward(b, w, vn, variant=variant, pooling=pooling, return_x4=True)
        got = V.forward(b, w, vn, variant=variant, pooling=pooling)
        assert np.abs(got.logits - want[0]).max() <= 1e-12 and np.abs(got.rows - want[1]).max() <= 1e-12
        assert abs(got.scale - want[2]) <= 1e-12 * want[2] and np.abs(got.x4 - want[3]).max() <= 1e-12


def test_with_zero_tensors_the_forward_is_gcn_wide_refs():
    b = gp.synth_molpcba_batch(24, seed=5)
    w = weights.synth_gcn_weights(seed=7, emb_dim=300)
    want, got = R.forward(b, w), V.forward(b, w, V.zero_virtual_node())
    assert np.array_equal(got.logits, want.logits) and np.array_equal(got.rows, want.rows) and np.array_equal(got.pooled, want.pooled)


def test_the_eight_wrong_forms_are_gcn_vn_refs():
    assert V.VARIANTS is gcn_vn_ref.VARIANTS and len(V.VARIANTS) == 8


# ---------------------------------------------------------------- files
def test_file_names_round_trip_and_size(tmp_path):
    assert weights.gcn_virtual_node_file(100) == weights.GCN_VIRTUAL_NODE_FILE == "gcn_ep1_virtualnode_dim100.bin"
    assert weights.gcn_virtual_node_file(300) == "gcn_ep1_virtualnode_dim300.bin"
    for bad in (0, 200, 301):
        with pytest.raises(ValueError):
            weights.gcn_virtual_node_file(bad)
    vn = weights.synth_gcn_virtual_node(seed=13, emb_dim=300)
    assert {k: v.shape for k, v in vn.items()} == dict(weights.gin_virtual_node_shapes(300))
    narrow = weights.synth_gcn_virtual_node(seed=13)
    assert all(np.array_equal(narrow[k], weights.synth_gin_virtual_node(seed=13)[k]) for k in narrow)  # at 100: what it always was
    target = tmp_path / "not_created"
    with pytest.raises(ValueError):  # without the keyword 300-wide tensors stay refused, before anything is created
        weights.save_gcn_virtual_node(vn, str(target))
    with pytest.raises(ValueError):
        weights.save_gcn_virtual_node(narrow, str(target), emb_dim=300)
    assert not target.exists()
    weights.save_gcn_virtual_node(vn, str(tmp_path), emb_dim=300)
    path = tmp_path / "gcn_ep1_virtualnode_dim300.bin"
    assert path.stat().st_size == 4 * 1443900 and os.listdir(tmp_path) == ["gcn_ep1_virtualnode_dim300.bin"]
    back = weights.load_gcn_virtual_node(str(tmp_path), emb_dim=300)
    assert list(back) == list(vn) and all(np.array_equal(back[k], vn[k]) for k in vn)
    flat = np.fromfile(path, "<f4")  # GIN's order and layout
    assert np.array_equal(flat[:300], vn["vn_embedding"]) and np.array_equal(flat[300:300 + 4 * 600 * 300], vn["w1"].ravel())
    assert np.array_equal(flat[-1200:], vn["b2"].ravel())
    with pytest.raises(IOError):
        weights.load_gcn_virtual_node(str(tmp_path))  # (no dim100 file here)
    with open(path, "r+b") as f:
        f.truncate(4 * 1443899)
    with pytest.raises(IOError):
        weights.load_gcn_virtual_node(str(tmp_path), emb_dim=300)


# ---------------------------------------------------------------- the exporter
@pytest.mark.parametrize("with_bn", [True, False], ids=["with BatchNorms", "without"])
def test_the_exporter_with_virtual_node_dim_reproduces_ogbs_own_forward(with_bn):
    sd = V.vn_state_dict(seed=4, with_bn=with_bn)
    b = gp.synth_molpcba_batch(40, seed=3)
    want = V.ogb_forward(sd, b)
    real = export._checked  # the exporter's own functions with the float32 cast taken out
    try:
        export._checked = lambda w, spec, shape_of: {k: np.asarray(w[k], np.float64).reshape(tuple(shape_of(k, v))) for k, v in spec.items()}
        w = export.gcn_weights_from_ogb_state_dict(sd, virtual_node=True, emb_dim=300, virtual_node_dim=300)
        vn = export.gcn_virtual_node_from_ogb_state_dict(sd, virtual_node_dim=300)
    finally:
        export._checked = real
    got = V.forward(b, w, vn)
    err = float(np.abs(got.logits - want).max())
    print(f"exporter (BatchNorms: {with_bn}): max |folded - OGB's own| = {err:.3e}, logits up to {np.abs(want).max():.3g}")
    assert err <= 1e-9
    # ... and the float32 tensors the engine gets are those, rounded once
    w32 = export.gcn_weights_from_ogb_state_dict(sd, virtual_node=True, emb_dim=300, virtual_node_dim=300)
    vn32 = export.gcn_virtual_node_from_ogb_state_dict(sd, virtual_node_dim=300)
    assert {k: v.shape for k, v in vn32.items()} == dict(weights.gin_virtual_node_shapes(300)) and w32["convs_weight"].shape == (5, 300, 300)
    assert all(v.dtype == np.float32 and np.array_equal(v, vn[k].astype(np.float32)) for k, v in vn32.items())
    assert all(v.dtype == np.float32 and np.array_equal(v, np.asarray(w[k]).astype(np.float32)) for k, v in w32.items())


def test_export_weights_writes_both_dim300_files(tmp_path):
    sd = V.vn_state_dict(seed=4)
    export.export_weights("GCN", sd, str(tmp_path), virtual_node=True, emb_dim=300, virtual_node_dim=300)
    assert sorted(os.listdir(tmp_path)) == ["gcn_ep1_dim300.weights.all.bin", "gcn_ep1_virtualnode_dim300.bin"]
    vn = weights.load_gcn_virtual_node(str(tmp_path), emb_dim=300)
    want = export.gcn_virtual_node_from_ogb_state_dict(sd, virtual_node_dim=300)
    assert all(np.array_equal(vn[k], want[k]) for k in want)


def test_exporter_refusals(tmp_path):
    sd300, sd100 = V.vn_state_dict(seed=4), gcn_vn_ref.vn_state_dict(seed=4)
    # without the keyword the refusal stands, and now names it
    with pytest.raises(ExportError, match="emb_dim 300.*100 only") as ei:
        export.gcn_weights_from_ogb_state_dict(sd300, emb_dim=300, virtual_node=True)
    assert "virtual_node_dim" in str(ei.value)
    with pytest.raises(ExportError, match="emb_dim 300.*100 only") as ei:
        export.export_weights("GCN", sd300, str(tmp_path), virtual_node=True, emb_dim=300)
    assert "virtual_node_dim" in str(ei.value)
    with pytest.raises(ExportError, match="100-wide"):
        export.gcn_virtual_node_from_ogb_state_dict(sd300)
    # the keyword alone is not enough: the weight set without its virtual node is a model nobody trained
    with pytest.raises(ExportError, match="virtual_node=True"):
        export.gcn_weights_from_ogb_state_dict(sd300, emb_dim=300, virtual_node_dim=300)
    # a virtual_node_dim other than emb_dim, or than the state_dict's width
    for call in (lambda: export.export_weights("GCN", sd300, str(tmp_path), virtual_node=True, virtual_node_dim=300),
                 lambda: export.export_weights("GCN", sd100, str(tmp_path), virtual_node=True, virtual_node_dim=300),
                 lambda: export.export_weights("GCN", sd100, str(tmp_path), virtual_node=True, emb_dim=300, virtual_node_dim=300),
                 lambda: export.gcn_weights_from_ogb_state_dict(sd300, emb_dim=300, virtual_node=True, virtual_node_dim=200),
                 lambda: export.gcn_virtual_node_from_ogb_state_dict(sd100, virtual_node_dim=300),
                 lambda: export.export_weights("GIN-VN", sd100, str(tmp_path), virtual_node_dim=300)):
        with pytest.raises(ExportError):
            call()
    assert not os.listdir(tmp_path)  # nothing is written on a refusal
    # the 100-wide route is what it was, with and without the keyword's default
    a = export.gcn_virtual_node_from_ogb_state_dict(sd100)
    b = export.gcn_virtual_node_from_ogb_state_dict(sd100, virtual_node_dim=100)
    assert all(np.array_equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------- the header
def test_the_header_and_the_loader_declare_the_two_functions():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    five = r"const float\* vn_embedding,\s*const float\* w1,\s*const float\* b1,\s*const float\* w2,\s*const float\* b2\)"
    assert re.search(r"int flowgnn_set_gcn_virtual_node_dim\(flowgnn_engine\* e, int emb_dim,\s*" + five, text)
    assert re.search(r"int flowgnn_group_set_gcn_virtual_node_dim\(flowgnn_group\* g, int emb_dim,\s*" + five, text)
    from flowgnn_amd import _lib
    src = open(_lib.__file__).read()
    assert '"flowgnn_set_gcn_virtual_node_dim"' in src and '"flowgnn_group_set_gcn_virtual_node_dim"' in src
    assert "lib.flowgnn_set_gcn_virtual_node_dim.argtypes = [eng, C.c_int] + [p_float] * 5" in src
    assert "lib.flowgnn_group_set_gcn_virtual_node_dim.argtypes = [grp, C.c_int] + [p_float] * 5" in src


# ---------------------------------------------------------------- the fixed input tells the wrong forms from the definition
def test_the_fixed_input_tells_every_wrong_form_from_the_definition():
    """Section 4.15's condition at width 300: with tensor scales chosen on the references alone, every wrong form moves at least half of
    the logits by more than 10 x the parity bound REL (scale + |want|) -- and the input is inside the split kernels' range."""
    b, w, vn = V.fixed_batch(), V.fixed_weights(), V.fixed_virtual_node()
    ref = V.forward(b, w, vn)
    assert ref.operands < 6.0e4 / 2, ref.operands
    bound = REL * (max(1.0, ref.scale) + np.abs(ref.logits))
    for variant in V.VARIANTS:
        got = V.forward(b, w, vn, variant=variant)
        moved = float((np.abs(got.logits - ref.logits) > 10.0 * bound).mean())
        print(f"{variant}: {100 * moved:.1f} % of {b.num_graphs} logits move by more than 10 x the bound")
        assert moved >= 0.5, (variant, moved)


def test_the_range_tensors_leave_the_range_in_xin_1_alone():
    b, w = gp.synth_molpcba_batch(24, seed=13), weights.synth_gcn_weights(seed=7, emb_dim=300)
    vn = V.range_virtual_node()
    assert vn["b2"].shape == (4, 300) and np.count_nonzero(np.concatenate([v.ravel() for v in vn.values()])) == 1
    assert V.forward(b, w, vn).operands > 6.6e4 and R.max_a(b, w) < 6.0e4 / 2


# ---------------------------------------------------------------- the separation table
def test_the_seed_list_is_the_smallest_seeds():
    assert V.SEEDS == (0, 1) and sorted(V.SEEDS_TRIED) == [0, 1]  # seeds 0 and 1 reach both ratios: nothing else was tried
    assert V.SEP_GRAPHS == 256
    with open(V.GOLDEN) as f:
        g = json.load(f)
    assert sorted(g) == [str(s) for s in V.SEEDS] and all(sorted(g[s]) == sorted(V.SEP_OUTPUTS) for s in g)


@pytest.mark.parametrize("seed", V.SEEDS)
def test_split_products_are_separated_from_their_wrong_variants(seed):
    """E_bad / E_ok >= split_ref.min_ratio("GCN", output) for rows (64) and logits (16) with the virtual node on and the restatement on
    all twelve products, on the references alone; B = sqrt(E_ok * E_bad) is the bound of tests/test_gcn_wide_vn_gpu.py's split-accuracy
    case, and the committed table is this one."""
    t = V.table(seed)
    gold = V.golden()[str(seed)]
    assert V.reference(seed).operands < 6.0e4 / 2
    for name in V.SEP_OUTPUTS:
        row = t[name]
        ratio = row.e_bad / row.e_ok
        print(f"seed {seed} {name}: E_ok {row.e_ok:.3e}  B {row.bound:.3e}  E_bad {row.e_bad:.3e}  ratio {ratio:.1f}  closest: {min(row.bad, key=row.bad.get)}")
        assert ratio >= split_ref.min_ratio("GCN", name), (name, ratio, row.ok, row.bad)
        assert abs(ratio - V.SEEDS_TRIED[seed][0 if name == "rows" else 1]) < 0.06
        for k in ("e_ok", "e_bad", "bound"):
            assert abs(gold[name][k] - getattr(row, k)) <= 1e-6 * getattr(row, k), (name, k, gold[name][k], getattr(row, k))
    assert all(v > t["rows"].e_ok for v in t["rows"].bad.values())  # every wrong variant is wrong
