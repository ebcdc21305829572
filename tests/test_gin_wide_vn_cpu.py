"""OGB's gin-virtual at width 300 without a GPU (flowgnn.h: flowgnn_set_ogb_virtual_node_dim): the reference
forward of tests/gin_wide_vn_ref.py against the 100-wide one it generalises, the exporter's virtual_node_dim keyword against OGB's own
forward, the dim300 file, the refusals, the header, and the condition on the fixed input -- that it tells every wrong form of the
virtual node from the definition, and the fixture of the split-accuracy table.  The self-checks of the reference forward (at width 100
it is tests/ogb_vn_ref.py's) hold on any tree, as they must; every other test here fails on a tree without the width-carrying call."""
import os
import re

import numpy as np
import pytest

from flowgnn_amd import export, graphpack as gp, weights
from flowgnn_amd.export import ExportError
from tests import gin_wide_ref as W, gin_wide_vn_ref as V, ogb_vn_ref
from tests.parity import REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.asarray(W.TRAINED_EPS, np.float32)


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("variant", [None] + V.VARIANTS + [V.NOOP_VARIANT])
def test_at_width_100_the_forward_is_ogb_vn_refs(variant):
    b = gp.synth_molhiv_batch(24, seed=5)
    w, vn = weights.synth_gin_weights(seed=7), ogb_vn_ref.fixed_virtual_node()
    for kw in (dict(), dict(eps=EPS, pooling="sum")):
        want = ogb_vn_ref.forward(b, w, vn, variant=variant, **kw)
        got = V.forward(b, w, vn, variant=variant, **kw)
        assert np.abs(got.logits - want[0]).max() <= 1e-12 and np.abs(got.rows - want[1]).max() <= 1e-12
        assert abs(got.scale - want[2]) <= 1e-12 * want[2]


def test_with_zero_tensors_the_forward_is_gin_wide_refs():
    b = gp.synth_molhiv_batch(24, seed=5)
    w = weights.synth_gin_weights(seed=7, emb_dim=300)
    want, got = W.forward(b, w, eps=EPS), V.forward(b, w, V.zero_virtual_node(), eps=EPS)
    assert np.array_equal(got.logits, want.logits) and np.array_equal(got.rows, want.rows)


# ---------------------------------------------------------------- shapes, files
def test_shapes_and_file_names():
    assert weights.gin_virtual_node_shapes(100) == weights.GIN_VIRTUAL_NODE_SHAPES
    assert weights.gin_virtual_node_file(100) == weights.GIN_VIRTUAL_NODE_FILE == "gin_ep1_virtualnode_dim100.bin"
    assert weights.gin_virtual_node_file(300) == "gin_ep1_virtualnode_dim300.bin"
    s = weights.gin_virtual_node_shapes(300)
    assert list(s.items()) == [("vn_embedding", (300,)), ("w1", (4, 600, 300)), ("b1", (4, 600)), ("w2", (4, 300, 600)), ("b2", (4, 300))]
    for bad in (0, 200, 301):
        with pytest.raises(ValueError):
            weights.gin_virtual_node_shapes(bad)
        with pytest.raises(ValueError):
            weights.gin_virtual_node_file(bad)


def test_synth_at_width_100_is_what_it_was_and_shrinks_the_matrices_at_300():
    a, b = weights.synth_gin_virtual_node(seed=11), weights.synth_gin_virtual_node(seed=11, emb_dim=100)
    rng = np.random.default_rng(11)
    first = (rng.standard_normal(100) * 0.11).astype(np.float32)
    assert all(np.array_equal(a[k], b[k]) for k in a) and np.array_equal(a["vn_embedding"], first)
    c = weights.synth_gin_virtual_node(seed=11, emb_dim=300)
    assert {k: v.shape for k, v in c.items()} == dict(weights.gin_virtual_node_shapes(300)) and all(v.dtype == np.float32 for v in c.values())
    k = np.sqrt(100.0 / 300.0)
    for name, s in (("w1", 0.075 * k), ("w2", 0.053 * k), ("b1", 0.91), ("b2", 0.49), ("vn_embedding", 0.11)):
        assert abs(float(c[name].std()) / s - 1.0) < (0.02 if c[name].size > 1000 else 0.15), (name, float(c[name].std()), s)


def test_file_round_trip_at_dim300(tmp_path):
    vn = weights.synth_gin_virtual_node(seed=11, emb_dim=300)
    weights.save_gin_virtual_node(vn, str(tmp_path))
    path = tmp_path / "gin_ep1_virtualnode_dim300.bin"
    assert path.stat().st_size == 4 * 1443900 and not (tmp_path / weights.GIN_VIRTUAL_NODE_FILE).exists()
    back = weights.load_gin_virtual_node(str(tmp_path), emb_dim=300)
    assert list(back) == list(vn) and all(np.array_equal(back[k], vn[k]) for k in vn)
    flat = np.fromfile(path, "<f4")
    assert np.array_equal(flat[:300], vn["vn_embedding"]) and np.array_equal(flat[-1200:], vn["b2"].ravel())
    with pytest.raises(IOError):
        weights.load_gin_virtual_node(str(tmp_path), emb_dim=100)  # (no dim100 file here)
    with pytest.raises(ValueError):
        weights.save_gin_virtual_node(vn, str(tmp_path), emb_dim=100)
    weights.save_gin_virtual_node(weights.synth_gin_virtual_node(seed=11), str(tmp_path), emb_dim=100)
    with open(path, "r+b") as f:
        f.truncate(4 * 1443899)
    with pytest.raises(IOError):
        weights.load_gin_virtual_node(str(tmp_path), emb_dim=300)


def test_checked_accepts_either_width_and_nothing_malformed(tmp_path):
    for d in (100, 300):
        vn = weights.synth_gin_virtual_node(seed=11, emb_dim=d)
        out = weights.checked_gin_virtual_node({k: v.astype(np.float64).ravel() for k, v in vn.items()})
        assert {k: v.shape for k, v in out.items()} == dict(weights.gin_virtual_node_shapes(d))
    vn = weights.synth_gin_virtual_node(seed=11, emb_dim=300)
    mixed = dict(vn, w1=weights.synth_gin_virtual_node(seed=11)["w1"])
    for bad in (mixed, dict(vn, vn_embedding=np.zeros(200, np.float32)), {k: v for k, v in vn.items() if k != "b2"}, dict(vn, extra=vn["b1"])):
        with pytest.raises(ValueError):
            weights.checked_gin_virtual_node(bad)
    with pytest.raises(ValueError):  # GCN's call has no wider form
        weights.checked_gin_virtual_node(vn, emb_dims=(100,))
    target = tmp_path / "not_created"
    with pytest.raises(ValueError):  # ... and is refused before a directory or a file exists
        weights.save_gcn_virtual_node(vn, str(target))
    with pytest.raises(ValueError):
        weights.save_gin_virtual_node(mixed, str(target))
    assert not target.exists()


# ---------------------------------------------------------------- the exporter
@pytest.mark.parametrize("with_bn", [True, False], ids=["with BatchNorms", "without"])
def test_the_exporter_with_virtual_node_dim_reproduces_ogbs_own_forward(with_bn):
    sd = V.vn_state_dict(seed=3, with_bn=with_bn)
    b = gp.synth_molhiv_batch(40, seed=3)
    want = V.ogb_forward(sd, b)
    real = export._checked  # the exporter's own functions with the float32 cast taken out (tests/gin_wide_ref.exported_unrounded)
    try:
        export._checked = lambda w, spec, shape_of: {k: np.asarray(w[k], np.float64).reshape(tuple(shape_of(k, v))) for k, v in spec.items()}
        w = export.gin_weights_from_ogb_state_dict(sd, keep_eps=True, virtual_node=True, virtual_node_dim=300)
        vn = export.gin_virtual_node_from_ogb_state_dict(sd, virtual_node_dim=300)
    finally:
        export._checked = real
    eps = np.array([float(np.asarray(sd[f"gnn_node.convs.{l}.eps"]).ravel()[0]) for l in range(5)])
    got = V.forward(b, w, vn, eps=eps, eps_f64=True)
    err = float(np.abs(got.logits - want).max())
    print(f"exporter (BatchNorms: {with_bn}): max |folded - OGB's own| = {err:.3e}, logits up to {np.abs(want).max():.3g}")
    assert err <= 1e-9
    # ... and the float32 tensors the engine gets are those, rounded once
    w32 = export.gin_weights_from_ogb_state_dict(sd, keep_eps=True, virtual_node=True, virtual_node_dim=300)
    vn32 = export.gin_virtual_node_from_ogb_state_dict(sd, virtual_node_dim=300)
    assert {k: v.shape for k, v in vn32.items()} == dict(weights.gin_virtual_node_shapes(300)) and weights.gin_emb_dim_of(w32) == 300
    assert all(v.dtype == np.float32 and np.array_equal(v, vn[k].astype(np.float32)) for k, v in vn32.items())


def test_export_weights_writes_the_dim300_set(tmp_path):
    sd = V.vn_state_dict(seed=3)
    export.export_weights("GIN", sd, str(tmp_path), keep_eps=True, virtual_node=True, virtual_node_dim=300)
    names = sorted(os.listdir(tmp_path))
    assert "gin_ep1_virtualnode_dim300.bin" in names and all("dim300" in n for n in names), names
    vn = weights.load_gin_virtual_node(str(tmp_path), emb_dim=300)
    want = export.gin_virtual_node_from_ogb_state_dict(sd, virtual_node_dim=300)
    assert all(np.array_equal(vn[k], want[k]) for k in want)


def test_exporter_refusals(tmp_path):
    sd300, sd100 = W.state_dict(seed=3, virtual_node=True), ogb_vn_ref.vn_state_dict(seed=3)
    # without the keyword the refusal stands, and now names it
    for kw in (dict(virtual_node=False), dict(virtual_node=True)):
        with pytest.raises(ExportError, match="100-wide") as ei:
            export.gin_weights_from_ogb_state_dict(sd300, keep_eps=True, **kw)
        assert "virtual_node_dim" in str(ei.value)
    with pytest.raises(ExportError, match="100-wide") as ei:
        export.export_weights("GIN", sd300, str(tmp_path), keep_eps=True, virtual_node=True)
    assert "virtual_node_dim" in str(ei.value) and not os.listdir(tmp_path)
    with pytest.raises(ExportError, match="100-wide"):
        export.gin_virtual_node_from_ogb_state_dict(sd300)
    # the keyword alone is not enough: the weight set without its virtual node is a model nobody trained
    with pytest.raises(ExportError, match="virtual_node=True"):
        export.gin_weights_from_ogb_state_dict(sd300, keep_eps=True, virtual_node_dim=300)
    # a width that is not the state_dict's
    for call in (lambda: export.gin_weights_from_ogb_state_dict(sd100, keep_eps=True, virtual_node=True, virtual_node_dim=300),
                 lambda: export.gin_virtual_node_from_ogb_state_dict(sd100, virtual_node_dim=300),
                 lambda: export.export_weights("GIN", sd100, str(tmp_path), keep_eps=True, virtual_node=True, virtual_node_dim=300),
                 lambda: export.gin_weights_from_ogb_state_dict(W.state_dict(seed=3, width=100), keep_eps=True, virtual_node_dim=300),
                 lambda: export.gin_weights_from_ogb_state_dict(sd300, keep_eps=True, virtual_node=True, virtual_node_dim=200),
                 lambda: export.export_weights("GCN", sd100, str(tmp_path), virtual_node=True, virtual_node_dim=300)):
        with pytest.raises(ExportError):
            call()
    assert not os.listdir(tmp_path)
    # the 100-wide route is what it was, with and without the keyword's default
    a = export.gin_virtual_node_from_ogb_state_dict(sd100)
    b = export.gin_virtual_node_from_ogb_state_dict(sd100, virtual_node_dim=100)
    assert all(np.array_equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------- the header
def test_the_header_declares_the_two_functions():
    text = open(os.path.join(ROOT, "include", "flowgnn.h")).read()
    five = r"const float\* vn_embedding,\s*const float\* w1,\s*const float\* b1,\s*const float\* w2,\s*const float\* b2\)"
    assert re.search(r"int flowgnn_set_ogb_virtual_node_dim\(flowgnn_engine\* e, int emb_dim,\s*" + five, text)
    assert re.search(r"int flowgnn_group_set_ogb_virtual_node_dim\(flowgnn_group\* g, int emb_dim,\s*" + five, text)
    from flowgnn_amd import _lib
    src = open(_lib.__file__).read()
    assert '"flowgnn_set_ogb_virtual_node_dim"' in src and '"flowgnn_group_set_ogb_virtual_node_dim"' in src


# ---------------------------------------------------------------- the fixed input tells the wrong forms from the definition
def test_the_fixed_input_tells_every_wrong_form_from_the_definition():
    """A condition on the INPUT (tests/test_gin_wide_vn_gpu.py's fixed-input test inherits it): each wrong form of ogb_vn_ref.VARIANTS
    moves at least half of the logits by more than 10 x the f32 bound REL (scale + |want|) of tests/parity.py; the no-op variant moves
    none.  The tensors' scales were chosen on these references alone (gin_wide_vn_ref.fixed_virtual_node)."""
    b, w, vn = V.fixed_batch(), weights.synth_gin_weights(seed=7, emb_dim=300), V.fixed_virtual_node()
    for eps in (None, EPS):
        ref = V.forward(b, w, vn, eps=eps)
        assert ref.scale < 6.0e4 / 8
        bound = REL * (ref.scale + np.abs(ref.logits))
        for variant in V.VARIANTS:
            bad = V.forward(b, w, vn, eps=eps, variant=variant)
            moved = float((np.abs(bad.logits - ref.logits) > 10 * bound).mean())
            print(f"eps {'on' if eps is not None else 'off'}  {variant:26s} moves {100 * moved:5.1f} % of the logits by more than 10 x the bound "
                  f"(median {float(np.median(np.abs(bad.logits - ref.logits) / bound)):.1f} x)")
            assert moved >= 0.5, (variant, moved)
        same = V.forward(b, w, vn, eps=eps, variant=V.NOOP_VARIANT)
        assert np.array_equal(same.logits, ref.logits)


def test_the_shape_tests_tensors_stay_in_the_split_kernels_range():
    """What tests/gin_wide_vn_ref.shapes_virtual_node says, on the float64 forward alone: at the synthetic scales the vector grows about
    tenfold per update and the forward passes 6e4; with the first linear layer scaled by 1 / 16 it stays three orders below."""
    b, w = gp.synth_molhiv_batch(200, seed=13), weights.synth_gin_weights(seed=7, emb_dim=300)
    raw = V.forward(b, w, weights.synth_gin_virtual_node(seed=11, emb_dim=300)).scale
    tamed = V.forward(b, w, V.shapes_virtual_node()).scale
    print(f"largest activation: synthetic scales {raw:.3g}, first linear layer / 16 {tamed:.3g}")
    assert raw > 6.0e4 and tamed < 6.0e4 / 8


@pytest.mark.parametrize("seed", V.SEEDS)
def test_the_golden_separation_table_is_what_the_references_give(seed):
    """tests/golden/gin_wide_vn_sep.json (read by tests/test_gin_wide_vn_gpu.py::test_split_accuracy) against a recomputation of
    gin_wide_vn_ref.table, and the condition the seeds were chosen for: E_bad / E_ok >= split_ref.MIN_RATIO for rows and logits."""
    from tests import split_ref
    t, g = V.table(seed), V.golden_table(seed)
    for name in V.SEP_OUTPUTS:
        print(f"seed {seed} {name}: E_ok {t[name].e_ok:.3e}  B {t[name].bound:.3e}  E_bad {t[name].e_bad:.3e}  ratio {t[name].e_bad / t[name].e_ok:.1f}  "
              f"closest wrong variant: {min(t[name].bad, key=t[name].bad.get)}")
        assert t[name].e_bad / t[name].e_ok >= split_ref.MIN_RATIO == V.MIN_RATIO
        assert set(g[name].ok) == set(t[name].ok) and set(g[name].bad) == set(t[name].bad)
        for got, want in ([(g[name].e_ok, t[name].e_ok), (g[name].e_bad, t[name].e_bad)] + [(g[name].ok[k], v) for k, v in t[name].ok.items()]
                          + [(g[name].bad[k], v) for k, v in t[name].bad.items()]):
            assert abs(got - want) <= 1e-6 * want, (name, got, want)
