"""OGB's num_layer at width 300 (flowgnn.h: flowgnn_set_num_layers), what needs no GPU: the exporter reads the
depth off a state_dict, the files' sizes follow it, savers and loaders round-trip and refuse a file of another depth, the refusals carry
their texts, the models of tests/ogb_layers.py stay under half the split-f16 kernels' range threshold, and the bound of the GPU tests
(tests/parity.py: REL = 1e-4 with the torch forward hooks' scale) tells a right depth from a wrong one.

Which outputs separate.  With scales near 1e3 (the virtual-node models) a defect moves the single logit by less than the bound in some
cases; the ROWS separate for every defect, depth and model, and the pooled vectors for all but the cases SEPARATES records as it runs.
tests/test_num_layers_gpu.py asserts rows, pooled vectors and logits alike; what this file guarantees is that a wrong depth cannot
pass the rows' comparison."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from flowgnn_amd import export, weights  # noqa: E402
from tests import ogb_layers as OL, ogb_torch as T  # noqa: E402
from tests.parity import err_ratio  # noqa: E402
from tests.test_ogb_torch_cpu import export_kwargs  # noqa: E402

HALF_THRESHOLD = 3.0e4  # the split-f16 kernels hand a pass to the fp32 pipe at 6e4 (dense_split.h)
D, H = 300, 600
CASES = [(k, vn, L) for k, vn in OL.KINDS for L in OL.DEPTHS]
IDS = [OL.name_of(*c) for c in CASES]
SEPARATES = {}  # (kind, vn, L, defect) -> {"rows": ratio, "pooled": ratio, "logits": ratio}, filled by test_scale_under_half_the_threshold_and_the_bound_tells_right_from_wrong


@pytest.fixture(autouse=True)
def torch_on_one_thread():
    """The forwards here are a few hundred rows by 300 columns: one thread each, so that a parallel run of the suite does not
    oversubscribe the machine with a thread pool per worker."""
    with OL.one_thread():
        yield


def floats(path):
    assert os.path.getsize(path) % 4 == 0
    return os.path.getsize(path) // 4


# ---------------------------------------------------------------- the exporter, the files, the round trip
@pytest.mark.parametrize("kind,vn,L", CASES, ids=IDS)
def test_exporter_infers_the_depth_and_file_sizes_follow_it(kind, vn, L, tmp_path):
    sd = OL.untrained_state_dict(kind, vn, L)  # (keys and shapes are what this test is about: no trained-looking model is built)
    assert export.num_layers_of_ogb_state_dict(sd) == L
    w = export.export_weights(kind.upper(), sd, str(tmp_path), **export_kwargs(kind, vn, D))
    assert weights.gin_num_layers_of(w) == L
    d = str(tmp_path)
    if kind == "gin":
        want = {"gin_ep1_nd_embed_dim300.bin": 173 * D, "gin_ep1_ed_embed_dim300.bin": L * 13 * D, "gin_ep1_mlp_1_weights_dim300.bin": L * H * D,
                "gin_ep1_mlp_1_bias_dim300.bin": L * H, "gin_ep1_mlp_2_weights_dim300.bin": L * D * H, "gin_ep1_mlp_2_bias_dim300.bin": L * D,
                "gin_ep1_pred_weights_dim300.bin": D, "gin_ep1_pred_bias_dim300.bin": 1, "gin_ep1_eps_dim300.bin": L}
    else:
        want = {"gcn_ep1_dim300.weights.all.bin": 173 * D + L * (D * D + 15 * D) + L * (4 * D + 1) + D + 1}
    if vn:
        want[f"{kind}_ep1_virtualnode_dim300.bin"] = D + (L - 1) * (2 * H * D + H + D)
    assert {f: floats(os.path.join(d, f)) for f in os.listdir(d)} == want  # the same names at every depth, nothing else written
    # ---- save -> load round-trips, bit for bit, at the depth; another depth is refused with both numbers
    load = weights.load_gin_weights if kind == "gin" else weights.load_gcn_weights
    back = load(d, emb_dim=D, num_layers=L)
    assert list(back) == list(w) and all(np.array_equal(back[k], w[k]) for k in w)
    other = 5 if L != 5 else 4
    with pytest.raises(ValueError) as ex:
        load(d, emb_dim=D, num_layers=other)
    assert f"{L} layers deep" in str(ex.value) and f"num_layers is {other}" in str(ex.value), str(ex.value)
    if kind == "gin":
        eps = weights.load_gin_eps(d, emb_dim=D, num_layers=L)
        assert eps.shape == (L,) and np.array_equal(eps, export.gin_eps_from_ogb_state_dict(sd, num_layers=L)) and (np.abs(eps) >= 0.05).all()
        assert np.allclose(eps, 0.05 * np.arange(1, L + 1))  # layer l's value at index l
        with pytest.raises(ValueError):
            weights.load_gin_eps(d, emb_dim=D, num_layers=other)
    if vn:
        loadv = weights.load_gin_virtual_node if kind == "gin" else weights.load_gcn_virtual_node
        v = loadv(d, emb_dim=D, num_layers=L)
        assert v["w1"].shape == (L - 1, H, D) and v["b2"].shape == (L - 1, D) and weights.gin_virtual_node_num_layers_of(v) == L
        with pytest.raises(ValueError) as ex:
            loadv(d, emb_dim=D, num_layers=other)
        assert f"{L} layers deep" in str(ex.value), str(ex.value)
        with pytest.raises(ValueError):  # tensors of one depth are not taken for an engine of another
            weights.checked_gin_virtual_node(v, num_layers=other)


def test_depth_5_is_what_it_was(tmp_path):
    """The default depth: the shapes, offsets and synthetic draws of the functions that grew a num_layers keyword are those without it."""
    assert weights.gin_files(300, 5) == weights.gin_files(300) and weights.gin_files(100, 5) == weights.gin_files()
    assert weights.gcn_shapes(300, 5) == weights.gcn_shapes(300) and weights.gcn_shapes(100) == weights.GCN_SHAPES
    assert weights.gin_virtual_node_shapes(100) == weights.GIN_VIRTUAL_NODE_SHAPES
    assert weights._gcn_offsets(1, 100)[("graph_pred_weights", None)] == 76805 and weights._gcn_offsets(1, 100)[("bn_weight", 0)] == 74800
    for a, b in ((weights.synth_gin_weights(emb_dim=300), weights.synth_gin_weights(emb_dim=300, num_layers=5)),
                 (weights.synth_gcn_weights(emb_dim=300), weights.synth_gcn_weights(emb_dim=300, num_layers=5))):
        assert all(np.array_equal(a[k], b[k]) for k in a)
    w = weights.synth_gcn_weights(emb_dim=300, num_layers=7, num_tasks=3)
    weights.save_gcn_weights(w, str(tmp_path))
    back = weights.load_gcn_weights(str(tmp_path), num_tasks=3, emb_dim=300, num_layers=7)
    assert all(np.array_equal(back[k], w[k]) for k in w)


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_refusals(kind, tmp_path):
    mk = lambda L, dim, vn=False: T.GNN(num_layer=L, emb_dim=dim, gnn_type=kind, virtual_node=vn).double().eval().state_dict()
    model = kind.upper()
    for L in (1, 9):  # outside 2 .. 8 (torch builds the model; OGB itself raises below 2)
        with pytest.raises(export.ExportError) as ex:
            export.export_weights(model, mk(L, 300), str(tmp_path / "x"), **export_kwargs(kind, False, 300))
        assert "flowgnn_set_num_layers" in str(ex.value) and str(L) in str(ex.value) and "2 .. 8" in str(ex.value), str(ex.value)
    for L in (2, 3, 6, 8):  # a depth other than 5 at width 100
        with pytest.raises(export.ExportError) as ex:
            export.export_weights(model, mk(L, 100), str(tmp_path / "x"), **export_kwargs(kind, False, 100))
        assert "flowgnn_set_num_layers" in str(ex.value) and "100" in str(ex.value) and str(L) in str(ex.value), str(ex.value)
    assert not os.path.exists(tmp_path / "x")  # refused before any file is written
    export.export_weights(model, mk(5, 100), str(tmp_path / "ok"), **export_kwargs(kind, False, 100))  # depth 5 at width 100: as ever
    sd = {k: v for k, v in mk(3, 300).items() if not k.startswith("gnn_node.convs.1.")}  # layers 0 and 2: not a depth
    with pytest.raises(export.ExportError) as ex:
        export.num_layers_of_ogb_state_dict(sd)
    assert "[0, 2]" in str(ex.value)
    with pytest.raises(export.ExportError):
        export.num_layers_of_ogb_state_dict({"graph_pred_linear.weight": np.zeros((1, 300))})
    # ---- the functions under export_weights and the weight helpers refuse the same depths
    for fn, kw in ((weights.gin_files, {}), (weights.gcn_shapes, {}), (weights.gin_virtual_node_shapes, {})):
        for L in (1, 9):
            with pytest.raises(ValueError):
                fn(300, L)
        with pytest.raises(ValueError) as ex:
            fn(100, 3)
        assert "flowgnn_set_num_layers" in str(ex.value)
    with pytest.raises(ValueError):
        weights.save_gin_weights(weights.synth_gin_weights(emb_dim=300, num_layers=3), str(tmp_path / "y"), num_layers=5)
    assert not os.path.exists(tmp_path / "y")


def test_set_weights_refuses_a_set_of_another_depth():
    """Engine.set_weights / EngineGroup.set_weights hand bare pointers to the C call, which reads num_layers blocks: the check in front."""
    from flowgnn_amd.engine import _check_weights_depth
    for model, synth in (("GIN", weights.synth_gin_weights), ("GCN", weights.synth_gcn_weights)):
        for L in (2, 5, 8):
            _check_weights_depth(model, synth(emb_dim=300, num_layers=L), L)
            for other in (3, 5, 8):
                if other != L:
                    with pytest.raises(ValueError) as ex:
                        _check_weights_depth(model, synth(emb_dim=300, num_layers=L), other)
                    assert f"{L} layers" in str(ex.value) and f"depth is {other}" in str(ex.value), str(ex.value)
        _check_weights_depth(model, synth(), 5)  # width 100
    _check_weights_depth("PNA", weights.synth_pna_weights(), 5)  # the other models: no per-layer edge table, nothing to check


@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_the_out_of_range_models_are_out_of_range(kind):
    """The models of the exact re-run's GPU test: past the 6e4 threshold by a margin, from a model that is under half of it, while the
    rows stay small (what leaves the range is the update's hidden layer for gin, one component of vn_1 for gcn).  gin's push must reach
    the kernel: the hidden unit's folded bias times the packed matrix's power-of-two scale, which the push leaves alone."""
    from tests import split_ref
    want, scale, _ = OL.out_of_range_expected(kind, 3)
    base, base_scale, _ = OL.expected(kind, True, 3)
    print(kind, f"scale {base_scale:.4g} -> {scale:.4g}; largest row value {np.abs(want.rows).max():.4g}")
    assert base_scale < HALF_THRESHOLD and scale > 6.6e4
    assert err_ratio(want.rows, base.rows, base_scale) > 1.0  # another model than the one it was made from
    if kind == "gin":
        sd, sd0 = OL.out_of_range_model(kind, 3).state_dict(), OL.make_model(kind, True, 3).state_dict()
        vn, vn0 = (export.gin_virtual_node_from_ogb_state_dict(x, num_layers=3, virtual_node_dim=D) for x in (sd, sd0))
        assert np.array_equal(vn["w1"], vn0["w1"])
        assert split_ref.pow2_scale(vn["w1"][0]) * float(vn["b1"][0].max()) > 6.6e4


# ---------------------------------------------------------------- the scales, and the bound
def defects_at(kind, vn, L):
    """The named wrong forms that are a DIFFERENT computation at this depth.  At L = 2 the virtual node has one update, so
    "update_indexed_l_plus_1" ((l + 1) mod (L - 1) = 0 = l) is the right model itself and is left out there."""
    out = OL.defects_of(kind)
    if vn:
        out = out + [v for v in T.VARIANTS if not (v == "update_indexed_l_plus_1" and L == 2)]
    return out


@pytest.mark.parametrize("kind,vn,L", CASES, ids=IDS)
def test_scale_under_half_the_threshold_and_the_bound_tells_right_from_wrong(kind, vn, L):
    """The hooked scale stays under half the range threshold (so the GPU tests assert exact_reruns() == 0), and for each named defect
    the torch model that has it misses the right model's ROWS by more than the GPU tests' bound.  (One test: the model is built once.)"""
    model = OL.make_model(kind, vn, L)
    want, scale, _ = OL.expected(kind, vn, L)
    print(OL.name_of(kind, vn, L), f"hooked scale {scale:.4g}")
    assert 1.0 < scale < HALF_THRESHOLD, scale
    for defect in defects_at(kind, vn, L):
        got, _, _ = T.run(OL.with_defect(model, defect), T.batch_of(kind))
        r = {name: err_ratio(getattr(got, name), getattr(want, name), scale) for name in ("rows", "pooled", "logits")}
        SEPARATES[(kind, vn, L, defect)] = r
        print(OL.name_of(kind, vn, L), defect, " ".join(f"{k} {v:.3g}x" for k, v in r.items()),
              "| separates:", [k for k, v in r.items() if v > 1.0])
        assert r["rows"] > 1.0, (defect, r)
    if vn and L == 2:  # (the reason the variant is left out above, checked: it is the same numbers)
        same, _, _ = T.run(OL.with_defect(model, "update_indexed_l_plus_1"), T.batch_of(kind))
        assert np.array_equal(same.rows, want.rows)
