"""OGB's JK="sum" and residual=True for GCN at width 300 (flowgnn.h: flowgnn_set_model_jk_residual), on the
references alone: what tests/test_gcn_jk_residual_gpu.py relies on.  No GPU.  Every figure is recomputed and printed here, none quoted.

  1. With ("last", False) tests/ogb_gcn_jk_torch.py's model IS tests/ogb_torch.make_model("gcn", vn, 300) on gcn_batch(): logits, rows
     and pooled array_equal and the state_dicts equal, with and without the virtual node; the flags add no parameter.
  2. The NumPy restatement in the engine's terms (ogb_gcn_jk_torch.forward) agrees with the torch model at 1e-9 of the scale on the
     state_dict's tensors (the update's BatchNorms folded in float64), the exported files are those tensors rounded to float32 (the
     layer BatchNorms' variance shifted to the engine's 2^-10), and the restatement on the files uses under a tenth of the 1e-4 rule.
  3. Every applicable wrong form's ROWS miss the rule 1e-4 (scale + |want|) of tests/parity.py by at least 10 x.
  4. The scales of the six damped models are below half the split-f16 threshold of 6e4, so the fast path is what they exercise; the
     largest split operand of the undamped gcn-virtual models passes the threshold: the models of the exact re-run's test.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from flowgnn_amd import export  # noqa: E402
from tests import ogb_gcn_jk_torch as K, ogb_torch as T  # noqa: E402
from tests.parity import err_ratio  # noqa: E402
from tests.test_jk_residual_cpu import _bn64  # noqa: E402

MODELS = [(vn, jk, res) for vn in (False, True) for jk, res in K.SETTINGS]
name_of = lambda vn, jk, res: f"gcn{'-virtual' if vn else ''}-{jk}{'-res' if res else ''}"
IDS = [name_of(*m) for m in MODELS]
THRESHOLD = 6.0e4  # the layer kernel's range guard (gcn_wide_body.h)


@pytest.mark.parametrize("vn", [False, True], ids=["gcn", "gcn-virtual"])
def test_last_without_residual_is_the_ogb_torch_model(vn):
    want, scale, _ = T.expected("gcn", vn, 300)
    got, gscale, _ = K.expected(vn, "last", False)
    assert np.array_equal(got.logits, want.logits) and np.array_equal(got.rows, want.rows) and np.array_equal(got.pooled, want.pooled)
    a, b = T.make_model("gcn", vn, 300).state_dict(), K.make_model(vn).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert gscale <= scale  # (r is hooked and the pooled t is not: never a wider bound than ogb_torch's)


def test_the_flags_add_no_parameter():
    for vn in (False, True):
        keys = list(T.make_model("gcn", vn, 300).state_dict())
        for jk, res in K.SETTINGS:
            assert list(K.make_model(vn, jk, res).state_dict()) == keys


def from_state_dict(sd, vn):
    """The tensors of weights.load_gcn_weights / load_gcn_virtual_node unrounded, from the state_dict: the layer BatchNorms as they are
    (forward(bn_eps=1e-5)), the update's folded in float64 as the exporter folds them."""
    Lr = K.L
    w = {"node_embedding_weight": np.concatenate([sd[f"gnn_node.atom_encoder.atom_embedding_list.{k}.weight"] for k in range(9)]),
         "edge_embedding_weight": np.stack([np.concatenate([sd[f"gnn_node.convs.{l}.bond_encoder.bond_embedding_list.{k}.weight"] for k in range(3)])
                                            for l in range(Lr)]),
         "convs_weight": np.stack([sd[f"gnn_node.convs.{l}.linear.weight"] for l in range(Lr)]),
         "convs_bias": np.stack([sd[f"gnn_node.convs.{l}.linear.bias"] for l in range(Lr)]),
         "convs_root_emb_weight": np.stack([sd[f"gnn_node.convs.{l}.root_emb.weight"].reshape(-1) for l in range(Lr)]),
         "bn_weight": np.stack([sd[f"gnn_node.batch_norms.{l}.weight"] for l in range(Lr)]),
         "bn_bias": np.stack([sd[f"gnn_node.batch_norms.{l}.bias"] for l in range(Lr)]),
         "bn_mean": np.stack([sd[f"gnn_node.batch_norms.{l}.running_mean"] for l in range(Lr)]),
         "bn_var": np.stack([sd[f"gnn_node.batch_norms.{l}.running_var"] for l in range(Lr)]),
         "graph_pred_weights": sd["graph_pred_linear.weight"], "graph_pred_bias": sd["graph_pred_linear.bias"]}
    vnt = None
    if vn:
        v1, c1, v2, c2 = [], [], [], []
        for l in range(Lr - 1):
            m = f"gnn_node.mlp_virtualnode_list.{l}"
            g, o = _bn64(sd, m + ".1")
            v1.append(sd[m + ".0.weight"] * g[:, None]); c1.append(sd[m + ".0.bias"] * g + o)
            g, o = _bn64(sd, m + ".4")
            v2.append(sd[m + ".3.weight"] * g[:, None]); c2.append(sd[m + ".3.bias"] * g + o)
        vnt = dict(vn_embedding=sd["gnn_node.virtualnode_embedding.weight"].reshape(-1), w1=np.stack(v1), b1=np.stack(c1), w2=np.stack(v2),
                   b2=np.stack(c2))
    return w, vnt


@pytest.mark.parametrize("vn,jk,res", MODELS + [(False, "last", False), (True, "last", False)], ids=IDS + ["gcn-last", "gcn-virtual-last"])
def test_numpy_restatement_agrees_with_the_torch_model(vn, jk, res, tmp_path):
    """The restatement reads the exported FILES (float32), the torch model its float64 parameters; the two differ by the files' rounding,
    far more than 1e-9.  So the 1e-9 comparison is made where both sides hold the same numbers -- the state_dict's tensors -- the files
    are checked against those at float32's rounding, and the restatement on the files themselves must use under a tenth of the rule."""
    model = K.make_model(vn, jk, res)
    want, scale, _ = K.expected(vn, jk, res)
    sd = {k: v.numpy() for k, v in model.state_dict().items()}
    w, vnt = from_state_dict(sd, vn)
    got = K.forward(T.gcn_batch(), w, vnt, jk=jk, residual=res, bn_eps=export.BN_EPS)
    for name in ("logits", "rows", "pooled"):
        r = err_ratio(getattr(got, name), getattr(want, name), scale, rel=1e-9)
        print(vn, jk, res, name, f"{r:.3g} x 1e-9 (scale {scale:.4g})")
        assert r <= 1.0, (name, r)
    # ... and the files are those tensors rounded to float32 (the variance carries the difference of the two BatchNorm constants)
    export.export_weights("GCN", model.state_dict(), str(tmp_path), emb_dim=300, **(dict(virtual_node=True, virtual_node_dim=300) if vn else {}))
    fw, fvn = K.load(str(tmp_path), vn)
    for k in fw:
        ref = w[k] + (export.BN_EPS - export.REF_BN_EPS) if k == "bn_var" else w[k]
        assert np.allclose(np.asarray(fw[k]).reshape(np.shape(ref)), ref, rtol=2.0 ** -22, atol=1e-30), k
    if vn:
        for k in fvn:
            assert np.allclose(np.asarray(fvn[k]).reshape(np.shape(vnt[k])), vnt[k], rtol=2.0 ** -23, atol=1e-30), k
    file_ref = K.forward(T.gcn_batch(), fw, fvn, jk=jk, residual=res)
    for name in ("logits", "rows", "pooled"):
        r = err_ratio(getattr(file_ref, name), getattr(want, name), scale)
        print(vn, jk, res, "files", name, f"{r:.4f} x the 1e-4 rule")
        assert r <= 0.1, (name, r)


@pytest.mark.parametrize("vn,jk,res", MODELS, ids=IDS)
def test_every_wrong_form_misses_the_rule_by_ten_times_on_rows(vn, jk, res):
    want, scale, _ = K.expected(vn, jk, res)
    names = K.variants_of(vn, jk, res)
    assert names
    for name in names:
        r = err_ratio(K.variant_rows(vn, jk, res, name), want.rows, scale)
        print(name_of(vn, jk, res), name, f"rows {r:.1f} x the rule")
        assert r >= 10.0, (name, r)


def test_every_wrong_form_is_exercised_by_some_model():
    seen = set()
    for vn, jk, res in MODELS:
        seen.update(K.variants_of(vn, jk, res))
    assert seen == set(K.VARIANTS)


@pytest.mark.parametrize("vn,jk,res", MODELS, ids=IDS)
def test_the_damped_models_stay_inside_the_fast_paths_range(vn, jk, res):
    _, scale, _ = K.expected(vn, jk, res)
    print(name_of(vn, jk, res), f"scale {scale:.4g}")
    assert scale < THRESHOLD / 2


@pytest.mark.parametrize("jk,res", K.SETTINGS, ids=[f"{jk}{'-res' if res else ''}" for jk, res in K.SETTINGS])
def test_the_undamped_virtual_node_models_leave_it(jk, res, tmp_path):
    """The largest operand the split kernels' range guards watch -- x_1 .. x_4, t, the update's pre-scaled hidden units -- of the
    restatement on the exported files: past the threshold, so the engine repeats the pass on the fp32 pipe."""
    model = K.make_model(True, jk, res, damped=False)
    export.export_weights("GCN", model.state_dict(), str(tmp_path), emb_dim=300, virtual_node=True, virtual_node_dim=300)
    fw, fvn = K.load(str(tmp_path), True)
    ref = K.forward(T.gcn_batch(), fw, fvn, jk=jk, residual=res)
    _, scale, _ = K.expected(True, jk, res, damped=False)
    print("undamped gcn-virtual", jk, res, f"largest split operand {ref.operands:.4g}, scale {scale:.4g}")
    assert ref.operands > THRESHOLD
