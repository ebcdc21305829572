"""OGB's JK="sum" and residual=True for GIN at width 300 (flowgnn.h: flowgnn_set_jk_residual), on the references
alone: what tests/test_jk_residual_gpu.py relies on.  No GPU.

  1. With ("last", False) tests/ogb_jk_torch.py's model IS tests/ogb_torch.make_model("gin", vn, 300) on gin_batch(): logits and rows
     array_equal, with and without the virtual node.
  2. The NumPy restatement in the engine's terms (ogb_jk_torch.forward) agrees with the torch model at 1e-9 of the scale on the
     state_dict's tensors folded in float64, the exported files are those tensors rounded to float32, and the restatement on the
     files uses under a tenth of the 1e-4 rule.
  3. Every named wrong form's ROWS miss the 1e-4 parity rule of tests/parity.py by at least 10 x.  Measured with seed 0 (printed by the
     test): the smallest ratio is 12.7 (jk_without_x0; gin-virtual; sum with residual), the next 29.9, all others >= 94.  The
     variants' logits are not all separable (2.0 for that variant), so the condition is on rows.
  4. The scales of the six models are below half the split-f16 threshold of 6e4 (measured: gin 40.4 / 25.7 / 41.4, gin-virtual
     4 506 / 668 / 4 947 for last + residual / sum / sum + residual), so the fast path is what they exercise; the undamped gin-virtual
     models with the residual leave it (1.39e5 and 3.89e5): the models of the exact re-run's test.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from flowgnn_amd import export  # noqa: E402
from tests import ogb_jk_torch as J, ogb_torch as T  # noqa: E402
from tests.parity import err_ratio  # noqa: E402

MODELS = [(vn, jk, res) for vn in (False, True) for jk, res in J.SETTINGS]
IDS = [f"gin{'-virtual' if vn else ''}-{jk}{'-res' if res else ''}" for vn, jk, res in MODELS]


@pytest.mark.parametrize("vn", [False, True], ids=["gin", "gin-virtual"])
def test_last_without_residual_is_the_ogb_torch_model(vn):
    want, scale, _ = T.expected("gin", vn, 300)
    got, gscale, _ = J.expected(vn, "last", False)
    assert np.array_equal(got.logits, want.logits) and np.array_equal(got.rows, want.rows) and np.array_equal(got.pooled, want.pooled)
    a, b = T.make_model("gin", vn, 300).state_dict(), J.make_model(vn).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert gscale <= scale  # (r is hooked and the pooled t is not: ogb_jk_torch.py says why; never a wider bound than ogb_torch's)


def test_the_flags_add_no_parameter():
    keys = list(T.make_model("gin", True, 300).state_dict())
    for jk, res in J.SETTINGS:
        assert list(J.make_model(True, jk, res).state_dict()) == keys


@pytest.mark.parametrize("vn,jk,res", MODELS + [(False, "last", False), (True, "last", False)], ids=IDS + ["gin-last", "gin-virtual-last"])
def test_numpy_restatement_agrees_with_the_torch_model(vn, jk, res, tmp_path):
    """The restatement reads the exported FILES (float32, BatchNorms folded), the torch model its float64 parameters; the two differ by
    the files' rounding, far more than 1e-9.  So the 1e-9 comparison is made where both sides hold the same numbers -- the
    state_dict's tensors folded here in float64 (fold64) and OGB's own 1 + eps -- the files are checked against that fold at float32's
    rounding, and the restatement on the files themselves must use under a tenth of the 1e-4 rule."""
    model = J.make_model(vn, jk, res)
    want, scale, _ = J.expected(vn, jk, res)
    sd = {k: v.numpy() for k, v in model.state_dict().items()}
    w, vnt, eps = fold64(sd, vn)
    got = J.forward(T.gin_batch(), w, vnt, eps=eps, jk=jk, residual=res, eps_f64=True)
    for name in ("logits", "rows", "pooled"):
        r = err_ratio(getattr(got, name), getattr(want, name), scale, rel=1e-9)
        print(vn, jk, res, name, f"{r:.3g} x 1e-9 (scale {scale:.4g})")
        assert r <= 1.0, (name, r)
    # ... and the files are that fold rounded to float32
    export.export_weights("GIN", model.state_dict(), str(tmp_path), keep_eps=True, **(dict(virtual_node=True, virtual_node_dim=300) if vn else {}))
    fw, fvn, feps = J.load(str(tmp_path), vn)
    for k in fw:
        assert np.allclose(fw[k], w[k], rtol=2.0 ** -23, atol=1e-30), k
    if vn:
        for k in fvn:
            assert np.allclose(fvn[k], vnt[k], rtol=2.0 ** -23, atol=1e-30), k
    assert np.allclose(feps, eps, rtol=2.0 ** -23)
    # the restatement on the files themselves stays inside the project's rule with room (the float32 files and (float)(1.0f + eps))
    file_ref = J.forward(T.gin_batch(), fw, fvn, eps=feps, jk=jk, residual=res)
    for name in ("logits", "rows", "pooled"):
        r = err_ratio(getattr(file_ref, name), getattr(want, name), scale)
        print(vn, jk, res, "files", name, f"{r:.4f} x the 1e-4 rule")
        assert r <= 0.1, (name, r)


def _bn64(sd, p):
    g = sd[p + ".weight"] / np.sqrt(sd[p + ".running_var"] + 1e-5)
    return g, sd[p + ".bias"] - g * sd[p + ".running_mean"]


def fold64(sd, vn):
    """The exporter's BatchNorm folds in float64, from the state_dict: the tensors of weights.load_gin_weights / load_gin_virtual_node
    unrounded, and the five eps."""
    D, Lr = J.WIDE, J.L
    w = {"node_embedding_weight": np.concatenate([sd[f"gnn_node.atom_encoder.atom_embedding_list.{k}.weight"] for k in range(9)]),
         "edge_embedding_weight": np.stack([np.concatenate([sd[f"gnn_node.convs.{l}.bond_encoder.bond_embedding_list.{k}.weight"] for k in range(3)])
                                            for l in range(Lr)])}
    w1, b1, w2, b2 = [], [], [], []
    for l in range(Lr):
        c = f"gnn_node.convs.{l}.mlp"
        g, o = _bn64(sd, c + ".1")
        w1.append(sd[c + ".0.weight"] * g[:, None]); b1.append(sd[c + ".0.bias"] * g + o)
        g, o = _bn64(sd, f"gnn_node.batch_norms.{l}")
        w2.append(sd[c + ".3.weight"] * g[:, None]); b2.append(sd[c + ".3.bias"] * g + o)
    w.update(node_mlp_1_weights=np.stack(w1), node_mlp_1_bias=np.stack(b1), node_mlp_2_weights=np.stack(w2), node_mlp_2_bias=np.stack(b2),
             graph_pred_weights=sd["graph_pred_linear.weight"], graph_pred_bias=sd["graph_pred_linear.bias"])
    assert w["node_embedding_weight"].shape == (173, D) and w["edge_embedding_weight"].shape == (Lr, 13, D)
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
    return w, vnt, np.array([sd[f"gnn_node.convs.{l}.eps"][0] for l in range(Lr)])


@pytest.mark.parametrize("vn,jk,res", MODELS, ids=IDS)
def test_every_wrong_form_misses_the_rule_by_ten_times_on_rows(vn, jk, res):
    want, scale, _ = J.expected(vn, jk, res)
    names = J.variants_of(vn, jk, res)
    assert names
    for name in names:
        rows = J.variant_rows(vn, jk, res, name)
        r = err_ratio(rows, want.rows, scale)
        lg = err_ratio(J.run(J.with_variant(J.make_model(vn, jk, res), name), T.gin_batch())[0].logits, want.logits, scale)
        print(IDS[MODELS.index((vn, jk, res))], name, f"rows {r:.1f} x the rule, logits {lg:.1f} x")
        assert r >= 10.0, (name, r)


def test_every_wrong_form_is_exercised_by_some_model():
    seen = set()
    for vn, jk, res in MODELS:
        seen.update(J.variants_of(vn, jk, res))
    assert seen == set(J.VARIANTS)


@pytest.mark.parametrize("vn,jk,res", MODELS, ids=IDS)
def test_the_models_stay_inside_the_fast_paths_range(vn, jk, res):
    _, scale, _ = J.expected(vn, jk, res)
    print(IDS[MODELS.index((vn, jk, res))], f"scale {scale:.4g}")
    assert scale < 3e4


@pytest.mark.parametrize("jk", ["last", "sum"])
def test_the_undamped_residual_models_leave_it(jk):
    _, scale, _ = J.expected(True, jk, True, damped=False)
    print("undamped gin-virtual", jk, "res", f"scale {scale:.4g}")
    assert scale > 1.2e5
