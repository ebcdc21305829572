"""A trained eps for GIN / GIN-VN (flowgnn.h: flowgnn_set_gin_eps), the part that needs no GPU: the float64 forward that serves as the
expected value of tests/test_gin_eps_gpu.py, the fixed input of those tests and the proof that it can tell a wrong eps from the right
one, and the exporter / weight-file side.

The oracle has no eps.  `gin_eps_forward` is tests/numpy_ref.gin_forward with a = m + float64(s_l) * h, s_l = float32(1 + eps[l]); before
it serves as a reference it reproduces numpy_ref.gin_forward exactly at s = 1 and the oracle's logits within the parity rule."""
import os

import numpy as np
import pytest

from flowgnn_amd import export, graphpack as gp, weights
from tests import numpy_ref
from tests.parity import REL, assert_close, oracle_scale
from tests.test_export import ogb_forward, ogb_state_dict
from tests.test_resident_limits_gpu import random_graph

ND_OFF, ED_OFF = numpy_ref.ND_OFF, numpy_ref.ED_OFF
EPS = [1.0, -0.5, 0.75, 2.0, -0.75]  # 1 + eps exact in fp32, all five distinct, both signs
REL_F16 = 2e-4                        # the f16 mode's rule (tests/test_f16_mode_gpu.py)
MODELS = ["GIN", "GIN-VN"]


def self_scale(eps):
    """s_l as the engine forms it: (float)(1.0f + eps[l])."""
    return (np.float32(1.0) + np.asarray(eps, np.float32)).astype(np.float32)


def gin_eps_forward(batch, w, eps):
    """(logits, hs [6][N][100], largest |a|, largest hidden value) in float64; eps = None: s = 1."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    s = np.ones(5) if eps is None else f64(self_scale(eps))
    nemb, eemb = f64(w["node_embedding_weight"]), f64(w["edge_embedding_weight"])
    w1, b1 = f64(w["node_mlp_1_weights"]), f64(w["node_mlp_1_bias"])
    w2, b2 = f64(w["node_mlp_2_weights"]), f64(w["node_mlp_2_bias"])
    pw, pb = f64(w["graph_pred_weights"]).reshape(-1, 100), f64(w["graph_pred_bias"]).reshape(-1)
    N = batch.total_nodes
    ge = batch.global_edges()
    u, v = ge[:, 0], ge[:, 1]
    h = nemb[batch.node_feature.astype(np.int64) + ND_OFF[None, :]].sum(axis=1)
    hs = [h]
    amax = hmax = 0.0
    for l in range(5):
        ee = eemb[l][batch.edge_attr.astype(np.int64) + ED_OFF[None, :]].sum(axis=1)
        msg = np.maximum(h[u] + ee, 0.0)
        m = np.zeros((N, 100))
        np.add.at(m, v, msg)
        a = m + s[l] * h
        hid = np.maximum(a @ w1[l].T + b1[l], 0.0)
        amax, hmax = max(amax, float(np.abs(a).max())), max(hmax, float(np.abs(hid).max()))
        h = hid @ w2[l].T + b2[l]
        if l != 4:
            h = np.maximum(h, 0.0)
        hs.append(h)
    off = batch.node_offsets()
    pooled = np.add.reduceat(h, off[:-1], axis=0) / batch.nums_of_nodes[:, None]
    out = pooled @ pw.T + pb
    if out.shape[1] == 1:
        out = out[:, 0]
    return out, np.stack(hs), amax, hmax


def one_node(seed):  # n = 1, e = 0: the logit depends on the self term alone
    rng = np.random.default_rng(seed)
    nf = np.stack([rng.integers(0, c, 1) for c in (119, 4, 12, 12, 10, 6, 6, 2, 2)], 1).astype(np.int32)
    return gp.GraphBatch(np.array([1], np.int32), np.array([0], np.int32), nf, np.zeros((0, 2), np.int32), np.zeros((0, 3), np.int32))


def fixed_batch(model="GIN"):
    tiny = [random_graph(n, n + k, seed=40 + 2 * n + k) for n in (2, 3, 4, 5) for k in (0, 1)]
    b = gp.concat_batches([one_node(1), gp.synth_molhiv_batch(300, seed=13), one_node(2)] + tiny + [one_node(3)])
    return gp.add_virtual_nodes(b) if model == "GIN-VN" else b


def fixed_weights(num_tasks=1):
    w = weights.synth_gin_weights(seed=7, num_tasks=num_tasks) if num_tasks != 1 else weights.synth_gin_weights(seed=7)
    w["graph_pred_weights"] = (np.asarray(w["graph_pred_weights"], np.float32) * np.float32(8)).astype(np.float32)
    return w


def bound(want, scale, rel):
    return rel * (scale + np.abs(want))


# ---------------------------------------------------------------- the reference is the project's own at s = 1
@pytest.mark.parametrize("model", MODELS)
def test_forward_reproduces_numpy_ref_and_the_oracle_without_eps(model, oracle):
    b, w = fixed_batch(model), fixed_weights()
    out, hs, amax, hmax = gin_eps_forward(b, w, None)
    want, want_hs = numpy_ref.gin_forward(b, w, return_h=True)
    assert np.array_equal(out, want) and np.array_equal(hs, want_hs)
    out0, hs0, _, _ = gin_eps_forward(b, w, [0.0] * 5)  # s_l = float32(1 + 0) = 1
    assert np.array_equal(out0, want) and np.array_equal(hs0, want_hs)
    orc, hd = oracle.gin_forward(b, [w], dump_h=True, nthreads=8)
    assert_close(np.asarray(orc, np.float64), out, scale=oracle_scale(hd), what=(model, "oracle vs the float64 forward at s = 1"))
    assert amax >= float(np.abs(hs[:5]).max()) and hmax > 0.0


# ---------------------------------------------------------------- the input proves something
def wrong_variants():
    out = [("all zero", [0.0] * 5)]
    for l in range(5):
        e = list(EPS)
        e[l] = 0.0
        out.append((f"layer {l} zeroed", e))
    for l in range(4):
        e = list(EPS)
        e[l], e[l + 1] = e[l + 1], e[l]
        out.append((f"layers {l} and {l + 1} swapped", e))
    return out


@pytest.mark.parametrize("model", MODELS)
def test_the_fixed_input_separates_every_wrong_eps(model):
    """A dropped term, a layer index off by one and a wrong sign must each move more than a quarter of the graphs' logits by more
    than 10 x the f32 bound (5 x the f16 mode's): otherwise the GPU tests' logit comparisons would pass with the eps applied wrongly."""
    b, w = fixed_batch(model), fixed_weights()
    want, hs, amax, hmax = gin_eps_forward(b, w, EPS)
    scale = oracle_scale(hs)
    assert max(amax, hmax) < 6.0e4  # far from the range threshold: the GPU runs assert exact_reruns() == 0
    variants = wrong_variants()
    assert len(variants) == 10
    shares = []
    for name, e in variants:
        got = gin_eps_forward(b, w, e)[0]
        d = np.abs(got - want)
        s32 = float((d > 10.0 * bound(want, scale, REL)).mean())
        s16 = float((d > 5.0 * bound(want, scale, REL_F16)).mean())
        shares.append(min(s32, s16))
        assert s32 > 0.25 and s16 > 0.25, (model, name, s32, s16)
    print(model, "smallest share of graphs moved:", min(shares), "scale", scale, "largest operand", max(amax, hmax))


# ---------------------------------------------------------------- exporter and weight files
def trained_state_dict(seed=3, with_bn=True):
    sd = ogb_state_dict("gin", seed, with_bn=with_bn)
    for l, e in enumerate([0.12, -0.07, 0.3, -0.21, 0.05]):
        sd[f"gnn_node.convs.{l}.eps"] = np.array([e])
    return sd


def test_default_export_still_refuses_a_trained_eps(tmp_path):
    sd = trained_state_dict()
    with pytest.raises(export.ExportError, match="the reference's GIN has no eps term"):
        export.gin_weights_from_ogb_state_dict(sd)
    with pytest.raises(export.ExportError, match="eps"):
        export.export_weights("GIN", sd, str(tmp_path))


def test_keep_eps_returns_weights_and_the_five_values():
    sd = trained_state_dict()
    w = export.gin_weights_from_ogb_state_dict(sd, keep_eps=True)
    assert list(w) == list(weights.GIN_FILES)
    e = export.gin_eps_from_ogb_state_dict(sd)
    assert e.dtype == np.float32 and e.shape == (5,)
    assert np.array_equal(e, np.array([0.12, -0.07, 0.3, -0.21, 0.05], np.float32))
    assert np.array_equal(export.gin_eps_from_ogb_state_dict(ogb_state_dict("gin", 3)), np.zeros(5, np.float32))


def test_eps_file_round_trip(tmp_path):
    w = weights.synth_gin_weights(seed=7)
    weights.save_gin_weights(w, str(tmp_path))
    assert np.array_equal(weights.load_gin_eps(str(tmp_path)), np.zeros(5, np.float32))  # the default still writes zeros
    weights.save_gin_weights(w, str(tmp_path), eps=EPS)
    got = weights.load_gin_eps(str(tmp_path))
    assert got.dtype == np.float32 and np.array_equal(got, np.asarray(EPS, np.float32))
    assert os.path.getsize(os.path.join(str(tmp_path), "gin_ep1_eps_dim100.bin")) == 20
    back = weights.load_gin_weights(str(tmp_path))
    assert all(np.array_equal(back[k], np.asarray(w[k], np.float32).reshape(back[k].shape)) for k in w)


@pytest.mark.parametrize("with_bn", [True, False])
def test_exported_set_with_eps_matches_ogb_semantics(tmp_path, with_bn):
    """tests/test_export.py's OGB restatement (which has the (1 + eps) term) against the float64 eps forward of the exported files."""
    sd = trained_state_dict(with_bn=with_bn)
    batch = gp.synth_molhiv_batch(24, seed=9)
    want = ogb_forward("gin", sd, batch)
    export.export_weights("GIN", sd, str(tmp_path), keep_eps=True)
    assert sorted(os.listdir(tmp_path)) == sorted([f for f, _ in weights.GIN_FILES.values()] + ["gin_ep1_eps_dim100.bin"])
    w, eps = weights.load_gin_weights(str(tmp_path)), weights.load_gin_eps(str(tmp_path))
    got = gin_eps_forward(batch, w, eps)[0]
    assert np.allclose(got, want, rtol=1e-4, atol=2e-5), np.abs(got - want).max()  # float32 files vs float64 source
    without = gin_eps_forward(batch, w, None)[0]
    assert np.abs(without - want).max() > 100 * np.abs(got - want).max()  # ... and the eps-less forward is a different model
