"""OGB's set2set readout on the references alone (tests/set2set_ref.py; flowgnn.h: flowgnn_set_set2set_pooling):
the float64 restatement against a torch.nn.LSTM driven as PyG's Set2Set drives it, the exporter and the files, the float32 restatement
against the parity rule, and the distance of every named wrong form from the definition.  No GPU."""
import functools

import numpy as np
import pytest

from flowgnn_amd import export, graphpack as gp, weights
from tests import gin_wide_ref as W, set2set_ref as S
from tests.parity import REL, err_ratio

LOW_RATIO = 16.0  # split_ref.LOW_RATIO's value: how many times the rule a wrong form must be away


@functools.lru_cache(maxsize=None)
def inputs(seed):
    """(batch, rows float32 [N][300]): 64 molhiv-shaped graphs, the float64 forward of the width-300 synthetic GIN weights, cast."""
    b = gp.synth_molhiv_batch(64, seed=seed)
    w = weights.synth_gin_weights(seed=7, emb_dim=300)
    return b, W.forward(b, w, eps=np.asarray(W.TRAINED_EPS, np.float32)).rows.astype(np.float32)


def scale_of(rows, q, logits):
    return max(1.0, float(np.abs(rows).max()), float(np.abs(q).max()), float(np.abs(logits).max()))


# ---------------------------------------------------------------- 1. the restatement is PyG's Set2Set on a torch.nn.LSTM
@pytest.mark.parametrize("steps", [2, 3])
@pytest.mark.parametrize("kind,vn,tasks", [("gin", False, 1), ("gcn", True, 3)])
def test_restatement_equals_the_torch_model(kind, vn, tasks, steps):
    torch = pytest.importorskip("torch")
    from tests import ogb_torch as T
    model = S.set2set_model(kind, vn, num_tasks=tasks, steps=steps)
    assert isinstance(model.pool.lstm, torch.nn.LSTM) and model.pool.lstm.input_size == 600 and model.pool.lstm.hidden_size == 300
    assert {"pool.lstm.weight_ih_l0", "pool.lstm.weight_hh_l0", "pool.lstm.bias_ih_l0", "pool.lstm.bias_hh_l0", "graph_pred_linear.weight"} <= set(model.state_dict())
    b = T.batch_of(kind)
    want, _, _ = T.run(model, b)
    q, logits, _ = S.readout(want.rows, b, S.s2s_of(model), steps=steps)
    dq, dl = float(np.abs(q - want.pooled).max()), float(np.abs(logits - want.logits).max())
    print(f"{kind} vn={vn} T={tasks} steps={steps}: max |q* - torch| {dq:.2e}, max |logits - torch| {dl:.2e}")
    assert want.pooled.shape == (b.num_graphs, 600)
    assert dq <= 1e-10 and dl <= 1e-10


# ---------------------------------------------------------------- 2. exporter and files
@pytest.mark.parametrize("kind,tasks", [("gin", 1), ("gcn", 3)])
def test_exporter_round_trip(kind, tasks, tmp_path):
    pytest.importorskip("torch")
    model = S.set2set_model(kind, False, num_tasks=tasks)
    sd = model.state_dict()
    kw = dict(keep_eps=True) if kind == "gin" else dict(emb_dim=300)
    w = export.export_weights(kind.upper(), sd, str(tmp_path), set2set=True, multi_task=tasks > 1, **kw)
    assert w["graph_pred_weights"].shape[-1] == 300 and not w["graph_pred_weights"].any() and not np.asarray(w["graph_pred_bias"]).any()
    assert weights.set2set_file(kind.upper(), 300) == f"{kind}_ep1_set2set_dim300.bin"
    assert (tmp_path / f"{kind}_ep1_set2set_dim300.bin").stat().st_size == 4 * (1200 * 902 + tasks * 601)
    got = weights.load_set2set(str(tmp_path), model=kind.upper(), emb_dim=300)
    want = export.set2set_from_ogb_state_dict(sd, emb_dim=300)
    assert tuple(got) == weights.SET2SET_KEYS == tuple(want)
    ref = S.s2s_of(model)
    for k, shp in weights.set2set_shapes(300, tasks).items():
        assert got[k].shape == shp and got[k].dtype == np.float32
        assert np.array_equal(got[k], ref[k].astype(np.float32).reshape(shp)), k  # bit for bit


def test_exporter_refusals(tmp_path):
    pytest.importorskip("torch")
    sd = S.set2set_model("gin", False).state_dict()
    with pytest.raises(export.ExportError, match="set2set=True"):
        export.export_weights("GIN", sd, str(tmp_path / "a"), keep_eps=True)
    with pytest.raises(export.ExportError, match="attention_pooling"):
        export.export_weights("GIN", sd, str(tmp_path / "b"), keep_eps=True, set2set=True, attention_pooling=True)
    with pytest.raises(export.ExportError, match="GIN's and GCN's"):
        export.export_weights("GIN-VN", sd, str(tmp_path / "c"), set2set=True)
    with pytest.raises(export.ExportError, match="pool.lstm"):
        export.set2set_from_ogb_state_dict({k: v for k, v in sd.items() if not k.startswith("pool.")})
    with pytest.raises(export.ExportError):
        export.set2set_from_ogb_state_dict(sd, emb_dim=100)
    assert not any((tmp_path / d).exists() for d in "abc")  # refused before anything is written
    with pytest.raises(ValueError):
        weights.set2set_file("GAT", 300)
    with pytest.raises(ValueError):
        weights.set2set_shapes(100)
    s = weights.synth_set2set()
    with pytest.raises(ValueError, match="w_ih"):
        weights.checked_set2set(dict(s, w_ih=s["w_ih"][:, :300]))
    with pytest.raises(ValueError, match="keys"):
        weights.checked_set2set({k: v for k, v in s.items() if k != "b_hh"})
    weights.save_set2set(s, str(tmp_path / "d"))
    with open(tmp_path / "d" / "gin_ep1_set2set_dim300.bin", "ab") as f:
        f.write(b"\0" * 8)
    with pytest.raises(ValueError, match="NUM_TASK"):
        weights.load_set2set(str(tmp_path / "d"))


def test_synth_set2set_is_what_the_docs_say():
    s = weights.synth_set2set()
    assert tuple(s) == weights.SET2SET_KEYS and [v.shape for v in s.values()] == list(weights.set2set_shapes(300, 1).values())
    k = 1 / np.sqrt(300)
    assert np.abs(s["w_ih"]).max() <= k and np.abs(s["w_hh"]).max() <= k and 0.25 < s["b_ih"].std() < 0.35 and 0.25 < s["b_hh"].std() < 0.35
    t3 = weights.synth_set2set(num_tasks=3)
    assert np.array_equal(t3["w_ih"], s["w_ih"]) and t3["head_w"].shape == (3, 600) and t3["head_b"].shape == (3,)


# ---------------------------------------------------------------- 3. float32 against the rule; the fold
@pytest.mark.parametrize("steps", [2, 3])
@pytest.mark.parametrize("seed", [5, 7])
def test_float32_restatement_within_half_the_rule(seed, steps):
    b, rows = inputs(seed)
    s2s = weights.synth_set2set()
    q, logits, _ = S.readout(rows, b, s2s, steps=steps)
    q32, l32, _ = S.readout(rows, b, s2s, steps=steps, dtype=np.float32)
    scale = scale_of(rows, q, logits)
    rq, rl = err_ratio(q32, q, scale), err_ratio(l32, logits, scale)
    print(f"seed {seed} steps {steps}: float32 restatement at {rq:.4f} (q*) and {rl:.4f} (logits) of the rule, scale {scale:.3g}")
    assert q32.dtype == np.float32 and rq <= 0.5 and rl <= 0.5


def test_fold_is_the_definition():
    """W_hh folded into W_ih's first D columns (float64, rounded once): the same z to fp32 rounding of the weights."""
    b, rows = inputs(5)
    s2s = weights.synth_set2set()
    w, bias = S.folded(s2s)
    f = dict(s2s, w_ih=w, w_hh=np.zeros_like(s2s["w_hh"]), b_ih=bias, b_hh=np.zeros_like(bias))
    q, logits, _ = S.readout(rows, b, s2s, steps=3)
    qf, lf, _ = S.readout(rows, b, f, steps=3)
    scale = scale_of(rows, q, logits)
    assert err_ratio(qf, q, scale) <= 0.01 and err_ratio(lf, logits, scale) <= 0.01


# ---------------------------------------------------------------- 4. every wrong form is far from the definition
@functools.lru_cache(maxsize=None)
def wrong_table(seed, steps):
    """wrong form -> (ratio of the worst graph's logit to the rule with the definition as the reference, the same with the wrong form as
    the reference)."""
    b, rows = inputs(seed)
    s2s = weights.synth_set2set()
    q, logits, _ = S.readout(rows, b, s2s, steps=steps)
    out = {}
    for name in S.WRONG:
        qw, lw, _ = S.readout(rows, b, s2s, steps=steps, wrong=name)
        out[name] = (err_ratio(lw, logits, scale_of(rows, q, logits)), err_ratio(logits, lw, scale_of(rows, qw, lw)))
    return out


@pytest.mark.parametrize("steps", [2, 3])
@pytest.mark.parametrize("seed", [5, 7])
def test_every_wrong_form_is_far_from_the_definition(seed, steps):
    """At least LOW_RATIO x the rule on at least one graph's logit, in both directions (whichever of the two is taken as the reference):
    a parity within the rule excludes each of them."""
    t = wrong_table(seed, steps)
    assert set(t) == set(S.WRONG) and len(S.WRONG) == 9
    for name, (fwd, back) in t.items():
        print(f"| {seed} | {steps} | {S.WRONG_NAMES[name]} | {fwd:.0f} | {back:.0f} |")
    for name, (fwd, back) in t.items():
        assert fwd >= LOW_RATIO and back >= LOW_RATIO, (name, fwd, back)
    b, rows = inputs(seed)
    ok = S.readout(rows, b, weights.synth_set2set(), steps=steps, dtype=np.float32)[1]
    q, logits, _ = S.readout(rows, b, weights.synth_set2set(), steps=steps)
    assert err_ratio(ok, logits, scale_of(rows, q, logits)) * LOW_RATIO <= min(min(v) for v in t.values())  # the right form is on the other side


def test_saturation_is_safe_in_the_restatement():
    """x 64: every gate and the softmax saturated, no NaN in either dtype (what the GPU test then compares with)."""
    b, rows = inputs(5)
    s = {k: v * np.float32(64) if k in ("w_ih", "w_hh", "b_ih", "b_hh") else v for k, v in weights.synth_set2set().items()}
    for dt in (np.float64, np.float32):
        q, logits, _ = S.readout(rows, b, s, steps=2, dtype=dt)
        assert np.isfinite(q).all() and np.isfinite(logits).all()
