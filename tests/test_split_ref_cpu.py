"""What tests/split_ref.py's bound can and cannot see, without a GPU.

DESIGN.md section 4 claims that the split-f16 dense products (hi.hi + hi.lo + lo.hi, fp32 accumulation) are fp32-accurate.  The parity
rule (tests/parity.py: 1e-4 of the activation scale) has 30 x to 1000 x of slack over the errors the kernels really make, so a kernel
that lost one cross term -- everywhere, in one K-step, in one 16-column output tile, in its K tail, in one layer -- would pass every
logits comparison of the suite.  This file proves that per model and input (the inputs tests/test_split_accuracy_gpu.py runs):
  * the float64 forward, the all-fp32 forward and the three-product split agree to E_ok, every named wrong variant is E_bad away, and
    E_bad / E_ok >= 64 (16 for the three outputs of split_ref.LOW_RATIO, which says why): B = sqrt(E_ok E_bad) has the room it claims;
  * every correct restatement stays below B / 8 and every wrong variant above 8 B (B / 4 and 4 B where the ratio asked is 16);
  * every wrong product variant PASSES today's parity rule on the logits -- the gap this bound closes, as a test.
It prints the table that DESIGN.md section 2 quotes (pytest -s)."""
import numpy as np
import pytest

from tests import numpy_ref, split_ref as sr
from tests.parity import err_ratio

CASES = sr.cases()
IDS = [f"{m}-seed{s}-{c}" for m, s, c in CASES]


def test_operand_splits_are_the_kernels():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 4, 4000), [0.0, 65504.0, -65504.0, 6.0e4, 2.0 ** -24, 1.0]]).astype(np.float32)
    hi = sr.rtz_f16(x)
    assert np.array_equal(hi.astype(np.float16).astype(np.float32), hi)                     # an f16 value,
    assert (np.abs(hi) <= np.abs(x)).all() and (np.sign(hi) * np.sign(x) >= 0).all()        # toward zero,
    inside = np.abs(x) < 65504.0
    up = np.nextafter(np.abs(hi[inside]).astype(np.float16), np.float16(np.inf)).astype(np.float32)
    assert (up > np.abs(x[inside])).all()                                                   # and the nearest such
    a_hi, a_lo = sr.split_act(x)
    normal = np.abs(x) >= 2.0 ** -3  # hi and lo both normal f16 values
    assert (np.abs(x.astype(np.float64) - a_hi - a_lo)[normal] <= 2.0 ** -20 * np.abs(x)[normal]).all()
    W = (rng.standard_normal((16, 100)) * 0.09).astype(np.float32)
    w_hi, w_lo, sc = sr.split_weight(W)
    m = float(np.abs(W).max()) * sc
    assert 1.0 <= m < 2.0 and np.log2(sc) == int(np.log2(sc))
    assert (np.abs(W.astype(np.float64) * sc - w_hi - w_lo) <= 2.0 ** -21 * np.abs(W * sc) + 2.0 ** -25).all()
    # the two sides of the ilogb boundary
    assert sr.pow2_scale(np.array([np.nextafter(np.float32(0.125), np.float32(0))])) == 16.0
    assert sr.pow2_scale(np.array([np.float32(0.125)])) == 8.0 and sr.pow2_scale(np.array([np.nextafter(np.float32(0.125), np.float32(1))])) == 8.0


@pytest.mark.parametrize("model", sr.MODELS)
def test_hooks_leave_the_float64_forward_alone(model):
    """dtype = float64 with the plain matmul as `dense` is the forward itself (bit for bit where the hook replaces a matmul; to float64
    rounding where it replaces PNA's einsum / DGN's two half products by one call), and the restated last stages are the forward's."""
    b, w = sr.batch_of(model, sr.SEEDS[model][0]), sr.weights_of(model)
    fwd = getattr(numpy_ref, f"{sr.base(model)}_forward")
    kw = {"return_x": True} if model == "GCN" else {"return_h": True}
    want, hs = fwd(b, w, **kw)
    got, hs2 = fwd(b, w, dtype=np.float64, dense=lambda a, W: a @ W.T, **kw)
    if model in ("PNA", "DGN"):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()) and np.abs(hs2 - hs).max() <= 1e-12 * np.abs(hs).max()
    else:
        assert np.array_equal(got, want) and np.array_equal(hs2, hs)
    ref = sr.reference(model, sr.SEEDS[model][0])
    assert np.abs(ref["logits"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    pw = sr.weights_of(model, "prescale")
    for k in sr.SPLIT_KEYS[model]:  # the pre-scale case's three scales, per split matrix
        tiny, below, above = sr.PRESCALE_LAYERS.get(k, (0, 1, 2))
        assert sr.pow2_scale(pw[k][tiny]) == 1024.0 * sr.pow2_scale(w[k][tiny])
        is_pow2 = lambda v: np.frexp(np.float64(v))[0] == 0.5
        mb, ma = np.abs(pw[k][below]).max(), np.abs(pw[k][above]).max()  # float32
        assert not is_pow2(mb) and is_pow2(np.nextafter(mb, np.float32(np.inf))) and sr.pow2_scale(pw[k][below]) * float(mb) > 1.999
        assert not is_pow2(ma) and is_pow2(np.nextafter(ma, np.float32(0))) and sr.pow2_scale(pw[k][above]) * float(ma) < 1.001


@pytest.mark.parametrize("model,seed,case", CASES, ids=IDS)
def test_the_bound_separates_every_wrong_variant(model, seed, case):
    tb = sr.table(model, seed, case)
    ref = sr.reference(model, seed, case)
    print(f"\n{model} seed {seed} {case}: N = {sr.batch_of(model, seed).total_nodes}, activation scale {ref['_acts']:.3g}")
    for name, r in tb.items():
        nearest = min(r.bad, key=r.bad.get)
        print(f"  {name:11s} E_ok {r.e_ok:.2e}  E_bad {r.e_bad:.2e}  ratio {r.e_bad / r.e_ok:7.1f}  B {r.bound:.2e}   nearest wrong: {nearest}")
    assert "logits" in tb and "rows" in tb and "h" in tb and "emb" in tb
    for name, r in tb.items():
        room = np.sqrt(sr.min_ratio(model, name, case))  # 8, or 4
        assert r.e_bad / r.e_ok >= sr.min_ratio(model, name, case), (model, seed, case, name, r.e_ok, r.e_bad)
        assert set(r.ok) == {"all fp32"} | {s.name for s in sr.OK_SPECS}
        for k, e in r.ok.items():
            assert e <= r.bound / room, (model, name, k, e, r.bound)
        assert len(r.bad) >= (8 if model in ("GAT", "PNA") else 10) - (0 if sr.BIASED[model] else 1)
        for k, e in r.bad.items():
            assert e >= r.bound * room, (model, name, k, e, r.bound)


@pytest.mark.parametrize("model,seed,case", [c for c in CASES if c[2] == "synth"], ids=[i for i, c in zip(IDS, CASES) if c[2] == "synth"])
def test_todays_parity_rule_passes_every_wrong_product_on_the_logits(model, seed, case):
    """The reason this file exists.  (The misplaced 1 / scale is not a lost term but a wrong bias, by a factor of 2 or more: the parity rule
    sees that one, and it is left out here.)"""
    ref = sr.reference(model, seed, case)
    _, bad, specs = sr.restatements(model, seed, case)
    worst = {}
    for name, spec in specs.items():
        r = err_ratio(bad[name]["logits"], ref["logits"], scale=ref["_acts"])
        # Every wrong product passes for five models.  GCN's logits are the exception, for the larger cross term only: a_lo.w_hi lost in
        # a K-step, a layer or everywhere (and the single product) reaches 1.04 x / 1.2 x / 2.5 x the rule's bound there -- asserted to stay
        # within 4 x; the smaller term lost anywhere, either term lost in one output tile and the K tail as one product pass for GCN too.
        must_pass = model != "GCN" or spec.drop in ("", "hl") or spec.where == "tile"
        worst[must_pass] = max(worst.get(must_pass, 0.0), r)
        assert r <= (1.0 if must_pass else 4.0), (model, seed, name, r)
    print(f"\n{model} seed {seed}: the wrong products reach {worst[True]:.3f} of the parity rule's bound on the logits"
          + (f" (GCN: the large term lost in a K-step, a layer or everywhere {worst[False]:.3f})" if False in worst else ""))
