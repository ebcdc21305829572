"""What the f16 exactness probe (tests/test_f16_probe_gpu.py) can prove, shown before a GPU is involved: its float64 references
(tests/f16_ref.gin_forward with eps, pooling and the extra outputs) are exact in fp32 on every case's input, agree with the project's
other references where they overlap, and differ from each wrong variant by far more than the probe's bound -- pair by pair, per output,
with the pairs that do not written out by name (tests/f16_probe.NOT_SEPARATED)."""
import numpy as np
import pytest

from tests import f16_probe as fp, f16_ref
from tests.test_gin_eps import EPS as EPS_TRAINED, fixed_batch, fixed_weights, gin_eps_forward

ALL = f16_ref.OUTPUTS


# ---------------------------------------------------------------- exactness and separation, per probe case
@pytest.mark.parametrize("model,case", fp.PARAMS, ids=fp.IDS)
def test_case_is_exact_and_separates(model, case):
    refs = fp.references(model, case)
    figures = {v: r[1] for v, r in refs.items() if r[1] is not None}
    print(f"{model} / {case.name}: fp32-exactness figure log2(sum |terms| / quantum), <= 24 passes:",
          ", ".join(f"{v} {f:.1f}" for v, f in figures.items()))
    assert set(figures) == {"rne", "rtz"} | (set(fp.WRONG_EPS) if case.eps else set())
    assert set(refs) - set(figures) == {"none"} | {n for n, (p, _) in fp.WRONG_POINT.items() if p != "u" or case.fold}
    for v, f in figures.items():
        assert f <= 24.0, f"fp32 would round on this input in the {v} forward (2^{f:.1f} > 2^24): the probe proves nothing"
    table = fp.separation(model, case)
    print("  output  variant: fraction of elements beyond 100 x the bound, median ratio to the bound")
    for (o, v), (ok, frac, med) in table.items():
        print(f"  {o:7s} {v:28s} {frac:5.2f} {med:12.1f}  {'separates' if ok else 'DOES NOT SEPARATE'}")
    # the two conditions that keep the named list from hiding anything
    for (o, v), (ok, frac, med) in table.items():
        if o == "logits" or (o in ("rows", "pooled") and v == "rtz"):
            assert ok, (model, case.name, o, v, frac, med)
    # ... and the list is the computed table's, in both directions, with the fractions it states
    failing = {(model, case.name, o, v): frac for (o, v), (ok, frac, _) in table.items() if not ok}
    named = {k: f for k, f in fp.NOT_SEPARATED.items() if k[0] == model and k[1] == case.name}
    assert set(failing) == set(named), (failing, named)
    for k in named:
        assert abs(failing[k] - named[k]) <= 0.01, (k, failing[k], named[k])


def test_the_named_list_names_cases_that_exist():
    ids = {(m, c.name) for m, c in fp.PARAMS}
    assert all((k[0], k[1]) in ids for k in fp.NOT_SEPARATED)
    assert len({c.name for c in fp.CASES}) == len(fp.CASES)


# ---------------------------------------------------------------- consistency with the other references
@pytest.mark.parametrize("model", fp.MODELS)
def test_unrounded_forward_is_the_eps_reference(model):
    """rnd = "none": tests/test_gin_eps.py::gin_eps_forward, logits and h_5 rows, on that file's input, weights and eps."""
    b, w = fixed_batch(model), fixed_weights()
    for eps in (EPS_TRAINED, None):
        want, hs, _, _ = gin_eps_forward(b, w, eps)
        got = f16_ref.gin_forward(b, w, fold=False, rnd="none", eps=eps, outputs=ALL)
        assert np.allclose(got["logits"], want, rtol=1e-12, atol=1e-12)
        assert np.allclose(got["rows"], hs[5], rtol=1e-12, atol=1e-12)
        folded = f16_ref.gin_forward(b, w, fold=True, rnd="none", eps=eps, outputs=("logits",))["logits"]
        assert np.allclose(folded, want, rtol=1e-12, atol=1e-12)  # (unrounded, the fold is algebra)


@pytest.mark.parametrize("model", fp.MODELS)
@pytest.mark.parametrize("tasks", [1, 2])
def test_without_eps_it_is_its_old_self(model, tasks):
    """The arguments this file's cases add leave the function's earlier results alone: the logits through `outputs` and with five
    zeros for eps carry the bits of the plain call, checked figure included."""
    b, w = fp.batch_of(model, "extra"), fp.weights_of(tasks)
    for fold in (True, False):
        for rnd in ("rne", "rtz", "none"):
            old = f16_ref.gin_forward(b, w, fold=fold, rnd=rnd)
            for eps in (None, [0.0] * 5):
                new = f16_ref.gin_forward(b, w, fold=fold, rnd=rnd, eps=eps, outputs=("logits",))
                assert np.array_equal(new["logits"], old), (fold, rnd, eps)
        old, fig = f16_ref.gin_forward(b, w, fold=fold, check=True)
        new, fig_new = f16_ref.gin_forward(b, w, fold=fold, check=True, outputs=("logits",))
        assert np.array_equal(new["logits"], old) and fig_new == fig


@pytest.mark.parametrize("model", fp.MODELS)
@pytest.mark.parametrize("tasks", [1, 2])
@pytest.mark.parametrize("pooling", ["mean", "sum", "max"])
def test_outputs_are_consistent_with_each_other(model, tasks, pooling):
    b, w = fp.batch_of(model, "extra"), fp.weights_of(tasks)
    pw, pb = np.asarray(w["graph_pred_weights"], np.float64).reshape(-1, 100), np.asarray(w["graph_pred_bias"], np.float64).reshape(-1)
    close = lambda a, c: np.allclose(a, c, rtol=1e-12, atol=1e-12)
    o = f16_ref.gin_forward(b, w, fold=False, eps=fp.EPS, pooling=pooling, outputs=ALL)
    assert o["rows"].shape == (b.total_nodes, 100) and o["pooled"].shape == (b.num_graphs, 100)
    assert np.array_equal(o["pooled"], f16_ref.pool(o["rows"], b, pooling))
    head = o["pooled"] @ pw.T + pb
    assert close(head[:, 0] if tasks == 1 else head, o["logits"])  # head(pool(rows)) is the logit
    terms = o["rows"] @ pw.T + pb
    assert close(terms[:, 0] if tasks == 1 else terms, o["terms"])
    if pooling == "mean":
        assert close(f16_ref.pool(o["terms"], b, "mean"), o["logits"])  # the mean of the terms is the logit
    if tasks == 1 and pooling != "max":  # the folded rule: its own terms, the same identities
        f = f16_ref.gin_forward(b, w, fold=True, eps=fp.EPS, pooling=pooling, outputs=("logits", "terms"))
        if pooling == "mean":
            assert close(f16_ref.pool(f["terms"], b, "mean"), f["logits"])
        else:
            assert close(f16_ref.pool(f["terms"], b, "sum") - (b.nums_of_nodes - 1) * pb[0], f["logits"])  # the bias once, not per node
        # u's rounding shows on these weights (r(u) is r(W2)^T w here, so the two rules agree; an unrounded u does not)
        g = f16_ref.gin_forward(b, w, fold=True, eps=fp.EPS, pooling=pooling, rnd={"u": "none"})
        assert float(np.abs(f["logits"] - g).max()) > 1e-5
        with pytest.raises(ValueError):
            f16_ref.gin_forward(b, w, fold=True, pooling=pooling, outputs=("rows",))
