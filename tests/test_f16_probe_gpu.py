"""The f16 exactness probe (tests/test_f16_mode_gpu.py::test_exactness_probe) on every F16 instance of gin_split.hip's kernels and on
every output they return -- tests/f16_probe.py lists the cases and, in a comment, the instance each one reaches.

The parity rule of the other tests (2e-4 of the activation scale) cannot tell FLOWGNN_NUMERIC_F16 from fp32.  Here the weights are
few-bit dyadic values and the graphs have power-of-two node counts, so that every fp32 sum of the mode is exact (tests/f16_ref.py
proves it per input; tests/test_f16_ref_cpu.py asserts it for each case without a GPU): the kernel must then reproduce the float64
restatement of the mode's WRITTEN definition (flowgnn.h, DESIGN.md, gin_split.hip's header) with f16 casts at the operand points
  * bit for bit where no inexact operation follows -- the h_5 rows, the pooled sum, the pooled maximum and the mean embedding (node
    counts are powers of two: the division is exact) -- and
  * to 1e-6 (1 + |want|) where the readout's final fp32 additions follow (logits, per-node logit terms),
and must NOT reproduce any wrong variant: rounding toward zero, no rounding (the f32 mode on the same engine included), the folded head
u unrounded or rounded toward zero, and with a trained eps each of three wrong eps vectors.  "Not reproduce" is the probe's criterion --
more than half of the elements, and the median, beyond 100 x the bound -- asserted for exactly the pairs that the references themselves
meet (tests/f16_probe.separation; the few that do not are named in tests/f16_probe.NOT_SEPARATED).

Every case checks which kernels ran (profile slots), that no exact re-run happened, and the default mode on the same engine against the
unrounded forward (1e-5: its fp32 roundings are not exact on this input).  What the engine refuses: nothing of the issue's list -- node
logits exclude sum / max pooling by contract (flowgnn.h), and no case asks for that."""
import numpy as np
import pytest

from flowgnn_amd import Engine
from tests import f16_probe as fp
from tests.test_embeddings_gpu import launched

pytestmark = pytest.mark.gpu
PER_SLOTS = {"gin_layer_fused", "gin_aggregate", "gin_mlp"}
BIT_EXACT = {"rows", "pooled"}  # no inexact fp32 operation between the exact sums and the stored value


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def run(e, b, c):
    """output name -> float64 array, in the shapes of the references"""
    ret = e.forward(b, **{k: True for k in c.fwd})
    ret = ret if isinstance(ret, tuple) else (ret,)
    assert len(ret) == 1 + len(c.fwd)
    return dict(zip(fp.outputs_of(c), ret))


@pytest.mark.parametrize("model,case", fp.PARAMS, ids=fp.IDS)
def test_probe(model, case):
    refs = fp.references(model, case)
    for v, (_, figure) in refs.items():
        assert figure is None or figure <= 24.0, f"fp32 would round in the {v} forward (2^{figure:.1f} > 2^24): the probe proves nothing"
    want_all = refs["rne"][0]
    table = fp.separation(model, case)
    b, w = fp.batch_of(model, case.batch), fp.case_weights(case)
    e = Engine(model, device=0, options=case.options)
    try:
        if case.tasks != 1:
            e.set_num_tasks(case.tasks)
        e.set_weights(w)
        e.set_numeric_mode("f16")
        if case.pooling != "mean":
            e.set_pooling(case.pooling)
        if case.eps:
            e.set_gin_eps(fp.EPS)
        e.profile_enable(True)
        if case.batch == "below_fill":
            assert e.graph_tile_fill(b.nums_of_nodes, b.nums_of_edges) < 0.5
        res = {}
        names = launched(e, lambda: res.update(got=run(e, b, case)))
        e.set_numeric_mode("f32")
        f32 = run(e, b, case)
        reruns = e.exact_reruns()
    finally:
        e.close()
    if case.kind == "resident":
        assert "gin_resident" in names and not (names & PER_SLOTS), names
        if "gin_tile_build" in case.options:
            assert ("gin_tile_build" in names) == bool(case.options["gin_tile_build"]), names
    else:
        assert names & PER_SLOTS and "gin_resident" not in names, names
    assert reruns == 0
    for o in fp.outputs_of(case):
        want = want_all[o]
        got32 = res["got"][o].reshape(want.shape)  # float32, as the engine returned it
        got, plain = got32.astype(np.float64), refs["none"][0][o]
        bound = fp.bound(want)
        ratio = float((np.abs(got - want) / bound).max())
        msg = f"{model} / {case.name} / {o}: worst ratio to the bound {ratio:.4f}"
        if o in BIT_EXACT:
            equal = int((got32 == want.astype(np.float32)).sum())
            msg += f", bit-equal to float32(want) {equal} of {want.size}"
        print(msg)
        assert ratio <= 1.0, msg
        if o in BIT_EXACT:
            assert np.array_equal(want.astype(np.float32).astype(np.float64), want)  # (an fp32 value: the exactness check's claim)
            assert equal == want.size, msg
        # the wrong variants, the pairs that the references themselves separate
        f32o = f32[o].reshape(want.shape).astype(np.float64)
        for v in refs:
            if v == "rne":
                continue
            if not table[(o, v)][0]:
                assert (model, case.name, o, v) in fp.NOT_SEPARATED
                continue
            ok, frac, med = fp.separated(got, refs[v][0][o], want)
            assert ok, (model, case.name, o, v, frac, med)
            if v == "none":  # control: the f32 mode on the same engine is that forward, and differs as much
                ok, frac, med = fp.separated(got, f32o, want)
                assert ok, (model, case.name, o, "f32 mode", frac, med)
        # control: the default mode computes the unrounded model
        assert (np.abs(f32o - plain) <= 1e-5 * (1.0 + np.abs(plain))).all(), (o, float(np.abs(f32o - plain).max()))
