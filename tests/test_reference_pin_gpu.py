"""The HIP engine against the REFERENCE's own outputs (tests/golden/reference_pin_<model>.npz: the reference's kernel sources run
against oracle/hls_standin, float form and ap_fixed form; tests/test_reference_pin_cpu.py pins the oracle to the same files).

Per model, on its fixture batch (64 molhiv- / molpcba-shaped or 24 hep10k-shaped graphs, a third of them directed with duplicate
edges and self loops, plus five tiny graphs):
  float mode   |gpu - reference| <= 1e-4 (scale + |reference|) (tests/parity.py), scale from the oracle's dumped activations, on the
               graph-resident path and on the per-layer path (<model>_resident 0), with synthetic and with the trained weights; which
               path ran is read from the profile slots, and no exact re-run may have happened.
  GAT          gat_reference_quirk 1 against the batched reference, the default against the reference called one graph per call.
  fixed point  the engine's patterns equal the reference's, bit for bit.
When the libraries themselves are there (oracle/_ref, built where the reference checkout is), three seeds of random_tileable_batch
inside the reference's caps run live, by the same rules.  Nothing here reads the reference checkout."""
import numpy as np
import pytest

from flowgnn_amd import Engine, graphpack as gp, weights
from tests import ref_pin as rp
from tests.golden import make_reference_pin as fx
from tests.parity import assert_close, oracle_scale
from tests.test_embeddings_gpu import launched
from tests.test_resident_limits_gpu import random_tileable_batch
from tests.test_split_accuracy_gpu import DENSE_SLOT, FUSED_SLOT, RESIDENT_SLOT

pytestmark = pytest.mark.gpu
PATHS = ("resident", "per_layer")


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def base(model):
    return model.replace("-VN", "").lower()


def activation_scale(oracle, model, b, w, quirk):
    kw = dict(feature_offset_quirk=quirk) if model == "GAT" else {}
    _, hd = getattr(oracle, base(model) + "_forward")(b, [w], dump_h=True, nthreads=8, **kw)
    return oracle_scale(hd)


def run_float(model, b, w, path, quirk=False, extra=None):
    """(logits, profile slots launched, exact re-runs)"""
    opts = dict(extra or {}) if path == "resident" else {f"{base(model)}_resident": 0}
    if quirk:
        opts["gat_reference_quirk"] = 1
    e = Engine(model, device=0, options=opts)
    try:
        e.set_weights(w)
        e.profile_enable(True)
        got = {}
        names = launched(e, lambda: got.update(out=e.forward(b)))
        return got["out"], names, e.exact_reruns()
    finally:
        e.close()


def check_float(oracle, model, b, w, want, path, quirk, what, extra=None):
    got, names, reruns = run_float(model, b, w, path, quirk, extra)
    must = (RESIDENT_SLOT if path == "resident" else FUSED_SLOT)[model]
    others = {RESIDENT_SLOT[model], FUSED_SLOT[model], DENSE_SLOT[model]} - {must, None}
    assert must in names and not (names & others), (what, path, sorted(names))
    assert reruns == 0, (what, path, "exact re-runs", reruns)
    assert_close(got, want, activation_scale(oracle, model, b, w, quirk), what=f"{what} / {path}")


def run_fixed(model, b, w, quirk=False):
    e = Engine(model, device=0, options={"gat_reference_quirk": 1} if quirk else {})
    try:
        e.set_weights(w)
        e.set_numeric_mode("q6.10")
        out = e.forward(b)
    finally:
        e.close()
    p = np.rint(out.astype(np.float64) * float(1 << rp.FRAC_BITS[model]))
    assert np.array_equal(p / float(1 << rp.FRAC_BITS[model]), out.astype(np.float64))  # exact multiples of the grid step
    return p.astype(np.int16)


def fixture(model):
    z = np.load(fx.path(model))
    b = fx.from_npz(z)
    cases = fx.weight_cases(model, b.num_graphs)
    return z, b, {k: cases[k][0][0] for k in ("synth", "trained")}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("model", rp.MODELS)
def test_float_mode_meets_the_reference(oracle, model, path):
    z, b, sets = fixture(model)
    for name, w in sets.items():
        check_float(oracle, model, b, w, z[f"f32_{name}"], path, model == "GAT", f"{model} / {name}")
    if model == "GAT":  # the default (per-graph feature offsets): the reference called one graph per call
        check_float(oracle, model, b, sets["synth"], z["f32_synth_per_graph"], path, False, "GAT / synth / one graph per call")


@pytest.mark.parametrize("model", rp.MODELS)
def test_fixed_point_mode_equals_the_reference(model):
    z, b, sets = fixture(model)
    for name, w in sets.items():
        got = run_fixed(model, b, w, quirk=(model == "GAT"))
        assert np.array_equal(got, z[f"fx_{name}"]), (model, name, np.flatnonzero(got != z[f"fx_{name}"])[:8])
    if model == "GAT":
        got = run_fixed(model, b, sets["synth"])
        assert np.array_equal(got, z["fx_synth_per_graph"]), np.flatnonzero(got != z["fx_synth_per_graph"])[:8]


def live_batch(model, seed):
    """tests/test_resident_limits_gpu.py's random batches (1-node graphs, no edges, isolated nodes, duplicates, self loops, hubs), every
    graph inside the model's smallest tile and far inside the reference's caps."""
    b = random_tileable_batch(9000 + 17 * seed + len(model), max_nodes=128 if model == "DGN" else 190, eigen=(model == "DGN"))
    if model not in ("PNA", "DGN"):  # the molecule models' tiles hold at most 960 in-edges
        keep = np.nonzero(b.nums_of_edges <= 900)[0]
        b = gp.concat_batches([b.slice(int(g), int(g) + 1) for g in keep])
    # GIN-VN takes the batch as it is, as tests/test_resident_limits_gpu.py gives it: a virtual node over 190 nodes of these dense
    # random graphs drives the sums past the f16 range, and the batch would (rightly) re-run on the fp32 kernels
    assert rp.inside_caps(model, b)
    return b


@pytest.mark.parametrize("model", rp.MODELS)
def test_live_reference_on_random_batches(oracle, model):
    if not rp.available():
        print(f"\nSKIP: no built libraries in {rp.REF_DIR} and no reference checkout")
        pytest.skip("no oracle/_ref libraries")
    w = weights.SYNTH[model](seed=11)
    for seed in range(3):
        b = live_batch(model, seed)
        quirk = model == "GAT"
        want = rp.run(model, "f32", b, [w])
        # DGN takes the resident kernel by the batch's density (E >= 8 N: kNN graphs, the fixture batch); these sparse batches would
        # go to the in-edge walk of the per-layer path by default, so the resident kernel is asked for (dgn_resident 2)
        extra = {"dgn_resident": 2} if model == "DGN" else None
        for path in PATHS:
            check_float(oracle, model, b, w, want, path, quirk, f"{model} / live seed {seed}", extra)
        assert np.array_equal(run_fixed(model, b, w, quirk), rp.run(model, "fx", b, [w])), (model, seed)
        if model == "GAT":
            check_float(oracle, model, b, w, rp.run_per_graph(model, "f32", b, w), "resident", False, f"GAT / live seed {seed} / one graph per call")
            assert np.array_equal(run_fixed(model, b, w), rp.run_per_graph(model, "fx", b, w)), (model, seed)
