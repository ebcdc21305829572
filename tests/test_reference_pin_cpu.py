"""The oracle against the reference's own kernel sources (tests/ref_pin.py; make -C oracle ref).

(a) float form -- the reference's program in fp32: oracle.<model>_forward equals it bit for bit (GAT: with feature_offset_quirk,
    which is what the batched reference does, GAT/src/GAT_compute.cc:72; without it the oracle differs from graph 1 on -- the
    negative control -- and equals the reference called one graph per call).
(b) fixed form -- the reference's program in ap_fixed under the operator rules of oracle/hls_standin/ap_fixed.h:
    oracle.gin_forward_q / q_forward give the same 16-bit patterns.
(c) committed fixtures of the reference's outputs (tests/golden/reference_pin_<model>.npz): the oracle against the fixture (runs
    everywhere), the fixture against the live libraries.

Inputs per model (INPUTS): the synthetic batch of its dataset shape; a directed variant; duplicate edges and self loops; one-node,
edgeless and two-node graphs; a graph at both caps of its dcl.h between ordinary ones; two weight sets with reload_weights switching
mid-batch; the shipped trained weights.  Left out: none -- built stand-alone with -fsanitize=address,undefined
(test_reference_stays_inside_its_arrays), every model in both forms stays inside its arrays on the tiny, capped, directed, duplicate
and reload inputs, so no input had to go; graphs BEYOND the caps are not inputs of the reference (ref_pin.run refuses them: MAX_NODE / MAX_EDGE size its tables, e.g. GIN/src/globals.cc:11-21).  Non-finite results
would be compared as such (equal_nan), none occurs.

The tests that need the libraries skip, and print that they do, only when there is neither a reference checkout nor a built
oracle/_ref."""
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import graphpack as gp, weights
from tests import ref_pin as rp
from tests.golden import make_ref_weights
from tests.golden import make_reference_pin as fx

ROOT = rp.ROOT


def need_libraries():
    if not rp.available():
        print(f"\nSKIP: no reference checkout at {rp.REF} and no built libraries in {rp.REF_DIR}")
        pytest.skip("neither a reference checkout nor built oracle/_ref libraries")


def oracle_float(oracle, model, b, sets, rw=None, quirk=True):
    kw = dict(feature_offset_quirk=quirk) if model == "GAT" else {}
    return getattr(oracle, model.replace("-VN", "").lower() + "_forward")(b, sets, rw, nthreads=8, **kw)


def oracle_fixed(oracle, model, b, sets, rw=None, quirk=True):
    if model in ("GIN", "GIN-VN"):
        return oracle.gin_forward_q(b, sets, rw, nthreads=8)[1]
    return oracle.q_forward(model, b, sets, rw, nthreads=8, feature_offset_quirk=quirk)[1]


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want, equal_nan=(got.dtype.kind == "f"))


def vn(model, b):
    return gp.add_virtual_nodes(b) if model == "GIN-VN" else b


def _dataset(model):
    return rp.dataset_batch(model, 48 if model in ("PNA", "DGN") else 200, 3)


def _directed(model):
    return vn(model, rp.directed_variant(rp.dataset_batch(model.replace("-VN", ""), 24, 5)))


def _duplicates(model):
    return vn(model, rp.with_duplicates(rp.dataset_batch(model.replace("-VN", ""), 24, 6), 5))


def _tiny(model):
    return vn(model, rp.tiny_graphs(9, model == "DGN"))


def _capped(model):
    return gp.concat_batches([rp.dataset_batch(model, 2, 1), rp.capped_graph(model, 41), rp.dataset_batch(model, 2, 2)])


def _synth(model):
    return [weights.SYNTH[model](seed=7)], None


def _reload(model):
    rw = np.zeros(12, np.int32)
    rw[0] = rw[5] = 1
    return [weights.SYNTH[model](seed=7), weights.SYNTH[model](seed=8)], rw


def _trained(model):
    return [make_ref_weights.load(model)], None


# name -> (batch of a model, (weight sets, reload_weights) of a model)
INPUTS = {
    "dataset": (_dataset, _synth),
    "directed": (_directed, _synth),
    "duplicates_self_loops": (_duplicates, _synth),
    "tiny_graphs": (_tiny, _synth),
    "graph_at_the_caps": (_capped, _synth),
    "reload_weights": (lambda m: rp.dataset_batch(m, 12, 7), _reload),
    "trained_weights": (lambda m: rp.dataset_batch(m, 24, 4), _trained),
}


# ------------------------------------------------------------------------------------------------ the stand-in itself
def test_standin_self_check_under_sanitizers(tmp_path):
    """oracle/hls_standin/check.cc (fixed form against plain integer formulas), built with UBSan + ASan and run as a child process of
    its own: the check guards the stand-in's own shifts and overflows."""
    exe = str(tmp_path / "check")
    inc = os.path.join(ROOT, "oracle", "hls_standin")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-DHLS_STANDIN_FIXED", "-I" + inc,
                           "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", exe, os.path.join(inc, "check.cc")])  # the runtimes inside the program: nothing to preload
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------- (a), (b): live libraries
@pytest.mark.parametrize("case", list(INPUTS))
@pytest.mark.parametrize("model", rp.MODELS)
def test_float_oracle_equals_the_reference(oracle, model, case):
    need_libraries()
    b = INPUTS[case][0](model)
    sets, rw = INPUTS[case][1](model)
    want = rp.run(model, "f32", b, sets, rw)
    got = oracle_float(oracle, model, b, sets, rw)
    assert same(got, want), (model, case, np.flatnonzero(got != want)[:8], got[got != want][:4], want[got != want][:4])


@pytest.mark.parametrize("case", list(INPUTS))
@pytest.mark.parametrize("model", rp.MODELS)
def test_fixed_oracle_equals_the_reference(oracle, model, case):
    need_libraries()
    b = INPUTS[case][0](model)
    sets, rw = INPUTS[case][1](model)
    want = rp.run(model, "fx", b, sets, rw)
    got = oracle_fixed(oracle, model, b, sets, rw)
    assert same(got, want), (model, case, np.flatnonzero(got != want)[:8], got[got != want][:4], want[got != want][:4])


def test_reference_stays_inside_its_arrays(tmp_path):
    """Which inputs had to be left out: none.  The reference's sources as stand-alone programs under ASan + UBSan (make -C oracle
    ref-replay; child processes, the runtimes linked in) replay the calls of the edge inputs -- tiny graphs, the graph at the caps, the
    directed / duplicate batch with a weight reload -- for every model in both forms, every array an exact-size heap block."""
    if not rp.have_reference_tree():
        print(f"\nSKIP: no reference checkout at {rp.REF}")
        pytest.skip("the replay programs are compiled from the reference checkout")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "-j8", "ref-replay", f"REF={rp.REF}"])
    for model in rp.MODELS:
        calls = {"tiny_graphs": (_tiny(model),) + _synth(model), "graph_at_the_caps": (_capped(model),) + _synth(model),
                 "directed_duplicates_reload": (vn(model, rp.with_duplicates(rp.directed_variant(rp.dataset_batch(model.replace("-VN", ""), 12, 6)), 5)),)
                 + _reload(model)}
        for form in rp.FORMS:
            files = []
            for name, (b, sets, rw) in calls.items():
                files.append(str(tmp_path / f"{model}_{form}_{name}.bin"))
                rp.dump_call(files[-1], model, form, b, sets, rw)
            exe = os.path.join(rp.REF_DIR, f"replay_{model.replace('-VN', '')}_{form}")
            r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and r.stdout.count("replay ok") == len(files), (model, form, r.stdout[-400:], r.stderr[-3000:])


@pytest.mark.parametrize("form", rp.FORMS)
def test_gat_offset_quirk_is_the_batched_reference(oracle, form):
    """Without the quirk the oracle agrees with the batched reference on graph 0 only (the negative control: the comparison can fail)
    and with the reference called one graph per call, where every offset is 0, on all of them."""
    need_libraries()
    b = rp.dataset_batch("GAT", 24, 11)
    w = weights.synth_gat_weights(seed=7)
    orc = oracle_float if form == "f32" else oracle_fixed
    batched, single = rp.run("GAT", form, b, [w]), rp.run_per_graph("GAT", form, b, w)
    with_quirk, without = orc(oracle, "GAT", b, [w], quirk=True), orc(oracle, "GAT", b, [w], quirk=False)
    assert same(with_quirk, batched)
    differs = without[1:] != batched[1:]
    # float: every later graph differs.  fixed: these logits lie within ten steps of the 2^-10 grid of each other (0.15 .. 0.16), so
    # the wrong atoms land on the same pattern for roughly one graph in five; most must still differ
    assert without[0] == batched[0] and (differs.all() if form == "f32" else differs.sum() > differs.size // 2), np.flatnonzero(~differs) + 1
    assert same(without, single)


# ----------------------------------------------------------------------------------------------------- (c): fixtures
def fixture_cases(model, z):
    b = fx.from_npz(z)
    assert tuple(z["weight_seeds"]) == fx.WEIGHT_SEEDS
    cases = fx.weight_cases(model, b.num_graphs)
    assert np.array_equal(cases["reload"][1], z["reload_weights"])
    return b, cases


@pytest.mark.parametrize("model", rp.MODELS)
def test_oracle_equals_the_committed_reference_outputs(oracle, model):
    """Runs everywhere: the reference's outputs are data under tests/golden."""
    z = np.load(fx.path(model))
    b, cases = fixture_cases(model, z)
    for name, (sets, rw) in cases.items():
        assert same(oracle_float(oracle, model, b, sets, rw), z[f"f32_{name}"]), (model, name, "float")
        assert same(oracle_fixed(oracle, model, b, sets, rw), z[f"fx_{name}"]), (model, name, "fixed")
        assert np.isfinite(z[f"f32_{name}"]).all()
    if model == "GAT":
        sets = cases["synth"][0]
        assert same(oracle_float(oracle, model, b, sets, quirk=False), z["f32_synth_per_graph"])
        assert same(oracle_fixed(oracle, model, b, sets, quirk=False), z["fx_synth_per_graph"])
        assert not same(z["f32_synth_per_graph"], z["f32_synth"]) and not same(z["fx_synth_per_graph"], z["fx_synth"])


@pytest.mark.parametrize("model", rp.MODELS)
def test_committed_reference_outputs_equal_the_live_libraries(model):
    need_libraries()
    z = np.load(fx.path(model))
    b = fx.from_npz(z)
    assert same(b.node_feature, fx.fixture_batch(model).node_feature) and same(b.edge_list, fx.fixture_batch(model).edge_list)
    live = fx.reference_outputs(model, b)
    assert sorted(live) == sorted(k for k in z.files if k.startswith(("f32_", "fx_")))
    for k, v in live.items():
        assert same(v, z[k]), (model, k)
