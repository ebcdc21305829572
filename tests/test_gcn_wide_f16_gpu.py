"""GCN and gcn-virtual at width 300 in the f16 numeric mode on the GPU (flowgnn.h: flowgnn_set_model_numeric_mode_dim; kernels:
flowgnn_amd/csrc/gcn_wide_f16.hip).

(a) The probe pins the arithmetic itself: on dyadic weights and graphs of degree 0, 3 and 15 the fp32 sums of the mode are exact
    (tests/test_gcn_wide_f16_cpu.py proves which, per case), so the kernels must reproduce the float64 restatement with f16 casts at
    the two operand points -- rows, pooled sums and maxima bit for bit, what passes through the mean's division or an unproven sum
    within 1e-6 (1 + |x|) -- and must stay apart, by more than 100 x that bound, from every restatement the references themselves tell
    apart (tests/gcn_wide_f16_ref.py).
(b) The four kernel instances on the fixed shape families of tests/wide_cases.py, against the restatement under the project's rule.
(c) At a realistic shape |gpu - f64| <= tol (scale + |f64|) on the logits, tol from the issue's ladder (tests/gcn_wide_f16_ref.TOL).
(d) An operand beyond the f16 range: one exact re-run, the f32 mode's bytes.
(e) The refusals of the call, which launch nothing; the mode across the other setters; the group form; the host CLI.
Every test here fails on a library without flowgnn_set_model_numeric_mode_dim."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, graphpack as gp, weights
from tests import gcn_wide_f16_ref as R, gcn_wide_ref as W, wide_cases
from tests.parity import assert_close, err_ratio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 8
F32, Q, F16 = 0, 1, 2
F16_SLOT, SPLIT_SLOT, EXACT_SLOT = "gcn_wide_layer_f16", "gcn_wide_layer", "gcn_wide_layer_f32"
REL = 1e-4  # the project's rule (tests/parity.py)
f64 = lambda a: np.asarray(a, dtype=np.float64)


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def _rc(fn):
    try:
        fn()
    except FlowGNNError as ex:
        return ex.code, str(ex)
    return OK, ""


def counts(e, fn):
    """slot -> launches gained while fn() runs (and is synchronised)"""
    before = {k: v["launches"] for k, v in e.profile_read().items()}
    fn()
    e.sync()
    after = e.profile_read()
    return {k: v["launches"] - before.get(k, 0) for k, v in after.items() if v["launches"] > before.get(k, 0)}


def make(w, mode="f16", vn=None, jk="last", res=False, tasks=1, pooling="mean"):
    e = Engine("GCN", device=0)
    e.set_model_emb_dim(300)
    if tasks != 1:
        e.set_num_tasks(tasks)
    e.set_weights(w)
    if mode is not None:
        e.set_numeric_mode(mode, emb_dim=300)
    if pooling != "mean":
        e.set_pooling(pooling)
    if vn is not None:
        e.set_gcn_virtual_node(vn)
    e.set_jk_residual(jk, res)
    e.profile_enable(True)
    return e


# ---------------------------------------------------------------- (a) the probe
def _outputs(c, res):
    """the forward's tuple -> {output name: float64 array}"""
    res = res if isinstance(res, tuple) else (res,)
    names = R.outputs_of(c)
    assert len(res) == len(names), (len(res), names)
    return {n: f64(r.cpu().numpy() if hasattr(r, "cpu") else r) for n, r in zip(names, res)}


def _member_counts(lib, h):
    n = C.c_int()
    names, ms, cnt = (C.c_char_p * 32)(), (C.c_double * 32)(), (C.c_longlong * 32)()
    assert lib.flowgnn_profile_read(h, C.byref(n), names, ms, cnt) == OK
    return {names[i].decode(): int(cnt[i]) for i in range(n.value) if cnt[i] > 0}


def _run_group(c, w, b, mode):
    """a two-member group on device 0 -> (outputs, launches per slot of each member, exact re-runs)"""
    g = EngineGroup("GCN", [0, 0])
    try:
        g.set_model_emb_dim(300)
        g.set_weights(w)
        if mode == "switched":
            g.set_numeric_mode("f16", emb_dim=300)
            g.set_numeric_mode("f32", emb_dim=300)
        elif mode is not None:
            g.set_numeric_mode(mode, emb_dim=300)
        g.set_node_embeddings(True)
        members = [g.lib.flowgnn_group_engine(g._h, i) for i in range(2)]
        for h in members:
            assert g.lib.flowgnn_profile_enable(C.c_void_p(h), 1) == OK
        logits = g.forward(b).copy()
        rows = g.node_embeddings()
        per_member = [_member_counts(g.lib, C.c_void_p(h)) for h in members]
        reruns = sum(g.lib.flowgnn_exact_reruns(C.c_void_p(h)) for h in members)
    finally:
        g.close()
    return _outputs(c, (logits, rows)), per_member, reruns


def _run(c, w, b, mode, vn=None):
    """one engine of its own -> (outputs, [launches per slot of the one run], exact re-runs).  mode: "f16", None (never switched) or
    "switched" (f16, then back to f32 through the call)"""
    if c.group:
        return _run_group(c, w, b, mode)
    e = make(w, "f16" if mode == "switched" else mode, vn, c.jk, c.res, c.tasks, c.pooling)
    try:
        if mode == "switched":
            e.set_numeric_mode("f32", emb_dim=300)
        fwd = {k: True for k in c.fwd}
        res = {}
        if c.device:
            pytest.importorskip("torch")
            from tests.test_device_batch_gpu import device_args
            args, kw = device_args(b, "pyg", "GCN")
            n = counts(e, lambda: res.update(got=e.forward_device(*args, **fwd, **kw)))
        else:
            n = counts(e, lambda: res.update(got=e.forward(b, **fwd)))
        return _outputs(c, res["got"]), [n], e.exact_reruns()
    finally:
        e.close()


@pytest.mark.parametrize("c", R.CASES, ids=R.IDS)
def test_probe(c):
    b, w = R.probe_batch(), R.weights_of(c.tasks)
    vn = R.virtual_node_of() if c.vn else None
    refs = R.references(c)
    rows_exact, pool_exact = R.rows_exact(c), R.pool_exact(c)
    assert rows_exact == (c.name not in R.ROWS_NOT_EXACT) and pool_exact == (c.name not in R.POOL_NOT_EXACT)
    want = refs["rne"][0]
    got, launches, reruns = _run(c, w, b, "f16", vn)
    assert reruns == 0
    for n in launches:  # four launches of the f16 slot per run and stage 4 under the default mode's slot
        assert n.get(F16_SLOT) == 4 and n.get(SPLIT_SLOT) == 1 and EXACT_SLOT not in n, n
    for o, g in got.items():
        x = getattr(want, o)
        g = g.reshape(x.shape)
        exact = (o == "rows" and rows_exact) or (o == "pooled" and c.pooling in ("sum", "max") and pool_exact)
        worst = float((np.abs(g - x) / R.bound(x)).max())
        print(f"{c.name}: {o}: max |gpu - rne| / bound = {worst:.3g}" + (" (asserted bit for bit)" if exact else ""))
        if exact:
            assert np.array_equal(g, x), (o, worst)
        else:
            assert worst <= 1.0, (o, worst)
    # every pair the references separate, apart on the GPU too
    table = R.separation(c)
    for (o, v), (sep, _, _) in table.items():
        assert sep or (c.name, o, v) in R.NOT_SEPARATED or o not in R.TABLE_OUTPUTS, (o, v)
        if sep:
            x = getattr(want, o)
            ok, frac, med = R.separated(got[o].reshape(x.shape), getattr(refs[v][0], o), x)
            assert ok, (o, v, frac, med)
    # back in F32 through the call: what an engine that never left it returns, byte for byte
    back, n_back, _ = _run(c, w, b, "switched", vn)
    never, n_never, _ = _run(c, w, b, None, vn)
    for n in n_back:
        assert n.get(SPLIT_SLOT) == 5 and F16_SLOT not in n, n
    assert n_back == n_never, (n_back, n_never)
    for o in got:
        assert np.array_equal(back[o], never[o]), o
        if o == "logits":  # (and the mode was engaged: the f32 mode's logits are other numbers)
            assert not np.array_equal(back[o], got[o])


# ---------------------------------------------------------------- (b) the four instances on the fixed shape families
INSTANCES = [wide_cases.Instance("gcn", vn, jk, res, False) for vn in (False, True) for jk, res in (("last", False), ("sum", True))]


@pytest.mark.parametrize("i", INSTANCES, ids=[wide_cases.name_of(i) + "-f16" for i in INSTANCES])
def test_fixed_shape_families(i):
    """plain, VN, EXT and VN + EXT: the 16- and 128-row tile edges, hubs, isolated nodes and (virtual node) the graph counts around 16,
    against the mode's restatement on the exported files of the instance's damped model.  The project's rule is asserted on the logits
    and the rows r and h_5 are printed, as tests/test_wide_shapes_gpu.py does for GIN's f16 rows: the kernel forms a in fp32 and the
    restatement in float64, and where the two fall on either side of an f16 rounding boundary the operands differ by a whole f16
    spacing, 2^-11 |a| -- on an isolated node, whose row nothing averages, that alone is several times 1e-4 of the scale (3.7 on the
    isolated-node family); the probe holds the same rows to bits, on inputs where fp32 and float64 agree."""
    w, vnt, _ = wide_cases.tensors("gcn", i.vn, i.jk, i.res)
    e = wide_cases.engine(i)
    try:
        e.set_numeric_mode("f16", emb_dim=300)
        for name in wide_cases.fixed_cases(i):
            b = wide_cases.fixed_batch(wide_cases.family_of(i), name)
            ref = R.forward(b, w, vnt, jk=i.jk, residual=i.res)
            res = {}
            n = counts(e, lambda: res.update(got=e.forward(b, return_node_embeddings=True)))
            assert n.get(F16_SLOT) == 4 and n.get(SPLIT_SLOT) == 1 and EXACT_SLOT not in n, (name, n)
            logits, rows = res["got"]
            h5 = e.final_h() if hasattr(e, "final_h") else None
            for what, g, x in (("logits", logits, ref.logits), ("rows", rows, ref.rows), ("h5", h5, ref.h5)):
                if g is None:
                    continue
                print(wide_cases.name_of(i), name, what, f"{err_ratio(f64(g).reshape(x.shape), x, ref.scale, REL):.4f} of the rule (scale {ref.scale:.4g})")
                if what == "logits":
                    assert_close(f64(g).reshape(x.shape), x, scale=ref.scale, rel=REL, what=(name, what))
        assert e.exact_reruns() == 0
    finally:
        e.close()


# ---------------------------------------------------------------- (c) accuracy at a realistic shape
@pytest.mark.parametrize("which", R.ACCURACY)
def test_accuracy_at_a_realistic_shape(which):
    b, w, vn = R.accuracy_inputs(which)
    ref, rne = R.accuracy_references(which)
    tol = R.TOL[which]
    assert R.rule(rne.logits, ref, tol) <= 0.5  # (tests/test_gcn_wide_f16_cpu.py: the ladder's rung)
    out = {}
    for mode in ("f16", None):
        e = make(w, mode=mode, vn=vn)
        try:
            res = {}
            n = counts(e, lambda: res.update(got=e.forward(b, return_node_embeddings=True)))
            assert (n.get(F16_SLOT), n.get(SPLIT_SLOT)) == ((4, 1) if mode else (None, 5)), n
            assert e.exact_reruns() == 0
            out[mode] = [f64(x) for x in res["got"]]
        finally:
            e.close()
    r16, r32, rr = R.rule(out["f16"][0], ref, tol), R.rule(out[None][0], ref, tol), R.rule(rne.logits, ref, tol)
    print(f"{which}: logits: f16 mode at {r16:.3f} of tol {tol:g} (restatement {rr:.3f}, f32 mode {r32:.4f}; scale {ref.scale:.1f})")
    # The rows are printed, not asserted: the probe pins their arithmetic bit for bit, and on weights of a trained size an fp32 rounding
    # now and then turns an f16 rounding the other way, which four products carry on
    x = ref.rows
    for name, g in (("f16 mode", out["f16"][1]), ("restatement", rne.rows)):
        print(f"{which}: rows: {name} at {float((np.abs(g.reshape(x.shape) - x) / (tol * (ref.scale + np.abs(x)))).max()):.3f} of tol")
    assert r16 <= 1.0, (which, r16)
    assert np.mean(out["f16"][0] != out[None][0]) > 0.5  # the mode is engaged


# ---------------------------------------------------------------- (d) range
def test_range_flag_reruns_on_the_exact_path():
    """tests/test_gcn_wide_gpu.py's out-of-range input: BatchNorm 0 scaled until some a_1 = relu(pre_0) passes 6e4.  In f16 mode the
    kernel raises the flag, the engine repeats the pass on the fp32 exact path, and that is what the f32 mode does on this input."""
    small, w300 = gp.synth_molpcba_batch(24, seed=13), weights.synth_gcn_weights(seed=7, emb_dim=300)
    factor = np.float32(8.0e4 / W.max_a_per_layer(small, w300)[0])
    above = dict(w300)
    for k in ("bn_weight", "bn_bias"):
        a = np.asarray(w300[k], np.float32).copy()
        a[0] *= factor
        above[k] = a
    assert W.max_a(small, w300) < 6.0e4 and W.max_a(small, above) > 6.6e4
    out = {}
    for mode in ("f16", None):
        e = make(above, mode=mode)
        try:
            res = {}
            n = counts(e, lambda: res.update(got=e.forward(small, return_node_embeddings=True)))
            assert e.exact_reruns() == 1 and n.get(EXACT_SLOT) == 5, (mode, e.exact_reruns(), n)
            assert (n.get(F16_SLOT), n.get(SPLIT_SLOT)) == ((4, 1) if mode else (None, 5)), n
            out[mode] = [np.asarray(x).copy() for x in res["got"]]
        finally:
            e.close()
    for a, f in zip(out["f16"], out[None]):
        assert a.tobytes() == f.tobytes()


# ---------------------------------------------------------------- (e) refusals: nothing is launched
def _model(e, d, mode):
    rc = e.lib.flowgnn_set_model_numeric_mode_dim(e._h, d, mode)
    return rc, (e.lib.flowgnn_last_error(e._h) or b"").decode()


def _dim(e, d, mode):
    rc = e.lib.flowgnn_set_numeric_mode_dim(e._h, d, mode)
    return rc, (e.lib.flowgnn_last_error(e._h) or b"").decode()


def test_refusals_on_a_gcn_engine_in_both_orders():
    e = Engine("GCN")
    try:
        # ---- at width 100 the call is flowgnn_set_numeric_mode
        for bad in (0, 200, -300, 301):
            rc, text = _model(e, bad, F16)
            assert rc == ERR_ARG and "100" in text and "300" in text, (bad, rc, text)
        for bad in (-1, 3, 16):
            assert _model(e, 100, bad)[0] == ERR_ARG
        rc, text = _model(e, 300, F16)  # not the engine's width: both numbers
        assert rc == ERR_ARG and "300" in text and "100" in text, (rc, text)
        for mode in (F32, Q, F16):
            want = e.lib.flowgnn_set_numeric_mode(e._h, mode)
            e.lib.flowgnn_set_numeric_mode(e._h, F32)
            assert _model(e, 100, mode)[0] == want, mode
            assert _model(e, 100, F32)[0] == OK
        assert _model(e, 100, F16)[0] == ERR_UNSUPPORTED  # GCN's F16 at width 100 stays refused
        # ---- at width 300
        e.set_model_emb_dim(300)
        rc, text = _model(e, 100, F16)
        assert rc == ERR_ARG and "100" in text and "300" in text, (rc, text)
        rc, text = _model(e, 300, Q)
        assert rc == ERR_UNSUPPORTED and "300" in text, (rc, text)
        for mode in ("f16", "q6.10"):  # the call without the width keeps its answer, and names the new one
            rc, text = _rc(lambda: e.set_numeric_mode(mode))
            assert rc == ERR_UNSUPPORTED and "300" in text and "flowgnn_set_model_numeric_mode_dim" in text, (rc, text)
        rc, text = _dim(e, 300, F16)  # ... and so does the call that carries the width but names GIN's kernels
        assert rc == ERR_UNSUPPORTED and "300" in text and "flowgnn_set_model_numeric_mode_dim" in text, (rc, text)
        e.set_model_emb_dim(100)  # nothing above left a mode behind
        e.set_model_emb_dim(300)
        assert _model(e, 300, F32)[0] == OK and _model(e, 300, F16)[0] == OK
        rc, text = _rc(lambda: e.set_numeric_mode("f16"))  # ... in f16 mode too
        assert rc == ERR_UNSUPPORTED and "300" in text, (rc, text)
        rc, text = _rc(lambda: e.set_model_emb_dim(100))  # the mirror of section 4.22's pinned direction
        assert rc == ERR_UNSUPPORTED and "numeric" in text and e.emb_dim == 300, (rc, text)
        e.set_model_emb_dim(300)  # the same width again: a no-op
        rc, text = _model(e, 300, Q)  # a refusal leaves the mode as it was
        assert rc == ERR_UNSUPPORTED
        assert _rc(lambda: e.set_model_emb_dim(100))[0] == ERR_UNSUPPORTED
        ms, d0, d1 = C.c_float(), C.c_int(), C.c_int()  # the aggregation probes stay refused at this width
        assert e.lib.flowgnn_run_aggregation_only(e._h, 0, 1, C.byref(ms)) == ERR_UNSUPPORTED
        assert e.lib.flowgnn_get_aggregate(e._h, 0, None, C.byref(d0), None, C.byref(d1)) == ERR_UNSUPPORTED
        e.set_numeric_mode("f32")  # the call without the width may always go back to F32
        e.set_model_emb_dim(100)
        assert e.emb_dim == 100
    finally:
        e.close()


def test_on_a_gin_engine_the_call_is_the_one_it_had():
    e = Engine("GIN")
    try:
        for d, mode in ((100, F16), (100, Q), (300, F16), (200, F16), (100, 7), (100, F32)):
            want = _dim(e, d, mode)
            e.lib.flowgnn_set_numeric_mode(e._h, F32)
            got = _model(e, d, mode)
            e.lib.flowgnn_set_numeric_mode(e._h, F32)
            assert got[0] == want[0] and got[1] == want[1], (d, mode, got, want)
        e.set_emb_dim(300)
        for d, mode in ((300, F16), (300, Q), (100, F16), (300, F32)):
            want = _dim(e, d, mode)
            assert _dim(e, 300, F32)[0] == OK
            got = _model(e, d, mode)
            assert _dim(e, 300, F32)[0] == OK
            assert got[0] == want[0] and got[1] == want[1], (d, mode, got, want)
    finally:
        e.close()


@pytest.mark.parametrize("model", ["GIN-VN", "GAT", "PNA", "DGN"])
def test_other_models(model):
    e = Engine(model)
    try:
        rc, text = _model(e, 300, F16)  # a width the engine does not have
        assert rc == ERR_ARG and "300" in text and "100" in text, (rc, text)
        want = e.lib.flowgnn_set_numeric_mode(e._h, F16)  # at 100 the call is exactly the one without the width
        e.lib.flowgnn_set_numeric_mode(e._h, F32)
        assert _model(e, 100, F16)[0] == want
        assert _model(e, 100, F32)[0] == OK
    finally:
        e.close()


def test_the_mode_survives_the_other_setters_in_either_order():
    from tests import gcn_wide_vn_ref as V
    b, b2 = gp.synth_molpcba_batch(12, seed=5), gp.synth_molpcba_batch(7, seed=6)
    w, w2 = weights.synth_gcn_weights(seed=7, emb_dim=300), weights.synth_gcn_weights(seed=7, num_tasks=2, emb_dim=300)
    vn = V.shapes_virtual_node()
    gate, s2s = weights.synth_attention_pooling(seed=11, emb_dim=300), weights.synth_set2set(seed=17, emb_dim=300)
    e = Engine("GCN")
    try:
        e.set_model_emb_dim(300)
        e.set_numeric_mode("f16", emb_dim=300)  # before the weights
        e.set_weights(w)
        e.profile_enable(True)
        steps = [lambda: e.set_weights(w), lambda: e.set_pooling("sum"), lambda: e.set_gcn_virtual_node(vn), lambda: e.set_jk_residual("sum", True),
                 lambda: e.set_gcn_virtual_node(None), lambda: e.set_jk_residual("last", False), lambda: e.set_pooling("mean"),
                 lambda: e.set_attention_pooling(gate), lambda: e.set_attention_pooling(None),
                 lambda: e.set_set2set_pooling(s2s), lambda: e.set_set2set_pooling(None),
                 lambda: (e.set_num_tasks(2), e.set_weights(w2)), lambda: (e.set_num_tasks(1), e.set_weights(w))]
        for k, step in enumerate(steps):
            step()
            n = counts(e, lambda: e.forward(b2 if k % 2 else b))
            assert n.get(F16_SLOT) == 4 and n.get(SPLIT_SLOT) == 1, (k, n)
        first = e.forward(b).copy()
        # the other order: everything set in f32 mode, the mode last
        o = Engine("GCN")
        try:
            o.set_model_emb_dim(300)
            o.set_weights(w)
            o.set_jk_residual("last", False)
            o.set_numeric_mode("f16", emb_dim=300)
            assert np.array_equal(o.forward(b), first)
        finally:
            o.close()
        assert e.exact_reruns() == 0
    finally:
        e.close()


def test_group_form():
    g = EngineGroup("GCN", [0, 0])
    try:
        rc, _ = _rc(lambda: g.set_numeric_mode("f16", emb_dim=300))  # the members are 100 wide
        assert rc == ERR_ARG
        g.set_model_emb_dim(300)
        rc, _ = _rc(lambda: g.set_numeric_mode("f16"))  # the call without the width
        assert rc == ERR_UNSUPPORTED
        assert g.lib.flowgnn_group_set_numeric_mode_dim(g._h, 300, F16) == ERR_UNSUPPORTED  # ... and the one that names GIN's kernels
        g.set_numeric_mode("f16", emb_dim=300)
        rc, text = _rc(lambda: g.set_model_emb_dim(100))
        assert rc == ERR_UNSUPPORTED and g.emb_dim == 300, (rc, text)
        assert g.lib.flowgnn_group_set_model_numeric_mode_dim(g._h, 200, F16) == ERR_ARG
        assert g.lib.flowgnn_group_set_model_numeric_mode_dim(g._h, 300, Q) == ERR_UNSUPPORTED
        g.set_numeric_mode("f32", emb_dim=300)
        g.set_model_emb_dim(100)
    finally:
        g.close()


def test_host_cli_runs_gcn_virtual_with_jk_sum_and_the_residual_in_f16_mode(tmp_path):
    """`host GCN --emb-dim 300 --numeric f16 --ogb-vn --jk sum --residual` on a written pack and the exported files of the damped
    gcn-virtual model trained with both flags: the mode's restatement under the project's rule, and not the f32 mode's numbers"""
    i = wide_cases.Instance("gcn", True, "sum", True, False)
    wdir = wide_cases.weights_dir("gcn", True, "sum", True)
    w, vnt, _ = wide_cases.tensors("gcn", True, "sum", True)
    b = gp.synth_molpcba_batch(40, seed=3)
    gdir = tmp_path / "graphs"
    gp.write_pack(b, str(gdir))
    got = {}
    for mode in ("f16", "f32"):
        out = tmp_path / f"out_{mode}.txt"
        cmd = [HOST, "GCN", "--emb-dim", "300", "--numeric", mode, "--ogb-vn", "--jk", "sum", "--residual", "--graphs", str(gdir),
               "--weights", wdir, "--trials", "1", "--out", str(out)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        got[mode] = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    ref = R.forward(b, w, vnt, jk="sum", residual=True)
    assert wide_cases.reference(i, b).operands < wide_cases.RANGE_LIMIT  # (on the fast kernels, not on the re-run)
    print(f"host, f16 mode against its restatement: {err_ratio(got['f16'], ref.logits, ref.scale, REL):.4f} of the rule")
    assert_close(got["f16"], ref.logits, scale=ref.scale, rel=REL, what="host GCN --emb-dim 300 --numeric f16 --ogb-vn --jk sum --residual")
    assert np.mean(got["f16"] != got["f32"]) > 0.5
    p = subprocess.run([HOST, "GCN", "--emb-dim", "300", "--numeric", "q6.10", "--graphs", str(gdir), "--weights", wdir, "--trials", "1"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "300" in p.stderr and "flowgnn_set_model_numeric_mode_dim" in p.stderr, p.stdout + p.stderr
