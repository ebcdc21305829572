"""GIN at width 300 in the f16 numeric mode on the GPU (flowgnn.h: flowgnn_set_numeric_mode_dim; kernels:
flowgnn_amd/csrc/gin_wide_f16.hip).

(a) The probe pins the arithmetic itself: on dyadic weights every fp32 sum of the mode is exact (tests/test_gin_wide_f16_cpu.py proves
    it per input), so the kernels must reproduce the float64 restatement with f16 casts at the operand points -- h_5 rows, pooled sums
    and maxima bit for bit, what passes through a last fp32 addition or the mean's division within 1e-6 (1 + |x|) -- and must stay
    apart, by more than 100 x that bound, from every restatement the references themselves tell apart (tests/gin_wide_f16_ref.py).
(b) At a realistic shape the project's f16 rule, |gpu - f64| <= 2e-4 (scale + |f64|).
(c) An operand beyond the f16 range: one exact re-run, the f32 mode's bytes.
(d) The refusals of the call, which launch nothing.
Every test here fails on a library without flowgnn_set_numeric_mode_dim."""
import ctypes as C

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, FlowGNNError, export, graphpack as gp, weights
from tests import gin_wide_f16_ref as R, gin_wide_ref as W
from tests.test_embeddings_gpu import launched

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 8
F16_SLOT, SPLIT_SLOT, EXACT_SLOT = "gin_wide_layer_f16", "gin_wide_layer", "gin_wide_layer_f32"
F16_REL = 2e-4  # the project's f16 rule (tests/test_f16_mode_gpu.py::test_accuracy_at_dataset_size)
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


def make(w, c=None, mode="f16", vn=None):
    e = Engine("GIN", device=0)
    e.set_emb_dim(300)
    if c is not None and c.tasks != 1:
        e.set_num_tasks(c.tasks)
    e.set_weights(w)
    if mode is not None:
        e.set_numeric_mode(mode, emb_dim=300)
    if c is not None and c.pooling != "mean":
        e.set_pooling(c.pooling)
    if c is not None and c.eps:
        e.set_gin_eps(np.asarray(R.EPS, np.float32))
    if vn is not None:
        e.set_ogb_virtual_node(vn)
    e.profile_enable(True)
    return e


# ---------------------------------------------------------------- (a) the probe
def _outputs(c, res):
    """the forward's tuple -> {output name: float64 array}"""
    res = res if isinstance(res, tuple) else (res,)
    names = R.outputs_of(c)
    assert len(res) == len(names), (len(res), names)
    return {n: f64(r.cpu().numpy() if hasattr(r, "cpu") else r) for n, r in zip(names, res)}


def _member_profile(lib, h):
    n = C.c_int()
    names, ms, cnt = (C.c_char_p * 32)(), (C.c_double * 32)(), (C.c_longlong * 32)()
    assert lib.flowgnn_profile_read(h, C.byref(n), names, ms, cnt) == OK
    return {names[i].decode() for i in range(n.value) if cnt[i] > 0}


def _run_group(c, w, b, mode):
    """a two-member group on device 0 -> (outputs, slots that ran on any member, exact re-runs)"""
    g = EngineGroup("GIN", [0, 0])
    try:
        g.set_emb_dim(300)
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
        names = set().union(*[_member_profile(g.lib, C.c_void_p(h)) for h in members])
        reruns = sum(g.lib.flowgnn_exact_reruns(C.c_void_p(h)) for h in members)
    finally:
        g.close()
    return _outputs(c, (logits, rows)), names, reruns


def _run(c, w, b, mode, vn=None):
    """one engine of its own -> (outputs, slots that ran, exact re-runs).  mode: "f16", None (never switched) or "switched" (f16, then
    back to f32 through the call)"""
    if c.group:
        return _run_group(c, w, b, mode)
    e = make(w, c, "f16" if mode == "switched" else mode, vn)
    try:
        if mode == "switched":
            e.set_numeric_mode("f32", emb_dim=300)
        fwd = {k: True for k in c.fwd}
        res = {}
        if c.device:
            pytest.importorskip("torch")
            from tests.test_device_batch_gpu import device_args
            args, kw = device_args(b, "pyg", "GIN")
            names = launched(e, lambda: res.update(got=e.forward_device(*args, **fwd, **kw)))
        else:
            names = launched(e, lambda: res.update(got=e.forward(b, **fwd)))
        out = _outputs(c, res["got"])
        return out, names, e.exact_reruns()
    finally:
        e.close()


@pytest.mark.parametrize("c", R.CASES, ids=R.IDS)
def test_probe(c):
    b, w = R.probe_batch(), R.weights_of(c.tasks)
    vn = R.virtual_node_of() if c.vn else None
    refs = R.references(c)
    for v in R.CHECKED:
        assert refs[v][1] <= 24.0, f"fp32 would round on this input (2^{refs[v][1]:.1f} > 2^24): the probe proves nothing"
    want = refs["rne"][0]
    got, names, reruns = _run(c, w, b, "f16", vn)
    assert reruns == 0
    assert F16_SLOT in names and SPLIT_SLOT not in names and EXACT_SLOT not in names, names
    for o, g in got.items():
        x = getattr(want, o)
        g = g.reshape(x.shape)
        exact = o == "rows" or (o == "pooled" and c.pooling in ("sum", "max"))
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
    back, names_back, _ = _run(c, w, b, "switched", vn)
    never, names_never, _ = _run(c, w, b, None, vn)
    assert SPLIT_SLOT in names_back and F16_SLOT not in names_back and names_back == names_never, (names_back, names_never)
    for o in got:
        assert np.array_equal(back[o], never[o]), o
        if o == "logits":  # (and the mode was engaged: the f32 mode's logits are other numbers)
            assert not np.array_equal(back[o], got[o])


# ---------------------------------------------------------------- (b) accuracy at a realistic shape
def _exported():
    sd = W.state_dict(seed=3)
    return export.gin_weights_from_ogb_state_dict(sd, keep_eps=True), np.asarray(export.gin_eps_from_ogb_state_dict(sd), np.float32)


@pytest.mark.parametrize("which", ["synthetic weights", "exported state_dict with eps"])
def test_accuracy_at_a_realistic_shape(which):
    b = W.sep_batch(5)
    if which == "synthetic weights":
        w, eps = W.sep_weights(), None
    else:
        w, eps = _exported()
    ref = W.forward(b, w, eps=eps)
    rne = R.forward(b, w, eps=None if eps is None else list(eps))
    # the references first: the mode's own restatement within half of the rule, or the rule could not be met by a right kernel.
    # The rule is the logits', as at width 100 (tests/test_f16_mode_gpu.py); the rows' figures are printed beside them -- a single
    # row carries the roundings that a graph's mean averages out (the restatement alone: 0.76 and 1.28 of the rule on these inputs).
    for name in ("logits", "rows"):
        x = getattr(ref, name)
        r = float((np.abs(getattr(rne, name) - x) / (F16_REL * (ref.scale + np.abs(x)))).max())
        print(f"{which}: {name}: rne restatement at {r:.3f} of the rule (scale {ref.scale:.1f})")
        assert name != "logits" or r <= 0.5, (name, r)
    out = {}
    for mode in ("f16", None):
        e = make(w, mode=mode)
        try:
            if eps is not None:
                e.set_gin_eps(eps)
            res = {}
            names = launched(e, lambda: res.update(got=e.forward(b, return_node_embeddings=True)))
            assert ((F16_SLOT if mode else SPLIT_SLOT) in names) and ((SPLIT_SLOT if mode else F16_SLOT) not in names), names
            assert e.exact_reruns() == 0
            out[mode] = [f64(x) for x in res["got"]]
        finally:
            e.close()
    for name, g, f in zip(("logits", "rows"), out["f16"], out[None]):
        x = getattr(ref, name)
        r16 = float((np.abs(g.reshape(x.shape) - x) / (F16_REL * (ref.scale + np.abs(x)))).max())
        print(f"{which}: {name}: max |f16 mode - f64| = {np.abs(g.reshape(x.shape) - x).max():.3e} ({r16:.3f} of the rule), "
              f"max |f32 mode - f64| = {np.abs(f.reshape(x.shape) - x).max():.3e}")
        r = getattr(rne, name)
        rr = float((np.abs(g.reshape(r.shape) - r) / (F16_REL * (ref.scale + np.abs(r)))).max())
        print(f"{which}: {name}: max |f16 mode - rne restatement| at {rr:.3f} of the rule")
        # The rule is asserted on the logits.  The rows are printed: the probe pins their arithmetic bit for bit, and on weights of a
        # trained size an fp32 rounding now and then turns an f16 rounding the other way, which five layers carry on -- the kernel's
        # rows are as far from the restatement's as both are from float64.
        if name == "logits":
            assert r16 <= 1.0, (name, r16)
    assert np.mean(out["f16"][0] != out[None][0]) > 0.5  # the mode is engaged


# ---------------------------------------------------------------- (c) range
def test_range_flag_reruns_on_the_exact_path():
    """tests/test_gin_wide_gpu.py's out-of-range input: the last layer's b1 scaled until a hidden value passes 7.5e4.  In f16 mode the
    kernel raises the flag, the engine repeats the pass on the fp32 exact path, and that is what the f32 mode does on this input."""
    b = gp.synth_molhiv_batch(64, seed=13)
    w = dict(weights.synth_gin_weights(seed=7, emb_dim=300))
    b1 = np.asarray(w["node_mlp_1_bias"], np.float32).copy()
    b1[4] *= np.float32(7.5e4 / float(b1[4].max()))
    w["node_mlp_1_bias"] = b1
    out = {}
    for mode in ("f16", None):
        e = make(w, mode=mode)
        try:
            res = {}
            names = launched(e, lambda: res.update(got=e.forward(b, return_node_embeddings=True)))
            assert e.exact_reruns() == 1 and EXACT_SLOT in names, (mode, e.exact_reruns(), names)
            assert ((F16_SLOT if mode else SPLIT_SLOT) in names) and ((SPLIT_SLOT if mode else F16_SLOT) not in names), names
            out[mode] = [np.asarray(x).copy() for x in res["got"]]
        finally:
            e.close()
    for a, f in zip(out["f16"], out[None]):
        assert a.tobytes() == f.tobytes()


# ---------------------------------------------------------------- (d) refusals: nothing is launched
def _dim(e, d, mode):
    rc = e.lib.flowgnn_set_numeric_mode_dim(e._h, d, mode)
    return rc, (e.lib.flowgnn_last_error(e._h) or b"").decode()


F32, Q, F16 = 0, 1, 2


def test_refusals_on_a_gin_engine_in_both_orders():
    e = Engine("GIN")
    try:
        # ---- at width 100 the call is flowgnn_set_numeric_mode
        for bad in (0, 200, -300, 301):
            rc, text = _dim(e, bad, F16)
            assert rc == ERR_ARG and "100" in text and "300" in text, (bad, rc, text)
        for bad in (-1, 3, 16):
            assert _dim(e, 100, bad)[0] == ERR_ARG
        rc, text = _dim(e, 300, F16)  # not the engine's width: both numbers
        assert rc == ERR_ARG and "300" in text and "100" in text, (rc, text)
        for mode in (F16, Q, F32):
            assert _dim(e, 100, mode)[0] == OK
        assert _dim(e, 100, F16)[0] == OK
        rc, text = _rc(lambda: e.set_emb_dim(300))  # the pinned direction
        assert rc == ERR_UNSUPPORTED and "numeric" in text and "300" in text and "flowgnn_set_numeric_mode_dim" in text and e.emb_dim == 100, (rc, text)
        assert _dim(e, 100, F32)[0] == OK
        # ---- at width 300
        e.set_emb_dim(300)
        rc, text = _dim(e, 100, F16)
        assert rc == ERR_ARG and "100" in text and "300" in text, (rc, text)
        rc, text = _dim(e, 300, Q)
        assert rc == ERR_UNSUPPORTED and "300" in text, (rc, text)
        rc, text = _rc(lambda: e.set_numeric_mode("f16"))  # the call without the width keeps its answer, and names the new one
        assert rc == ERR_UNSUPPORTED and "300" in text and "flowgnn_set_numeric_mode_dim" in text, (rc, text)
        e.set_emb_dim(100)  # nothing above left a mode behind
        e.set_emb_dim(300)
        assert _dim(e, 300, F16)[0] == OK
        rc, text = _rc(lambda: e.set_numeric_mode("f16"))  # ... in f16 mode too
        assert rc == ERR_UNSUPPORTED and "300" in text, (rc, text)
        for call in (e.set_emb_dim, e.set_model_emb_dim):  # the mirror of the pinned direction
            rc, text = _rc(lambda: call(100))
            assert rc == ERR_UNSUPPORTED and "numeric" in text and e.emb_dim == 300, (rc, text)
            call(300)  # the same width again: a no-op
        rc, text = _dim(e, 300, Q)  # a refusal leaves the mode as it was
        assert rc == ERR_UNSUPPORTED
        rc, _ = _rc(lambda: e.set_emb_dim(100))
        assert rc == ERR_UNSUPPORTED
        ms, d0, d1 = C.c_float(), C.c_int(), C.c_int()  # the aggregation probes stay refused at this width
        assert e.lib.flowgnn_run_aggregation_only(e._h, 0, 1, C.byref(ms)) == ERR_UNSUPPORTED
        assert e.lib.flowgnn_get_aggregate(e._h, 0, None, C.byref(d0), None, C.byref(d1)) == ERR_UNSUPPORTED
        e.set_numeric_mode("f32")  # the call without the width may always go back to F32
        e.set_emb_dim(100)
        assert e.emb_dim == 100
    finally:
        e.close()


def test_the_mode_survives_the_other_setters_in_either_order():
    b = gp.synth_molhiv_batch(12, seed=5)
    w, w2 = weights.synth_gin_weights(seed=7, emb_dim=300), weights.synth_gin_weights(seed=7, num_tasks=2, emb_dim=300)
    from tests import gin_wide_vn_ref as V
    vn = V.shapes_virtual_node()
    rng = np.random.default_rng(3)
    gate = {"w1": (0.05 * rng.standard_normal((600, 300))).astype(np.float32), "b1": (0.1 * rng.standard_normal(600)).astype(np.float32),
            "w2": (0.05 * rng.standard_normal(600)).astype(np.float32)}
    e = Engine("GIN")
    try:
        e.set_emb_dim(300)
        e.set_numeric_mode("f16", emb_dim=300)  # before the weights
        e.set_weights(w)
        e.profile_enable(True)
        steps = [lambda: e.set_weights(w), lambda: e.set_gin_eps(np.asarray(R.EPS, np.float32)), lambda: e.set_pooling("sum"),
                 lambda: e.set_ogb_virtual_node(vn), lambda: e.set_ogb_virtual_node(None), lambda: e.set_pooling("mean"), lambda: e.set_gin_eps(None),
                 lambda: e.set_attention_pooling(gate), lambda: e.set_attention_pooling(None),
                 lambda: (e.set_num_tasks(2), e.set_weights(w2)), lambda: (e.set_num_tasks(1), e.set_weights(w))]
        for step in steps:
            step()
            names = launched(e, lambda: e.forward(b))
            assert F16_SLOT in names and SPLIT_SLOT not in names, names
        first = e.forward(b).copy()
        # the other order: everything set in f32 mode, the mode last
        o = Engine("GIN")
        try:
            o.set_emb_dim(300)
            o.set_weights(w)
            o.set_gin_eps(None)
            o.set_numeric_mode("f16", emb_dim=300)
            assert np.array_equal(o.forward(b), first)
        finally:
            o.close()
        assert e.exact_reruns() == 0
    finally:
        e.close()


@pytest.mark.parametrize("model", ["GCN", "GIN-VN", "GAT", "PNA", "DGN"])
def test_other_models(model):
    e = Engine(model)
    try:
        if model == "GCN":
            e.set_model_emb_dim(300)
            for mode in (F16, Q):
                rc, text = _dim(e, 300, mode)
                assert rc == ERR_UNSUPPORTED and "300" in text, (mode, rc, text)
            assert _dim(e, 300, F32)[0] == OK
            assert _dim(e, 100, F32)[0] == ERR_ARG
            e.set_model_emb_dim(100)
        rc, text = _dim(e, 300, F16)  # a width the engine does not have
        assert rc == ERR_ARG and "300" in text and "100" in text, (rc, text)
        assert _dim(e, 100, F32)[0] == OK
        want = e.lib.flowgnn_set_numeric_mode(e._h, F16)  # at 100 the call is exactly the one without the width
        e.lib.flowgnn_set_numeric_mode(e._h, F32)
        assert _dim(e, 100, F16)[0] == want
        assert _dim(e, 100, F32)[0] == OK
    finally:
        e.close()


def test_group_form():
    g = EngineGroup("GIN", [0, 0])
    try:
        rc, _ = _rc(lambda: g.set_numeric_mode("f16", emb_dim=300))  # the members are 100 wide
        assert rc == ERR_ARG
        g.set_emb_dim(300)
        rc, _ = _rc(lambda: g.set_numeric_mode("f16"))  # the call without the width
        assert rc == ERR_UNSUPPORTED
        g.set_numeric_mode("f16", emb_dim=300)
        rc, text = _rc(lambda: g.set_emb_dim(100))
        assert rc == ERR_UNSUPPORTED and g.emb_dim == 300, (rc, text)
        assert g.lib.flowgnn_group_set_numeric_mode_dim(g._h, 200, F16) == ERR_ARG
        assert g.lib.flowgnn_group_set_numeric_mode_dim(g._h, 300, Q) == ERR_UNSUPPORTED
        g.set_numeric_mode("f32", emb_dim=300)
        g.set_emb_dim(100)
    finally:
        g.close()
