"""GCN at width 300 in the f16 numeric mode (flowgnn.h: flowgnn_set_model_numeric_mode_dim), what can be shown
without a GPU: that the probe of tests/test_gcn_wide_f16_gpu.py can prove what it claims (which fp32 sums are exact on its inputs, the
references apart from one another), that the restatement with nothing rounded is the float64 forwards the project already has, that
the realistic-shape rule has the tolerance the issue's ladder gives, and that the call exists in every layer -- header, library, ctypes
prototypes, wrappers, host CLI, build lists.  The last group fails on a tree without the call."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from flowgnn_amd import Engine, EngineGroup, _lib
from tests import gcn_wide_f16_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flowgnn_amd", "csrc")
ERR_ARG = 1
CONFIGS = {"plain": {}, "virtual node": dict(vn=True), "residual": dict(residual=True), "JK sum": dict(jk="sum"),
           "virtual node, JK sum, residual": dict(vn=True, jk="sum", residual=True)}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _kw(cfg):
    kw = dict(cfg)
    kw["vn"] = R.virtual_node_of() if kw.get("vn") else None
    return kw


# ---------------------------------------------------------------- the probe's inputs
def test_probe_batch_shape():
    b = R.probe_batch()
    assert (b.num_graphs, b.total_nodes) == (60, 900)
    n, off = np.asarray(b.nums_of_nodes), b.node_offsets()
    assert int(n[0]) == 1 and (np.asarray(b.nums_of_edges) == 0).sum() >= 3 and (n[np.asarray(b.nums_of_edges) == 0] > 1).any()  # edgeless, one of several nodes
    assert b.total_nodes > 7 * 128 and b.total_nodes % 16 != 0  # eight workgroups, the last one ending inside a 16-row tile
    first, last = off[:-1], off[1:] - 1
    assert ((first // 128) != (last // 128)).any()  # a graph straddles a workgroup boundary
    assert (((first // 16) != (last // 16)) & ((first // 128) == (last // 128))).any()  # ... and one a 16-row tile inside a workgroup
    ge = b.global_edges()
    deg = np.bincount(ge[:, 0], minlength=b.total_nodes)
    assert set(deg.tolist()) == {0, 3, 15} and np.array_equal(deg, np.bincount(ge[:, 1], minlength=b.total_nodes))
    assert len({(int(u), int(v)) for u, v in ge}) == len(ge)  # no pair twice: the degrees are the graphs'


def test_probe_weights_are_what_the_docstring_says():
    w = R.weights_of(1)
    cw = np.asarray(w["convs_weight"], np.float64)
    assert ((cw != 0).sum(axis=2) == 2).all() and set(np.unique(cw[0])) == {0.0, 0.25, 0.5}
    s = R.pow2_scale(cw[1])
    assert set(np.unique(R.rounder("rne")(cw[1:] * s) / s)) == {0.0, 0.25, 0.5}  # to nearest: the few-bit values ...
    assert not set(np.unique(R.rounder("rtz")(cw[1:] * s) / s)) & {0.25, 0.5}  # ... toward zero: not
    scale = np.asarray(w["bn_weight"], np.float32) / np.sqrt(np.asarray(w["bn_var"], np.float32) + np.float32(R.BN_EPS))
    assert set(np.unique(scale)) == {0.5, 1.0} and not np.asarray(w["bn_mean"]).any()  # the folded scale: a power of two


@pytest.mark.parametrize("c", R.CASES, ids=R.IDS)
def test_which_fp32_sums_of_the_mode_are_exact_on_the_probe(c):
    """The rows' sums in every case but the one named in ROWS_NOT_EXACT, the pools' and the head's in every case but POOL_NOT_EXACT
    (which pool the mean): what the GPU test holds to bits is proven here, and nothing else is held to bits."""
    refs = R.references(c)
    for v in R.CHECKED:
        print(c.name, v, f"rows 2^{refs[v][1].rows:.2f}, pools and head 2^{refs[v][1].pool:.2f}")
    assert R.rows_exact(c) == (c.name not in R.ROWS_NOT_EXACT)
    assert R.pool_exact(c) == (c.name not in R.POOL_NOT_EXACT)
    assert c.pooling == "mean" or R.pool_exact(c)  # a pooled sum or maximum is only ever asserted where it is proven


@pytest.mark.parametrize("name", ["plain", "virtual node", "residual", "JK sum"])
@pytest.mark.parametrize("pooling", ["sum", "max"])
def test_all_fp32_evaluation_equals_the_float64_one_bit_for_bit(name, pooling):
    """where the figures are at most 24, the forward evaluated in fp32 throughout IS the float64 one: rows always, pooled rows too"""
    kw = _kw(CONFIGS[name])
    a = R.forward(R.probe_batch(), R.weights_of(1), pooling=pooling, **kw)
    b = R.forward(R.probe_batch(), R.weights_of(1), pooling=pooling, dtype=np.float32, **kw)
    assert b.rows.dtype == np.float32 and np.array_equal(b.rows.astype(np.float64), a.rows)
    if name == "plain" or pooling == "max":  # (a maximum of exact rows is exact; a sum where the pool's figure says so: the plain case)
        assert np.array_equal(b.pooled.astype(np.float64), a.pooled)
    if name == "plain":  # ... and the head on it
        assert np.array_equal(b.logits.astype(np.float64), a.logits)


def test_separation_table_and_the_named_exceptions():
    """NOT_SEPARATED is the computed table's complement, in both directions; logits, rows and pooled rows against rtz, the unrounded
    forward and both weight variants must separate in every case."""
    found, spread = {}, {}
    for c in R.CASES:
        for (o, v), (ok, frac, med) in R.separation(c, R.TABLE_OUTPUTS).items():
            spread.setdefault((v, o), []).append(frac)
            if not ok:
                found[(c.name, o, v)] = frac
    for (v, o), f in sorted(spread.items()):
        print(f"{v:30s} {o:7s} {100 * min(f):.0f} .. {100 * max(f):.0f} %")
    assert set(found) == set(R.NOT_SEPARATED), (set(found) ^ set(R.NOT_SEPARATED))
    for k, frac in found.items():
        assert abs(frac - R.NOT_SEPARATED[k]) < 0.01, (k, frac)
        assert k[2] == "activations not rounded", k  # nothing else may be listed


# ---------------------------------------------------------------- the restatement is the forwards the project has
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("pooling", ["mean", "max"])
def test_with_nothing_rounded_it_is_the_float64_forward_of_the_jk_module(name, pooling):
    from tests import ogb_gcn_jk_torch as J
    from tests import gcn_wide_ref as W
    b, w = W.sep_batch(0).slice(0, 40), W.sep_weights()
    cfg = dict(CONFIGS[name])
    if cfg.pop("vn", False):
        from tests import gcn_wide_vn_ref as V
        cfg["vn"] = V.shapes_virtual_node()
    got, want = R.forward(b, w, rnd="none", pooling=pooling, **cfg), J.forward(b, w, cfg.get("vn"), jk=cfg.get("jk", "last"),
                                                                               residual=cfg.get("residual", False), pooling=pooling)
    tol = 1e-9 * want.scale
    for o, x in (("logits", want.logits), ("rows", want.rows), ("pooled", want.pooled), ("h5", want.h5)):
        assert np.abs(getattr(got, o) - x).max() <= tol, o
    assert abs(got.scale - want.scale) <= tol
    if name == "plain":
        ref = W.forward(b, w, pooling=pooling)
        assert np.abs(got.logits - ref.logits).max() <= 1e-9 * ref.scale and np.abs(got.rows - ref.rows).max() <= 1e-9 * ref.scale
        assert np.abs(got.terms - W.node_logits(w, ref.rows)).max() <= 1e-9 * ref.scale
    if name == "virtual node":
        from tests import gcn_wide_vn_ref as V
        ref = V.forward(b, w, cfg["vn"], pooling=pooling)
        assert np.abs(got.logits - ref.logits).max() <= 1e-9 * ref.scale and np.abs(got.rows - ref.rows).max() <= 1e-9 * ref.scale


def test_the_mode_rounds_exactly_the_two_operands():
    """rne differs from the unrounded forward, each operand point alone moves the result, and layer 0's product is not touched: with
    W_1 .. W_4 = 0 every variant is the unrounded forward bit for bit"""
    from tests import gcn_wide_ref as W
    b, w = W.sep_batch(0).slice(0, 12), dict(W.sep_weights())
    outs = {k: R.forward(b, w, rnd=r).rows for k, r in (("rne", "rne"), ("none", "none"), ("a", {"w": "none"}), ("w", {"a": "none"}))}
    assert all(np.mean(outs[k] != outs["none"]) > 0.5 for k in ("rne", "a", "w")) and np.mean(outs["a"] != outs["w"]) > 0.5
    cw = np.asarray(w["convs_weight"], np.float32).copy()
    cw[1:] = 0.0
    w["convs_weight"] = cw
    assert np.array_equal(R.forward(b, w).rows, R.forward(b, w, rnd="none").rows)


# ---------------------------------------------------------------- accuracy at a realistic shape: the tolerance
@pytest.mark.parametrize("which", R.ACCURACY)
def test_the_restatement_is_within_half_of_the_ladders_tolerance(which):
    """tol: the smallest of 1e-4 x {1, 2, 5, 10, ..} the restatement stays within half of, |rne - f64| <= tol / 2 (scale + |f64|) on the
    logits of 256 molpcba-shaped graphs; the GPU test holds the kernel to tol.  Measured: 0.490, 0.029, 0.327 and 0.014 of 1e-4 -- tol
    is 1e-4, the first rung, in all four.  The rows are printed (2.46, 0.07, 2.36 and 0.09 of 1e-4): a single row carries the
    roundings a graph's mean averages out."""
    f64, rne = R.accuracy_references(which)
    frac = R.rule(rne.logits, f64, R.TOL[which])
    rows = float((np.abs(rne.rows - f64.rows) / (R.TOL[which] * (f64.scale + np.abs(f64.rows)))).max())
    print(f"{which}: restatement at {frac:.3f} of tol {R.TOL[which]:g} on the logits (scale {f64.scale:.1f}); rows {rows:.3f}")
    assert R.TOL[which] == R.ladder_tol(which) and frac <= 0.5
    assert np.mean(rne.logits != f64.logits) > 0.5


# ---------------------------------------------------------------- the call, layer by layer
def test_header_declares_and_defines_the_call():
    h = _read("include", "flowgnn.h")
    assert re.search(r"int\s+flowgnn_set_model_numeric_mode_dim\(flowgnn_engine\*\s*e,\s*int\s+emb_dim,\s*int\s+mode\);", h)
    assert re.search(r"int\s+flowgnn_group_set_model_numeric_mode_dim\(flowgnn_group\*\s*g,\s*int\s+emb_dim,\s*int\s+mode\);", h)
    at = h.index("int flowgnn_set_numeric_mode_dim(flowgnn_engine")
    decl = h.index("int flowgnn_set_model_numeric_mode_dim(flowgnn_engine")
    assert at < decl < at + 4500  # next to the call it is the model form of
    text = h[at:decl]
    for word in ("r(W s) / s", "nearest even", "FLOWGNN_ERR_ARG", "FLOWGNN_ERR_UNSUPPORTED", "flowgnn_set_model_emb_dim(e, 100)", "unrounded", "6e4"):
        assert word in text, word
    assert h.index("flowgnn_group_set_numeric_mode_dim(flowgnn_group") < h.index("flowgnn_group_set_model_numeric_mode_dim(flowgnn_group")


def test_library_exports_prototypes_and_null_handles():
    lib = _lib.load()
    null = C.c_void_p()
    assert lib.flowgnn_set_model_numeric_mode_dim(null, 300, 2) == ERR_ARG
    assert lib.flowgnn_group_set_model_numeric_mode_dim(null, 300, 2) == ERR_ARG
    assert lib.flowgnn_set_model_numeric_mode_dim.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert lib.flowgnn_group_set_model_numeric_mode_dim.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert lib.flowgnn_set_model_numeric_mode_dim.restype == C.c_int and lib.flowgnn_group_set_model_numeric_mode_dim.restype == C.c_int


@pytest.mark.parametrize("cls", [Engine, EngineGroup])
def test_wrappers_pick_the_model_form_for_a_gcn_engine(cls):
    p = inspect.signature(cls.set_numeric_mode).parameters
    assert list(p)[1:] == ["mode", "emb_dim"] and p["emb_dim"].default is None and p["mode"].default == "f32"
    src = inspect.getsource(cls.set_numeric_mode)
    assert "_set_numeric_mode_dim" in src and "if emb_dim is None" in src  # (what tests/test_gin_wide_f16_cpu.py pins stays)
    assert re.search(r'elif self\.model == "GCN":\s+self\._check\(self\.lib\.flowgnn_(group_)?set_model_numeric_mode_dim\(', src)


def test_host_cli_branches_on_the_model_in_front_of_the_old_expression():
    src = _read("flowgnn_amd", "csrc", "host_main.cpp")
    old = ("emb_dim != FLOWGNN_EMB_DIM_REFERENCE ? flowgnn_group_set_numeric_mode_dim(eng, emb_dim, numeric) : "
           "flowgnn_group_set_numeric_mode(eng, numeric)")
    new = "flowgnn_group_set_model_numeric_mode_dim(eng, emb_dim, numeric)"
    assert old in src and new in src and src.index("mid == FLOWGNN_MODEL_GCN && emb_dim != FLOWGNN_EMB_DIM_REFERENCE) rc = " + new) < src.index(old)
    assert "host GCN --emb-dim 300 --numeric f16" in src[:src.index("#include")]  # the usage comment


def test_build_lists_and_the_width_written_once():
    mk = _read("flowgnn_amd", "csrc", "Makefile")
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "gcn_wide_f16.hip" in srcs and "gcn_wide_f16.h" in mk
    dev = _read("scripts", "dev", "devlib.sh")
    assert re.search(r"^for f in .*\bgcn_wide_f16\b.*; do", dev, re.M)
    # templates on D: no literal width in the new translation unit or its header, comments included
    for name in ("gcn_wide_f16.hip", "gcn_wide_f16.h"):
        text = open(os.path.join(CSRC, name)).read()
        for lit in ("300", "320", "600"):
            assert not re.search(rf"\b{lit}\b", text), (name, lit)
    hip = open(os.path.join(CSRC, "gcn_wide_f16.hip")).read()
    for k in ("gcw_layer_f16_kernel", "gcw_layer_vn_f16_kernel", "gcw_layer_jk_f16_kernel", "gcw_layer_vn_jk_f16_kernel", "gcw_layer_f16_body"):
        assert k in hip, k
    for fn in ("gcw_walk<D, true>", "gcw_vn_add_partials<D>", "gcw_ext_residual<D>", "gcw_ext_store<D>"):  # gcn_wide_body.h's, as they stand
        assert fn in hip, fn
    assert "gcw_layer_body" not in hip.replace("gcw_layer_body calls", "").replace("instance of gcw_layer_body", "").replace(
        "gcw_layer_body (gcn_wide_body.h)", "")  # a copy, not an instance
    model = open(os.path.join(CSRC, "gcn_wide.hip")).read()
    assert '"gcn_wide_layer_f16"' in model and "gcw_pack_layer_f16" in model
