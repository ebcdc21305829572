"""GCN at width 300: the f16 product beside OGB's linear edge encoder on the GPU (flowgnn.h: flowgnn_set_model_edge_linear_numeric;
kernels: flowgnn_amd/csrc/gcn_wide_el_f16.hip).
(1) With all-zero features and a dyadic bias the encoder gives exactly b_e, so the stages must return the bytes of gcn_wide_f16.hip's
    kernels on an edge table whose one used row is b_e: that pins the epilogue, the virtual node's add and partial rows, the ONE
    rounding of a and the product.  The same identity is asserted in the default mode first: the two walks agree on this input.
(2) Real features: the logits against the mode's float64 restatement under the project's rule, and against the plain float64 forward
    by the f16 rule at the ladder's rung the restatement itself allows (rows are printed: an fp32-versus-float64 tie in a moves a
    whole f16 spacing).  (3) The range guard.  (4) Off is off, the state rules and the refusals.
Every test fails on a library without the call."""
import dataclasses

import numpy as np
import pytest

from flowgnn_amd import Engine, graphpack as gp
from flowgnn_amd.engine import FlowGNNError
from tests import gcn_edge_linear_f16_ref as R16, gcn_edge_linear_ref as R, gcn_wide_f16_ref as F16R, gin_edge_linear_ref as GR
from tests.parity import assert_close, err_ratio
from tests.test_embeddings_gpu import launched, torch_context_first  # noqa: F401  (torch's context before the first engine: see there)
from tests.test_gcn_edge_linear_gpu import ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, EXACT, FAST, engine, in_range, ragged, vn300, w300
from tests.test_gcn_wide_f16_gpu import REL
from tests.wide_cases import graph, isolated, path

pytestmark = pytest.mark.gpu
FAST16, OTHERS = "gcn_wide_layer_el_f16", ("gcn_wide_layer_f16", "gcn_wide_layer")


def run(e, batch, ef=None):
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(batch, return_node_embeddings=True, edge_features=ef)))
    return res["got"], names


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def tiles():
    return gp.concat_batches([f(n, 10 * i + k) for i, n in enumerate((15, 16, 17, 127, 128, 129)) for k, f in enumerate((path, isolated))])


def vn_batch():  # tests/test_gcn_edge_linear_gpu.test_virtual_node_and_depth's: graphs inside and across a 16-node tile
    return gp.concat_batches([path(5, 3), isolated(2, 2), graph(5, [(i, (3 * i + 1) % 5) for i in range(5)] * 2, 4), path(17, 1)])


@pytest.mark.parametrize("vn,shape,L", [(False, tiles, 3), (True, tiles, 3), (False, ragged, 3), (True, ragged, 3), (True, vn_batch, 2), (True, vn_batch, 8)],
                         ids=["gcn-tiles", "vn-tiles", "gcn-ragged", "vn-ragged", "vn-L2", "vn-L8"])
def test_bytes_of_the_f16_kernel_on_a_table_of_the_bias(vn, shape, L):
    batch, rng = shape(), np.random.default_rng(41)
    batch = dataclasses.replace(batch, edge_attr=np.zeros_like(batch.edge_attr))  # bond code (0, 0, 0) on every edge
    el = dict(GR.edge_linear(L, 7, 43), b=(rng.integers(-128, 129, (L, 300)) / 64.0).astype(np.float32))  # multiples of 2^-6 in [-2, 2]
    table = np.zeros((L, 13, 300), np.float32)
    table[:, 0] = el["b"]  # the row of (0, 0, 0) is b_e + 0 + 0
    v, zeros = vn300(L) if vn else None, np.zeros((batch.total_edges, 7), np.float32)
    e, t = engine(L, el=el, vn=v), Engine("GCN", device=0)
    t.set_model_emb_dim(300)
    t.set_num_layers(L)
    t.set_weights(dict(w300(L), edge_embedding_weight=table))
    if vn:
        t.set_gcn_virtual_node(v)
    assert same(run(e, batch, zeros)[0], t.forward(batch, return_node_embeddings=True))  # the default mode: existing code, the two walks agree
    e.set_model_edge_linear_numeric("f16")
    t.set_numeric_mode("f16", emb_dim=300)
    got, names = run(e, batch, zeros)
    assert FAST16 in names and FAST in names and not set(OTHERS) & names and e.exact_reruns() == 0, (names, e.exact_reruns())  # (FAST: the last stage)
    want = t.forward(batch, return_node_embeddings=True)
    assert t.exact_reruns() == 0 and same(got, want)


@pytest.mark.parametrize("dim,L,vn", [(1, 5, False), (7, 5, False), (10, 5, False), (7, 2, True), (7, 8, True)])
def test_real_features_against_float64(dim, L, vn):
    batch, seed, v = ragged(), 30 + dim + L, vn300(L) if vn else None
    el, ef = GR.edge_linear(L, dim, seed), GR.features(batch.total_edges, dim, seed + 1)
    ref, rne = R.forward(batch, w300(L), el, ef, vn=v), R16.forward(batch, w300(L), el, ef, vn=v)
    assert in_range(ref), (ref.operands, ref.max_feature)
    tol = next(t for t in F16R.LADDER if F16R.rule(rne.logits, ref, t) <= 0.5)  # from the two references alone, before the GPU runs
    e = engine(L, el=el, vn=v)
    (base, _), _ = run(e, batch, ef)
    e.set_model_edge_linear_numeric("f16")
    (logits, rows), names = run(e, batch, ef)
    print(f"F {dim}, L {L}, vn {vn}: tol {tol:g}; restatement at {F16R.rule(rne.logits, ref, tol):.3f}, kernel at {F16R.rule(logits, ref, tol):.3f} of the f16 rule; "
          f"kernel against the restatement: logits {err_ratio(logits, rne.logits, rne.scale, REL):.4f}, rows {err_ratio(rows, rne.rows, rne.scale, REL):.4f} "
          f"of the project's rule (scale {rne.scale:.1f})")
    assert FAST16 in names and not set(OTHERS) & names and e.exact_reruns() == 0, (names, e.exact_reruns())
    assert_close(np.asarray(logits, np.float64).reshape(rne.logits.shape), rne.logits, scale=rne.scale, rel=REL, what="logits against the restatement")
    assert F16R.rule(logits, ref, tol) <= 1.0
    assert np.mean(logits != base) > 0.5  # the mode is visibly on


def test_range_guard():
    batch = gp.concat_batches([path(17, 1), isolated(3, 2)])
    el, ef = GR.edge_linear(5, 7, 71), GR.features(batch.total_edges, 7, 72)
    ef[11, 3] = 1.0e5
    e = engine(el=el)
    e.set_model_edge_linear_numeric("f16")
    got, names = run(e, batch, ef)
    assert e.exact_reruns() == 1 and FAST16 in names and EXACT in names, (e.exact_reruns(), names)
    assert same(got, run(engine(el=el), batch, ef)[0])


def test_off_is_off_state_and_refusals():
    mol = gp.synth_molhiv_batch(8, seed=3)
    el, ef = GR.edge_linear(5, 7, 81), GR.features(mol.total_edges, 7, 82)
    never, names_never = run(engine(el=el), mol, ef)
    e = engine()
    e.set_model_edge_linear_numeric("f16")  # the mode first, the encoder second
    e.set_model_edge_linear(el["w"], el["b"])
    on, names = run(e, mol, ef)
    assert FAST16 in names and not set(OTHERS) & names and e.lib.flowgnn_edge_linear_numeric(e._h) == 2 and not same(on, never), names
    e.set_model_edge_linear(None, None)  # the setting survives the encoder going off and on again ...
    assert "gcn_wide_layer" in run(e, mol)[1]
    e.set_model_edge_linear(el["w"], el["b"])
    e.set_weights(w300())
    again, names = run(e, mol, ef)
    assert FAST16 in names and same(again, on), names
    o = engine(el=el)  # ... and the other call order gives the same bytes
    o.set_model_edge_linear_numeric("f16")
    assert same(run(o, mol, ef)[0], on)

    def refused(code, fn):
        with pytest.raises(FlowGNNError) as x:
            fn()
        assert x.value.code == code and len(str(x.value)) > 40, x.value

    raw = lambda h, dim, mode: h._check(h.lib.flowgnn_set_model_edge_linear_numeric(h._h, dim, mode), "flowgnn_set_model_edge_linear_numeric")
    for dim, mode in ((300, 1), (300, 3), (200, 2), (100, 2), (200, 0)):  # Q6_10, no mode, no width, not the engine's width
        refused(ERR_ARG, lambda: raw(e, dim, mode))
    assert e.lib.flowgnn_set_model_edge_linear_numeric(None, 300, 2) == ERR_ARG
    refused(ERR_STATE, lambda: e.set_numeric_mode("f16", emb_dim=300))  # the stages' own mode stays refused beside the encoder
    refused(ERR_UNSUPPORTED, lambda: raw(Engine("PNA", device=0), 100, 2))
    refused(ERR_UNSUPPORTED, lambda: raw(Engine("GCN", device=0), 100, 2))  # width 100
    raw(Engine("PNA", device=0), 300, 0)  # the default is accepted wherever a handle is valid
    e.set_model_edge_linear_numeric("f32")  # back: the bytes and the launches of an engine that never made the call
    back, names_back = run(e, mol, ef)
    assert e.lib.flowgnn_edge_linear_numeric(e._h) == 0 and names_back == names_never and FAST in names_back and same(back, never)
    from tests.test_gin_edge_linear_gpu import engine as gin_engine  # on a GIN engine the two forms of the call are one
    a, b = gin_engine(el=el), gin_engine(el=el)
    a.set_model_edge_linear_numeric("f16")
    b.set_edge_linear_numeric("f16")
    got_a, names_a = run(a, mol, ef)
    assert "gin_wide_layer_el_f16" in names_a and same(got_a, run(b, mol, ef)[0])
