"""GIN at width 300: the f16 node MLP beside OGB's linear edge encoder on the GPU (flowgnn.h: flowgnn_set_edge_linear_numeric; kernels:
flowgnn_amd/csrc/gin_wide_el_f16.hip).
(1) With all-zero features and a dyadic bias the encoder gives exactly b_e, so the layer must return the bytes of gin_wide_f16.hip's
    kernels on an edge table whose one used row is b_e: that pins the self term, the MLP half, the epilogue and the virtual node.
(2) Real features against the plain float64 forward by the project's f16 rule, |gpu - f64| <= 2e-4 (scale + |f64|), on the logits (the
    rows are printed: at depth 2 the mode's own restatement is at 0.67 of the rule on w300(2), beyond the half a fair test may use).
(3) The range guard.  (4) Off is off, the state rules and the refusals.  Every test fails on a library without the call."""
import dataclasses

import numpy as np
import pytest

from flowgnn_amd import Engine, graphpack as gp
from flowgnn_amd.engine import FlowGNNError
from tests import gin_edge_linear_f16_ref as R16, gin_edge_linear_ref as R
from tests.test_embeddings_gpu import launched, torch_context_first  # noqa: F401  (torch's context before the first engine: see there)
from tests.test_gin_edge_linear_gpu import ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, EXACT, FAST, engine, in_range, ragged, vn300, w300
from tests.test_gin_wide_f16_gpu import F16_REL
from tests.wide_cases import hub, isolated, path

pytestmark = pytest.mark.gpu
FAST16, OTHERS = "gin_wide_layer_el_f16", (FAST, "gin_wide_layer_f16", "gin_wide_layer")


def run(e, batch, ef=None):
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(batch, return_node_embeddings=True, edge_features=ef)))
    return res["got"], names


@pytest.mark.parametrize("vn", [False, True], ids=["gin", "gin-virtual"])
def test_bytes_of_the_f16_kernel_on_a_table_of_the_bias(vn):
    L, rng = 3, np.random.default_rng(41)  # (layers 0, 1 ReLU'd -- the virtual node's instance when it is on --, layer 2 not)
    parts = [f(n, 10 * i + k) for i, n in enumerate((15, 16, 17, 127, 128, 129)) for k, f in enumerate((path, isolated))] + [hub(40, 7)]
    batch = gp.concat_batches(parts)
    batch = dataclasses.replace(batch, edge_attr=np.zeros_like(batch.edge_attr))  # bond code (0, 0, 0) on every edge
    el = dict(R.edge_linear(L, 7, 43), b=(rng.integers(-128, 129, (L, 300)) / 64.0).astype(np.float32))  # multiples of 2^-6 in [-2, 2]
    table = np.zeros((L, 13, 300), np.float32)
    table[:, 0] = el["b"]  # the row of (0, 0, 0) is b_e + 0 + 0
    eps, v = [0.5, -0.25, 0.25], vn300(L) if vn else None
    e = engine(L, el=el, vn=v)
    e.set_gin_eps(eps)
    e.set_edge_linear_numeric("f16")
    (logits, rows), names = run(e, batch, np.zeros((batch.total_edges, 7), np.float32))
    assert FAST16 in names and not set(OTHERS) & names and e.exact_reruns() == 0, (names, e.exact_reruns())
    t = Engine("GIN", device=0)
    t.set_emb_dim(300)
    t.set_num_layers(L)
    t.set_weights(dict(w300(L), edge_embedding_weight=table))
    t.set_numeric_mode("f16", emb_dim=300)
    t.set_ogb_virtual_node(v)
    t.set_gin_eps(eps)
    want_logits, want_rows = t.forward(batch, return_node_embeddings=True)
    assert t.exact_reruns() == 0
    assert rows.tobytes() == want_rows.tobytes() and logits.tobytes() == want_logits.tobytes()


@pytest.mark.parametrize("dim,L,vn", [(1, 5, False), (7, 5, False), (10, 5, False), (7, 2, True), (7, 8, True)])
def test_real_features_against_float64(dim, L, vn):
    batch, seed = ragged(), 30 + dim + L
    el, ef = R.edge_linear(L, dim, seed), R.features(batch.total_edges, dim, seed + 1)
    kw = dict(vn=vn300(L), eps=[0.1 * (-1) ** l for l in range(L)]) if vn else {}
    ref, rne = R.forward(batch, w300(L), el, ef, **kw), R16.forward(batch, w300(L), el, ef, **kw)
    assert in_range(ref, w300(L))
    ratio = lambda got, x: float((np.abs(np.asarray(got, np.float64).reshape(x.shape) - x) / (F16_REL * (ref.scale + np.abs(x)))).max())
    own = ratio(rne.logits, ref.logits)  # the references first: a right kernel can meet the rule only if the restatement has room
    print(f"F {dim}, L {L}, vn {vn}: restatement at {own:.3f} (logits) and {ratio(rne.rows, ref.rows):.3f} (rows) of the rule, scale {ref.scale:.1f}")
    assert own <= 0.5, own
    e = engine(L, el=el, vn=kw.get("vn"))
    e.set_gin_eps(kw.get("eps"))
    (base, _), _ = run(e, batch, ef)
    e.set_edge_linear_numeric("f16")
    (logits, rows), names = run(e, batch, ef)
    print(f"F {dim}, L {L}, vn {vn}: f16 mode at {ratio(logits, ref.logits):.3f} (logits) and {ratio(rows, ref.rows):.3f} (rows) of the rule")
    assert FAST16 in names and not set(OTHERS) & names and e.exact_reruns() == 0, (names, e.exact_reruns())
    assert ratio(logits, ref.logits) <= 1.0
    assert np.mean(logits != base) > 0.5  # the mode is visibly on


def test_range_guard():
    batch = gp.concat_batches([path(17, 1), isolated(3, 2)])
    el, ef = R.edge_linear(5, 7, 71), R.features(batch.total_edges, 7, 72)
    ef[11, 3] = 1.0e5
    e = engine(el=el)
    e.set_edge_linear_numeric("f16")
    got, names = run(e, batch, ef)
    assert e.exact_reruns() == 1 and FAST16 in names and EXACT in names and FAST not in names, (e.exact_reruns(), names)
    want, _ = run(engine(el=el), batch, ef)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_off_is_off_state_and_refusals():
    mol = gp.synth_molhiv_batch(8, seed=3)
    el, ef = R.edge_linear(5, 7, 81), R.features(mol.total_edges, 7, 82)
    never, names_never = run(engine(el=el), mol, ef)
    e = engine()
    e.set_edge_linear_numeric("f16")  # the mode first, the encoder second
    e.set_edge_linear(el["w"], el["b"])
    (on, _), names = run(e, mol, ef)
    assert FAST16 in names and not set(OTHERS) & names and e.edge_linear_numeric == "f16", names
    e.set_edge_linear(None, None)  # the setting survives the encoder going off and on again ...
    assert "gin_wide_layer" in run(e, mol)[1]
    e.set_edge_linear(el["w"], el["b"])
    e.set_weights(w300())
    (again, _), names = run(e, mol, ef)
    assert FAST16 in names and again.tobytes() == on.tobytes(), names
    o = engine(el=el)  # ... and the other call order gives the same bytes
    o.set_edge_linear_numeric("f16")
    assert run(o, mol, ef)[0][0].tobytes() == on.tobytes()

    def refused(code, fn):
        with pytest.raises(FlowGNNError) as x:
            fn()
        assert x.value.code == code and len(str(x.value)) > 40, x.value

    raw = lambda dim, mode: e._check(e.lib.flowgnn_set_edge_linear_numeric(e._h, dim, mode), "flowgnn_set_edge_linear_numeric")
    for dim, mode in ((300, 1), (300, 3), (200, 2), (100, 2), (200, 0)):  # Q6_10, no mode, no width, not the engine's width
        refused(ERR_ARG, lambda: raw(dim, mode))
    assert e.lib.flowgnn_set_edge_linear_numeric(None, 300, 2) == ERR_ARG and e.lib.flowgnn_edge_linear_numeric(None) == -1
    refused(ERR_STATE, lambda: e.set_numeric_mode("f16", emb_dim=300))  # the layers' own mode stays refused beside the encoder
    gcn = Engine("GCN", device=0)
    gcn.set_model_emb_dim(300)
    refused(ERR_UNSUPPORTED, lambda: gcn.set_edge_linear_numeric("f16"))
    refused(ERR_UNSUPPORTED, lambda: Engine("GIN", device=0).set_edge_linear_numeric("f16"))  # width 100
    Engine("GIN", device=0).set_edge_linear_numeric("f32")  # the default is accepted wherever a handle is valid
    e.set_edge_linear_numeric("f32")  # back: the bytes and the launches of an engine that never made the call
    back, names_back = run(e, mol, ef)
    assert names_back == names_never and FAST in names_back and all(b.tobytes() == n.tobytes() for b, n in zip(back, never))
