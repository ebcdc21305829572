"""GCN at width 300 with OGB's linear edge encoder on the GPU (flowgnn.h: flowgnn_set_model_edge_linear): rows and
logits of gcn_wide_el.hip's kernels against tests/gcn_edge_linear_ref.forward (float64) by tests/parity.py's rule alone, at the smallest
shapes at which the walk can go wrong: the 16-row and 128-row tiles' edges, rows with no edge (the norm = 0 trips), one busy row among
idle ones, an edge list whose CSR order is not its input order, the slot map's two ends, graphs inside and across a 16-node tile for
the virtual node's partial rows, the first and last stage at depths 2 and 8.

Measured on one MI355X (the figures each case prints): the worst ratio to the rule's bound is 0.003 on rows and 0.002 on logits."""
import functools

import numpy as np
import pytest

from flowgnn_amd import Engine, graphpack as gp, weights
from flowgnn_amd.engine import FlowGNNError
from tests import gcn_edge_linear_ref as R, gin_edge_linear_ref as GR
from tests.parity import assert_close, err_ratio
from tests.test_embeddings_gpu import launched, torch_context_first  # noqa: F401  (torch's context before the first engine: see there)
from tests.test_gin_edge_linear_gpu import ragged  # a 40-in-edge hub among one-node graphs, a shuffled edge list with repeated edges
from tests.wide_cases import graph, isolated, path

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, FAST, EXACT = 1, 6, 8, "gcn_wide_layer_el", "gcn_wide_aggregate_el"


@functools.lru_cache(maxsize=None)
def w300(L=5):
    return weights.synth_gcn_weights(seed=7, emb_dim=300, num_layers=L)


@functools.lru_cache(maxsize=None)
def vn300(L):
    vn = weights.synth_gcn_virtual_node(seed=13, emb_dim=300, num_layers=L)  # (w1 / 16: tests/gcn_wide_vn_ref.shapes_virtual_node)
    return dict(vn, w1=vn["w1"] * np.float32(1.0 / 16))


def engine(L=5, el=None, vn=None):
    e = Engine("GCN", device=0)
    e.set_model_emb_dim(300)
    e.set_num_layers(L)
    e.set_weights(w300(L))
    if vn is not None:
        e.set_gcn_virtual_node(vn)
    if el is not None:
        e.set_model_edge_linear(el["w"], el["b"])
    e.profile_enable(True)
    return e


def in_range(ref):  # from the reference alone (tests/test_gcn_wide_vn_gpu.in_range, and the features the walk guards)
    return ref.operands < 6.0e4 / 2 and ref.max_feature < 6.0e4


def check(e, batch, ef, ref, what, reruns=0):
    res = {}
    before = e.exact_reruns()
    names = launched(e, lambda: res.update(got=e.forward(batch, return_node_embeddings=True, edge_features=ef)))
    logits, rows = res["got"]
    print(what, f"worst ratio to the bound: logits {err_ratio(logits, ref.logits, ref.scale):.3f}, rows {err_ratio(rows, ref.rows, ref.scale):.3f}")
    assert FAST in names and "gcn_wide_layer" not in names, names
    assert e.exact_reruns() - before == reruns and (EXACT in names) == (reruns > 0), (e.exact_reruns(), before, names)
    assert_close(rows, ref.rows, scale=ref.scale, what=what + " rows")
    assert_close(logits, ref.logits, scale=ref.scale, what=what + " logits")


def run_case(batch, dim, seed, what, L=5, vn=None):
    el, ef = GR.edge_linear(L, dim, seed), GR.features(batch.total_edges, dim, seed + 1)
    ref = R.forward(batch, w300(L), el, ef, vn=vn)
    assert in_range(ref), (ref.operands, ref.max_feature)
    check(engine(L, el=el, vn=vn), batch, ef, ref, what)


def test_tile_edges():
    parts = [f(n, 10 * i + k) for i, n in enumerate((15, 16, 17, 127, 128, 129)) for k, f in enumerate((path, isolated))]
    run_case(gp.concat_batches(parts), 7, 21, "tile edges")


def test_ragged_trips_and_edge_order():
    batch = ragged()
    ge = batch.global_edges()
    csr = np.lexsort((np.arange(len(ge)), ge[:, 0], ge[:, 1]))  # by destination, then source, ties in input order
    assert (csr != np.arange(len(ge))).any() and len(np.unique(ge, axis=0)) < len(ge)  # eid must carry the features: CSR position cannot
    run_case(batch, 7, 23, "ragged")


@pytest.mark.parametrize("dim", [1, 7, 10])
def test_edge_dim(dim):
    run_case(ragged(seed=6), dim, 30 + dim, f"edge_dim {dim}")


@pytest.mark.parametrize("L", [2, 8])
def test_virtual_node_and_depth(L):  # 5-, 2- and 5-node graphs inside the first 16-node tile, the 17-node path across its boundary
    batch = gp.concat_batches([path(5, 3), isolated(2, 2), graph(5, [(i, (3 * i + 1) % 5) for i in range(5)] * 2, 4), path(17, 1)])
    run_case(batch, 7, 50 + L, f"gcn-virtual, {L} layers", L=L, vn=vn300(L))


def test_range_guard():
    batch = gp.concat_batches([path(17, 1), isolated(3, 2)])
    el, ef = GR.edge_linear(5, 7, 71), GR.features(batch.total_edges, 7, 72)
    ef[11, 3] = 1.0e5
    check(engine(el=el), batch, ef, R.forward(batch, w300(), el, ef), "one feature of 1e5", reruns=1)


def test_off_is_off_and_device_features():
    import torch
    mol = gp.synth_molhiv_batch(8, seed=3)
    el, ef = GR.edge_linear(5, 7, 81), GR.features(mol.total_edges, 7, 82)
    e = engine(el=el)
    assert np.array_equal(e.forward(mol, edge_features=ef), e.forward(mol, edge_features=torch.from_numpy(ef).to("cuda:0")))
    e.set_model_edge_linear(None, None)
    res = {}
    names = launched(e, lambda: res.update(got=e.forward(mol)))
    assert e.edge_linear == 0 and "gcn_wide_layer" in names and FAST not in names, names
    assert np.array_equal(res["got"], engine().forward(mol))  # the bits of an engine that never had the encoder


def test_refusals():
    mol = gp.synth_molhiv_batch(4, seed=3)
    el, zeros = GR.edge_linear(5, 7, 91), lambda *shape: np.zeros(shape, np.float32)
    e = engine(el=el)

    def refused(code, fn):
        with pytest.raises(FlowGNNError) as x:
            fn()
        assert x.value.code == code and len(str(x.value)) > 40, x.value

    refused(ERR_STATE, lambda: e.set_numeric_mode("f16", emb_dim=300))
    refused(ERR_STATE, lambda: e.set_jk_residual("sum", False))
    refused(ERR_STATE, lambda: e.set_jk_residual("last", True))
    refused(ERR_UNSUPPORTED, lambda: e.set_edge_linear(el["w"], el["b"]))  # the GIN form of the call, on a GCN engine
    ef = GR.features(mol.total_edges, 7, 92)  # the engine stays usable, and the encoder is still on:
    check(e, mol, ef, R.forward(mol, w300(), el, ef), "after the refusals")
    for first in (lambda x: x.set_numeric_mode("f16", emb_dim=300), lambda x: x.set_jk_residual("sum", False), lambda x: x.set_jk_residual("last", True)):
        other = engine()
        first(other)
        refused(ERR_STATE, lambda: other.set_model_edge_linear(el["w"], el["b"]))
    refused(ERR_UNSUPPORTED, lambda: Engine("GCN", device=0).set_model_edge_linear(zeros(5, 100, 7), zeros(5, 100)))  # width 100
