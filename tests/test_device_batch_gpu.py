"""flowgnn_set_batch_device (include/flowgnn.h): a batch already in GPU memory, in the PyG layout (int64, batch-global ids,
edge_index [2][E]) or the reference layout (int32, local ids), gives results bit-identical to flowgnn_set_batch with the same
arrays on the same engine; errors carry the host path's codes; the ingest is ordered on the engine's launch stream."""
import ctypes

import numpy as np
import pytest

from flowgnn_amd import Engine, FlowGNNError, GraphBatch, graphpack as gp, weights

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
ERR_ARG, ERR_EDGE_RANGE, ERR_EDGE_ATTR, ERR_NODE_FEAT = 1, 2, 3, 4
MODELS = ["GIN", "GIN-VN", "GCN", "GAT", "PNA", "DGN"]


def model_weights(model, seed=7, num_tasks=1):
    base = model.replace("-VN", "").lower()
    fn = getattr(weights, f"synth_{base}_weights")
    return fn(seed=seed, num_tasks=num_tasks) if num_tasks != 1 else fn(seed=seed)


def model_batch(model, num_graphs, seed):
    if model == "DGN":
        return gp.synth_hep10k_batch(num_graphs, seed=seed)
    if model == "PNA":
        return gp.synth_hep10k_batch(num_graphs, seed=seed, with_eigen=False)
    b = gp.synth_molpcba_batch(num_graphs, seed=seed) if model == "GCN" else gp.synth_molhiv_batch(num_graphs, seed=seed)
    return gp.add_virtual_nodes(b) if model == "GIN-VN" else b


def has_attr(model):
    return model in ("GIN", "GIN-VN", "GCN")


def device_args(b: GraphBatch, layout: str, model: str):
    """(positional tensors, keyword args) of Engine.set_batch_device for `b` on the GPU."""
    eig = None if b.node_eigen is None or model != "DGN" else torch.from_numpy(b.node_eigen).to(DEV)
    if layout == "pyg":
        d = b.to_pyg(DEV)
        return (d["x"], d["edge_index"], d["edge_attr"] if has_attr(model) else None, eig), {"ptr": d["ptr"]}
    x = torch.from_numpy(np.ascontiguousarray(b.node_feature, dtype=np.int32)).to(DEV)
    el = torch.from_numpy(np.ascontiguousarray(b.edge_list, dtype=np.int32)).to(DEV)
    ea = torch.from_numpy(np.ascontiguousarray(b.edge_attr, dtype=np.int32)).to(DEV) if has_attr(model) else None
    return (x, el, ea, eig), {"ptr": b.node_offsets(), "nums_of_edges": b.nums_of_edges}


def host_results(e: Engine, b: GraphBatch):
    e.set_batch(b)
    e.run()
    return e.results()


def device_results(e: Engine, b: GraphBatch, layout: str, model: str):
    args, kw = device_args(b, layout, model)
    e.set_batch_device(*args, **kw)
    e.run()
    return e.results()


def error_code(fn):
    try:
        fn()
    except FlowGNNError as ex:
        return ex.code
    return 0


@pytest.mark.parametrize("layout", ["pyg", "reference"])
@pytest.mark.parametrize("model", MODELS)
def test_bit_identical_to_host_path(model, layout):
    e = Engine(model, device=0)
    try:
        e.set_weights(model_weights(model))
        for n, seed in ((300, 3), (37, 4)):
            b = model_batch(model, n, seed)
            want = host_results(e, b)
            want_csr = e.csr() if model in ("PNA", "GAT") else None
            got = device_results(e, b, layout, model)
            assert got.shape == want.shape and np.isfinite(got).all()
            assert np.array_equal(got, want), (model, layout, n, np.abs(got - want).max())
            if want_csr is not None:
                for a, c in zip(e.csr(), want_csr):
                    assert np.array_equal(a, c)
    finally:
        e.close()


@pytest.mark.parametrize("layout", ["pyg", "reference"])
def test_large_batch_past_the_packed_host_copy(layout):
    """2^16 molhiv graphs: ~130 MB of int32 arrays, so the host path narrows them on the host (option h2d_pack) and widens them on
    the GPU; the device path ingests the same batch."""
    b = gp.synth_molhiv_batch(1 << 16, seed=21)
    assert 4 * (b.total_nodes * 9 + b.total_edges * 5) >= 8 << 20
    e = Engine("GIN", device=0)
    try:
        e.set_weights(model_weights("GIN"))
        want = host_results(e, b)
        got = device_results(e, b, layout, "GIN")
        assert np.array_equal(got, want), np.abs(got - want).max()
    finally:
        e.close()


@pytest.mark.parametrize("model", ["GIN", "GAT", "PNA", "DGN"])
@pytest.mark.parametrize("layout", ["pyg", "reference"])
def test_tiny_batches_with_an_edgeless_graph(model, layout):
    big = model_batch(model, 3, 9)
    n = 3
    lone = GraphBatch(np.array([n], np.int32), np.array([0], np.int32), np.ones((n, 9), np.int32), np.zeros((0, 2), np.int32),
                      np.zeros((0, 3), np.int32), np.full((n, 4), 0.5, np.float32) if model == "DGN" else None)
    e = Engine(model, device=0)
    try:
        e.set_weights(model_weights(model))
        for b in (big.slice(0, 1), lone, gp.concat_batches([big.slice(0, 1), lone, big.slice(1, 2)])):
            want = host_results(e, b)
            got = device_results(e, b, layout, model)
            assert np.array_equal(got, want, equal_nan=True), (b.num_graphs, np.abs(got - want).max())
    finally:
        e.close()


def test_forward_device_multi_task_gin():
    b = gp.synth_molpcba_batch(500, seed=12)
    e = Engine("GIN", device=0)
    try:
        e.set_num_tasks(128)
        e.set_weights(model_weights("GIN", num_tasks=128))
        want = host_results(e, b)
        d = b.to_pyg(DEV)
        out = e.forward_device(d["x"], d["edge_index"], d["edge_attr"], ptr=d["ptr"])
        assert isinstance(out, torch.Tensor) and out.device == torch.device(DEV) and tuple(out.shape) == (500, 128)
        e.sync()
        assert np.array_equal(out.cpu().numpy(), want)
        # edge counts given instead of derived from edge_index[0]
        out2 = e.forward_device(d["x"], d["edge_index"], d["edge_attr"], ptr=d["ptr"].cpu(), nums_of_edges=b.nums_of_edges)
        e.sync()
        assert np.array_equal(out2.cpu().numpy(), want)
    finally:
        e.close()


def test_errors_carry_the_host_codes_then_a_good_batch_runs():
    good = gp.synth_molhiv_batch(50, seed=31)
    e = Engine("GIN", device=0)
    try:
        e.set_weights(model_weights("GIN"))
        want = host_results(e, good)

        # an endpoint in the NEXT graph (global id = first node of graph 1) -> local id num_nodes[0] on the host path
        d = good.to_pyg(DEV)
        k = 0  # graph 0's first edge
        d["edge_index"][1, k] = int(good.nums_of_nodes[0])
        hb = good.slice(0, good.num_graphs)
        hb.edge_list[k, 1] = good.nums_of_nodes[0]
        assert error_code(lambda: host_results(e, hb)) == ERR_EDGE_RANGE
        e.set_batch_device(d["x"], d["edge_index"], d["edge_attr"], ptr=d["ptr"], nums_of_edges=good.nums_of_edges)
        e.run()
        assert error_code(e.results) == ERR_EDGE_RANGE
        assert error_code(e.sync) == ERR_EDGE_RANGE  # held until the next set_batch
        assert np.array_equal(device_results(e, good, "pyg", "GIN"), want)

        # an int64 node feature that int32 cannot hold -> -1 -> refused as the host path refuses -1
        d = good.to_pyg(DEV)
        d["x"][5, 2] = 2 ** 32 + 1
        hb = good.slice(0, good.num_graphs)
        hb.node_feature[5, 2] = -1
        assert error_code(lambda: host_results(e, hb)) == ERR_NODE_FEAT
        e.set_batch_device(d["x"], d["edge_index"], d["edge_attr"], ptr=d["ptr"])
        e.run()
        assert error_code(e.results) == ERR_NODE_FEAT
        assert np.array_equal(device_results(e, good, "pyg", "GIN"), want)

        # edge attributes outside their table: a representable one and one beyond int32
        for bad in (7, 2 ** 40):
            d = good.to_pyg(DEV)
            d["edge_attr"][3, 0] = bad
            hb = good.slice(0, good.num_graphs)
            hb.edge_attr[3, 0] = bad if bad < 2 ** 31 else -1
            assert error_code(lambda: host_results(e, hb)) == ERR_EDGE_ATTR
            e.set_batch_device(d["x"], d["edge_index"], d["edge_attr"], ptr=d["ptr"])
            e.run()
            assert error_code(e.results) == ERR_EDGE_ATTR
        assert np.array_equal(device_results(e, good, "reference", "GIN"), want)
    finally:
        e.close()


def test_gat_feature_beyond_int32_sets_node_feat():
    good = gp.synth_molhiv_batch(40, seed=32)
    e = Engine("GAT", device=0)
    try:
        e.set_weights(model_weights("GAT"))
        want = host_results(e, good)
        d = good.to_pyg(DEV)
        d["x"][7, 4] = 2 ** 32 + 1
        e.set_batch_device(d["x"], d["edge_index"], None, ptr=d["ptr"])
        e.run()
        assert error_code(e.results) == ERR_NODE_FEAT
        # -1, a valid raw number for GAT, is not an error on either path
        hb = good.slice(0, good.num_graphs)
        hb.node_feature[7, 4] = -1
        d = hb.to_pyg(DEV)
        w1 = host_results(e, hb)
        e.set_batch_device(d["x"], d["edge_index"], None, ptr=d["ptr"])
        e.run()
        assert np.array_equal(e.results(), w1)
        assert np.array_equal(device_results(e, good, "pyg", "GAT"), want)
    finally:
        e.close()


def test_guard_refuses_pinned_host_memory_and_bad_layouts_without_a_launch():
    good = gp.synth_molhiv_batch(30, seed=33)
    e = Engine("GIN", device=0)
    try:
        e.set_weights(model_weights("GIN"))
        want = device_results(e, good, "pyg", "GIN")
        d = good.to_pyg(DEV)
        x_pinned = d["x"].cpu().pin_memory()
        ne, nn = good.nums_of_edges, good.nums_of_nodes
        with pytest.raises(FlowGNNError) as ex:
            e.set_batch_device_ptrs(nn, ne, "pyg", x_pinned.data_ptr(), d["edge_index"].data_ptr(), d["edge_attr"].data_ptr())
        assert ex.value.code == ERR_ARG and "node_feature" in str(ex.value)
        # NULL where the model needs an array; an unknown layout
        with pytest.raises(FlowGNNError) as ex:
            e.set_batch_device_ptrs(nn, ne, "pyg", d["x"].data_ptr(), d["edge_index"].data_ptr(), 0)
        assert ex.value.code == ERR_ARG
        nn_c, ne_c = np.ascontiguousarray(nn, np.int32), np.ascontiguousarray(ne, np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))  # noqa: E731
        rc = e.lib.flowgnn_set_batch_device(e._h, len(nn_c), p(nn_c), p(ne_c), 5, ctypes.c_void_p(d["x"].data_ptr()),
                                            ctypes.c_void_p(d["edge_index"].data_ptr()), ctypes.c_void_p(d["edge_attr"].data_ptr()), None)
        assert rc == ERR_ARG
        # nothing was enqueued and the resident batch is untouched
        e.run()
        assert np.array_equal(e.results(), want)
    finally:
        e.close()


def _stream_order_case(e: Engine, b: GraphBatch, want):
    """Inputs finished by torch work on the current stream right before the call, results consumed by torch work right after,
    one synchronisation at the end."""
    d = b.to_pyg(DEV)
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream()
    x = torch.full_like(d["x"], 77777)           # garbage first ...
    ei = torch.full_like(d["edge_index"], -5)
    torch.cuda._sleep(20_000_000)                # ... a long kernel on the current stream ...
    x.copy_(d["x"])                              # ... then the real values
    ei.copy_(d["edge_index"])
    ea = d["edge_attr"] * 1
    out = e.forward_device(x, ei, ea, ptr=d["ptr"], nums_of_edges=b.nums_of_edges)
    del x, ei, ea                                # the engine recorded them on its stream: torch may recycle them afterwards
    y = out * 2.0
    z = out.clone()
    assert torch.cuda.current_stream() == cur
    torch.cuda.synchronize()
    e.sync()
    assert np.array_equal(z.cpu().numpy(), want)
    assert np.array_equal(y.cpu().numpy(), want * np.float32(2.0))


def test_stream_order_own_and_torch_stream():
    b = gp.synth_molhiv_batch(2000, seed=41)
    e = Engine("GIN", device=0)
    try:
        e.set_weights(model_weights("GIN"))
        want = host_results(e, b)
        _stream_order_case(e, b, want)                       # the engine's own stream
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            e.set_stream(torch.cuda.current_stream().cuda_stream)
            _stream_order_case(e, b, want)                   # torch's current stream
        with torch.cuda.stream(s2):                          # another current stream, the engine still on s1
            _stream_order_case(e, b, want)
        e.set_stream(None)
        torch.cuda.synchronize()
    finally:
        e.close()


def test_hipgraph_replay_then_new_batch_and_reallocation():
    e = Engine("GIN", device=0, options={"hipgraph": 1})
    ref = Engine("GIN", device=0)
    try:
        w = model_weights("GIN")
        e.set_weights(w)
        ref.set_weights(w)
        b1, b2 = gp.synth_molhiv_batch(200, seed=51), gp.synth_molhiv_batch(180, seed=52)
        w1, w2 = host_results(ref, b1), host_results(ref, b2)
        args, kw = device_args(b1, "pyg", "GIN")
        e.set_batch_device(*args, **kw)
        for _ in range(3):
            e.run()
            assert np.array_equal(e.results(), w1)
        assert e.graph_replays() >= 1
        args, kw = device_args(b2, "pyg", "GIN")
        e.set_batch_device(*args, **kw)
        for _ in range(3):
            e.run()
            assert np.array_equal(e.results(), w2)
        # growing, then shrinking batches: the engine's buffers are reallocated under the ingest
        for n, seed in ((100, 53), (3000, 54), (12000, 55), (40, 56), (5000, 57)):
            b = gp.synth_molhiv_batch(n, seed=seed)
            want = host_results(ref, b)
            for layout in ("pyg", "reference"):
                assert np.array_equal(device_results(e, b, layout, "GIN"), want), (n, layout)
    finally:
        e.close()
        ref.close()


def test_profiler_reports_the_ingest():
    b = gp.synth_molhiv_batch(300, seed=61)
    e = Engine("GIN", device=0)
    try:
        e.set_weights(model_weights("GIN"))
        e.profile_enable(True)
        device_results(e, b, "pyg", "GIN")
        prof = e.profile_read()
        assert "ingest" in prof and prof["ingest"]["launches"] == 1 and prof["ingest"]["total_ms"] > 0
    finally:
        e.close()
