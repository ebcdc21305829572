"""The NumPy restatements of OGB, the exporter and the float64 reference forwards against an executable torch.nn model of OGB
(tests/ogb_torch.py).  No GPU.

What is compared with what, and the bound of each comparison:
  * the seven NumPy "OGB sides" of the suite, on the torch model's own state_dict(): both are float64 and differ by summation order
    only, so |a - b| <= 1e-9 * scale -- five orders above the rounding of a 600-term float64 sum, six or more below any semantic
    difference (those move the logits by 1e-3 of the scale or more);
  * export_weights -> .bin files -> weights.load_* -> the repository's float64 reference forwards: tests/parity.py's rule,
    |a - b| <= 1e-4 * (scale + |b|), the bound the GPU tests use; what is left is the float32 rounding of the files and the BatchNorm
    folds.  scale is each time the torch model's hooked scale (ogb_torch.run).
"""
import os
from collections.abc import Mapping

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from flowgnn_amd import export, graphpack as gp, weights  # noqa: E402
from tests import (gcn_vn_ref, gcn_wide_ref, gcn_wide_vn_ref, gin_wide_ref, gin_wide_vn_ref, numpy_ref, ogb_torch as T,  # noqa: E402
                   ogb_vn_ref, test_export)
from tests.parity import REL, assert_close, err_ratio  # noqa: E402

KINDS = [("gin", False), ("gin", True), ("gcn", False), ("gcn", True)]
MODELS = [(k, vn, d) for k, vn in KINDS for d in (100, 300)]
POOLINGS = ("mean", "sum", "max")
IDS = [f"{k}{'-virtual' if vn else ''}-{d}" for k, vn, d in MODELS]
HALF_THRESHOLD, THRESHOLD = 3.0e4, 6.0e4  # the split-f16 kernels hand a pass to the fp32 pipe at 6e4 (dense_split.h)
SAME = 1e-9


def same(got, want, scale, what):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    print(what, f"max |restatement - torch| = {err:.3e}, {err / (SAME * scale):.3e} x the bound (scale {scale:.4g})")
    assert np.asarray(got).shape == np.asarray(want).shape and err <= SAME * scale, (what, err, scale)


# ---------------------------------------------------------------- 1. the model is what the issue of a checkpoint looks like
@pytest.mark.parametrize("kind,vn,dim", MODELS, ids=IDS)
def test_state_dict_has_ogbs_keys_and_shapes_and_looks_trained(kind, vn, dim):
    model = T.make_model(kind, vn, dim)
    sd = model.state_dict()
    want = [f"gnn_node.atom_encoder.atom_embedding_list.{i}.weight" for i in range(9)]
    bn = lambda p: [f"{p}.{s}" for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    lin = lambda p: [f"{p}.weight", f"{p}.bias"]
    for l in range(5):
        c = f"gnn_node.convs.{l}"
        want += [f"{c}.bond_encoder.bond_embedding_list.{i}.weight" for i in range(3)]
        want += (lin(f"{c}.mlp.0") + bn(f"{c}.mlp.1") + lin(f"{c}.mlp.3") + [f"{c}.eps"]) if kind == "gin" else (lin(f"{c}.linear") + [f"{c}.root_emb.weight"])
        want += bn(f"gnn_node.batch_norms.{l}")
    if vn:
        want.append("gnn_node.virtualnode_embedding.weight")
        for l in range(4):
            m = f"gnn_node.mlp_virtualnode_list.{l}"
            want += lin(f"{m}.0") + bn(f"{m}.1") + lin(f"{m}.3") + bn(f"{m}.4")
    want += lin("graph_pred_linear")
    assert sorted(sd) == sorted(want)
    assert all(v.dtype == torch.float64 for k, v in sd.items() if not k.endswith("num_batches_tracked"))
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert v.dtype == torch.int64 and v.dim() == 0 and int(v) > 0, k
        if k.endswith(".eps"):
            assert tuple(v.shape) == (1,) and abs(float(v)) >= 0.05, (k, v)
        if k.endswith("root_emb.weight") or k.endswith("virtualnode_embedding.weight"):
            assert tuple(v.shape) == (1, dim), k
        if k.endswith("running_mean"):
            assert float(v.abs().mean()) > 0.02, (k, float(v.abs().mean()))  # (the tensor as a whole is away from 0 ...)
        if k.endswith("running_var"):
            assert float((v - 1).abs().mean()) > 0.1 and float(v.min()) > 0, (k, float((v - 1).abs().mean()))  # (... and from 1)
    if vn:
        assert float(sd["gnn_node.virtualnode_embedding.weight"].abs().min()) > 0
    assert tuple(sd["gnn_node.convs.0.bond_encoder.bond_embedding_list.1.weight"].shape) == (6, dim)
    assert not model.training


# ---------------------------------------------------------------- 2. the seven NumPy restatements
def _restatements(kind, vn, dim):
    """[(name, callable(sd, batch) -> logits)] that claim to be this model."""
    if kind == "gin" and not vn:
        out = [("gin_wide_ref.ogb_forward", gin_wide_ref.ogb_forward)]
    elif kind == "gcn" and not vn:
        out = [("gcn_wide_ref.ogb_forward", gcn_wide_ref.ogb_forward)]
    elif kind == "gin":
        out = [("gin_wide_vn_ref.ogb_forward", gin_wide_vn_ref.ogb_forward)] + ([("ogb_vn_ref.ogb_vn_forward", ogb_vn_ref.ogb_vn_forward)] if dim == 100 else [])
    else:
        out = [("gcn_wide_vn_ref.ogb_forward", gcn_wide_vn_ref.ogb_forward)] + ([("gcn_vn_ref.ogb_vn_forward", gcn_vn_ref.ogb_vn_forward)] if dim == 100 else [])
    if not vn and dim == 100:
        out.append(("test_export.ogb_forward", lambda sd, b: test_export.ogb_forward(kind, sd, b)))
    return out


def test_every_restatement_is_covered():
    names = {n for k, vn, d in MODELS for n, _ in _restatements(k, vn, d)}
    assert names == {"test_export.ogb_forward", "gin_wide_ref.ogb_forward", "gcn_wide_ref.ogb_forward", "gin_wide_vn_ref.ogb_forward",
                     "gcn_wide_vn_ref.ogb_forward", "ogb_vn_ref.ogb_vn_forward", "gcn_vn_ref.ogb_vn_forward"}


@pytest.mark.parametrize("kind,vn,dim", MODELS, ids=IDS)
@pytest.mark.parametrize("tasks", [1, 3])
def test_numpy_restatements_agree_with_the_torch_model(kind, vn, dim, tasks):
    """The restatements return the logits of the mean readout (none returns rows), for one task or several."""
    model = T.make_model(kind, vn, dim, num_tasks=tasks)
    out, scale, _ = T.expected(kind, vn, dim, num_tasks=tasks)
    sd, b = T.numpy_state_dict(model), T.batch_of(kind)
    for name, fn in _restatements(kind, vn, dim):
        same(fn(sd, b), out.logits, scale, (IDS[MODELS.index((kind, vn, dim))], tasks, name))


# ---------------------------------------------------------------- 3. key coverage
class Recording(Mapping):
    """A state_dict that remembers which entries were read (`in` does not read)."""

    def __init__(self, sd):
        self.sd, self.read = sd, set()

    def __getitem__(self, k):
        self.read.add(k)
        return self.sd[k]

    def __contains__(self, k):
        return k in self.sd

    def __iter__(self):
        return iter(self.sd)

    def __len__(self):
        return len(self.sd)


def export_kwargs(kind, vn, dim, tasks=1):
    kw = dict(multi_task=tasks != 1)
    if kind == "gin":
        kw["keep_eps"] = True
    else:
        kw["emb_dim"] = dim
    if vn:
        kw.update(virtual_node=True, virtual_node_dim=dim)
    return kw


@pytest.mark.parametrize("kind,vn,dim", MODELS, ids=IDS)
def test_the_exporter_reads_every_key_but_the_batch_counters(kind, vn, dim, tmp_path):
    rec = Recording(T.make_model(kind, vn, dim).state_dict())
    export.export_weights(kind.upper(), rec, str(tmp_path), **export_kwargs(kind, vn, dim))
    unread = set(rec.sd) - rec.read
    assert unread == {k for k in rec.sd if k.endswith("num_batches_tracked")}, sorted(unread)


# ---------------------------------------------------------------- 4. export round trip
def round_trip(kind, vn, dim, directory, batch, pooling="mean", tasks=1):
    """{forward's name: (logits, rows or None, pooled or None)} of the repository's float64 reference forwards on the files of `directory`."""
    out = {}
    if kind == "gin":
        w, eps = weights.load_gin_weights(directory, num_tasks=tasks, emb_dim=dim), weights.load_gin_eps(directory, emb_dim=dim)
        if vn:
            v = weights.load_gin_virtual_node(directory, emb_dim=dim)
            r = gin_wide_vn_ref.forward(batch, w, v, eps=eps, pooling=pooling, num_tasks=tasks)
            out["gin_wide_vn_ref.forward"] = (r.logits, r.rows, r.pooled)
            if dim == 100:
                logits, rows, _ = ogb_vn_ref.forward(batch, w, v, eps=eps, pooling=pooling, num_tasks=tasks)
                out["ogb_vn_ref.forward"] = (logits, rows, None)
        else:
            r = gin_wide_ref.forward(batch, w, eps=eps, pooling=pooling, num_tasks=tasks)
            out["gin_wide_ref.forward"] = (r.logits, r.rows, r.pooled)
    else:
        w = weights.load_gcn_weights(directory, num_tasks=tasks, emb_dim=dim)
        if vn:
            v = weights.load_gcn_virtual_node(directory, emb_dim=dim)
            r = gcn_wide_vn_ref.forward(batch, w, v, pooling=pooling, num_tasks=tasks)
            out["gcn_wide_vn_ref.forward"] = (r.logits, r.rows, r.pooled)
            if dim == 100:
                logits, rows, _ = gcn_vn_ref.forward(batch, w, v, pooling=pooling, num_tasks=tasks)
                out["gcn_vn_ref.forward"] = (logits, rows, None)
        else:
            r = gcn_wide_ref.forward(batch, w, pooling=pooling, num_tasks=tasks)
            out["gcn_wide_ref.forward"] = (r.logits, r.rows, r.pooled)
            if dim == 100 and pooling == "mean":
                out["numpy_ref.gcn_forward"] = (numpy_ref.gcn_forward(batch, w), None, None)
    return out


@pytest.mark.parametrize("kind,vn,dim", MODELS, ids=IDS)
def test_export_round_trip_stays_inside_the_gpu_tests_bound(kind, vn, dim, tmp_path):
    """state_dict() -> export_weights -> .bin -> weights.load_* -> the float64 reference forwards, for the three readouts: float32 files
    and the BatchNorm folds alone stay inside tests/parity.py's bound, with the torch model's values and scale."""
    worst, scales = 0.0, []
    b = T.batch_of(kind)
    for pooling in POOLINGS:
        model = T.make_model(kind, vn, dim, pooling=pooling)
        want, scale, _ = T.expected(kind, vn, dim, pooling=pooling)
        d = str(tmp_path / pooling)
        export.export_weights(kind.upper(), model.state_dict(), d, **export_kwargs(kind, vn, dim))
        for name, (logits, rows, pooled) in round_trip(kind, vn, dim, d, b, pooling=pooling).items():
            for what, got, ref in (("logits", logits, want.logits), ("rows", rows, want.rows), ("pooled", pooled, want.pooled)):
                if got is not None:
                    worst = max(worst, err_ratio(got, ref, scale))
                    assert_close(got, ref, scale=scale, what=(name, pooling, what))
        scales.append(scale)
    print(f"{IDS[MODELS.index((kind, vn, dim))]}: scale {max(scales):.4g}, worst round-trip ratio {worst:.4f}")


@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_export_round_trip_multi_task(kind, tmp_path):
    for vn in (False, True):
        model = T.make_model(kind, vn, 300, num_tasks=128)
        want, scale, _ = T.expected(kind, vn, 300, num_tasks=128)
        d = str(tmp_path / str(vn))
        export.export_weights(kind.upper(), model.state_dict(), d, **export_kwargs(kind, vn, 300, tasks=128))
        for name, (logits, _, _) in round_trip(kind, vn, 300, d, T.batch_of(kind), tasks=128).items():
            assert logits.shape == (T.batch_of(kind).num_graphs, 128)
            print(kind, vn, name, f"128 tasks: ratio {err_ratio(logits, want.logits, scale):.4f}")
            assert_close(logits, want.logits, scale=scale, what=(name, "128 tasks"))


def test_export_round_trip_through_the_references_own_gin_file_set(tmp_path):
    """numpy_ref.gin_forward restates the reference's GIN, which has no eps: the one model it can hold is the torch model with eps = 0,
    exported without keep_eps."""
    model = T.make_model("gin", False, 100, zero_eps=True)
    want, scale, _ = T.run(model, T.gin_batch())
    export.export_weights("GIN", model.state_dict(), str(tmp_path))
    got = numpy_ref.gin_forward(T.gin_batch(), weights.load_gin_weights(str(tmp_path)))
    print(f"gin-100, eps = 0, numpy_ref.gin_forward: ratio {err_ratio(got, want.logits, scale):.4f}")
    assert_close(got, want.logits, scale=scale, what="numpy_ref.gin_forward")


# ---------------------------------------------------------------- 5. range
def kernel_operands(kind, vn, dim, directory, batch, tasks=1):
    """The largest operand the split-f16 kernels' range guards watch, from the exported files and the repository's float64 forwards
    alone (gin_wide_vn_ref.split_operands, gcn_wide_vn_ref.forward's `operands`).  Not what the hooks see: the kernels keep a hidden
    layer multiplied by its first matrix's power-of-two pre-scale 2^-ilogb(max |W1|), and a BatchNorm folded into W1 makes that matrix
    as small as the sums it normalises are large -- in the virtual node's update the guarded value is hundreds of times the hidden unit."""
    if kind == "gin":
        w, eps = weights.load_gin_weights(directory, num_tasks=tasks, emb_dim=dim), weights.load_gin_eps(directory, emb_dim=dim)
        v = weights.load_gin_virtual_node(directory, emb_dim=dim) if vn else gin_wide_vn_ref.zero_virtual_node(dim)
        node, update = gin_wide_vn_ref.split_operands(batch, w, v, eps=eps, num_tasks=tasks)
        return max(node, update) if vn else node
    w = weights.load_gcn_weights(directory, num_tasks=tasks, emb_dim=dim)
    if not vn:
        return gcn_wide_ref.max_a(batch, w)
    return gcn_wide_vn_ref.forward(batch, w, weights.load_gcn_virtual_node(directory, emb_dim=dim), num_tasks=tasks).operands


@pytest.mark.parametrize("kind,vn,dim", MODELS, ids=IDS)
def test_the_models_stay_in_the_fast_paths_range(kind, vn, dim, tmp_path):
    """A condition, not a measurement: every magnitude the hooks see (aggregates, hidden units, rows, the pooled t) is below half the
    threshold at which a split-f16 kernel hands its pass to the fp32 pipe, for every model and readout the GPU tests run -- and so is
    every operand the kernels' own guards watch (kernel_operands)."""
    for tasks, pooling in [(1, p) for p in POOLINGS] + ([(128, "mean")] if dim == 300 else []):
        scale = T.expected(kind, vn, dim, num_tasks=tasks, pooling=pooling)[1]
        print(f"{IDS[MODELS.index((kind, vn, dim))]} {pooling} {tasks} task(s): scale {scale:.4g}")
        assert scale < HALF_THRESHOLD, (pooling, tasks, scale)
    for tasks in (1, 128) if dim == 300 else (1,):  # (the readout's pooling is behind every guarded operand)
        d = str(tmp_path / str(tasks))
        export.export_weights(kind.upper(), T.make_model(kind, vn, dim, num_tasks=tasks).state_dict(), d, **export_kwargs(kind, vn, dim, tasks=tasks))
        ops = kernel_operands(kind, vn, dim, d, T.batch_of(kind), tasks=tasks)
        print(f"{IDS[MODELS.index((kind, vn, dim))]} {tasks} task(s): largest guarded operand {ops:.4g}")
        assert ops < HALF_THRESHOLD, (tasks, ops)


@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_the_undamped_models_leave_it(kind, tmp_path):
    """The fallback cases of tests/test_ogb_torch_gpu.py: the same recipe without the settling passes.  The hooked scale, the pooled t
    and the kernels' guarded operands all pass the threshold."""
    model = T.make_model(kind, True, 300, damped=False)
    out, scale, _ = T.expected(kind, True, 300, damped=False)
    seen = []
    h = model.gnn_node.pool.register_forward_hook(lambda _m, _i, o: seen.append(float(o.abs().max())))
    try:
        T.run(model, T.batch_of(kind))
    finally:
        h.remove()
    export.export_weights(kind.upper(), model.state_dict(), str(tmp_path), **export_kwargs(kind, True, 300))
    ops = kernel_operands(kind, True, 300, str(tmp_path), T.batch_of(kind))
    print(f"{kind}-virtual-300 undamped: scale {scale:.4g}, largest |t| {max(seen):.4g}, largest guarded operand {ops:.4g}")
    assert scale > THRESHOLD and max(seen) > 1.1 * THRESHOLD and ops > 1.1 * THRESHOLD and np.isfinite(out.logits).all()


# ---------------------------------------------------------------- 6. mutation: the batch tells the wrong forms from the definition
@pytest.mark.parametrize("kind", ["gin", "gcn"])
@pytest.mark.parametrize("dim", [100, 300])
@pytest.mark.parametrize("variant", T.VARIANTS)
def test_wrong_forms_of_the_virtual_node_miss_the_bound(kind, dim, variant):
    assert variant in ogb_vn_ref.VARIANTS
    want, scale, _ = T.expected(kind, True, dim)
    got, _, _ = T.run(T.with_variant(T.make_model(kind, True, dim), variant), T.batch_of(kind))
    ratios = {n: err_ratio(getattr(got, n), getattr(want, n), scale) for n in ("logits", "rows", "pooled")}
    print(kind, dim, variant, {n: f"{r:.3g}" for n, r in ratios.items()})
    assert max(ratios.values()) > 1.0, ratios


# ---------------------------------------------------------------- 7. the engine's GCN is OGB's only where both directions are listed
def test_gcn_differs_from_ogb_on_a_one_directional_edge(tmp_path):
    """The engine follows the reference: dinv = 0 at out-degree 0, so a message INTO a node without out-edges is dropped.  OGB's GCNConv
    takes deg^-1/2 of out-degree + 1 and delivers it.  The two agree on batches that list both directions of every edge (every OGB
    molecule dataset does); include/flowgnn.h and INTEGRATION.md state the limit."""
    model = T.make_model("gcn", False, 100)
    export.export_weights("GCN", model.state_dict(), str(tmp_path))
    w = weights.load_gcn_weights(str(tmp_path))
    one_way = T._graph(3, [(0, 1)], 7)
    both = gp.GraphBatch(one_way.nums_of_nodes, np.array([2], np.int32), one_way.node_feature, np.array([[0, 1], [1, 0]], np.int32),
                         np.concatenate([one_way.edge_attr, one_way.edge_attr]))
    for b, agree in ((one_way, False), (both, True)):
        want, scale, _ = T.run(model, b)
        r = err_ratio(numpy_ref.gcn_forward(b, w), want.logits, scale)
        print("one direction" if not agree else "both directions", f"ratio {r:.4g} (scale {scale:.4g})")
        assert (r <= 1.0) == agree, (agree, r)
