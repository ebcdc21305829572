"""OGB checkpoints on the GPU against an executable torch.nn model of OGB (tests/ogb_torch.py): gin, gin-virtual, gcn and gcn-virtual at
emb_dim 100 and 300, through the route a user takes -- model.state_dict() -> export_weights -> .bin files -> Engine.load_weights_dir ->
kernels.

Expected values: the torch model's own float64 forward, nothing restated.  Tolerance: the project's rule and nothing else,
|gpu - torch| <= REL (scale + |torch|), REL = 1e-4, scale = the largest magnitude the torch model's forward hooks saw (tests/parity.py;
tests/test_ogb_torch_cpu.py shows that the float32 files and the BatchNorm folds alone use under 2 % of it).  Every comparison prints
its ratio to the bound.  tests/test_ogb_torch_cpu.py asserts that every model here but the two fallback ones stays below half the
split-f16 kernels' range threshold, so `exact_reruns() == 0` is asserted wherever the fast path is what is under test."""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from flowgnn_amd import Engine, export, graphpack as gp  # noqa: E402
from tests import ogb_torch as T  # noqa: E402
from tests.parity import assert_close, err_ratio  # noqa: E402
from tests.test_embeddings_gpu import launched  # noqa: E402
from tests.test_ogb_torch_cpu import export_kwargs  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
KINDS = [("gin", False), ("gin", True), ("gcn", False), ("gcn", True)]
name_of = lambda kind, vn, dim: f"{kind}{'-virtual' if vn else ''}-{dim}"


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    if torch.cuda.is_available():
        torch.cuda.init()


def close(got, want, scale, what):
    print(what, f"err_ratio {err_ratio(got, want, scale):.4f} (scale {scale:.4g})")
    assert_close(got, want, scale=scale, what=what)


def exported(kind, vn, dim, directory, tasks=1, damped=True):
    """make_model(...).state_dict() -> export_weights into `directory`."""
    model = T.make_model(kind, vn, dim, num_tasks=tasks, damped=damped)
    export.export_weights(kind.upper(), model.state_dict(), str(directory), **export_kwargs(kind, vn, dim, tasks=tasks))
    return str(directory)


def engine(kind, vn, dim, directory, tasks=1, pooling="mean", options=None):
    """The width first, then the files: Engine.load_weights_dir(dir, eps=..., virtual_node=...)."""
    e = Engine(kind.upper(), device=0, options=options or {})
    if kind == "gin":
        e.set_emb_dim(dim)
    else:
        e.set_model_emb_dim(dim)
    if tasks != 1:
        e.set_num_tasks(tasks)
    e.load_weights_dir(directory, eps=kind == "gin", virtual_node=vn)
    if pooling != "mean":
        e.set_pooling(pooling)
    assert e.emb_dim == dim
    return e


def check_all(e, kind, want, scale, what):
    """Logits, node rows and pooled vectors of one forward of the host batch against the torch model."""
    logits, pooled, rows = (np.array(x) for x in e.forward(T.batch_of(kind), return_embeddings=True, return_node_embeddings=True))
    close(rows, want.rows, scale, (what, "rows"))
    close(pooled, want.pooled, scale, (what, "pooled"))
    close(logits, want.logits, scale, (what, "logits"))


# ---------------------------------------------------------------- 1. checkpoint parity
@pytest.mark.parametrize("pooling", ["mean", "sum", "max"])
@pytest.mark.parametrize("dim", [100, 300])
@pytest.mark.parametrize("kind,vn", KINDS, ids=[name_of(k, v, "")[:-1] for k, v in KINDS])
def test_checkpoint_parity(kind, vn, dim, pooling, tmp_path):
    want, scale, _ = T.expected(kind, vn, dim, pooling=pooling)
    e = engine(kind, vn, dim, exported(kind, vn, dim, tmp_path), pooling=pooling)
    try:
        check_all(e, kind, want, scale, (name_of(kind, vn, dim), pooling))
        print(name_of(kind, vn, dim), pooling, "exact_reruns", e.exact_reruns())
        assert e.exact_reruns() == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 2. both kernel families at width 100
@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_resident_and_per_layer_kernels_at_width_100(kind, tmp_path):
    """The same files on the graph-resident kernel (the default for this batch) and on the per-layer kernels.  GIN's resident kernel
    applies a trained eps in its folded mean-pooling instances, which produce the logits alone; every other run gives all three outputs."""
    want, scale, _ = T.expected(kind, False, 100)
    d = exported(kind, False, 100, tmp_path)
    slot = f"{kind}_resident"
    for options in ({}, {slot: 0}):
        e = engine(kind, False, 100, d, options=options)
        e.profile_enable(True)
        try:
            res = {}
            names = launched(e, lambda: res.update(logits=np.array(e.forward(T.batch_of(kind)))))
            assert (slot in names) == (not options), (options, names)
            close(res["logits"], want.logits, scale, (name_of(kind, False, 100), options or "resident", "logits"))
            if options or kind == "gcn":
                check_all(e, kind, want, scale, (name_of(kind, False, 100), options or "resident"))
            assert e.exact_reruns() == 0
        finally:
            e.close()


# ---------------------------------------------------------------- 3. multi-task heads
@pytest.mark.parametrize("kind,vn", KINDS, ids=[name_of(k, v, "")[:-1] for k, v in KINDS])
def test_multi_task_300(kind, vn, tmp_path):
    want, scale, _ = T.expected(kind, vn, 300, num_tasks=128)
    e = engine(kind, vn, 300, exported(kind, vn, 300, tmp_path, tasks=128), tasks=128)
    try:
        assert want.logits.shape == (T.batch_of(kind).num_graphs, 128)
        check_all(e, kind, want, scale, (name_of(kind, vn, 300), "128 tasks"))
        assert e.exact_reruns() == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 4. device batches
@pytest.mark.parametrize("kind,vn", KINDS, ids=[name_of(k, v, "")[:-1] for k, v in KINDS])
def test_device_batch_300(kind, vn, tmp_path):
    """forward_device on the very tensors the torch model consumed, moved to the GPU as int64 (a PyG Batch's x, edge_index, edge_attr, ptr)."""
    want, scale, (x, edge_index, edge_attr, ptr) = T.expected(kind, vn, 300)
    assert all(t.dtype == torch.int64 for t in (x, edge_index, edge_attr, ptr))
    e = engine(kind, vn, 300, exported(kind, vn, 300, tmp_path))
    try:
        dev = torch.device("cuda", 0)
        logits, pooled, rows = e.forward_device(x.to(dev), edge_index.to(dev), edge_attr.to(dev), ptr=ptr.to(dev), return_embeddings=True,
                                                return_node_embeddings=True)
        e.sync()
        what = (name_of(kind, vn, 300), "forward_device")
        close(rows.cpu().numpy(), want.rows, scale, (what, "rows"))
        close(pooled.cpu().numpy(), want.pooled, scale, (what, "pooled"))
        close(logits.cpu().numpy(), want.logits, scale, (what, "logits"))
        assert e.exact_reruns() == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 5. out of the fast path's range
@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_fallback_300(kind, tmp_path):
    """The undamped model (tests/test_ogb_torch_cpu.py asserts that its pooled t passes 6e4): the pass is repeated on the fp32 pipe and
    lands inside the same bound."""
    want, scale, _ = T.expected(kind, True, 300, damped=False)
    assert scale > 6.0e4
    e = engine(kind, True, 300, exported(kind, True, 300, tmp_path, damped=False))
    try:
        check_all(e, kind, want, scale, (name_of(kind, True, 300), "undamped"))
        print(name_of(kind, True, 300), "undamped: exact_reruns", e.exact_reruns())
        assert e.exact_reruns() >= 1
    finally:
        e.close()


# ---------------------------------------------------------------- 6. the host CLI
@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_host_cli_300_ogb_vn(kind, tmp_path):
    """`host GIN --emb-dim 300 --eps --ogb-vn` / `host GCN --emb-dim 300 --ogb-vn` on a written pack and the exported directory."""
    want, scale, _ = T.expected(kind, True, 300)
    gdir, wdir, out = tmp_path / "graphs", tmp_path / "weights", tmp_path / "HLS_output.txt"
    gp.write_pack(T.batch_of(kind), str(gdir))
    exported(kind, True, 300, wdir)
    flags = ["--eps", "--ogb-vn"] if kind == "gin" else ["--ogb-vn"]
    p = subprocess.run([HOST, kind.upper(), "--emb-dim", "300"] + flags + ["--graphs", str(gdir), "--weights", str(wdir), "--trials", "1",
                       "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    close(got, want.logits, scale, (name_of(kind, True, 300), "host CLI"))
