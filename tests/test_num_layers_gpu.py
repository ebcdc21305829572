"""OGB's num_layer at width 300 on the GPU (flowgnn.h: flowgnn_set_num_layers), through the route a user takes:
GNN(num_layer=L).state_dict() -> export_weights -> .bin files -> Engine.set_num_layers -> load_weights_dir -> forward.

Expected values: the float64 forward of the torch models of tests/ogb_layers.py, nothing restated.  Tolerance: tests/parity.py's rule,
|gpu - torch| <= REL (scale + |torch|), REL = 1e-4, scale = what the torch forward hooks saw; tests/test_num_layers_cpu.py asserts that
every model here stays under half the split-f16 kernels' range threshold -- so exact_reruns() == 0 is asserted -- and that a wrong depth
misses the rows by more than this bound.  Every test here needs the new call and fails on a tree without it."""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from flowgnn_amd import Engine, EngineGroup, export, graphpack as gp, weights  # noqa: E402
from tests import attn_pool_ref, ogb_layers as OL, ogb_torch as T  # noqa: E402
from tests.parity import assert_close, err_ratio  # noqa: E402
from tests.test_ogb_torch_cpu import export_kwargs  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
D = 300
F16_REL = 2e-4  # the rule GIN's f16 test at this width asserts on the logits (tests/test_gin_wide_f16_gpu.py)
CASES = [(k, vn, L) for k, vn in OL.KINDS for L in (2, 3, 6)] + [(k, False, 8) for k in ("gin", "gcn")]
IDS = [OL.name_of(*c) for c in CASES]
JK_CASES = [(k, vn, L) for k, vn in OL.KINDS for L in (2, 3, 6)]


@pytest.fixture(scope="module", autouse=True)
def torch_context_first():
    """torch's HIP context before the first engine exists (tests/test_embeddings_gpu.py says why)."""
    if torch.cuda.is_available():
        torch.cuda.init()


def close(got, want, scale, what, rel=1e-4):
    print(what, f"err_ratio {err_ratio(got, want, scale, rel):.4f} (scale {scale:.4g})")
    assert_close(got, want, scale=scale, rel=rel, what=what)


def exported(kind, vn, L, directory, jk="last", residual=False):
    model = OL.make_model(kind, vn, L, jk, residual)
    export.export_weights(kind.upper(), model.state_dict(), str(directory), **export_kwargs(kind, vn, D))
    return str(directory)


def configure(e, kind, vn, L, directory):
    """The width, the depth, then the files."""
    (e.set_emb_dim if kind == "gin" else e.set_model_emb_dim)(D)
    e.set_num_layers(L)
    assert e.num_layers == L and e.emb_dim == D
    if isinstance(e, Engine):
        e.load_weights_dir(directory, eps=kind == "gin", virtual_node=vn)
    return e


def engine(kind, vn, L, directory):
    return configure(Engine(kind.upper(), device=0), kind, vn, L, directory)


def check_all(e, kind, want, scale, what):
    logits, pooled, rows = (np.array(x) for x in e.forward(T.batch_of(kind), return_embeddings=True, return_node_embeddings=True))
    close(rows, want.rows, scale, (what, "rows"))
    close(pooled, want.pooled, scale, (what, "pooled"))
    close(logits, want.logits, scale, (what, "logits"))


# ---------------------------------------------------------------- 1. parity at every depth, both branches of the last layer's buffer choice
@pytest.mark.parametrize("kind,vn,L", CASES, ids=IDS)
def test_depth_parity(kind, vn, L, tmp_path):
    want, scale, _ = OL.expected(kind, vn, L)
    e = engine(kind, vn, L, exported(kind, vn, L, tmp_path))
    try:
        what = OL.name_of(kind, vn, L)
        check_all(e, kind, want, scale, what)  # node embeddings on: the last layer writes into the caller's buffer
        e.set_node_embeddings(False)            # ... and off: into the ping-pong buffer, whose parity follows L
        logits, pooled = (np.array(x) for x in e.forward(T.batch_of(kind), return_embeddings=True))
        close(pooled, want.pooled, scale, (what, "pooled, node embeddings off"))
        close(logits, want.logits, scale, (what, "logits, node embeddings off"))
        h = np.array(e.final_h()).reshape(-1, D)  # flowgnn_get_h: h_L
        close(h, want.rows, scale, (what, "get_h"))
        assert e.exact_reruns() == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 2. JK sum + residual: L + 1 terms
@pytest.mark.parametrize("kind,vn,L", JK_CASES, ids=[OL.name_of(*c) for c in JK_CASES])
def test_jk_sum_and_residual(kind, vn, L, tmp_path):
    want, scale, _ = OL.expected(kind, vn, L, "sum", True)
    e = engine(kind, vn, L, exported(kind, vn, L, tmp_path, "sum", True))
    try:
        e.set_jk_residual("sum", True)
        check_all(e, kind, want, scale, (OL.name_of(kind, vn, L), "JK sum + residual"))
        assert e.exact_reruns() == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 3. GIN's f16 mode
@pytest.mark.parametrize("vn", [False, True])
@pytest.mark.parametrize("L", [2, 6])
def test_gin_f16_mode(vn, L, tmp_path):
    want, scale, _ = OL.expected("gin", vn, L)
    e = engine("gin", vn, L, exported("gin", vn, L, tmp_path))
    try:
        e.set_numeric_mode("f16", emb_dim=D)
        logits = np.array(e.forward(T.batch_of("gin")))
        close(logits, want.logits, scale, (OL.name_of("gin", vn, L), "f16 logits"), rel=F16_REL)
        assert e.exact_reruns() == 0
    finally:
        e.close()


@pytest.mark.parametrize("vn", [False, True])
@pytest.mark.parametrize("L", [2, 6])
def test_gcn_f16_mode(vn, L, tmp_path):
    """The rule tests/test_gcn_wide_f16_gpu.py asserts on the logits: REL = 1e-4, the project's own."""
    want, scale, _ = OL.expected("gcn", vn, L)
    e = engine("gcn", vn, L, exported("gcn", vn, L, tmp_path))
    try:
        f32 = np.array(e.forward(T.batch_of("gcn")))
        e.set_numeric_mode("f16", emb_dim=D)
        logits = np.array(e.forward(T.batch_of("gcn")))
        close(logits, want.logits, scale, (OL.name_of("gcn", vn, L), "f16 logits"), rel=1e-4)
        assert np.mean(logits != f32) > 0.5  # the mode is engaged
        assert e.exact_reruns() == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 3b. the exact fp32 re-run at L = 3
@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_exact_rerun_at_depth_3(kind, tmp_path):
    """tests/ogb_layers.out_of_range_model: update 0 pushed past 6e4 the way tests/test_gin_wide_vn_gpu.py (the update's hidden layer) and
    tests/test_gcn_wide_vn_gpu.py (a component of vn_1) push theirs.  The pass is repeated once on the fp32 path -- L launches of the
    *_layer_f32 slot, the exact update and, for gcn, the exact pool under feeds_update -- and lands inside the same bound."""
    L = 3
    want, scale, _ = OL.out_of_range_expected(kind, L)
    assert scale > 6.6e4 and OL.expected(kind, True, L)[1] < 3.0e4, scale
    export.export_weights(kind.upper(), OL.out_of_range_model(kind, L).state_dict(), str(tmp_path), **export_kwargs(kind, True, D))
    e = engine(kind, True, L, str(tmp_path))
    try:
        e.profile_enable(True)
        before = {k: v["launches"] for k, v in e.profile_read().items()}
        logits, pooled, rows = (np.array(x) for x in e.forward(T.batch_of(kind), return_embeddings=True, return_node_embeddings=True))
        e.sync()
        n = {k: v["launches"] - before.get(k, 0) for k, v in e.profile_read().items()}
        print(kind, {k: v for k, v in n.items() if v}, "exact_reruns", e.exact_reruns())
        assert e.exact_reruns() == 1
        assert n.get(f"{kind}_wide_layer_f32", 0) == L and n.get(f"{kind}_wide_layer", 0) == L, n  # the fast pass, then the exact one
        assert n.get(f"{kind}_wide_vn_update", 0) == 2 * (L - 1), n
        what = (OL.name_of(kind, True, L), "exact re-run")
        close(rows, want.rows, scale, (what, "rows"))
        close(pooled, want.pooled, scale, (what, "pooled"))
        close(logits, want.logits, scale, (what, "logits"))
        e.set_node_embeddings(False)  # the other branch of the last layer's buffer choice, on the exact path (the batch stays on it)
        logits2, pooled2 = (np.array(x) for x in e.forward(T.batch_of(kind), return_embeddings=True))
        close(pooled2, want.pooled, scale, (what, "pooled, node embeddings off"))
        close(logits2, want.logits, scale, (what, "logits, node embeddings off"))
        close(np.array(e.final_h()).reshape(-1, D), want.rows, scale, (what, "get_h"))
    finally:
        e.close()


# ---------------------------------------------------------------- 4. the depth really runs
@pytest.mark.parametrize("kind,L", [("gin", 2), ("gin", 6), ("gcn", 3), ("gcn", 8)])
def test_profiler_counts_L_layers_and_L_minus_1_updates(kind, L, tmp_path):
    vn = L < 8
    e = engine(kind, vn, L, exported(kind, vn, L, tmp_path))
    try:
        b = T.batch_of(kind)
        e.forward(b)  # (buffers sized, code loaded)
        e.profile_enable(True)
        before = {k: v["launches"] for k, v in e.profile_read().items()}
        e.forward(b)
        e.sync()
        n = {k: v["launches"] - before.get(k, 0) for k, v in e.profile_read().items()}
        print(kind, L, {k: v for k, v in n.items() if v})
        assert n.get(f"{kind}_wide_layer", 0) == L, n
        assert n.get(f"{kind}_wide_vn_update", 0) == (L - 1 if vn else 0), n
        assert e.exact_reruns() == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 5. depth 5 through the call is the engine that never made it
@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_depth_5_is_a_no_op(kind, tmp_path):
    model = T.make_model(kind, True, D)
    export.export_weights(kind.upper(), model.state_dict(), str(tmp_path), **export_kwargs(kind, True, D))
    out = []
    for call in (False, True):
        e = Engine(kind.upper(), device=0)
        try:
            (e.set_emb_dim if kind == "gin" else e.set_model_emb_dim)(D)
            e.load_weights_dir(str(tmp_path), eps=kind == "gin", virtual_node=True)
            if call:
                e.set_num_layers(5)  # behind the weights and with eps / the virtual node on: the same depth changes nothing
                assert e.num_layers == 5
            out.append(np.array(e.forward(T.batch_of(kind))))
        finally:
            e.close()
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))


# ---------------------------------------------------------------- 6. one case each
def test_device_batch(tmp_path):
    want, scale, (x, edge_index, edge_attr, ptr) = OL.expected("gcn", True, 3)
    e = engine("gcn", True, 3, exported("gcn", True, 3, tmp_path))
    try:
        dev = torch.device("cuda", 0)
        logits, pooled, rows = e.forward_device(x.to(dev), edge_index.to(dev), edge_attr.to(dev), ptr=ptr.to(dev), return_embeddings=True,
                                                return_node_embeddings=True)
        e.sync()
        close(rows.cpu().numpy(), want.rows, scale, "device batch rows")
        close(logits.cpu().numpy(), want.logits, scale, "device batch logits")
        assert e.exact_reruns() == 0
    finally:
        e.close()


@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_host_cli_num_layer_3(kind, tmp_path):
    want, scale, _ = OL.expected(kind, True, 3)
    gdir, wdir, out = tmp_path / "graphs", tmp_path / "weights", tmp_path / "HLS_output.txt"
    gp.write_pack(T.batch_of(kind), str(gdir))
    exported(kind, True, 3, wdir)
    flags = ["--eps", "--ogb-vn"] if kind == "gin" else ["--ogb-vn"]
    cmd = [HOST, kind.upper(), "--emb-dim", "300", "--num-layer", "3"] + flags + ["--graphs", str(gdir), "--weights", str(wdir), "--trials", "1", "--out", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array([float(ln.split(":")[1]) for ln in open(out).read().strip().splitlines()])
    close(got, want.logits, scale, (kind, "host --num-layer 3"))
    # the same directory without the flag: the files are those of another depth, and the loader says both numbers
    p = subprocess.run([c for c in cmd if c not in ("--num-layer", "3")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "3 layers deep" in p.stderr and "5" in p.stderr, p.stdout + p.stderr


def test_engine_group(tmp_path):
    want, scale, _ = OL.expected("gin", False, 6)
    d = exported("gin", False, 6, tmp_path)
    g = EngineGroup("GIN", [0, 0])
    try:
        configure(g, "gin", False, 6, d)
        g.load_weights_dir(d)
        g.set_gin_eps(weights.load_gin_eps(d, emb_dim=D, num_layers=6))
        logits = np.array(g.forward(T.batch_of("gin")))
        close(logits, want.logits, scale, "group {0, 0}, L = 6")
    finally:
        g.close()


def test_attention_readout_at_depth_2(tmp_path):
    """The rows are the torch model's; the readout on them is tests/attn_pool_ref.readout in float64 (the definition the attention tests use)."""
    want, scale, _ = OL.expected("gin", True, 2)
    d = exported("gin", True, 2, tmp_path)
    gate = weights.synth_attention_pooling(seed=11, emb_dim=D)
    w = weights.load_gin_weights(d, emb_dim=D, num_layers=2)
    stats = {}
    pooled, logits, _ = attn_pool_ref.readout(want.rows, T.batch_of("gin"), gate, w["graph_pred_weights"], w["graph_pred_bias"], stats=stats)
    scale = max(scale, stats["hidden_max"], stats["s_max"])
    e = engine("gin", True, 2, d)
    try:
        e.set_attention_pooling(gate)
        e.set_num_layers(2)  # the depth it has, with the readout on: a no-op; the readout survives a change of depth as well
        got_logits, got_pooled = (np.array(x) for x in e.forward(T.batch_of("gin"), return_embeddings=True))
        close(got_pooled, pooled, scale, "attention readout, L = 2: pooled")
        close(got_logits, np.asarray(logits).reshape(got_logits.shape), scale, "attention readout, L = 2: logits")
        assert e.exact_reruns() == 0
    finally:
        e.close()
