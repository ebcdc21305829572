"""flowgnn_laplacian_eigen / flowgnn_laplacian_eigen_device (include/flowgnn.h, kernels: flowgnn_amd/csrc/eigen.hip): DGN's node_eigen
computed on the GPU, against graphpack.laplacian_eigen (float64 eigh of the same definition).

Bounds (derived, not tuned): eps = 2^-24, ||L||_2 <= 2, m = max(n, 8); residual R(n) = 8 m eps, orthonormality 32 m eps -- the
c * n * eps * ||L|| form of a backward-stable fp32 eigensolver; a wrong vector, ordering or a missed rotation shows at the size of
the spectral gaps, 1e-2 and above.  Where an eigenvalue is gamma >= 0.01 away from its neighbours the vector itself is compared,
min(|v - r|, |v + r|) <= 2 R(n) / gamma (Davis-Kahan with the residual above)."""
import os
import re
import subprocess

import numpy as np
import pytest

from flowgnn_amd import Engine, FlowGNNError, GraphBatch, _lib, concat_batches, graphpack as gp, weights
from tests.parity import assert_close, oracle_scale

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
EPS = 2.0 ** -24
GAMMA = 0.01
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flowgnn_amd", "host")
SIZES = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128)  # both sides of every size class's edge


def R(n):
    return 8 * max(n, 8) * EPS


def one_graph(n, edges):
    e = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    return GraphBatch(np.array([n], np.int32), np.array([len(e)], np.int32), np.zeros((n, 9), np.int32), e,
                      np.zeros((len(e), 3), np.int32))


def both_ways(pairs):
    return [(a, b) for a, b in pairs] + [(b, a) for a, b in pairs]


def random_connected(n, rng):
    """A random spanning tree plus n random extra bonds, both directions listed."""
    pairs = [(int(rng.integers(i)), i) for i in range(1, n)]
    pairs += [tuple(int(x) for x in rng.integers(n, size=2)) for _ in range(n if n > 2 else 0)]
    return one_graph(n, both_ways([p for p in pairs if p[0] != p[1]]))


def graph_list():
    """(name, single-graph batch) of every graph of the test batch, in batch order."""
    rng = np.random.default_rng(5)
    parts = [(f"random{n}", random_connected(n, rng)) for n in SIZES]
    parts.append(("edgeless", one_graph(6, [])))
    parts.append(("isolated node", one_graph(7, both_ways([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (1, 4)]))))
    parts.append(("loops, duplicates, one direction", one_graph(9, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 0),
                                                                    (0, 1), (0, 1), (1, 0), (3, 3), (5, 5), (2, 6), (6, 2), (6, 2)])))
    parts.append(("two components", one_graph(10, both_ways([(0, 1), (1, 2), (2, 3), (3, 4), (5, 6), (6, 7), (7, 8), (8, 9), (9, 5)]))))
    parts.append(("star100", one_graph(100, both_ways([(0, i) for i in range(1, 100)]))))
    parts.append(("K12", one_graph(12, [(i, j) for i in range(12) for j in range(12) if i != j])))
    for name, b in (("molhiv", gp.synth_molhiv_batch(40, seed=3)), ("hep10k", gp.synth_hep10k_batch(24, seed=3, with_eigen=False))):
        parts += [(f"{name}{g}", b.slice(g, g + 1)) for g in range(b.num_graphs)]
    return parts


def device_eigen(e: Engine, b: GraphBatch, layout: str):
    if layout == "pyg":
        d = b.to_pyg(DEV)
        out = e.laplacian_eigen_device(d["edge_index"], ptr=d["ptr"], nums_of_edges=b.nums_of_edges)
    else:
        el = torch.from_numpy(np.ascontiguousarray(b.edge_list, dtype=np.int32)).to(DEV)
        out = e.laplacian_eigen_device(el, ptr=b.node_offsets(), nums_of_edges=b.nums_of_edges)
    return out.cpu().numpy()


class Case:
    """The test batch, its float64 reference, and the GPU's answers through both functions and both device layouts: computed once."""

    def __init__(self):
        self.parts = graph_list()
        self.names = [n for n, _ in self.parts]
        self.batch = concat_batches([b for _, b in self.parts])
        self.ref = gp.laplacian_eigen(self.batch)
        no, eo = self.batch.node_offsets(), self.batch.edge_offsets()
        self.no = no
        self.L = [gp.normalized_laplacian(int(self.batch.nums_of_nodes[g]), self.batch.edge_list[eo[g]:eo[g + 1]])
                  for g in range(self.batch.num_graphs)]
        self.spectrum = [np.linalg.eigvalsh(L) for L in self.L]
        self.eng = Engine("DGN", device=0)
        self.got = {"host": self.eng.laplacian_eigen(self.batch),
                    "device reference": device_eigen(self.eng, self.batch, "reference"),
                    "device pyg": device_eigen(self.eng, self.batch, "pyg")}


@pytest.fixture(scope="module")
def case():
    c = Case()
    yield c
    c.eng.close()


def rayleigh(L, v):
    return np.einsum("ik,ij,jk->k", v, L, v) / (v * v).sum(axis=0)


@pytest.mark.parametrize("path", ["host", "device reference", "device pyg"])
def test_eigenpair_properties_on_every_graph(case, path):
    out = case.got[path]
    assert out.shape == (case.batch.total_nodes, 4) and out.dtype == np.float32 and np.isfinite(out).all()
    worst = {}  # size class -> (residual / R, orthonormality / bound, eigenvalue / R): printed, for DESIGN.md section 4.13
    for g, name in enumerate(case.names):
        L, n = case.L[g], case.L[g].shape[0]
        k = min(4, n)
        rows = out[case.no[g]:case.no[g + 1]]
        v = rows[:, :k].astype(np.float64)
        lam = rayleigh(L, v)
        res = np.abs(L @ v - v * lam).max()
        orth = np.abs(v.T @ v - np.eye(k)).max()
        dlam = np.abs(lam - case.spectrum[g][:k]).max()
        cls = 32 if n <= 32 else 64 if n <= 64 else 128
        worst[cls] = np.maximum(worst.get(cls, np.zeros(3)), [res / R(n), orth / (32 * max(n, 8) * EPS), dlam / R(n)])
        assert res <= R(n), (path, name, n, f"residual {res:.3e} > {R(n):.3e}")
        assert orth <= 32 * max(n, 8) * EPS, (path, name, n, f"|V^T V - I| {orth:.3e}")
        assert dlam <= R(n), (path, name, n, f"eigenvalues off by {dlam:.3e}: not the smallest {k} in order")
        assert not rows[:, k:].any(), (path, name, "columns k >= n must be exactly 0")
    for cls in sorted(worst):
        print(f"{path}: class {cls}: residual {worst[cls][0]:.3f} R, orthonormality {worst[cls][1]:.3f} of its bound, eigenvalue {worst[cls][2]:.3f} R")


def test_vectors_where_the_basis_is_determined(case):
    out = case.got["host"]
    synthetic = qualified = 0
    for g, name in enumerate(case.names):
        n, full = case.L[g].shape[0], case.spectrum[g]
        is_synth = name.startswith(("molhiv", "hep10k"))
        for k in range(min(4, n)):
            synthetic += is_synth
            gap = min([abs(full[k] - full[j]) for j in (k - 1, k + 1) if 0 <= j < n], default=np.inf)
            if gap < GAMMA:
                continue
            qualified += is_synth
            v = out[case.no[g]:case.no[g + 1], k].astype(np.float64)
            r = case.ref[case.no[g]:case.no[g + 1], k].astype(np.float64)
            d = min(np.abs(v - r).max(), np.abs(v + r).max())
            assert d <= 2 * R(n) / gap, (name, k, f"|v -+ r| = {d:.3e} > 2 R / gap = {2 * R(n) / gap:.3e} (gap {gap:.3e})")
    assert qualified >= 0.9 * synthetic, (qualified, synthetic)


def test_dgn_end_to_end_with_the_gpus_eigenvectors(case, oracle):
    w = weights.synth_dgn_weights(seed=7)
    b = gp.synth_hep10k_batch(24, seed=3)
    b.node_eigen = gp.laplacian_eigen(b)
    want, hd = oracle.dgn_forward(b, [w], dump_h=True)
    scale = oracle_scale(hd)
    e = case.eng
    e.set_weights(w)
    b.node_eigen = e.laplacian_eigen(b)
    assert_close(e.forward(b), want, scale, what="forward with laplacian_eigen")
    d = b.to_pyg(DEV)
    out = e.forward_device(d["x"], d["edge_index"], None, e.laplacian_eigen_device(d["edge_index"], ptr=d["ptr"]), ptr=d["ptr"])
    e.sync()
    assert_close(out.cpu().numpy(), want, scale, what="forward_device with laplacian_eigen_device")


def test_one_writer_one_order(case):
    host = case.got["host"]
    assert np.array_equal(host, case.got["device reference"]) and np.array_equal(host, case.got["device pyg"])
    per_graph = [host[case.no[g]:case.no[g + 1]] for g in range(len(case.parts))]
    rev = case.eng.laplacian_eigen(concat_batches([b for _, b in reversed(case.parts)]))
    assert np.array_equal(rev, np.concatenate(per_graph[::-1]))
    for g0, g1 in ((3, 30), (11, len(case.parts))):
        part = case.eng.laplacian_eigen(case.batch.slice(g0, g1))
        assert np.array_equal(part, host[case.no[g0]:case.no[g1]]), (g0, g1)


def test_refusals(case):
    e = case.eng
    lib = _lib.load()
    rng = np.random.default_rng(9)
    big = concat_batches([random_connected(20, rng), random_connected(129, rng), random_connected(130, rng)])
    nn, ne, el = (np.ascontiguousarray(a, dtype=np.int32) for a in (big.nums_of_nodes, big.nums_of_edges, big.edge_list))
    pi = lambda a: a.ctypes.data_as(_lib.p_int)
    out = np.full((big.total_nodes, 4), 7.0, np.float32)
    assert lib.flowgnn_laplacian_eigen(e._h, 3, pi(nn), pi(ne), pi(el), out.ctypes.data_as(_lib.p_float)) == 8
    text = lib.flowgnn_last_error(e._h).decode()
    assert "graph 1 " in text and "129" in text, text
    assert (out == 7.0).all()
    d_el = torch.from_numpy(el).to(DEV)
    d_out = torch.full((big.total_nodes, 4), 7.0, dtype=torch.float32, device=DEV)
    with pytest.raises(FlowGNNError) as ex:
        e.laplacian_eigen_device_ptrs(nn, ne, "reference", d_el.data_ptr(), d_out.data_ptr())
    assert ex.value.code == 8 and "graph 1 " in str(ex.value)
    e.sync()
    assert bool((d_out == 7.0).all())
    # a host edge out of range
    bad = random_connected(10, rng)
    bad.edge_list[3, 1] = 10
    with pytest.raises(FlowGNNError) as ex:
        e.laplacian_eigen(bad)
    assert ex.value.code == 2
    # nulls and negative counts, as flowgnn_set_batch gives
    assert lib.flowgnn_laplacian_eigen(e._h, -1, pi(nn), pi(ne), pi(el), out.ctypes.data_as(_lib.p_float)) == 1
    assert lib.flowgnn_laplacian_eigen(e._h, 3, pi(nn), pi(ne), pi(el), None) == 1
    assert lib.flowgnn_laplacian_eigen_device(e._h, 3, pi(nn), pi(ne), 2, d_el.data_ptr(), d_out.data_ptr()) == 1
    # host memory is no device array
    with pytest.raises(FlowGNNError) as ex:
        e.laplacian_eigen_device_ptrs(nn[:1], ne[:1], "reference", d_el.data_ptr(), out.ctypes.data)
    assert ex.value.code == 1 and (out == 7.0).all()
    # no graphs: OK, nothing to do
    empty = GraphBatch(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 9), np.int32), np.zeros((0, 2), np.int32),
                       np.zeros((0, 3), np.int32))
    assert e.laplacian_eigen(empty).shape == (0, 4)
    assert lib.flowgnn_laplacian_eigen_device(e._h, 0, None, None, 0, None, None) == 0


def test_the_engine_is_left_alone(case):
    """Any model's engine will do, and its resident batch, its results and a recorded launch sequence survive the call."""
    g = Engine("GIN", device=0, options={"hipgraph": 1})
    try:
        g.set_weights(weights.synth_gin_weights(seed=7))
        g.set_batch(gp.synth_molhiv_batch(64, seed=3))
        for _ in range(3):  # plain, captured, replay
            g.run()
        before, replays = g.results(), g.graph_replays()
        assert replays >= 1
        hep = gp.synth_hep10k_batch(24, seed=3, with_eigen=False)
        eig = g.laplacian_eigen(hep)
        no = case.no[case.names.index("hep10k0")]
        assert np.array_equal(eig, case.got["host"][no:no + hep.total_nodes])
        assert np.array_equal(g.results(), before)
        g.run()
        assert g.graph_replays() == replays + 1 and np.array_equal(g.results(), before)
        assert np.array_equal(device_eigen(g, hep, "pyg"), eig)
        g.run()
        assert g.graph_replays() == replays + 2 and np.array_equal(g.results(), before)
    finally:
        g.close()


def test_host_cli_computes_the_eigenvectors(tmp_path, oracle):
    w = weights.synth_dgn_weights(seed=7)
    b = gp.synth_hep10k_batch(24, seed=3)
    b.node_eigen = gp.laplacian_eigen(b)
    want = oracle.dgn_forward(b, [w])
    gdir, wdir, out = tmp_path / "graphs", tmp_path / "weights", tmp_path / "HLS_output.txt"
    gp.write_pack(b, str(gdir))  # no eig directory
    weights.SAVERS["DGN"](w, str(wdir))
    cmd = [HOST, "DGN", "--graphs", str(gdir), "--weights", str(wdir), "--eig", str(tmp_path / "no_such_dir"), "--trials", "1", "--out", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "cannot read" in r.stderr  # without the flag nothing changes: the text files are required
    r = subprocess.run(cmd + ["--compute-eig"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = open(out).read().strip().splitlines()
    assert all(re.fullmatch(r"g\d+: -?\d+\.\d{8}", ln) for ln in lines), lines[:3]
    got = np.array([float(ln.split(":")[1]) for ln in lines], dtype=np.float32)
    assert np.allclose(got, want, rtol=3e-4, atol=3e-4 * max(1.0, np.abs(want).max())), np.abs(got - want).max()
