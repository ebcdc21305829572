"""graphpack.laplacian_eigen, the float64 definition of DGN's node_eigen (include/flowgnn.h: flowgnn_laplacian_eigen) and the
reference of the GPU tests: hand-made graphs, the upstream DGN preprocessing's formula, and DGN's blindness to the sign and scale
of the eigenvector column."""
import numpy as np

from flowgnn_amd import graphpack as gp, weights
from tests import numpy_ref


def one_graph(n, edges):
    e = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    return gp.GraphBatch(np.array([n], np.int32), np.array([len(e)], np.int32), np.zeros((n, 9), np.int32), e,
                         np.zeros((len(e), 3), np.int32))


def both_ways(pairs):
    return [(a, b) for a, b in pairs] + [(b, a) for a, b in pairs]


def rayleigh(L, v):
    v = v.astype(np.float64)
    return np.einsum("ik,ij,jk->k", v, L, v) / (v * v).sum(axis=0)


def check_eigenpairs(n, edges, want_L=None):
    """The returned columns are unit eigenvectors of the definition's L for its smallest min(4, n) eigenvalues, in order."""
    L = gp.normalized_laplacian(n, edges)
    if want_L is not None:
        assert np.allclose(L, want_L, atol=1e-15)
    eig = gp.laplacian_eigen(one_graph(n, edges))
    assert eig.shape == (n, 4) and eig.dtype == np.float32
    k = min(4, n)
    v = eig[:, :k]
    lam = rayleigh(L, v)
    # float32 storage of a float64 eigenvector: 2^-24 relative per entry, rows of |L| sum to at most 2
    assert np.abs(L @ v.astype(np.float64) - v * lam).max() <= 4 * 2.0 ** -24
    assert np.abs(v.T.astype(np.float64) @ v - np.eye(k)).max() <= 4 * 2.0 ** -24
    assert np.abs(lam - np.linalg.eigvalsh(L)[:k]).max() <= 1e-6
    assert not eig[:, k:].any()
    return L, eig, lam


def test_path_has_the_known_spectrum():
    for n in (2, 5, 12):
        L, eig, lam = check_eigenpairs(n, both_ways([(i, i + 1) for i in range(n - 1)]))
        assert np.allclose(lam, 1.0 - np.cos(np.pi * np.arange(min(4, n)) / (n - 1)), atol=1e-6)
    # the constant-sign vector D^1/2 1 of eigenvalue 0
    d = np.array([1, 2, 2, 2, 1], dtype=np.float64) ** 0.5
    v0 = gp.laplacian_eigen(one_graph(5, both_ways([(i, i + 1) for i in range(4)])))[:, 0]
    assert np.allclose(np.abs(v0), d / np.linalg.norm(d), atol=1e-6)


def test_one_direction_listed_only_is_symmetrised():
    pairs = [(0, 1), (1, 2), (2, 3), (3, 0), (1, 3), (3, 4)]
    L1 = gp.normalized_laplacian(5, pairs)
    assert np.array_equal(L1, gp.normalized_laplacian(5, both_ways(pairs))) and np.array_equal(L1, L1.T)
    check_eigenpairs(5, pairs)
    assert np.array_equal(gp.laplacian_eigen(one_graph(5, pairs)), gp.laplacian_eigen(one_graph(5, both_ways(pairs))))


def test_duplicates_and_a_self_loop_do_not_count():
    clean = both_ways([(0, 1), (1, 2), (2, 0), (2, 3)])
    messy = clean + [(0, 1), (0, 1), (2, 2), (3, 2), (1, 1)]
    assert np.array_equal(gp.normalized_laplacian(4, messy), gp.normalized_laplacian(4, clean))
    deg = np.array([2, 2, 3, 1], dtype=np.float64)
    A = np.zeros((4, 4))
    for a, b in clean:
        A[a, b] = 1
    check_eigenpairs(4, messy, want_L=np.eye(4) - A / np.sqrt(deg[:, None] * deg[None, :]))


def test_isolated_node_and_edgeless_graph():
    L, eig, lam = check_eigenpairs(4, both_ways([(0, 1), (1, 2)]))
    assert L[3, 3] == 1.0 and not L[3, :3].any() and not L[:3, 3].any()
    L, eig, lam = check_eigenpairs(3, [])
    assert np.array_equal(L, np.eye(3)) and np.allclose(lam, 1.0)
    # fewer than four nodes: the columns k >= n stay 0
    assert not gp.laplacian_eigen(one_graph(1, []))[:, 1:].any()
    assert gp.laplacian_eigen(one_graph(1, []))[0, 0] in (1.0, -1.0)


def test_a_batch_is_its_graphs_one_by_one():
    b = gp.synth_molhiv_batch(6, seed=3)
    whole = gp.laplacian_eigen(b)
    parts = np.concatenate([gp.laplacian_eigen(b.slice(g, g + 1)) for g in range(b.num_graphs)])
    assert whole.shape == (b.total_nodes, 4) and np.array_equal(whole, parts)


def upstream_eigen(n, edges, k=4):
    """The upstream DGN preprocessing: A[src][dst] = 1, N = diag(in_degree.clip(1) ** -0.5), eig of I - N A N, sorted by eigenvalue."""
    A = np.zeros((n, n))
    e = np.asarray(edges).reshape(-1, 2)
    A[e[:, 0], e[:, 1]] = 1.0
    Nm = np.diag(np.clip(A.sum(axis=0), 1, None) ** -0.5)
    val, vec = np.linalg.eig(np.eye(n) - Nm @ A @ Nm)
    idx = val.argsort()
    return np.real(val[idx][:k]), np.real(vec[:, idx][:, :k])


def test_equals_the_upstream_formula_on_graphs_that_list_both_directions():
    b = gp.synth_molhiv_batch(12, seed=3)
    no, eo = b.node_offsets(), b.edge_offsets()
    eig = gp.laplacian_eigen(b)
    simple = 0
    for g in range(b.num_graphs):
        n, edges = int(b.nums_of_nodes[g]), b.edge_list[eo[g]:eo[g + 1]]
        val, vec = upstream_eigen(n, edges)
        ours = eig[no[g]:no[g + 1]].astype(np.float64)
        full = np.linalg.eigvalsh(gp.normalized_laplacian(n, edges))
        assert np.allclose(rayleigh(gp.normalized_laplacian(n, edges), ours), val, atol=1e-6)
        for k in range(4):
            gap = min(abs(full[k] - full[j]) for j in (k - 1, k + 1) if 0 <= j < n)
            if gap < 1e-3:
                continue  # inside a (nearly) repeated eigenvalue the basis is arbitrary
            simple += 1
            u = vec[:, k] / np.linalg.norm(vec[:, k])
            assert min(np.abs(ours[:, k] - u).max(), np.abs(ours[:, k] + u).max()) <= 1e-6 / gap
    assert simple >= 3 * b.num_graphs  # (most columns are determined, so the comparison above says something)


def test_dgn_does_not_see_sign_or_scale_of_the_eigenvectors():
    b = gp.synth_hep10k_batch(6, seed=3, with_eigen=False)
    w = weights.synth_dgn_weights(seed=7)
    b.node_eigen = gp.laplacian_eigen(b)
    want = numpy_ref.dgn_forward(b, w)
    b.node_eigen = -3.0 * b.node_eigen.astype(np.float64)  # (exact in float64: only the rounding of the float64 forward remains)
    got = numpy_ref.dgn_forward(b, w)
    assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
