"""float32 CPU transcription of flowgnn_amd/csrc/eigen.hip's Jacobi iteration: the same round-robin rotation order, the same
rotation formula and identity selects, the same stopping rule.  It is where the kernel's threshold (EIGEN_TOL) and sweep cap
(EIGEN_MAX_SWEEPS) come from; no GPU needed.
usage: eigen_sweeps.py [TOL [CAP]]      (defaults: the kernel's 5e-7 and 16)
Prints, per graph: sweeps taken, the residual |L v - lambda v|, |V^T V - I| and the eigenvalue error of the four smallest pairs as
fractions of the tests' bounds (8 m eps, 32 m eps, 8 m eps; m = max(n, 8), eps = 2^-24), and the history of ||off(A)||_F / ||L||_F when the
cap was reached; then the maxima.  With TOL below the float32 floor of that ratio (1e-7 .. 2e-7) every graph runs to the cap."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flowgnn_amd import graphpack as gp  # noqa: E402

f32 = np.float32
EPS = 2.0 ** -24


def pairs(m, r):
    """Step r of the round-robin over m (even) players: player m - 1 stays, the others turn."""
    k = np.arange(1, m // 2)
    return np.concatenate([[m - 1], (r + k) % (m - 1)]), np.concatenate([[r], (r - k + m - 1) % (m - 1)])


def jacobi(L, tol, cap):
    n = L.shape[0]
    m = n + (n & 1)
    A = np.zeros((m, m), f32)
    A[:n, :n] = L.astype(f32)
    if m > n:
        A[n, n] = 1.0  # the padding row: no rotation touches it
    V = np.eye(m, dtype=f32)
    fro2 = (A[:n, :n] ** 2).sum(dtype=f32)
    sweeps, hist = 0, []
    for _ in range(cap):
        B = A.copy()
        np.fill_diagonal(B, 0)
        off2 = (B ** 2).sum(dtype=f32)
        hist.append(float(np.sqrt(off2 / fro2)))
        if off2 <= f32(tol) * f32(tol) * fro2:
            break
        sweeps += 1
        for r in range(m - 1):
            p, q = pairs(m, r)
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            skip = (np.abs(apq) < f32(1e-30)) | (p >= n) | (q >= n)
            with np.errstate(all="ignore"):
                th = (aqq - app) / (f32(2) * np.where(skip, f32(1), apq))
                t = np.copysign(f32(1), th) / (np.abs(th) + np.sqrt(th * th + f32(1)))
            t = np.where(skip, f32(0), t).astype(f32)
            c = (f32(1) / np.sqrt(t * t + f32(1))).astype(f32)
            s = (t * c).astype(f32)
            for M in (A, V):  # columns
                mp, mq = M[:, p].copy(), M[:, q].copy()
                M[:, p], M[:, q] = c * mp - s * mq, s * mp + c * mq
            mp, mq = A[p, :].copy(), A[q, :].copy()  # rows
            A[p, :], A[q, :] = c[:, None] * mp - s[:, None] * mq, s[:, None] * mp + c[:, None] * mq
    d = np.diag(A)[:n]
    o = np.argsort(d, kind="stable")
    return d[o], V[:n, :n][:, o], sweeps, hist


def main():
    tol = float(sys.argv[1]) if len(sys.argv) > 1 else 5e-7
    cap = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    rng = np.random.default_rng(0)
    worst = np.zeros(3)
    count = {}

    def run(n, edges, tag):
        L = gp.normalized_laplacian(n, edges)
        _, V, sw, h = jacobi(L, tol, cap)
        k = min(4, n)
        v = V[:, :k].astype(np.float64)
        lam = np.einsum("ik,ij,jk->k", v, L, v) / (v * v).sum(axis=0)
        m = max(n, 8)
        fr = np.array([np.abs(L @ v - v * lam).max() / (8 * m * EPS), np.abs(v.T @ v - np.eye(k)).max() / (32 * m * EPS),
                       np.abs(lam - np.linalg.eigvalsh(L)[:k]).max() / (8 * m * EPS)])
        worst[:] = np.maximum(worst, fr)
        count[sw] = count.get(sw, 0) + 1
        print(f"{tag:6s} n {n:3d} sweeps {sw:2d}  residual {fr[0]:.3f}  orthonormality {fr[1]:.3f}  eigenvalue {fr[2]:.3f}  off/fro {h[-1]:.1e}",
              " ".join(f"{x:.0e}" for x in h) if sw >= cap else "")

    for b in (gp.synth_hep10k_batch(24, seed=3, with_eigen=False), gp.synth_molhiv_batch(40, seed=3)):
        eo = b.edge_offsets()
        for g in range(b.num_graphs):
            run(int(b.nums_of_nodes[g]), b.edge_list[eo[g]:eo[g + 1]], "synth")
    for n in (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128):
        e = [(i, i + 1) for i in range(n - 1)] + [(int(rng.integers(n)), int(rng.integers(n))) for _ in range(2 * n)]
        run(n, np.array(e).reshape(-1, 2), "random")
    run(100, np.array([(0, i) for i in range(1, 100)]), "star")
    run(12, np.array([(i, j) for i in range(12) for j in range(12)]), "K12")
    run(7, np.zeros((0, 2), int), "empty")
    print(f"tol {tol:g} cap {cap}: worst residual {worst[0]:.3f}, orthonormality {worst[1]:.3f}, eigenvalue {worst[2]:.3f} of their bounds; "
          f"graphs by sweeps: {dict(sorted(count.items()))}")


if __name__ == "__main__":
    main()
