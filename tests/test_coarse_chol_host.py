"""The coarsest-level factorisation of the normal-equation multigrid (csrc/coarse_chol.hip) restated in NumPy, panel by
panel as the kernels run it: blocked right-looking Cholesky on [A | I] with pivots <= 1e-13 max_i A_ii dropped, then
B = Y^T Y.  Checked against the eigen-decomposition pseudo-inverse of the host route (gmg.NormalGMG._coarse_inverse):
equal on SPD matrices, a generalised inverse with A B b = b on the range of a singular one.  Also: the library exports
the two entry points."""

import numpy as np
import pytest

PANEL = 64  # kCcPanel


def blocked_inverse(amat, tol_rel=1e-13, panel=PANEL):
    n = amat.shape[0]
    npad = -(-n // panel) * panel
    work = np.zeros((npad, 2 * npad))
    work[:n, :n] = 0.5 * (amat + amat.T)
    work[:, npad:] = np.eye(npad)
    thr = tol_rel * max(np.diag(amat).max(), 0.0)
    drops = 0
    for k0 in range(0, npad, panel):
        k1 = k0 + panel
        s = np.triu(work[k0:k1, k0:k1])
        rd = np.zeros(panel)
        for j in range(panel):  # the diagonal block, in LDS
            p = s[j, j]
            keep = p > thr
            d = np.sqrt(p) if keep else 0.0
            s[j, j + 1:] = s[j, j + 1:] / d if keep else 0.0
            s[j, j] = d
            rd[j] = 1.0 / d if keep else 0.0
            drops += int(not keep and k0 + j < n)
            s[j + 1:, j + 1:] -= np.triu(np.outer(s[j, j + 1:], s[j, j + 1:]))
        x = work[k0:k1, k1:npad + k1].copy()  # U11^-T on the panel's columns, one column per thread
        for j in range(panel):
            x[j] *= rd[j]
            x[j + 1:] -= np.outer(s[j, j + 1:], x[j])
        work[k0:k1, k1:npad + k1] = x
        # trailing update (the MFMA kernel): rows [k1, npad), columns [k1, npad + k1)
        work[k1:, k1:npad + k1] -= work[k0:k1, k1:npad].T @ work[k0:k1, k1:npad + k1]
    y = work[:, npad:]
    return (y.T @ y)[:n, :n], drops


def pinv_eigh(amat):
    amat = 0.5 * (amat + amat.T)
    w, v = np.linalg.eigh(amat)
    keep = w > 1e-13 * max(float(np.abs(w).max()), 1e-300)
    return (v[:, keep] / w[keep]) @ v[:, keep].T


@pytest.mark.parametrize("n", [1, 15, 16, 17, 64, 65, 130])
def test_spd_equals_the_inverse(n):
    rng = np.random.default_rng(n)
    g = rng.standard_normal((n, n))
    amat = g @ g.T / n + 0.5 * np.eye(n)
    inv, drops = blocked_inverse(amat)
    assert drops == 0
    assert np.abs(inv - np.linalg.inv(amat)).max() <= 1e-12 * np.abs(np.linalg.inv(amat)).max()
    assert np.abs(inv - pinv_eigh(amat)).max() <= 1e-12 * np.abs(inv).max()


def neumann(nx, ny):
    idx = np.arange(nx * ny).reshape(nx, ny)
    amat = np.zeros((nx * ny, nx * ny))
    for i in range(nx):
        for j in range(ny):
            for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                if 0 <= i + di < nx and 0 <= j + dj < ny:
                    amat[idx[i, j], idx[i, j]] += 1.0
                    amat[idx[i, j], idx[i + di, j + dj]] -= 1.0
    return amat


def test_one_dimensional_nullspace():
    amat = neumann(12, 10)
    inv, drops = blocked_inverse(amat)
    assert drops == 1
    assert np.array_equal(inv, inv.T)
    assert np.linalg.eigvalsh(inv).min() >= -1e-12 * np.abs(inv).max()  # positive semidefinite
    b = np.random.default_rng(0).standard_normal(amat.shape[0])
    b -= b.mean()
    z = inv @ b
    assert np.abs(amat @ z - b).max() <= 1e-11 * np.abs(b).max()
    d = z - pinv_eigh(amat) @ b
    assert np.abs(d - d.mean()).max() <= 1e-11 * np.abs(z).max()  # the pseudo-inverse's answer up to a constant


def test_zero_matrix_drops_everything():
    inv, drops = blocked_inverse(np.zeros((5, 5)))
    assert drops == 5 and not inv.any()


def test_library_exports_the_entry_points():
    from odil_amd import _lib

    for name in ("odil_bmg_coarse_dense_f64", "odil_bmg_coarse_chol_f64"):
        assert name in _lib.EXPORTED
        assert hasattr(_lib.load(), name)
