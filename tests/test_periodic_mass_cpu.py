"""CPU tests of the exact periodic mass inverse's host side: the numpy
reference (tests/periodic_mass_ref.py) against a sparse direct solve of the
condensed cell-loop matrix, the Woodbury tables of gdm_mass_periodic_tables
(pure host) against dense solves, and the claim the line passes rest on: the
Cholesky rows of blockdiag(M[0:N-1, 0:N-1], 1) are M's except the last one.
"""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import oracle as O
import periodic_mass_ref as R
from gdm_amd import _capi


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("dim,p,n,mask", [(1, 3, 30, 1), (2, 5, (11, 13), 1), (2, 5, (11, 13), 2),
                                          (2, 5, (11, 13), 3), (3, 3, (6, 7, 8), 5), (3, 3, (6, 7, 8), 7)])
def test_reference_matches_sparse_condensed_solve(dim, p, n, mask):
    m = O.Mesh(dim, p, n)
    ref = R.PeriodicMassRef(m, mask)
    b = ref.condense(np.random.default_rng(7).uniform(-1, 1, m.n_dofs))
    x = ref.distribute(spla.spsolve(ref.sparse_condensed(), b))
    err = rel(ref.solve(b), x)
    print("reference vs spsolve: %.3e" % err)
    assert err <= 1e-13
    # the entries on constrained DoFs are ignored
    g = b.copy()
    g[ref.constrained] = 3.25
    assert np.array_equal(ref.solve(g), ref.solve(b))


@pytest.mark.parametrize("p", [1, 3, 5, 7, 9])
@pytest.mark.parametrize("which", ["p+1", "2p+1", "30", "200"])
def test_periodic_tables(p, which):
    n = {"p+1": p + 1, "2p+1": 2 * p + 1, "30": 30, "200": 200}[which]
    N = n + 1
    mesh = _capi.mesh_desc(1, p, n)
    T, mv, lo, hi = _capi.mass_periodic_tables(mesh, 0)
    M = R.dense_1d(O.Mesh(1, p, n), 0)
    assert np.allclose(mv, M[N - 1 - p:N - 1, N - 1], rtol=1e-13, atol=0.0)  # two assemblies of the same integrals
    A = M[:N - 1, :N - 1]
    m_full = M[:N - 1, N - 1]
    b = np.random.default_rng(p + n).uniform(-1, 1, N - 1)
    g = np.linalg.solve(A, b)
    x = g - T @ np.array([g[0], m_full @ g])
    err = rel(x, np.linalg.solve(R.condensed_1d(M), b))
    print("p %d n %d: woodbury vs dense %.3e, rows %d + %d of %d" % (p, n, err, lo, hi, N - 1))
    assert err <= 1e-13
    assert lo >= 1 and hi >= 0 and lo + hi <= N - 1
    if which in ("p+1", "2p+1"):
        assert lo + hi >= N - 1
    if which == "200":
        assert lo + hi < N - 1
    skipped = T[lo:N - 1 - hi]
    size = np.maximum(np.abs(skipped[:, 0]), np.abs(skipped[:, 1]) * np.abs(mv).max())
    assert np.all(size <= 1e-18)
    # only the skipped rows were dropped: the truncated correction is as exact
    Tt = T.copy()
    Tt[lo:N - 1 - hi] = 0.0
    assert rel(g - Tt @ np.array([g[0], m_full @ g]), x) <= 1e-16


@pytest.mark.parametrize("p,n", [(1, 2), (3, 4), (3, 30), (5, 11), (7, 60), (9, 10), (9, 200)])
def test_modified_factor_rows_equal_the_mass_factor(p, n):
    mesh = _capi.mesh_desc(1, p, n, 0.0, 1.7)
    l0, d0 = _capi.mass_cholesky_1d(mesh, 0, periodic=False)
    l1, d1 = _capi.mass_cholesky_1d(mesh, 0, periodic=True)
    assert np.array_equal(l0[:-1], l1[:-1]) and np.array_equal(d0[:-1], d1[:-1])
    assert np.array_equal(l1[-1], np.r_[np.zeros(p), 1.0]) and d1[-1] == 1.0
    # and the factor is M's: L L^T = M
    M = R.dense_1d(O.Mesh(1, p, n, 0.0, 1.7), 0)
    L = np.zeros_like(M)
    for i in range(n + 1):
        for k in range(p + 1):
            if i - p + k >= 0:
                L[i, i - p + k] = l0[i, k]
    assert rel(L @ L.T, M) <= 1e-14
    assert np.allclose(d0 * np.diag(L), 1.0, rtol=1e-15)


def test_tables_refuse_bad_arguments():
    with pytest.raises(_capi.GdmError):
        _capi.mass_periodic_tables(_capi.mesh_desc(1, 3, 30), 1)
    with pytest.raises(_capi.GdmError):
        _capi.mass_periodic_tables(_capi.mesh_desc(1, 4, 30), 0)
    with pytest.raises(_capi.GdmError):
        _capi.mass_periodic_tables(_capi.mesh_desc(1, 5, 3), 0)
