"""Fast diagonalisation of the uncut wave / heat system, host side (no GPU):

(a) the numpy helper tests/fastdiag_ref.py against np.linalg.solve on the
    dense Kronecker system, p = 1 .. 9, n_sub = (p, p+2, p+3) on an anisotropic
    box; the rel-L2 error of each case is the reference's own noise err_ref
    (about 1e-17 cond: 1e-15 at p = 1, 1e-14 at p = 5, a few 1e-11 at p = 9);
(b) gdm_fastdiag_tables (banded Cholesky + Householder / QL on the host)
    against scipy.linalg.eigh on the same matrices: eigenvalues, M-
    orthonormality, the diagonalisation residual, the sign convention and
    bitwise repeatability;
(c) argument checks of the pure-host entry point.
"""
import ctypes

import numpy as np
import pytest

import fastdiag_ref as F
import oracle as O

from gdm_amd import _capi

DEGREES = [1, 3, 5, 7, 9]


def _mesh3(p):
    return O.Mesh(3, p, list(F.small_n_sub(p)), list(F.BOX_LO), list(F.BOX_HI))


def _desc(m):
    d = _capi.mesh_desc(m.dim, m.p, [int(m.nsub[e]) for e in range(m.dim)])
    for e in range(m.dim):
        d.lo[e], d.hi[e] = float(m.lo[e]), float(m.hi[e])
    return d


@pytest.mark.parametrize("p", DEGREES)
def test_helper_equals_dense_solve(p):
    m = _mesh3(p)
    for gamma, alpha, tau in F.DENSE_CASES:
        _, _, err_ref = F.dense_reference(m, gamma, alpha, tau, seed=p)
        cond = np.linalg.cond(F.dense_system(m, gamma, alpha, tau)) if p <= 5 else float("nan")
        print("helper vs dense p %d gamma %g alpha %g tau %g: err_ref %.2e cond %.1e" % (p, gamma, alpha, tau, err_ref, cond))
        # 1e-17 cond, cond <= 1e8 on these meshes, with a decade to spare
        assert err_ref <= 1e-9


TABLE_MESHES = [("3d-p%d" % p, 3, p, F.small_n_sub(p), F.BOX_LO, F.BOX_HI) for p in DEGREES] + [
    ("1d-p5-256", 1, 5, (256,), (-0.3,), (1.1,))]


@pytest.mark.parametrize("name,dim,p,n_sub,lo,hi", TABLE_MESHES, ids=[c[0] for c in TABLE_MESHES])
@pytest.mark.parametrize("gamma", [15.0, 0.0])
def test_tables_against_scipy(name, dim, p, n_sub, lo, hi, gamma):
    m = O.Mesh(dim, p, list(n_sub), list(lo), list(hi))
    desc = _desc(m)
    ref = F.eigenpairs(m, gamma)
    AM = F.matrices(m, gamma)
    for d in range(dim):
        S, lam = _capi.fastdiag_tables(desc, gamma, d)
        S2, lam2 = _capi.fastdiag_tables(desc, gamma, d)
        assert S.tobytes() == S2.tobytes() and lam.tobytes() == lam2.tobytes()
        A, M = AM[d]
        Sr, lr = ref[d]
        lmax = np.abs(lr).max()
        n = lam.size
        e_lam = np.abs(lam - lr).max() / lmax
        orth = np.abs(S.T @ M @ S - np.eye(n)).max()
        diag = np.abs(S.T @ A @ S - np.diag(lam)).max() / lmax
        orth_r = np.abs(Sr.T @ M @ Sr - np.eye(n)).max()
        diag_r = np.abs(Sr.T @ A @ Sr - np.diag(lr)).max() / lmax
        print("%s gamma %g axis %d N %d: lambda %.2e  S^T M S - I %.2e (scipy %.2e)  S^T A S - L %.2e (scipy %.2e)"
              % (name, gamma, d, n, e_lam, orth, orth_r, diag, diag_r))
        assert np.all(np.diff(lam) >= 0.0)
        assert e_lam <= 1e-11
        assert orth <= 1e-11
        assert diag <= 1e-11
        big = np.abs(S).argmax(axis=0)
        assert np.all(S[big, np.arange(n)] > 0.0)


def test_penalty_too_small_is_indefinite():
    """gamma = 4 at p = 5, n_sub = p + 2: the 1D operator has a negative eigenvalue"""
    m = O.Mesh(1, 5, [7], [0.0], [1.0])
    _, lam = _capi.fastdiag_tables(_desc(m), 4.0, 0)
    print("lambda_min at gamma = 4, p = 5, n_sub = 7: %.4g" % lam[0])
    assert lam[0] < -1.0


def test_argument_checks():
    lib = _capi.load()
    m = _desc(_mesh3(3))
    n = m.n_subdivisions[0] + 1
    S, lam = np.zeros((n, n)), np.zeros(n)
    ps, pl = S.ctypes.data_as(ctypes.c_void_p), lam.ctypes.data_as(ctypes.c_void_p)
    assert lib.gdm_fastdiag_tables(None, 15.0, 0, ps, pl) == -1
    assert lib.gdm_fastdiag_tables(ctypes.byref(m), 15.0, 0, None, pl) == -1
    assert lib.gdm_fastdiag_tables(ctypes.byref(m), 15.0, 0, ps, None) == -1
    assert lib.gdm_fastdiag_tables(ctypes.byref(m), 15.0, 3, ps, pl) == -1
    assert lib.gdm_fastdiag_tables(ctypes.byref(m), 15.0, -1, ps, pl) == -1
    assert "axis" in _capi.last_error()
    even = _desc(_mesh3(3))
    even.fe_degree = 4
    assert lib.gdm_fastdiag_tables(ctypes.byref(even), 15.0, 0, ps, pl) == -3
    few = _desc(_mesh3(3))
    few.n_subdivisions[0] = 2
    assert lib.gdm_fastdiag_tables(ctypes.byref(few), 15.0, 0, ps, pl) == -1
    assert lib.gdm_fastdiag_tables(ctypes.byref(m), 15.0, 0, ps, pl) == _capi.GDM_OK
