"""Separable density (the weighted mass M[rho]), host side (no GPU): the numpy
restatement tests/varmass_ref.py against the oracle, and the pure-host C ABI
functions gdm_density_cholesky_1d / gdm_density_tile.

(a) the restatement with rho = 1 equals the oracle's mass matrix (its cell
    loop, pinned to the reference goldens) to rel-L2 1e-13;
(b) the Kronecker sum of the engine's bands gdm_coef_matrix_1d(which = 0)
    equals the restatement for a pointwise rho to 1e-13: the factorisation
    itself;
(c) gdm_density_cholesky_1d: L L^T reproduces the band; f = None gives
    gdm_mass_cholesky_1d; a factor that is not positive is refused;
(d) gdm_density_tile returns sane values;
(e) the reference PCG with the engine's preconditioner converges for the test
    densities of tests/test_gpu_varmass_solve.py.
"""
import ctypes

import numpy as np
import pytest

import oracle as O
import vardiff_ref as RD
import varmass_ref as R
from varmass_ref import MAX_IT, bump_terms

from gdm_amd import _capi

GDM_ERR_ARG, GDM_ERR_UNSUPPORTED = -1, -3


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _one(x):
    return np.ones(x.shape[0])


def _csr_apply(csr, u):
    rowptr, cols, vals = csr
    out = np.zeros(len(rowptr) - 1)
    for i in range(len(out)):
        out[i] = vals[rowptr[i]:rowptr[i + 1]] @ u[cols[rowptr[i]:rowptr[i + 1]]]
    return out


@pytest.mark.parametrize("dim,n_sub,lo,hi", [
    (1, (9,), (-0.3,), (1.1,)),
    (2, (6, 5), (0.0, -1.0), (1.5, 0.2)),
    (3, (7, 5, 4), (0.0, -0.5, 0.1), (1.0, 0.7, 0.9)),
])
def test_restatement_unit_density_equals_oracle(dim, n_sub, lo, hi):
    p = 3
    m = O.Mesh(dim, p, list(n_sub), list(lo), list(hi))
    u = np.random.default_rng(dim).uniform(-1, 1, m.n_dofs)
    got = R.mass_apply(m, _one, u)
    assert _rel(got, _csr_apply(m.matrix_csr(0), u)) < 1e-13
    M = [m.matrices_1d(d)[0] for d in range(dim)]
    assert _rel(got, m.kron_apply([tuple(M)], u)) < 1e-13


TERMS = {
    2: [[lambda x: 1.3 + 0.6 * np.sin(2.1 * x), lambda y: np.exp(0.5 * y)],
        [lambda x: 0.2 * x * x, None]],
    3: [[lambda x: 1.3 + 0.6 * np.sin(2.1 * x), lambda y: np.exp(0.5 * y), None],
        [None, lambda y: 0.3 * np.cos(y), lambda z: z],
        [lambda x: 2.0, None, None]],
}


@pytest.mark.parametrize("dim,p,n_sub,lo,hi", [
    (2, 1, (4, 3), (0.0, -1.0), (1.5, 0.2)),
    (2, 3, (6, 5), (0.0, -1.0), (1.5, 0.2)),
    (2, 5, (6, 7), (0.0, -1.0), (1.5, 0.2)),
    (3, 3, (5, 4, 6), (0.0, -0.5, 0.1), (1.0, 0.7, 0.9)),
])
def test_kronecker_sum_of_the_bands_equals_the_restatement(dim, p, n_sub, lo, hi):
    """sum_t kron_d band(M_d[r_td]) u against the cell loop for the pointwise rho"""
    m = O.Mesh(dim, p, list(n_sub), list(lo), list(hi))
    mesh = _capi.mesh_desc(dim, p, n_sub, 0.0, 1.0)
    for d in range(dim):
        mesh.lo[d], mesh.hi[d] = lo[d], hi[d]
    terms = TERMS[dim]
    u = np.random.default_rng(10 * dim + p).uniform(-1, 1, m.n_dofs)
    want = R.mass_apply(m, R.pointwise(terms, dim), u)
    A = 0.0
    for t in terms:
        fac = []
        for d in range(dim):
            x = _capi.field_points(mesh, d)
            f = None if t[d] is None else t[d](x) + 0.0 * x
            fac.append(RD.band_to_dense(_capi.coef_matrix_1d(mesh, 0.0, d, 0, f)))
        A = A + R.kron_matrix(fac)
    r = _rel(A @ u, want)
    print("kronecker sum %dD p=%d: %.2e" % (dim, p, r))
    assert r < 1e-13
    # the restatement's own Kronecker form (the dense reference of the GPU tests)
    assert _rel(R.kron_dense(m, terms) @ u, want) < 1e-13


def _f(x):
    return 1.3 + 0.6 * np.sin(2.1 * x) + 0.2 * x * x


@pytest.mark.parametrize("p", [1, 3, 5, 7, 9])
def test_density_cholesky_1d(p):
    n, lo, hi = p + 3, -0.4, 0.9
    mesh = _capi.mesh_desc(1, p, n, lo, hi)
    f = _f(_capi.field_points(mesh, 0))
    band = _capi.coef_matrix_1d(mesh, 0.0, 0, 0, f)
    lrow, invd = _capi.density_cholesky_1d(mesh, 0, f)
    N = n + 1
    L = np.zeros((N, N))
    for i in range(N):
        for k in range(p + 1):
            j = i - p + k
            if j >= 0:
                L[i, j] = lrow[i, k]
    assert np.allclose(np.diag(L) * invd, 1.0, rtol=1e-15, atol=0)
    A = RD.band_to_dense(band)
    assert np.abs(L @ L.T - A).max() <= 1e-14 * np.abs(A).max()
    # f = None: the factor of the unweighted mass, bit for bit
    l0, d0 = _capi.density_cholesky_1d(mesh, 0, None)
    l1, d1 = _capi.mass_cholesky_1d(mesh, 0)
    assert np.array_equal(l0, l1) and np.array_equal(d0, d1)


def test_density_cholesky_errors_and_tile():
    lib = _capi.load()
    mesh = _capi.mesh_desc(2, 3, (5, 4))
    x = _capi.field_points(mesh, 0)
    with pytest.raises(_capi.GdmError, match="positive definite"):
        _capi.density_cholesky_1d(mesh, 0, x - 0.5)
    bad = np.ones_like(x)
    bad[2] = np.nan
    with pytest.raises(_capi.GdmError, match="finite"):
        _capi.density_cholesky_1d(mesh, 0, bad)
    with pytest.raises(_capi.GdmError):
        _capi.density_cholesky_1d(mesh, 2, None)
    buf = np.zeros(64)
    assert lib.gdm_density_cholesky_1d(ctypes.byref(mesh), 0, None, None, buf.ctypes.data_as(ctypes.c_void_p)) \
        == GDM_ERR_ARG
    for p in (1, 3, 5, 7, 9):
        for dim in (1, 2, 3):
            tx, ty, zc = _capi.density_tile(p, dim)
            assert tx == 64 and 1 <= ty <= 64 and 1 <= zc <= 256
    t = ctypes.c_int(0)
    assert lib.gdm_density_tile(4, 3, ctypes.byref(t), None, None) == GDM_ERR_UNSUPPORTED
    assert lib.gdm_density_tile(3, 4, ctypes.byref(t), None, None) == GDM_ERR_ARG
    assert lib.gdm_density_tile(3, 3, None, None, None) == 0


@pytest.mark.parametrize("dim,n,max_it", [(2, 24, MAX_IT), (3, 12, MAX_IT)])
def test_reference_pcg_converges(dim, n, max_it):
    """numpy PCG on M[rho], p = 3, contrast-10 bump, rel 1e-8, preconditioned by
    W^-1/2 M^-1 W^-1/2: numpy takes 5 iterations in 2D at n = 24 and 7 in 3D at
    n = 12 (measured with this file); MAX_IT = 20 leaves more than a factor 2"""
    m = O.Mesh(dim, 3, n)
    S = R.MassSystem(m, bump_terms(dim))
    b = np.random.default_rng(dim).uniform(-1, 1, m.n_dofs)
    x, its, hist = S.solve(b, rel_tol=1e-8, max_it=max_it)  # raises when max_it is reached
    print("reference pcg %dD n=%d: %d iterations" % (dim, n, its))
    assert 0 < its <= max_it
    assert np.linalg.norm(S.A @ x - b) <= 2e-8 * np.linalg.norm(b)
