"""Separable coefficient of the wave / heat / Poisson operator, host side (no
GPU): the numpy restatement tests/vardiff_ref.py against the oracle, and the
pure-host C ABI functions gdm_coef_matrix_1d / gdm_coef_tile.

(a) the restatement with kappa = 1 equals Mesh.wave_rhs (the oracle's cell
    loop, pinned to the reference goldens) with nitsche 0 and > 0 and with
    Dirichlet data, to rel-L2 1e-13;
(b) gdm_coef_matrix_1d: f = 1 gives the homogeneous band, the band is
    symmetric, and for a non-trivial f it equals the restatement's 1D assembly
    at every odd p to 1e-13 relative;
(c) the Kronecker sum of the bands equals the restatement for a 2-term kappa
    in 2D and 3D on p-cell meshes: the factorisation itself;
(d) argument errors.
"""
import ctypes

import numpy as np
import pytest

import oracle as O
import vardiff_ref as R

from gdm_amd import _capi

GDM_ERR_ARG, GDM_ERR_UNSUPPORTED = -1, -3


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _one(x):
    return np.ones(x.shape[0])


@pytest.mark.parametrize("dim,n_sub,lo,hi", [
    (1, (9,), (-0.3,), (1.1,)),
    (2, (6, 5), (0.0, -1.0), (1.5, 0.2)),
    (3, (7, 5, 4), (0.0, -0.5, 0.1), (1.0, 0.7, 0.9)),
])
def test_restatement_unit_coefficient_equals_oracle(dim, n_sub, lo, hi):
    p = 3
    m = O.Mesh(dim, p, list(n_sub), list(lo), list(hi))
    rng = np.random.default_rng(dim)
    u = rng.uniform(-1, 1, m.n_dofs)
    g = rng.uniform(-1, 1, m.n_boundary_points())
    assert _rel(R.wave_rhs(m, _one, u), m.wave_rhs(u)) < 1e-13
    assert _rel(R.wave_rhs(m, _one, u, 7.5), m.wave_rhs(u, nitsche=7.5)) < 1e-13
    assert _rel(R.wave_rhs(m, _one, u, 7.5, g), m.wave_rhs(u, nitsche=7.5, gbc=g)) < 1e-13
    assert _rel(R.wave_rhs(m, _one, None, 7.5, g), m.wave_rhs(u, impl=False, nitsche=7.5, gbc=g)) < 1e-13


def _f(x):
    return 1.3 + 0.6 * np.sin(2.1 * x) + 0.2 * x * x


@pytest.mark.parametrize("p", [1, 3, 5, 7, 9])
def test_coef_matrix_1d(p):
    n, lo, hi, nitsche = p + 3, -0.4, 0.9, 6.0 * p * p
    mesh = _capi.mesh_desc(1, p, n, lo, hi)
    m = O.Mesh(1, p, n, lo, hi)
    x = _capi.field_points(mesh, 0)
    for nit in (0.0, nitsche):
        # f = 1: the homogeneous operator
        ref = R.dense_to_band(R.dense_matrix(m, _one, nit), p)
        for f in (None, np.ones_like(x)):
            B1 = _capi.coef_matrix_1d(mesh, nit, 0, 1, f)
            assert np.abs(B1 - ref).max() <= 1e-13 * np.abs(ref).max()
            M1 = _capi.coef_matrix_1d(mesh, nit, 0, 0, f)
            assert np.abs(M1 - m.matrices_1d(0)[0]).max() <= 1e-13 * np.abs(M1).max()
        # a non-trivial f against the restatement's 1D assembly
        Mr, Br = R.factors_1d(m, 0, _f, nit)
        Mf = R.band_to_dense(_capi.coef_matrix_1d(mesh, nit, 0, 0, _f(x)))
        Bf = R.band_to_dense(_capi.coef_matrix_1d(mesh, nit, 0, 1, _f(x)))
        assert np.abs(Mf - Mr).max() <= 1e-13 * np.abs(Mr).max()
        assert np.abs(Bf - Br).max() <= 1e-13 * np.abs(Br).max()
        assert np.array_equal(Mf, Mf.T) or np.abs(Mf - Mf.T).max() <= 1e-15 * np.abs(Mf).max()
        assert np.abs(Bf - Bf.T).max() <= 1e-14 * np.abs(Bf).max()


def test_unit_factor_gives_the_bits_of_the_homogeneous_band():
    mesh = _capi.mesh_desc(2, 5, [7, 9], 0.0, 1.0)
    for axis in (0, 1):
        assert np.array_equal(_capi.coef_matrix_1d(mesh, 0.0, axis, 0), _capi.field_matrix_1d(mesh, axis, 0))


@pytest.mark.parametrize("dim,p", [(2, 3), (3, 3), (2, 5)])
def test_kronecker_sum_equals_restatement(dim, p):
    lo, hi = (-0.5, 0.0, 0.2)[:dim], (0.7, 0.9, 1.5)[:dim]
    n_sub = [p, p + 1, p][:dim]
    nitsche = 5.0 * p * p
    m = O.Mesh(dim, p, n_sub, list(lo), list(hi))
    mesh = _capi.MeshDesc()
    mesh.dim, mesh.fe_degree, mesh.n_ranks = dim, p, 1
    for d in range(3):
        mesh.n_subdivisions[d] = n_sub[d] if d < dim else 1
        mesh.lo[d], mesh.hi[d] = (lo[d], hi[d]) if d < dim else (0.0, 1.0)
    # kappa = (1 + 0.5 sin 3x) e^y [1 + z^2] + 0.3 (2 + x) (1 + y) [cos z]
    terms = [[lambda x: 1 + 0.5 * np.sin(3 * x), np.exp, lambda z: 1 + z * z][:dim],
             [lambda x: 0.3 * (2 + x), lambda y: 1 + y, np.cos][:dim]]

    def kappa(x):
        return sum(np.prod([t[d](x[:, d]) for d in range(dim)], axis=0) for t in terms)

    rng = np.random.default_rng(p)
    u = rng.uniform(-1, 1, m.n_dofs)
    for nit in (0.0, nitsche):
        kron = []
        for t in terms:
            M = [_capi.coef_matrix_1d(mesh, nit, d, 0, t[d](_capi.field_points(mesh, d))) for d in range(dim)]
            B = [_capi.coef_matrix_1d(mesh, nit, d, 1, t[d](_capi.field_points(mesh, d))) for d in range(dim)]
            for d in range(dim):
                kron.append(tuple(B[e] if e == d else M[e] for e in range(dim)))
        assert _rel(m.kron_apply(kron, u), R.wave_rhs(m, kappa, u, nit)) < 1e-13


def test_argument_errors():
    L = _capi.load()
    mesh = _capi.mesh_desc(2, 3, 5, 0.0, 1.0)
    band = np.zeros((6, 7))
    bp = band.ctypes.data_as(ctypes.c_void_p)
    assert L.gdm_coef_matrix_1d(ctypes.byref(mesh), 0.0, 0, 2, None, bp) == GDM_ERR_ARG
    assert L.gdm_coef_matrix_1d(ctypes.byref(mesh), 0.0, 2, 0, None, bp) == GDM_ERR_ARG
    assert L.gdm_coef_matrix_1d(ctypes.byref(mesh), float("nan"), 0, 1, None, bp) == GDM_ERR_ARG
    assert L.gdm_coef_matrix_1d(ctypes.byref(mesh), 0.0, 0, 0, None, None) == GDM_ERR_ARG
    assert L.gdm_coef_matrix_1d(None, 0.0, 0, 0, None, bp) == GDM_ERR_ARG
    even = _capi.mesh_desc(2, 4, 5, 0.0, 1.0)
    assert L.gdm_coef_matrix_1d(ctypes.byref(even), 0.0, 0, 0, None, bp) == GDM_ERR_UNSUPPORTED
    # the advection entry point keeps its range
    assert L.gdm_field_matrix_1d(ctypes.byref(mesh), 0, 2, None, bp) == GDM_ERR_ARG
    t = [ctypes.c_int(0) for _ in range(3)]
    assert L.gdm_coef_tile(4, 3, *[ctypes.byref(v) for v in t]) == GDM_ERR_UNSUPPORTED
    assert L.gdm_coef_tile(3, 4, *[ctypes.byref(v) for v in t]) == GDM_ERR_ARG
    for p in (1, 3, 5, 7, 9):
        tx, ty, zc = _capi.coef_tile(p, 3)
        assert tx >= 1 and ty >= 1 and zc >= 1
    assert _capi.COEF_MAX_TERMS == 4
