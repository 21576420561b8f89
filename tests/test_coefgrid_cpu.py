"""General coefficient on the Gauss grid, host side (no GPU): the tables of the
grid kernel (gdm_coef_grid_tables_1d) and its tile (gdm_coef_grid_tile).

For p in {1, 3, 5, 7, 9} on an anisotropic box with n_sub = p and p + 3 and a
non-trivial f, the tables composed in numpy,
  B^T diag(w h f) B   and   D^T diag(w h f) D,
must reproduce the bands of gdm_coef_matrix_1d(which = 0) and of which = 1 at
nitsche = 0 (up to its sign: B[f] = -L[f]) to 1e-13 relative; `first` equals
the oracle's DoF-box offset.
"""
import ctypes

import numpy as np
import pytest

import oracle as O
import vardiff_ref as R

from gdm_amd import _capi

GDM_ERR_ARG, GDM_ERR_UNSUPPORTED = -1, -3
LO, HI = (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)


def _mesh_desc(dim, p, n_sub, lo, hi):
    m = _capi.MeshDesc()
    m.dim, m.fe_degree, m.n_ranks = dim, p, 1
    for d in range(3):
        m.n_subdivisions[d] = n_sub[d] if d < dim else 1
        m.lo[d], m.hi[d] = (lo[d], hi[d]) if d < dim else (0.0, 1.0)
    return m


def _f(x):
    return 1.3 + 0.6 * np.sin(2.1 * x) + 0.2 * x * x


@pytest.mark.parametrize("p", [1, 3, 5, 7, 9])
def test_tables_reproduce_the_weighted_bands(p):
    n_sub = [p, p + 3, p]
    mesh = _mesh_desc(3, p, n_sub, LO, HI)
    xq, wq = O.gauss(p + 1)
    for axis in range(3):
        n, n1 = n_sub[axis], p + 1
        h = (HI[axis] - LO[axis]) / n
        val, der, first = _capi.coef_grid_tables_1d(mesh, axis)
        assert val.shape == (n * n1, n1) and der.shape == (n * n1, n1) and first.shape == (n * n1,)
        # first: the oracle's DoF-box offset of the point's cell
        m1 = O.Mesh(1, p, n, LO[axis], HI[axis])
        want_first = np.repeat([int(m1.cell_dofs(c)[0]) for c in range(n)], n1)
        assert np.array_equal(first, want_first)
        # dense (Q x N) matrices of values and derivatives
        Bv, Dv = np.zeros((n * n1, n + 1)), np.zeros((n * n1, n + 1))
        for q in range(n * n1):
            Bv[q, first[q]:first[q] + n1] = val[q]
            Dv[q, first[q]:first[q] + n1] = der[q]
        x = _capi.field_points(mesh, axis)
        f = _f(x)
        w = np.tile(wq, n) * h * f[1:-1]
        M = R.band_to_dense(_capi.coef_matrix_1d(mesh, 0.0, axis, 0, f))
        L = -R.band_to_dense(_capi.coef_matrix_1d(mesh, 0.0, axis, 1, f))
        gotM, gotL = Bv.T @ (w[:, None] * Bv), Dv.T @ (w[:, None] * Dv)
        eM, eL = np.abs(gotM - M).max() / np.abs(M).max(), np.abs(gotL - L).max() / np.abs(L).max()
        print("tables p=%d axis=%d: M %.2e L %.2e" % (p, axis, eM, eL))
        assert eM <= 1e-13 and eL <= 1e-13
        # partition of unity at every Gauss point
        assert np.abs(val.sum(axis=1) - 1.0).max() <= 1e-12 and np.abs(der.sum(axis=1)).max() * h <= 1e-10


def test_tile_abi_and_argument_errors():
    L = _capi.load()
    assert L.gdm_abi_version() == 19
    for p in (1, 3, 5, 7, 9):
        for dim in (1, 2, 3):
            tx, ty, zc = _capi.coef_grid_tile(p, dim)
            assert tx >= 1 and ty >= 1 and zc >= 1
    t = [ctypes.c_int(0) for _ in range(3)]
    assert L.gdm_coef_grid_tile(4, 3, *[ctypes.byref(v) for v in t]) == GDM_ERR_UNSUPPORTED
    assert L.gdm_coef_grid_tile(3, 4, *[ctypes.byref(v) for v in t]) == GDM_ERR_ARG
    mesh = _capi.mesh_desc(2, 3, 5, 0.0, 1.0)
    val, der, first = np.zeros((20, 4)), np.zeros((20, 4)), np.zeros(20, dtype=np.int32)
    ptr = [a.ctypes.data_as(ctypes.c_void_p) for a in (val, der, first)]
    assert L.gdm_coef_grid_tables_1d(ctypes.byref(mesh), 2, *ptr) == GDM_ERR_ARG
    assert L.gdm_coef_grid_tables_1d(ctypes.byref(mesh), 0, None, ptr[1], ptr[2]) == GDM_ERR_ARG
    assert L.gdm_coef_grid_tables_1d(None, 0, *ptr) == GDM_ERR_ARG
    even = _capi.mesh_desc(2, 4, 5, 0.0, 1.0)
    assert L.gdm_coef_grid_tables_1d(ctypes.byref(even), 0, *ptr) == GDM_ERR_UNSUPPORTED
    assert "gdm_op_set_coefficient_grid" in _capi.declared_symbols()
