"""Forcing and Dirichlet data of the uncut wave operator, host side (no GPU):
the numpy helper tests/load_ref.py against the oracle, and the pure-host C ABI
functions gdm_load_vector_1d / gdm_load_tile.

(a) the helper's two terms equal Mesh.wave_rhs(0, impl=False, fq, nitsche,
    gbc) (the oracle's cell loop, pinned to the reference goldens) to rel-L2
    1e-13, each alone and both together, on small anisotropic meshes;
(b) gdm_load_vector_1d equals the 1D oracle to 1e-14;
(c) the outer product of three 1D load vectors equals the helper's load of a
    sine product to 1e-13: the factorisation the rank-1 device path uses;
(d) argument and error-code checks of the pure-host entry points.
"""
import ctypes

import numpy as np
import pytest

import load_ref as R
import oracle as O

from gdm_amd import _capi


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


PIN = [
    (3, 3, (5, 4, 6), (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)),
    (3, 5, (6, 5, 7), (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)),
    (2, 7, (9, 8), (0.0, -1.0), (1.5, 0.2)),
    (2, 9, (12, 10), (0.0, -1.0), (1.5, 0.2)),
] + [(1, p, (p + 4,), (-0.3,), (1.1,)) for p in (1, 3, 5, 7, 9)]


@pytest.mark.parametrize("dim,p,n_sub,lo,hi", PIN, ids=["%dd-p%d" % (c[0], c[1]) for c in PIN])
def test_helper_equals_oracle(dim, p, n_sub, lo, hi):
    m = O.Mesh(dim, p, list(n_sub), list(lo), list(hi))
    rng = np.random.default_rng(10 * dim + p)
    fgrid = rng.uniform(-1, 1, [int(m.nsub[d]) * (p + 1) for d in reversed(range(dim))])
    gbc = rng.uniform(-1, 1, m.n_boundary_points())
    zero = np.zeros(m.n_dofs)
    fq = R.cell_major(m, fgrid)
    load, data = R.load_vector(m, fgrid), R.dirichlet_data(m, 15.0, gbc)
    e_load = _rel(load, m.wave_rhs(zero, impl=False, fq=fq))
    e_data = _rel(data, m.wave_rhs(zero, impl=False, nitsche=15.0, gbc=gbc))
    e_both = _rel(load + data, m.wave_rhs(zero, impl=False, fq=fq, nitsche=15.0, gbc=gbc))
    print("helper vs oracle dim %d p %d: load %.2e data %.2e both %.2e" % (dim, p, e_load, e_data, e_both))
    assert e_load <= 1e-13 and e_data <= 1e-13 and e_both <= 1e-13


def test_helper_cell_major_is_the_oracle_point_order():
    """x at the Gauss points through cell_major equals Mesh.cell_qpoints"""
    m = O.Mesh(3, 3, [4, 3, 5], [-0.5, 0.0, 0.2], [0.7, 0.9, 1.5])
    xyz = m.cell_qpoints()
    for d, pick in enumerate((lambda x, y, z: x, lambda x, y, z: y, lambda x, y, z: z)):
        assert np.abs(R.cell_major(m, R.grid_values(m, pick)) - xyz[:, d]).max() <= 1e-15


@pytest.mark.parametrize("p", [1, 3, 5, 7, 9])
def test_load_vector_1d_equals_oracle(p):
    n, lo, hi = p + 6, -0.3, 1.1
    mesh = _capi.mesh_desc(1, p, [n], lo, hi)
    m = O.Mesh(1, p, [n], lo, hi)
    rng = np.random.default_rng(p)
    f = rng.uniform(-1, 1, n * (p + 1) + 2)
    zero = np.zeros(m.n_dofs)
    for samples, fq in ((f, f[1:-1]), (None, np.ones(n * (p + 1)))):
        got = _capi.load_vector_1d(mesh, 0, samples)
        want = m.wave_rhs(zero, impl=False, fq=fq)
        assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    # the two end values (the box faces' samples of gdm_field_points) are not read
    f2 = f.copy()
    f2[0], f2[-1] = 7.0, -9.0
    assert np.array_equal(_capi.load_vector_1d(mesh, 0, f2), _capi.load_vector_1d(mesh, 0, f))


@pytest.mark.parametrize("dim,p,n_sub", [(3, 3, (5, 4, 6)), (3, 5, (6, 5, 7)), (2, 7, (9, 8)), (1, 9, (11,))])
def test_outer_product_of_1d_load_vectors_is_the_sine_load(dim, p, n_sub):
    lo, hi = (-0.5, 0.0, 0.2)[:dim], (0.7, 0.9, 1.5)[:dim]
    m = O.Mesh(dim, p, list(n_sub), list(lo), list(hi))
    mesh = _capi.mesh_desc(dim, p, list(n_sub))
    for d in range(dim):
        mesh.lo[d], mesh.hi[d] = lo[d], hi[d]
    a, k, phi, t = (0.3, 0.0, -0.2), (1.0, 0.75, 1.25), (0.1, 0.4, -0.3), 0.37
    want = R.load_vector(m, R.grid_values(m, R.fn_sine_product(a, k, phi, t, dim)))
    b = []
    for d in range(dim):
        x = _capi.field_points(mesh, d)
        b.append(_capi.load_vector_1d(mesh, d, np.sin(2 * np.pi * k[d] * (x - a[d] * t) + phi[d])))
    got = b[0]
    for d in range(1, dim):
        got = np.multiply.outer(b[d], got)
    assert _rel(got.reshape(-1), want) <= 1e-13


def test_pure_host_entry_points_check_their_arguments():
    L = _capi.load()
    assert L.gdm_abi_version() == 19
    mesh = _capi.mesh_desc(2, 3, [5, 4])
    b = np.zeros(8)
    bp = b.ctypes.data_as(ctypes.c_void_p)
    assert L.gdm_load_vector_1d(ctypes.byref(mesh), 0, None, bp) == 0
    assert L.gdm_load_vector_1d(ctypes.byref(mesh), 2, None, bp) == -1   # axis outside [0, dim)
    assert L.gdm_load_vector_1d(ctypes.byref(mesh), -1, None, bp) == -1
    assert L.gdm_load_vector_1d(ctypes.byref(mesh), 0, None, None) == -1  # NULL output
    assert L.gdm_load_vector_1d(None, 0, None, bp) == -1
    assert "b_host" in _capi.last_error() or "NULL" in _capi.last_error()
    even = _capi.mesh_desc(2, 4, [5, 4])
    assert L.gdm_load_vector_1d(ctypes.byref(even), 0, None, bp) == -3    # even degree: not tabulated
    thin = _capi.mesh_desc(2, 5, [4, 6])
    assert L.gdm_load_vector_1d(ctypes.byref(thin), 0, None, bp) == -1    # n_subdivisions < fe_degree
    with pytest.raises(_capi.GdmError):
        _capi.load_vector_1d(mesh, 0, np.zeros(7))                        # wrong sample count
    for p in (1, 3, 5, 7, 9):
        for dim in (1, 2, 3):
            tx, ty, zc = _capi.load_tile(p, dim)
            assert tx > 0 and ty > 0 and zc > 0
    t = ctypes.c_int(0)
    assert L.gdm_load_tile(4, 3, ctypes.byref(t), ctypes.byref(t), ctypes.byref(t)) == -3
    assert L.gdm_load_tile(11, 3, ctypes.byref(t), ctypes.byref(t), ctypes.byref(t)) == -3
    assert L.gdm_load_tile(3, 0, ctypes.byref(t), ctypes.byref(t), ctypes.byref(t)) == -1
    assert L.gdm_load_tile(3, 4, ctypes.byref(t), ctypes.byref(t), ctypes.byref(t)) == -1
    assert L.gdm_load_tile(3, 3, None, None, None) == 0
