"""Grid evaluation, host side (no GPU): the numpy restatement
tests/evalgrid_ref.py against the oracle, and the pure-host C ABI function
gdm_eval_grid_tile.

Meshes: small ones in 1D, 2D and 3D on the anisotropic box (-0.5, 0, 0.2) -
(0.7, 0.9, 1.5) with a different n_sub per axis, so that every h_d differs.

(a) Mesh.error_norms(u, values(u)) is 0 to 1e-13;
(b) load_ref.load_vector(values(u)) equals the oracle mass matrix times u (1e-12);
(c) -flux_load(kappa gradients(u)) equals vardiff_ref.wave_rhs(m, kappa, u, 0)
    (1e-12) for the non-separable kappa of test_gpu_coefgrid.py;
(d) trace identity: with g the exact trace every Nitsche term except
    <v, du/dn> cancels, Mesh.wave_rhs(u, nitsche, gbc=U) - Mesh.wave_rhs(u) =
    h_min (dirichlet_data(m, 1, Dn) - dirichlet_data(m, 0, Dn)) (1e-12);
(e) polynomial exactness: values, gradients, trace and normal derivative of
    the nodal interpolant of a polynomial of degree <= p per variable (1e-11);
(f) wave_rhs_grid equals vardiff_ref.wave_rhs for a callable kappa sampled at
    the same points (1e-13);
(g) the restatement's 1D factors equal gdm_coef_grid_tables_1d;
(h) gdm_eval_grid_tile returns positive extents; the ABI version stays 19.
"""
import ctypes

import numpy as np
import pytest

import evalgrid_ref as E
import load_ref as L
import oracle as O
import vardiff_ref as R

from gdm_amd import _capi

LO3, HI3 = (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)
PIN = [(3, 3, (5, 4, 6)), (3, 1, (3, 2, 4)), (3, 5, (6, 5, 7)), (2, 3, (5, 7)), (2, 7, (9, 8)), (2, 9, (11, 10)),
       (1, 1, (4,)), (1, 5, (8,)), (1, 9, (12,))]
PIN_IDS = ["%dd-p%d" % (c[0], c[1]) for c in PIN]


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(b), 1e-300))


def _mesh(dim, p, n_sub):
    return O.Mesh(dim, p, list(n_sub), list(LO3[:dim]), list(HI3[:dim]))


def _u(m):
    return np.random.default_rng(100 * m.dim + m.p).uniform(-1, 1, m.n_dofs)


def _kappa(dim):
    """the coefficient of test_gpu_coefgrid.py"""
    if dim == 3:
        return lambda x: 2 + np.sin(3 * x[:, 0] * x[:, 1] + 2 * x[:, 2]) + 0.5 * np.cos(5 * (x[:, 0] - x[:, 1] * x[:, 2]))
    if dim == 2:
        return lambda x: 2 + np.sin(3 * x[:, 0] * x[:, 1]) + 0.5 * np.cos(5 * x[:, 0])
    return lambda x: 2 + np.sin(3 * x[:, 0]) + 0.5 * np.cos(5 * x[:, 0])


def _grid_xyz(m):
    """the Gauss grid as (n, 3) points, x fastest"""
    g = [L.grid_values(m, pick) for pick in (lambda x, y, z: x, lambda x, y, z: y, lambda x, y, z: z)]
    return np.stack([a.reshape(-1) for a in g], axis=1)


@pytest.mark.parametrize("dim,p,n_sub", PIN, ids=PIN_IDS)
def test_values_against_error_norms_and_mass(dim, p, n_sub):
    m = _mesh(dim, p, n_sub)
    u = _u(m)
    uq = E.values(m, u)
    assert uq.shape == E.grid_shape(m)
    linf, l1, l2 = m.error_norms(u, L.cell_major(m, uq))
    print("values %dD p=%d: error norms %.2e %.2e %.2e" % (dim, p, linf, l1, l2))
    assert max(linf, l1, l2) <= 1e-13
    rowptr, cols, vals = m.matrix_csr(0)
    r = _rel(L.load_vector(m, uq), O.csr_vmult(rowptr, cols, vals, u))
    print("load(values) vs M u: %.2e" % r)
    assert r <= 1e-12


@pytest.mark.parametrize("dim,p,n_sub", PIN, ids=PIN_IDS)
def test_flux_of_kappa_gradient_is_the_operator(dim, p, n_sub):
    m = _mesh(dim, p, n_sub)
    u = _u(m)
    kq = _kappa(dim)(_grid_xyz(m)).reshape(E.grid_shape(m))
    g = E.gradients(m, u)
    assert g.shape == (dim,) + E.grid_shape(m)
    r = _rel(-E.flux_load(m, kq[None] * g), R.wave_rhs(m, _kappa(dim), u, 0.0))
    print("-flux(kappa grad u) vs K[kappa] u %dD p=%d: %.2e" % (dim, p, r))
    assert r <= 1e-12


@pytest.mark.parametrize("dim,p,n_sub", PIN, ids=PIN_IDS)
def test_trace_identity(dim, p, n_sub):
    m = _mesh(dim, p, n_sub)
    u = _u(m)
    U, Dn = E.trace(m, u)
    assert U.shape == (m.n_boundary_points(),)
    gamma = 6.0 * p * p
    hmin = min(float(m.h[d]) for d in range(dim))
    lhs = m.wave_rhs(u, nitsche=gamma, gbc=U) - m.wave_rhs(u, nitsche=0.0)
    rhs = hmin * (L.dirichlet_data(m, 1.0, Dn) - L.dirichlet_data(m, 0.0, Dn))
    r = _rel(lhs, rhs)
    print("trace identity %dD p=%d: %.2e" % (dim, p, r))
    assert r <= 1e-12


def _poly(dim, p):
    """a polynomial of degree p per variable with its gradient, on points x (n, 3)"""
    c = np.random.default_rng(p).uniform(-1, 1, (dim, p + 1))

    def f1(d, t, deriv):
        k = np.arange(p + 1)
        if not deriv:
            return (c[d][None, :] * t[:, None] ** k[None, :]).sum(axis=1)
        return (c[d][None, 1:] * k[None, 1:] * t[:, None] ** (k[None, 1:] - 1)).sum(axis=1)

    def value(x):
        return np.prod([f1(d, x[:, d], False) for d in range(dim)], axis=0)

    def grad(x, e):
        return np.prod([f1(d, x[:, d], d == e) for d in range(dim)], axis=0)

    return value, grad


@pytest.mark.parametrize("dim,p,n_sub", PIN, ids=PIN_IDS)
def test_polynomial_exactness(dim, p, n_sub):
    m = _mesh(dim, p, n_sub)
    value, grad = _poly(dim, p)
    vc = m.vertex_coords()
    xv = np.stack(list(vc) + [np.zeros_like(vc[0])] * (3 - dim), axis=1)
    u = value(xv)
    xq = _grid_xyz(m)
    assert _rel(E.values(m, u), value(xq)) <= 1e-11
    g = E.gradients(m, u)
    for e in range(dim):
        assert _rel(g[e], grad(xq, e)) <= 1e-11
    xb = m.boundary_points()
    U, Dn = E.trace(m, u)
    assert _rel(U, value(xb)) <= 1e-11
    # the outward normal of a boundary point: the direction in which it sits on the box
    want = np.zeros(xb.shape[0])
    hit = np.zeros(xb.shape[0], dtype=int)
    for d in range(dim):
        for side, wall in ((-1.0, float(m.lo[d])), (1.0, float(m.hi[d]))):
            on = np.abs(xb[:, d] - wall) <= 1e-12
            want[on] = side * grad(xb[on], d)
            hit[on] += 1
    assert np.all(hit == 1)  # face Gauss points lie inside their faces
    assert _rel(Dn, want) <= 1e-11


@pytest.mark.parametrize("dim,p,n_sub", PIN, ids=PIN_IDS)
def test_wave_rhs_grid_equals_the_callable_form(dim, p, n_sub):
    m = _mesh(dim, p, n_sub)
    u = _u(m)
    kappa = _kappa(dim)
    kq, kbc = kappa(_grid_xyz(m)), kappa(m.boundary_points())
    gbc = np.random.default_rng(p + dim).uniform(-1, 1, m.n_boundary_points())
    gamma = 6.0 * p * p
    for nit, g in ((0.0, None), (gamma, None), (gamma, gbc)):
        r = _rel(E.wave_rhs_grid(m, kq, kbc, u, nit, g), R.wave_rhs(m, kappa, u, nit, g))
        print("wave_rhs_grid %dD p=%d nitsche=%g: %.2e" % (dim, p, nit, r))
        assert r <= 1e-13
    assert _rel(E.wave_rhs_grid(m, kq, kbc, None, gamma, gbc), R.wave_rhs(m, kappa, None, gamma, gbc)) <= 1e-13


@pytest.mark.parametrize("p", [1, 3, 5, 7, 9])
def test_factors_equal_the_kernel_tables(p):
    m = _mesh(3, p, (p + 2, p, p + 5))
    mesh = _capi.mesh_desc(3, p, [p + 2, p, p + 5])
    for d in range(3):
        mesh.lo[d], mesh.hi[d] = LO3[d], HI3[d]
    for d in range(3):
        val, der, first = _capi.coef_grid_tables_1d(mesh, d)
        v, g, f = E.factors_1d(m, d)
        assert np.array_equal(np.asarray(first).reshape(-1), f)
        assert np.abs(np.asarray(val).reshape(v.shape) - v).max() <= 1e-14 * np.abs(v).max()
        assert np.abs(np.asarray(der).reshape(g.shape) - g).max() <= 1e-13 * np.abs(g).max()


def test_eval_grid_tile_and_abi_version():
    lib = _capi.load()
    assert lib.gdm_abi_version() == 19
    for p in (1, 3, 5, 7, 9):
        for dim in (1, 2, 3):
            cx, cy, cz = _capi.eval_grid_tile(p, dim)
            assert cx > 0 and cy > 0 and cz > 0
    t = ctypes.c_int(0)
    assert lib.gdm_eval_grid_tile(4, 3, ctypes.byref(t), ctypes.byref(t), ctypes.byref(t)) == -3
    assert lib.gdm_eval_grid_tile(3, 0, ctypes.byref(t), ctypes.byref(t), ctypes.byref(t)) == -1
    assert lib.gdm_eval_grid_tile(3, 3, None, None, None) == 0
