"""Separable advection field, host side (no GPU): the numpy helper
tests/varfield_ref.py against the oracle, and the pure-host C ABI functions
gdm_field_points / gdm_field_matrix_1d.

(a) the helper with a constant field equals Mesh.advection_rhs (the oracle's
    cell loop, pinned to the reference goldens) to rel-L2 1e-13;
(b) gdm_field_matrix_1d with f = 1 equals Mesh.matrices_1d, and the Kronecker
    products of the returned bands equal the helper's volume term for a
    rotation and a swirl field to 1e-13: the factorisation itself;
(c) gdm_field_points = lo, the cells' Gauss points along the axis, hi.
"""
import numpy as np
import pytest

import oracle as O
import varfield_ref as R

from gdm_amd import _capi


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("dim,n_sub,lo,hi", [
    (1, (9,), (-0.3,), (1.1,)),
    (2, (6, 5), (0.0, -1.0), (1.5, 0.2)),
    (3, (7, 5, 4), (0.0, -0.5, 0.1), (1.0, 0.7, 0.9)),
])
def test_helper_constant_field_equals_oracle(dim, n_sub, lo, hi):
    p = 3
    m = O.Mesh(dim, p, list(n_sub), list(lo), list(hi))
    rng = np.random.default_rng(dim)
    u = rng.uniform(-1, 1, m.n_dofs)
    bc = rng.uniform(-1, 1, m.n_boundary_points())
    for a in [(0.8, -0.45, 0.3)[:dim], (-0.6, 0.2, -0.9)[:dim]]:
        field = lambda x, a=a: np.tile(np.asarray(a), (x.shape[0], 1))  # noqa: E731
        assert _rel(R.advection_rhs(m, field, u, bc), m.advection_rhs(a, u, bc)) < 1e-13
        assert _rel(R.advection_rhs(m, field, u), m.advection_rhs(a, u)) < 1e-13


def test_field_matrix_unit_factor_equals_oracle_matrices():
    for p, n, lo, hi in [(1, 4, 0.0, 1.0), (3, 7, -0.5, 0.7), (5, 11, 0.0, 2.0), (9, 9, 0.0, 1.0)]:
        mesh = _capi.mesh_desc(1, p, [n], lo, hi)
        M, C, _ = O.Mesh(1, p, [n], lo, hi).matrices_1d(0)
        ones = np.ones(n * (p + 1) + 2)
        # both sides sum the same (p+1)-point quadrature products per cell in fp64: entries agree to a few
        # ulps of the largest entry (1e-13 relative to it leaves two digits of margin at p = 9)
        for f in (None, ones):
            for which, want in ((0, M), (1, C)):
                got = _capi.field_matrix_1d(mesh, 0, which, f)
                assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


FIELDS_2D = {
    # rotation about (0.4, 0.3): (-(y - yc), x - xc)
    "rotation": ([(0, [None, lambda y: -(y - 0.3)]), (1, [lambda x: x - 0.4, None])],
                 lambda x: np.stack([-(x[:, 1] - 0.3), x[:, 0] - 0.4], axis=1)),
    # LeVeque's swirl: (sin^2(pi x) sin(2 pi y), -sin^2(pi y) sin(2 pi x))
    "swirl": ([(0, [lambda x: np.sin(np.pi * x) ** 2, lambda y: np.sin(2 * np.pi * y)]),
               (1, [lambda x: -np.sin(2 * np.pi * x), lambda y: np.sin(np.pi * y) ** 2])],
              lambda x: np.stack([np.sin(np.pi * x[:, 0]) ** 2 * np.sin(2 * np.pi * x[:, 1]),
                                  -np.sin(np.pi * x[:, 1]) ** 2 * np.sin(2 * np.pi * x[:, 0])], axis=1)),
}


@pytest.mark.parametrize("name", sorted(FIELDS_2D))
def test_field_matrices_kron_equals_helper_volume_term(name):
    terms, field = FIELDS_2D[name]
    mesh = _capi.mesh_desc(2, 3, [9, 7], 0.0, 1.0)
    mesh.hi[1] = 0.8
    m = O.Mesh(2, 3, [9, 7], [0.0, 0.0], [1.0, 0.8])
    u = np.random.default_rng(5).uniform(-1, 1, m.n_dofs)
    kron = []
    for comp, factors in terms:
        ops = []
        for d in range(2):
            f = factors[d]
            s = None if f is None else np.array([f(x) for x in _capi.field_points(mesh, d)])
            ops.append(_capi.field_matrix_1d(mesh, d, 1 if d == comp else 0, s))
        kron.append((ops[0], ops[1], None))
    assert _rel(m.kron_apply(kron, u), R.advection_rhs(m, field, u, faces=False)) < 1e-13


@pytest.mark.parametrize("dim,p,n_sub", [(1, 1, (4,)), (2, 3, (9, 7)), (3, 5, (6, 5, 7))])
def test_field_points(dim, p, n_sub):
    lo, hi = [-0.2, 0.1, 0.0][:dim], [0.9, 1.3, 2.0][:dim]
    mesh = _capi.mesh_desc(dim, p, list(n_sub))
    for d in range(dim):
        mesh.lo[d], mesh.hi[d] = lo[d], hi[d]
    m = O.Mesh(dim, p, list(n_sub), lo, hi)
    xyz = m.cell_qpoints().reshape(m.n_cells, (p + 1) ** dim, 3)
    for d in range(dim):
        x = _capi.field_points(mesh, d)
        assert x.size == n_sub[d] * (p + 1) + 2
        assert x[0] == lo[d] and x[-1] == hi[d]
        # the cells along direction d (the other cell indices 0), their points along d
        stride_c = int(np.prod(n_sub[:d]))
        stride_q = (p + 1) ** d
        want = np.concatenate([xyz[c * stride_c, stride_q * np.arange(p + 1), d] for c in range(n_sub[d])])
        assert np.allclose(x[1:-1], want, rtol=0, atol=1e-15)


def test_field_host_errors():
    mesh = _capi.mesh_desc(2, 3, [9, 7])
    lib = _capi.load()
    x = np.zeros(64)
    import ctypes

    assert lib.gdm_field_points(ctypes.byref(mesh), 2, x.ctypes.data_as(ctypes.c_void_p)) == -1
    assert "axis" in _capi.last_error()
    assert lib.gdm_field_matrix_1d(ctypes.byref(mesh), 0, 2, None, x.ctypes.data_as(ctypes.c_void_p)) == -1
    assert _capi.field_tile(5) == _capi.field_tile(3)
