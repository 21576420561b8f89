"""tests/stencil_ref.py (1D bands of every kind in Kronecker form) against the
oracle's reference-faithful cell loops, for every degree.  CPU only.

Tolerance: rel-L2 1e-13, the tighter of the two figures tests/test_oracle_kron.py
uses for cell loop against Kronecker form (measured here: at most 1.2e-15).

The wave cases in 3D at p = 7, 9 take 5 to 50 s each (the cell loop costs
O((p+1)^6) per cell and every cell of these meshes has its own category
tuple); they carry the `slow` marker.  The convective band is checked in 3D up
to p = 7: its 3D form differs from the wave's only by the 1D band, which the
2D cases pin at every degree.
"""
import numpy as np
import pytest

import oracle as O
import stencil_ref as R

RTOL = 1e-13
DEGREES = (1, 3, 5, 7, 9)
A = (0.8, -0.45, 0.3)
# anisotropic boxes: h_min differs from h_d in every direction but one
BOX2 = ((-0.5, 0.0), (0.7, 0.9))
BOX3 = ((-0.5, 0.0, 0.2), (0.7, 0.9, 1.5))


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _u(m, seed):
    return np.random.default_rng(seed).uniform(-1, 1, m.n_dofs)


def _nsub_2d(p):
    return (2 * p + 3, p + 2)


def _cases_3d():
    """the smallest meshes: n_sub = p and p + 2 per direction"""
    out = []
    for p in DEGREES:
        for n in (p, p + 2):
            out.append(pytest.param(p, (n, n, n), id="p%d-n%d" % (p, n), marks=[pytest.mark.slow] if p >= 7 else []))
    return out


def test_band_transpose_is_the_dense_transpose():
    p, n = 3, 9
    rng = np.random.default_rng(1)
    D = np.triu(np.tril(rng.uniform(-1, 1, (n, n)), p), -p)
    band = np.zeros((n, 2 * p + 1))
    for i in range(n):
        for k in range(2 * p + 1):
            j = i - p + k
            if 0 <= j < n:
                band[i, k] = D[i, j]
    T = R.band_transpose(band, p)
    for i in range(n):
        for k in range(2 * p + 1):
            j = i - p + k
            assert T[i, k] == (D[j, i] if 0 <= j < n else 0.0)


@pytest.mark.parametrize("p", DEGREES)
def test_convective_2d(p):
    m = O.Mesh(2, p, _nsub_2d(p), *BOX2)
    u = _u(m, 10 + p)
    err = _rel(R.apply(m, "convective", A, u), m.convective_rhs(A[:2], u))
    print("convective 2D p=%d rel %.3e" % (p, err))
    assert err <= RTOL


@pytest.mark.parametrize("p,nsub", [(1, (1, 1, 1)), (1, (3, 3, 3)), (3, (5, 5, 5)), (5, (7, 7, 7)), (7, (7, 7, 7))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_convective_3d(p, nsub):
    m = O.Mesh(3, p, nsub, *BOX3)
    u = _u(m, 20 + p)
    err = _rel(R.apply(m, "convective", A, u), m.convective_rhs(A, u))
    print("convective 3D p=%d %s rel %.3e" % (p, nsub, err))
    assert err <= RTOL


@pytest.mark.parametrize("gamma", (4.0, 15.0))
@pytest.mark.parametrize("p", DEGREES)
def test_wave_nitsche_2d(p, gamma):
    m = O.Mesh(2, p, _nsub_2d(p), *BOX2)
    assert R.h_min(m) < max(m.h[:2])
    u = _u(m, 30 + p)
    err = _rel(R.apply(m, "wave", (gamma,), u), m.wave_rhs(u, impl=True, nitsche=gamma))
    print("wave 2D p=%d gamma=%g rel %.3e" % (p, gamma, err))
    assert err <= RTOL


@pytest.mark.parametrize("gamma", (4.0, 15.0))
@pytest.mark.parametrize("p,nsub", _cases_3d())
def test_wave_nitsche_3d(p, nsub, gamma):
    m = O.Mesh(3, p, nsub, *BOX3)
    assert R.h_min(m) < max(m.h)
    u = _u(m, 40 + p)
    err = _rel(R.apply(m, "wave", (gamma,), u), m.wave_rhs(u, impl=True, nitsche=gamma))
    print("wave 3D p=%d %s gamma=%g rel %.3e" % (p, nsub, gamma, err))
    assert err <= RTOL


@pytest.mark.parametrize("p", (3, 9))
def test_wave_without_nitsche_is_minus_L(p):
    m = O.Mesh(2, p, _nsub_2d(p), *BOX2)
    for d in range(2):
        assert np.array_equal(R.band_1d(m, d, "wave"), -m.matrices_1d(d)[2])
        assert np.array_equal(R.band_1d(m, d, "advection", A), m.advection_outflow_B(d, A[d]))
