"""The host side of the grid density (gdm_op_set_density_grid): the pure-host
entry points, and the numpy side of tests/test_gpu_massgrid_solve.py
(tests/massgrid_ref.py): the PCG counts that the GPU tests compare against are
pinned here and shown not to be borderline.

density_solve, rel_tol 1e-8, preconditioner W^-1/2 M^-1 W^-1/2 with W from the
dense diagonals (counts, margin = smallest relative distance of a residual from
the threshold):
  2D n = 24: osc 4, ellipse 5 (margins >= 0.8);  3D n = 8: osc 6, ellipse 8 (>= 0.45).
With the preconditioner of ANOTHER density (osc's W for the ellipse: what an
in-place overwrite would leave if W were kept from the set call) the same recipe
needs 33 (2D) and 22 (3D) iterations: still convergent, but more than MAX_IT =
20, which is why gdm_density_solve forms W from the samples of each solve.

coef_solve, alpha = 1, tau = 0.01, rho = ellipse, preconditioner (alpha
mean(rho) M - tau mean(kappa) K_0)^-1: kappa absent / separable / on the grid
  2D n = 24: 14 / 30 / 14;  3D n = 8: 12 / 22 / 18 (margins >= 0.11).
"""
import numpy as np
import pytest

import massgrid_ref as G
import varmass_ref as R


def test_abi_version_is_unchanged():
    from gdm_amd import _capi

    assert _capi.load().gdm_abi_version() == 19


@pytest.mark.parametrize("p", [1, 3, 5, 7, 9])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_density_grid_tile(dim, p):
    from gdm_amd import _capi

    t = _capi.density_grid_tile(p, dim)
    assert len(t) == 3 and all(isinstance(v, int) and v > 0 for v in t)


def test_density_grid_tile_refuses_other_degrees():
    from gdm_amd import GdmError, _capi

    for p in (0, 2, 11):
        with pytest.raises(GdmError):
            _capi.density_grid_tile(p, 3)
    with pytest.raises(GdmError):
        _capi.density_grid_tile(3, 4)


def test_dense_matrix_of_a_separable_density_is_the_kronecker_sum():
    """the restatement the GPU tests rely on, for a pointwise rho that happens to be separable"""
    m = G.mesh(2, 6)
    terms = R.bump_terms(2)
    A = R.dense_matrix(m, R.pointwise(terms, 2))
    B = R.kron_dense(m, terms)
    assert np.linalg.norm(A - B) <= 1e-13 * np.linalg.norm(B)
    assert abs(G.gauss_mean(m, R.pointwise(terms, 2)) - R.gauss_mean(m, terms)) <= 1e-13


@pytest.mark.parametrize("dim,p,n", [(1, 5, 7), (2, 3, 4), (2, 7, 7), (3, 1, 3), (3, 3, 3)])
def test_mass_diag_is_the_diagonal_of_the_dense_matrix(dim, p, n):
    """the direct diagonal that the GPU tests use where the dense matrix is too dear (3D p = 7, 9)"""
    import oracle as O

    m = O.Mesh(dim, p, [n + d for d in range(dim)], [-0.5, 0.0, 0.2][:dim], [0.7, 0.9, 1.5][:dim])
    want = np.diag(R.dense_matrix(m, G.osc(dim)))
    got = G.mass_diag(m, G.osc(dim))
    assert np.linalg.norm(got - want) <= 1e-13 * np.linalg.norm(want)


@pytest.mark.parametrize("name", ["osc", "ellipse"])
@pytest.mark.parametrize("dim,n", G.MASS_CASES, ids=["2d-n24", "3d-n8"])
def test_mass_pcg_counts(dim, n, name):
    A, b, x, its, margin = G.cpu_mass_solve(dim, n, name)
    print("M[%s] %dD n=%d: %d iterations, margin %.3g" % (name, dim, n, its, margin))
    assert np.linalg.eigvalsh(A)[0] > 0.0
    assert its == G.MASS_ITS[(dim, n, name)]
    assert its <= R.MAX_IT / 2
    assert margin >= (0.8 if dim == 2 else 0.45)
    assert np.linalg.norm(b - A @ x) <= 1e-8 * np.linalg.norm(b)


STALE_ITS = {(2, 24): 33, (3, 8): 22}


@pytest.mark.parametrize("dim,n", G.MASS_CASES, ids=["2d-n24", "3d-n8"])
def test_mass_pcg_with_the_preconditioner_of_another_density(dim, n):
    """osc's W for the ellipse: SPD, so the PCG converges, only more slowly"""
    A, b, x, its, margin = G.cpu_mass_solve(dim, n, "ellipse", "osc")
    print("M[ellipse] with osc's W %dD n=%d: %d iterations, margin %.3g" % (dim, n, its, margin))
    assert its == STALE_ITS[(dim, n)]
    assert its > G.MASS_ITS[(dim, n, "ellipse")]


SYSTEM_ITS = {(2, 24, "none"): 14, (2, 24, "separable"): 30, (2, 24, "grid"): 14,
              (3, 8, "none"): 12, (3, 8, "separable"): 22, (3, 8, "grid"): 18}


@pytest.mark.parametrize("kind", G.SYSTEM_KAPPAS)
@pytest.mark.parametrize("dim,n", G.SYSTEM_CASES, ids=["2d-n24", "3d-n8"])
def test_system_pcg_counts(dim, n, kind):
    apply, b, x, its, margin = G.cpu_system_solve(dim, n, kind)
    print("(M[ellipse] - tau K[%s]) %dD n=%d: %d iterations, margin %.3g" % (kind, dim, n, its, margin))
    assert its == SYSTEM_ITS[(dim, n, kind)]
    assert margin >= 0.1
    assert np.linalg.norm(b - apply(x)) <= 1e-8 * np.linalg.norm(b)
