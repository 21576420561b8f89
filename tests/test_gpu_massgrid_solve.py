"""gdm_density_solve and gdm_coef_solve with a density on the Gauss grid
(gdm_op_set_density_grid), and the drivers on top of them, against dense numpy
matrices from the restatements (tests/massgrid_ref.py; the numpy counts are
pinned and shown stable in tests/test_massgrid_cpu.py).

[0, 1]^dim, p = 3, 2D n = 24 and 3D n = 8, rel_tol 1e-8; densities osc and
ellipse (massgrid_ref).  The GPU count is within 1 of the numpy PCG with the
same preconditioner, the true residual at most 2e-8 |b|.
"""
import ctypes
import functools

import numpy as np
import pytest

import cut1d
import massgrid_ref as G
import oracle as O
import vardiff_ref as RD
import varmass_ref as R
from massgrid_ref import ALPHA, MAX_IT, NITSCHE, P, TAU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ERR_STATE = -5
CASE_IDS = ["2d-n24", "3d-n8"]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _op(dim, n, rho=None, lo=0.0, hi=1.0):
    import gdm_amd

    op = gdm_amd.GdmOperator(dim, P, n, lo, hi, "wave", params=(NITSCHE,))
    if rho is not None:
        op.set_density_grid(rho)
    return op


@pytest.mark.parametrize("name", ["osc", "ellipse"])
@pytest.mark.parametrize("dim,n", G.MASS_CASES, ids=CASE_IDS)
def test_density_solve_residual_and_iterations(dim, n, name):
    A, b, x_cpu, its_cpu, _ = G.cpu_mass_solve(dim, n, name)
    op = _op(dim, n, G.DENSITIES[name](dim))
    x = op.new_vector(False)
    its, res = op.density_solve(_dev(b), x, rel_tol=1e-8, max_it=MAX_IT)
    xh = _host(x)
    true_res = float(np.linalg.norm(b - A @ xh) / np.linalg.norm(b))
    print("grid density CG %s %dD n=%d: GPU %d iterations (CPU %d), recurrence residual %.3e, true residual / |b| "
          "%.3e, vs CPU solution %.2e" % (name, dim, n, its, its_cpu, res, true_res, _rel(xh, x_cpu)))
    assert true_res <= 2e-8
    assert abs(its - its_cpu) <= 1
    # from the solution: the first residual is already below an absolute tolerance of 1e-6 |b|
    its2, res2 = op.density_solve(_dev(b), x, rel_tol=1e-8, abs_tol=1e-6 * float(np.linalg.norm(b)))
    assert its2 == 0 and res2 <= 2e-8 * float(np.linalg.norm(b))


@pytest.mark.parametrize("dim,n", G.MASS_CASES, ids=CASE_IDS)
def test_in_place_overwrite_converges_within_max_it(dim, n):
    """osc overwritten in place by the ellipse, no set call: the apply is the
    ellipse's and the solve converges within MAX_IT = 20 at rel_tol 1e-8.

    gdm_density_solve forms W from the samples it finds, so the count is the
    ellipse's.  With osc's W kept, the numpy PCG of tests/massgrid_ref.py for
    this pair needs 33 iterations in 2D n = 24 and 22 in 3D n = 8 (pinned in
    tests/test_massgrid_cpu.py): convergent, but not within MAX_IT."""
    op = _op(dim, n)
    rq = _dev(G.osc(dim)(op.gauss_grid_points()))
    op.set_density_grid(rq)
    rq.copy_(_dev(G.ellipse(dim)(op.gauss_grid_points())))
    A, b, _, its_cpu, _ = G.cpu_mass_solve(dim, n, "ellipse")
    x = op.new_vector(False)
    its, res = op.density_solve(_dev(b), x, rel_tol=1e-8, max_it=MAX_IT)
    print("in-place overwrite, no set call %dD n=%d: GPU %d iterations (CPU with the ellipse's W %d)"
          % (dim, n, its, its_cpu))
    assert float(np.linalg.norm(b - A @ _host(x)) / np.linalg.norm(b)) <= 2e-8
    assert abs(its - its_cpu) <= 1


@pytest.mark.parametrize("dim,n", G.MASS_CASES, ids=CASE_IDS)
def test_in_place_overwrite_then_refresh(dim, n):
    """after the refresh call (the same pointer) the count is the ellipse's, and
    the solution has the bits of an operator that was given the ellipse at once"""
    op = _op(dim, n)
    rq = _dev(G.osc(dim)(op.gauss_grid_points()))
    op.set_density_grid(rq)
    rq.copy_(_dev(G.ellipse(dim)(op.gauss_grid_points())))
    op.set_density_grid(rq)
    A, b, _, its_cpu, _ = G.cpu_mass_solve(dim, n, "ellipse")
    x = op.new_vector(False)
    its, _ = op.density_solve(_dev(b), x, rel_tol=1e-8, max_it=MAX_IT)
    print("after the refresh %dD n=%d: GPU %d iterations (CPU %d)" % (dim, n, its, its_cpu))
    assert float(np.linalg.norm(b - A @ _host(x)) / np.linalg.norm(b)) <= 2e-8
    assert abs(its - its_cpu) <= 1
    fresh = _op(dim, n, G.ellipse(dim))
    x2 = fresh.new_vector(False)
    its2, _ = fresh.density_solve(_dev(b), x2, rel_tol=1e-8, max_it=MAX_IT)
    assert its2 == its and torch.equal(x2, x)


def test_breakdown_and_max_it_are_error_returns():
    """max_it = 1 on the ellipse; a negative density written in place after a
    valid set call: p^T M[rho] p <= 0 shows up, GDM_ERR_STATE"""
    from gdm_amd import _capi

    dim, n = 2, 24
    lib = _capi.load()
    b = G.rhs_of(G.mesh(dim, n))
    for negative, max_it in ((False, 1), (True, 200)):
        op = _op(dim, n)
        rq = _dev(G.ellipse(dim)(op.gauss_grid_points()))
        op.set_density_grid(rq)
        if negative:
            rq.mul_(-1.0)
        x, bd = op.new_vector(False), _dev(b)
        its, res = ctypes.c_int(-1), ctypes.c_double(0.0)
        rc = lib.gdm_density_solve(op.h, ctypes.c_void_p(bd.data_ptr()), ctypes.c_void_p(x.data_ptr()), 1e-8, 0.0,
                                   max_it, ctypes.byref(its), ctypes.byref(res))
        print("rc %d after %d iterations: %s" % (rc, its.value, _capi.last_error()))
        assert rc == ERR_STATE and its.value >= 1
        assert ("breakdown" if negative else "max_it") in _capi.last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", G.SYSTEM_KAPPAS)
@pytest.mark.parametrize("dim,n", G.SYSTEM_CASES, ids=CASE_IDS)
def test_coef_solve_with_a_grid_density(dim, n, kind):
    """(M[rho] - 0.01 K[kappa]) x = b, rho = ellipse on the grid; kappa absent
    (K_0), separable, or osc on the grid"""
    apply, b, x_cpu, its_cpu, _ = G.cpu_system_solve(dim, n, kind)
    op = _op(dim, n, G.ellipse(dim))
    kappa, terms = G.system_kappa(dim, kind)
    if terms is not None:
        op.set_coefficient(terms)
    elif kappa is not None:
        op.set_coefficient_grid(kappa)
    op.system_solve_setup()
    x = op.new_vector(False)
    its, res = op.coef_solve(ALPHA, TAU, _dev(b), x, rel_tol=1e-8)
    xh = _host(x)
    true_res = float(np.linalg.norm(b - apply(xh)) / np.linalg.norm(b))
    print("system %dD n=%d kappa=%s: GPU %d iterations (CPU %d), true residual / |b| %.3e, vs CPU solution %.2e"
          % (dim, n, kind, its, its_cpu, true_res, _rel(xh, x_cpu)))
    assert true_res <= 2e-8
    assert abs(its - its_cpu) <= 1


# ---- drivers: rho = ellipse and kappa = osc on the grid, 2D p = 3 n = 12 on [0, 1]^2 ----
@functools.lru_cache(maxsize=None)
def driver_setup():
    n = (12, 12)
    m = O.Mesh(2, P, list(n))
    Mrho = R.dense_matrix(m, G.ellipse(2))
    K = RD.dense_matrix(m, G.osc(2), NITSCHE)
    X = m.vertex_coords()
    u0 = np.cos(2.0 * X[0]) * np.sin(3.0 * X[1] + 0.2)
    return n, m, Mrho, K, u0


def _driver_op():
    op = _op(2, driver_setup()[0], G.ellipse(2))
    op.set_coefficient_grid(G.osc(2))
    return op


def test_wave_problem_rk4():
    """three RK4 steps of rho u_tt = div(kappa grad u) against the same scheme with
    dense matrices; the CG runs to rel_tol 1e-13, so its error is far below 1e-9"""
    import gdm_amd

    n, m, Mrho, K, u0 = driver_setup()
    N = m.n_dofs
    h = 0.05 * min(m.h)
    A = np.linalg.solve(Mrho, K)
    y = np.concatenate([u0, np.zeros(N)])
    for s in range(3):
        y = cut1d.rk4_step(lambda t, y: np.concatenate([y[N:], A @ y[:N]]), s * h, h, y)
    prob = gdm_amd.WaveProblem(_driver_op(), rel_tol=1e-13, max_it=100)
    prob.u.copy_(_dev(u0))
    for s in range(3):
        prob.step(s * h, h)
    ru, rv = _rel(_host(prob.u), y[:N]), _rel(_host(prob.v), y[N:])
    print("WaveProblem with a grid rho: u %.2e v %.2e, iterations %s" % (ru, rv, prob.iterations))
    assert len(prob.iterations) == 12 and all(i > 0 for i in prob.iterations)
    assert ru < 1e-9 and rv < 1e-9


def test_heat_problem_rk4():
    import gdm_amd

    n, m, Mrho, K, u0 = driver_setup()
    h = 0.02 * min(m.h) ** 2
    A = np.linalg.solve(Mrho, K)
    u = u0.copy()
    for s in range(3):
        u = cut1d.rk4_step(lambda t, y: A @ y, s * h, h, u)
    prob = gdm_amd.HeatProblem(_driver_op(), scheme="rk", rel_tol=1e-13, max_it=100)
    prob.u.copy_(_dev(u0))
    for s in range(3):
        prob.step(s * h, h)
    r = _rel(_host(prob.u), u)
    print("HeatProblem rk with a grid rho: %.2e, iterations %s" % (r, prob.iterations))
    assert len(prob.iterations) == 12 and all(i > 0 for i in prob.iterations)
    assert r < 1e-9


def test_heat_problem_implicit():
    import gdm_amd

    n, m, Mrho, K, u0 = driver_setup()
    dt = TAU
    u = u0.copy()
    for _ in range(3):
        u = np.linalg.solve(Mrho - dt * K, Mrho @ u)
    prob = gdm_amd.HeatProblem(_driver_op(), scheme="impl", rel_tol=1e-13)
    prob.u.copy_(_dev(u0))
    for s in range(3):
        prob.step(s * dt, dt)
    r = _rel(_host(prob.u), u)
    print("HeatProblem impl with a grid rho: %.2e, iterations %s" % (r, prob.iterations))
    assert len(prob.iterations) == 3 and all(i > 0 for i in prob.iterations)
    assert r < 1e-9
