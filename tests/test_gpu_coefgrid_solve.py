"""gdm_coef_solve and the drivers with a general coefficient on the Gauss grid
(gdm_op_set_coefficient_grid) against the numpy restatement
(tests/vardiff_ref.py) and its PCG with the exact inverse of the homogeneous
operator at the Gauss-weighted mean of kappa.

p = 3, nitsche = 6 p^2, [0, 1]^dim.  Solves: Poisson (alpha = 0, tau = 1) and
heat-implicit (alpha = 1, tau = 0.01), 2D n = 24 and 3D n = 12, the Lorentzian
inclusion kappa = 1 + 9 / (1 + 40 sum_d (x_d - 0.5 + 0.1 d)^2) (contrast 10, not
separable), rel_tol 1e-8, the right-hand side of tests/test_gpu_vardiff_solve.py:
  * the true residual |b - A x| / |b| through the restatement is <= 2e-8;
  * the GPU iteration count is within 1 of the restatement's PCG, whose count
    is checked to be stable (no residual of the history within 1e-6 relative of
    the threshold, the same count under a 1e-12 perturbation).
Driver runs: 1e-10 (tests/test_gpu_vardiff_solve.py).
"""
import ctypes
import functools

import numpy as np
import pytest

import cut1d
import oracle as O
import vardiff_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

P = 3
NITSCHE = 6.0 * P * P
DT = 0.01
ERR_STATE = -5


def lorentz(x, dim):
    return 1.0 + 9.0 / (1.0 + 40.0 * sum((x[:, d] - 0.5 + 0.1 * d) ** 2 for d in range(dim)))


def kappa_of(dim):
    return lambda x: lorentz(x, dim)


def gauss_mean(m, kappa):
    """the Gauss-weighted domain mean of kappa: the preconditioner's kappa"""
    xq, wq = O.gauss(m.p + 1)
    ax, w = [], []
    for d in range(3):
        if d < m.dim:
            n = int(m.nsub[d])
            ax.append((float(m.lo[d]) + (np.arange(n)[:, None] + xq[None, :]) * float(m.h[d])).reshape(-1))
            w.append(np.tile(wq, n) / n)
        else:
            ax.append(np.zeros(1))
            w.append(np.ones(1))
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    W = w[2][:, None, None] * w[1][None, :, None] * w[0][None, None, :]
    return float((W * kappa(np.stack([X, Y, Z], axis=-1).reshape(-1, 3)).reshape(W.shape)).sum())


def rhs_of(m):
    """M applied to a smooth function plus a rough part: every mode is present
    (rhs_of of tests/test_gpu_vardiff_solve.py)"""
    X = m.vertex_coords()
    rng = np.random.default_rng(m.n_dofs)
    f = np.prod([np.sin(2.3 * X[d] + 0.4 * d) for d in range(m.dim)], axis=0) + 0.3 * rng.uniform(-1, 1, m.n_dofs)
    M = [m.matrices_1d(d)[0] for d in range(m.dim)]
    return m.kron_apply([tuple(M)], f)


SOLVES = [(2, 24), (3, 12)]
SYSTEMS = {"poisson": (0.0, 1.0), "heat": (1.0, DT)}


def stable_pcg(apply_A, apply_Pinv, b):
    """the restatement's PCG at rel_tol 1e-8 with the stability checks of its count"""
    x, its, hist = R.pcg(apply_A, apply_Pinv, b, rel_tol=1e-8)
    tol = 1e-8 * hist[0]
    assert min(abs(h - tol) / tol for h in hist) > 1e-6, (its, hist[-2:], tol)
    rng = np.random.default_rng(1)
    _, its2, _ = R.pcg(apply_A, apply_Pinv, b * (1.0 + 1e-12 * rng.uniform(-1, 1, b.size)), rel_tol=1e-8)
    assert its2 == its
    return x, its


@functools.lru_cache(maxsize=None)
def cpu_solve(dim, n, system):
    alpha, tau = SYSTEMS[system]
    m = O.Mesh(dim, P, n)
    S = R.System(m, kappa_of(dim), NITSCHE, alpha, tau, gauss_mean(m, kappa_of(dim)))
    b = rhs_of(m)
    x, its = stable_pcg(S.apply, lambda r: S.P @ r, b)
    return m, S, b, x, its


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _op(dim, n, kappa, lo=0.0, hi=1.0):
    import gdm_amd

    op = gdm_amd.GdmOperator(dim, P, n, lo, hi, "wave", params=(NITSCHE,))
    op.set_coefficient_grid(kappa)
    return op


@pytest.mark.parametrize("system", sorted(SYSTEMS))
@pytest.mark.parametrize("dim,n", SOLVES, ids=["2d-n24", "3d-n12"])
def test_solve_residual_and_iterations(dim, n, system):
    alpha, tau = SYSTEMS[system]
    m, S, b, x_cpu, its_cpu = cpu_solve(dim, n, system)
    op = _op(dim, n, kappa_of(dim))
    op.system_solve_setup()
    x = op.new_vector(local=False)
    its, res = op.coef_solve(alpha, tau, _dev(b), x, rel_tol=1e-8)
    xh = _host(x)
    true_res = float(np.linalg.norm(b - S.apply(xh)) / np.linalg.norm(b))
    print("%s %dD n=%d: GPU %d iterations (CPU %d), recurrence residual %.3e, true residual / |b| %.3e, "
          "vs CPU solution %.2e" % (system, dim, n, its, its_cpu, res, true_res, _rel(xh, x_cpu)))
    assert true_res <= 2e-8
    assert abs(its - its_cpu) <= 1


def test_solve_with_a_separable_density():
    """(alpha M[rho] - tau K[kappa]) x = b, rho = (1 + 0.5 x)(2 - y) as one
    separable term, kappa on the grid; preconditioner (alpha mean(rho) M - tau
    mean(kappa) K_0)^-1"""
    dim, n, (alpha, tau) = 2, 24, SYSTEMS["heat"]
    m = O.Mesh(dim, P, n)
    rho = [lambda x: 1 + 0.5 * x, lambda y: 2 - y]
    kappa = kappa_of(dim)
    Mrho = R.kron_matrix([R.factors_1d(m, d, rho[d])[0] for d in range(dim)])
    M, K0 = R.homogeneous_matrices(m, NITSCHE)
    xq, wq = O.gauss(P + 1)
    mean_rho = 1.0
    for d in range(dim):
        x = (np.arange(n)[:, None] + xq[None, :]) / n
        mean_rho *= float((wq[None, :] * rho[d](x)).sum()) / n
    Pinv = np.linalg.inv(alpha * mean_rho * M - tau * gauss_mean(m, kappa) * K0)
    apply_A = lambda v: alpha * (Mrho @ v) - tau * R.wave_rhs(m, kappa, v, NITSCHE)  # noqa: E731
    b = rhs_of(m)
    _, its_cpu = stable_pcg(apply_A, lambda r: Pinv @ r, b)
    op = _op(dim, n, kappa)
    op.set_density([rho])
    op.system_solve_setup()
    x = op.new_vector(local=False)
    its, res = op.coef_solve(alpha, tau, _dev(b), x, rel_tol=1e-8)
    true_res = float(np.linalg.norm(b - apply_A(_host(x))) / np.linalg.norm(b))
    print("heat with density 2D n=%d: GPU %d iterations (CPU %d), true residual / |b| %.3e" % (n, its, its_cpu, true_res))
    assert true_res <= 2e-8
    assert abs(its - its_cpu) <= 1


def exact_u(x, y):
    return np.sin(np.pi * x + 0.3) * np.cos(np.pi * y)


def conv_kappa(x):
    return 2.0 + np.sin(3.0 * x[:, 0] * x[:, 1])


def exact_f(x, y):
    """-div(kappa grad u), kappa = 2 + sin(3 x y)"""
    u = exact_u(x, y)
    ux = np.pi * np.cos(np.pi * x + 0.3) * np.cos(np.pi * y)
    uy = -np.pi * np.sin(np.pi * x + 0.3) * np.sin(np.pi * y)
    kappa = 2.0 + np.sin(3.0 * x * y)
    kx, ky = 3.0 * y * np.cos(3.0 * x * y), 3.0 * x * np.cos(3.0 * x * y)
    return -(kx * ux + ky * uy) + 2 * np.pi ** 2 * kappa * u


def cpu_poisson_error(n):
    """L2 error of the restatement's dense Poisson solve"""
    m = O.Mesh(2, P, n)
    K = R.dense_matrix(m, conv_kappa, NITSCHE)
    q, bp = m.cell_qpoints(), m.boundary_points()
    rhs = m.wave_rhs(np.zeros(m.n_dofs), impl=False, fq=exact_f(q[:, 0], q[:, 1]), nitsche=NITSCHE)
    rhs = rhs + R.wave_rhs(m, conv_kappa, None, NITSCHE, exact_u(bp[:, 0], bp[:, 1]))
    u = np.linalg.solve(-K, rhs)
    return m.l2_error(u, exact_u(q[:, 0], q[:, 1]))


def test_poisson_convergence():
    """u = sin(pi x + 0.3) cos(pi y), kappa = 2 + sin(3 x y), f analytic on the
    Gauss grid, g = u: the L2 error falls by at least 2^p from n = 8 to n = 16
    (the restatement's dense solve: 2.16e-4 -> 1.11e-5, ratio 19.4), and each
    GPU error is within 1 % of the restatement's"""
    import gdm_amd

    e_cpu = [cpu_poisson_error(n) for n in (8, 16)]
    print("restatement: L2 errors %.3e %.3e, ratio %.2f" % (e_cpu[0], e_cpu[1], e_cpu[0] / e_cpu[1]))
    assert e_cpu[0] / e_cpu[1] >= 2 ** P
    err = []
    for n in (8, 16):
        op = _op(2, n, conv_kappa)
        xq, yq = op.quadrature_points()
        X, Y = np.meshgrid(xq, yq, indexing="xy")  # fq[qy Q_x + qx]
        fq = _dev(exact_f(X, Y).reshape(-1))
        bp = op.bc_points()
        g = _dev(exact_u(bp[:, 0], bp[:, 1]))
        info = {}
        u = gdm_amd.solve_poisson(op, forcing=lambda t: fq, dirichlet=lambda t: g, rel_tol=1e-12, info=info)
        err.append(op.error_norms_grid(u, _dev(exact_u(X, Y).reshape(-1)))[2])
        print("n=%d: %d iterations, L2 error %.3e (restatement %.3e)" % (n, info["iterations"], err[-1],
                                                                        e_cpu[len(err) - 1]))
        assert info["iterations"] > 0
        assert abs(err[-1] - e_cpu[len(err) - 1]) <= 1e-2 * e_cpu[len(err) - 1]
    assert err[0] / err[1] >= 2 ** P


def driver_kappa(x):
    return 2.0 + np.sin(3.0 * x[:, 0] * x[:, 1]) + 0.5 * np.cos(5.0 * (x[:, 0] - x[:, 1]))


def test_wave_problem_rk4():
    """three RK4 steps of WaveProblem against RK4 over the restatement and the
    exact mass inverse (the setup of test_gpu_vardiff_solve.py::test_wave_problem_rk4)"""
    import gdm_amd

    n, lo, hi = (10, 8), (0.0, -0.2), (1.0, 0.6)
    m = O.Mesh(2, P, list(n), list(lo), list(hi))
    op = _op(2, n, driver_kappa, lo, hi)
    X = m.vertex_coords()
    u0 = np.cos(2.0 * X[0]) * np.sin(3.0 * X[1] + 0.2)
    N = m.n_dofs
    h, steps = 0.05 * min(m.h), 3
    y = np.concatenate([u0, np.zeros(N)])
    for s in range(steps):
        y = cut1d.rk4_step(lambda t, y: np.concatenate(
            [y[N:], m.kron_mass_inverse(R.wave_rhs(m, driver_kappa, y[:N], NITSCHE))]), s * h, h, y)
    prob = gdm_amd.WaveProblem(op)
    prob.u.copy_(_dev(u0))
    for s in range(steps):
        prob.step(s * h, h)
    ru, rv = _rel(_host(prob.u), y[:N]), _rel(_host(prob.v), y[N:])
    print("WaveProblem with a grid kappa: u %.2e v %.2e" % (ru, rv))
    assert ru <= 1e-10 and rv <= 1e-10


def test_heat_problem_implicit():
    """two backward Euler steps of HeatProblem(scheme="impl", rel_tol=1e-12)
    against the dense solve"""
    import gdm_amd

    n, lo, hi = (8, 7), (0.0, -0.2), (1.0, 0.6)
    m = O.Mesh(2, P, list(n), list(lo), list(hi))
    op = _op(2, n, driver_kappa, lo, hi)
    X = m.vertex_coords()
    u0 = np.cos(2.0 * X[0]) * np.sin(3.0 * X[1] + 0.2)
    M, _ = R.homogeneous_matrices(m, NITSCHE)
    K = R.dense_matrix(m, driver_kappa, NITSCHE)
    u = u0.copy()
    for _ in range(2):
        u = np.linalg.solve(M - DT * K, M @ u)
    prob = gdm_amd.HeatProblem(op, scheme="impl", rel_tol=1e-12)
    prob.u.copy_(_dev(u0))
    prob.step(0.0, DT)
    prob.step(DT, DT)
    r = _rel(_host(prob.u), u)
    print("HeatProblem impl with a grid kappa: %.2e, iterations %s" % (r, prob.iterations))
    assert len(prob.iterations) == 2 and all(i > 0 for i in prob.iterations)
    assert r <= 1e-10


def test_breakdown_is_an_error_return():
    """kappa made negative in place after a valid set (1 - 4 b(x) b(y), -3 at
    the centre): alpha M - tau K is indefinite, the solve returns GDM_ERR_STATE
    (p^T A p <= 0), no fault"""
    from gdm_amd import _capi

    n = 24
    m = O.Mesh(2, P, n)
    bump = lambda t: np.exp(-((t - 0.5) / 0.2) ** 2)  # noqa: E731
    bad = lambda x: 1.0 - 4.0 * bump(x[:, 0]) * bump(x[:, 1])  # noqa: E731
    op = _op(2, n, lambda x: np.ones(x.shape[0]))
    kq, kbc = op._coef_grid
    xq, yq = op.quadrature_points()
    X, Y = np.meshgrid(xq, yq, indexing="xy")
    kq.copy_(_dev(bad(np.stack([X.reshape(-1), Y.reshape(-1)], axis=1))))
    assert float(kq.min()) < -2.0
    op.system_solve_setup()
    x = op.new_vector(local=False)
    its, res = ctypes.c_int(-1), ctypes.c_double(0.0)
    bd = _dev(rhs_of(m))
    rc = _capi.load().gdm_coef_solve(op.h, 0.0, 1.0, ctypes.c_void_p(bd.data_ptr()),
                                     ctypes.c_void_p(x.data_ptr()), 1e-8, 0.0, 200, ctypes.byref(its),
                                     ctypes.byref(res))
    print("breakdown: rc %d after %d iterations: %s" % (rc, its.value, _capi.last_error()))
    assert rc == ERR_STATE and "breakdown" in _capi.last_error()
    assert its.value >= 1
    torch.cuda.synchronize()
