"""gdm_coef_solve: x = (alpha M - tau K[kappa])^-1 rhs by CG, preconditioned by
the constant-coefficient fast diagonalisation with the domain mean of kappa,
against the numpy restatement (tests/vardiff_ref.py) and its PCG with the exact
inverse of the homogeneous operator; the drivers on top of it.

Solves: Poisson (alpha = 0, tau = 1) and heat-implicit (alpha = 1, tau = dt) on
[0, 1]^dim, 2D p = 3 with n = 24 and n = 48, 3D p = 3 with n = 12, kappa = 1 + 9
b(x) b(y) [b(z)], b(t) = exp(-((t - 1/2) / 0.2)^2): contrast 10.  rel_tol 1e-8.
  * the true residual |b - A x| / |b| through the restatement is <= 2e-8 (the
    recurrence residual is <= 1e-8 |b|; its drift from the true one is ~1e-13
    at these sizes);
  * the GPU iteration count is within 1 of the restatement's PCG; the
    right-hand sides are such that the CPU count does not change under 1e-12
    perturbations (checked here, the practice of tests/test_elasticity_cpu.py).
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


def bump(t):
    return np.exp(-((t - 0.5) / 0.2) ** 2)


def contrast_terms(dim, amp=9.0):
    return [[None] * dim, [lambda t: amp * bump(t)] + [bump] * (dim - 1)]


def contrast_kappa(dim, amp=9.0):
    def kappa(x):
        return 1.0 + amp * np.prod([bump(x[:, d]) for d in range(dim)], axis=0)

    return kappa


def mean_of(m, terms):
    """sum_t prod_d mean(k_td) with the Gauss weights: the preconditioner's kappa"""
    xq, wq = O.gauss(m.p + 1)
    total = 0.0
    for t in terms:
        prod = 1.0
        for d in range(m.dim):
            if t[d] is None:
                continue
            n = int(m.nsub[d])
            x = float(m.lo[d]) + (np.arange(n)[:, None] + xq[None, :]) * float(m.h[d])
            prod *= float((wq[None, :] * t[d](x)).sum()) / n
        total += prod
    return total


def rhs_of(m):
    """M applied to a smooth function plus a rough part: every mode is present"""
    X = m.vertex_coords()
    rng = np.random.default_rng(m.n_dofs)
    f = np.prod([np.sin(2.3 * X[d] + 0.4 * d) for d in range(m.dim)], axis=0) + 0.3 * rng.uniform(-1, 1, m.n_dofs)
    M = [m.matrices_1d(d)[0] for d in range(m.dim)]
    return m.kron_apply([tuple(M)], f)


SOLVES = [(2, 24), (2, 48), (3, 12)]
SYSTEMS = {"poisson": (0.0, 1.0), "heat": (1.0, DT)}


@functools.lru_cache(maxsize=None)
def cpu_solve(dim, n, system):
    """(mesh, rhs, x, iterations) of the restatement's PCG"""
    alpha, tau = SYSTEMS[system]
    m = O.Mesh(dim, P, n)
    S = R.System(m, contrast_kappa(dim), NITSCHE, alpha, tau, mean_of(m, contrast_terms(dim)))
    b = rhs_of(m)
    x, its, hist = S.solve(b, rel_tol=1e-8)
    # the count is stable: no residual of the history is within 1e-9 (relative) of the
    # threshold, and a 1e-12 perturbation of the right-hand side keeps it
    tol = 1e-8 * hist[0]
    assert min(abs(h - tol) / tol for h in hist) > 1e-6, (its, hist[-2:], tol)
    rng = np.random.default_rng(1)
    _, its2, _ = S.solve(b * (1.0 + 1e-12 * rng.uniform(-1, 1, b.size)), rel_tol=1e-8)
    assert its2 == its
    return m, S, b, x, its


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _op(dim, n, terms, lo=0.0, hi=1.0):
    import gdm_amd

    op = gdm_amd.GdmOperator(dim, P, n, lo, hi, "wave", params=(NITSCHE,))
    op.set_coefficient(terms)
    return op


@pytest.mark.parametrize("system", sorted(SYSTEMS))
@pytest.mark.parametrize("dim,n", SOLVES, ids=["2d-n24", "2d-n48", "3d-n12"])
def test_solve_residual_and_iterations(dim, n, system):
    alpha, tau = SYSTEMS[system]
    m, S, b, x_cpu, its_cpu = cpu_solve(dim, n, system)
    op = _op(dim, n, contrast_terms(dim))
    op.system_solve_setup()
    x = op.new_vector(local=False)
    its, res = op.coef_solve(alpha, tau, _dev(b), x, rel_tol=1e-8)
    xh = _host(x)
    true_res = float(np.linalg.norm(b - S.apply(xh)) / np.linalg.norm(b))
    print("%s %dD n=%d: GPU %d iterations (CPU %d), recurrence residual %.3e, true residual / |b| %.3e, "
          "vs CPU solution %.2e" % (system, dim, n, its, its_cpu, res, true_res, _rel(xh, x_cpu)))
    assert true_res <= 2e-8
    assert abs(its - its_cpu) <= 1
    # x is the initial guess: from the solution the first residual (<= 2e-8 |b|) is already
    # below an absolute tolerance of 1e-6 |b|, so no step is taken (the relative tolerance
    # counts from that first residual, ReductionControl's rule)
    its2, res2 = op.coef_solve(alpha, tau, _dev(b), x, rel_tol=1e-8, abs_tol=1e-6 * float(np.linalg.norm(b)))
    assert its2 == 0 and res2 <= 2e-8 * float(np.linalg.norm(b))


def exact_u(x, y):
    return np.sin(np.pi * x + 0.3) * np.cos(np.pi * y)


def exact_f(x, y):
    """-div(kappa grad u), kappa = (1 + x)(1 + y^2)"""
    u = exact_u(x, y)
    ux = np.pi * np.cos(np.pi * x + 0.3) * np.cos(np.pi * y)
    uy = -np.pi * np.sin(np.pi * x + 0.3) * np.sin(np.pi * y)
    kappa = (1 + x) * (1 + y * y)
    return -(1 + y * y) * ux - 2 * y * (1 + x) * uy + 2 * np.pi ** 2 * kappa * u


CONV_TERMS = [[lambda x: 1 + x, lambda y: 1 + y * y]]


def cpu_poisson_error(n):
    """L2 error of the restatement's dense Poisson solve"""
    m = O.Mesh(2, P, n)
    kappa = lambda x: (1 + x[:, 0]) * (1 + x[:, 1] ** 2)  # noqa: E731
    K = R.dense_matrix(m, kappa, NITSCHE)
    q, bp = m.cell_qpoints(), m.boundary_points()
    rhs = m.wave_rhs(np.zeros(m.n_dofs), impl=False, fq=exact_f(q[:, 0], q[:, 1]), nitsche=NITSCHE)
    rhs = rhs + R.wave_rhs(m, kappa, None, NITSCHE, exact_u(bp[:, 0], bp[:, 1]))
    u = np.linalg.solve(-K, rhs)
    return m.l2_error(u, exact_u(q[:, 0], q[:, 1]))


def test_poisson_convergence():
    """u = sin(pi x + 0.3) cos(pi y), kappa = (1 + x)(1 + y^2), g = u on the
    boundary (the data term uses kappa g), f analytic on the Gauss grid: the L2
    error falls by at least 2^p from n = 8 to n = 16 (theory 2^(p+1)); the
    restatement alone satisfies this too"""
    import gdm_amd

    e_cpu = [cpu_poisson_error(n) for n in (8, 16)]
    print("restatement: L2 errors %.3e %.3e, ratio %.2f" % (e_cpu[0], e_cpu[1], e_cpu[0] / e_cpu[1]))
    assert e_cpu[0] / e_cpu[1] >= 2 ** P
    err = []
    for n in (8, 16):
        op = _op(2, n, CONV_TERMS)
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
        # both are the same discrete solution up to the solver's error (rel_tol 1e-12 against a
        # discretisation error of 1e-5): the two norms agree to well under a percent
        assert abs(err[-1] - e_cpu[len(err) - 1]) <= 1e-2 * e_cpu[len(err) - 1]
    assert err[0] / err[1] >= 2 ** P


TWO_TERMS = [[lambda x: 1 + 0.5 * np.sin(3 * x), np.exp], [lambda x: 0.3 * (2 + x), lambda y: 1 + y]]


def two_term_kappa(x):
    return (1 + 0.5 * np.sin(3 * x[:, 0])) * np.exp(x[:, 1]) + 0.3 * (2 + x[:, 0]) * (1 + x[:, 1])


def test_wave_problem_rk4():
    """three RK4 steps of WaveProblem with a 2-term kappa against RK4 over the
    restatement and the exact mass inverse (tolerance of tests/test_gpu_rk.py)"""
    import gdm_amd

    n, lo, hi = (10, 8), (0.0, -0.2), (1.0, 0.6)
    m = O.Mesh(2, P, list(n), list(lo), list(hi))
    op = _op(2, n, TWO_TERMS, lo, hi)
    X = m.vertex_coords()
    u0 = np.cos(2.0 * X[0]) * np.sin(3.0 * X[1] + 0.2)
    N = m.n_dofs
    h, steps = 0.05 * min(m.h), 3
    y = np.concatenate([u0, np.zeros(N)])
    for s in range(steps):
        y = cut1d.rk4_step(lambda t, y: np.concatenate(
            [y[N:], m.kron_mass_inverse(R.wave_rhs(m, two_term_kappa, y[:N], NITSCHE))]), s * h, h, y)
    prob = gdm_amd.WaveProblem(op)
    prob.u.copy_(_dev(u0))
    for s in range(steps):
        prob.step(s * h, h)
    ru, rv = _rel(_host(prob.u), y[:N]), _rel(_host(prob.v), y[N:])
    print("WaveProblem with kappa: u %.2e v %.2e" % (ru, rv))
    assert ru < 1e-10 and rv < 1e-10


def test_heat_problem_implicit():
    """two backward Euler steps of HeatProblem(scheme="impl") against the dense solve"""
    import gdm_amd

    n, lo, hi = (8, 7), (0.0, -0.2), (1.0, 0.6)
    m = O.Mesh(2, P, list(n), list(lo), list(hi))
    op = _op(2, n, TWO_TERMS, lo, hi)
    X = m.vertex_coords()
    u0 = np.cos(2.0 * X[0]) * np.sin(3.0 * X[1] + 0.2)
    M, _ = R.homogeneous_matrices(m, NITSCHE)
    K = R.dense_matrix(m, two_term_kappa, NITSCHE)
    u = u0.copy()
    for _ in range(2):
        u = np.linalg.solve(M - DT * K, M @ u)
    prob = gdm_amd.HeatProblem(op, scheme="impl", rel_tol=1e-12)
    prob.u.copy_(_dev(u0))
    prob.step(0.0, DT)
    prob.step(DT, DT)
    r = _rel(_host(prob.u), u)
    print("HeatProblem impl with kappa: %.2e, iterations %s" % (r, prob.iterations))
    assert len(prob.iterations) == 2 and all(i > 0 for i in prob.iterations)
    assert r < 1e-10


def test_breakdown_is_an_error_return():
    """a sign-changing 2-term kappa = 1 - 4 b(x) b(y) (mean 0.5 > 0, -3 at the
    centre): alpha M - tau K is indefinite, the solve returns GDM_ERR_STATE"""
    from gdm_amd import _capi

    n = 24
    m = O.Mesh(2, P, n)
    terms = contrast_terms(2, -4.0)
    assert mean_of(m, terms) > 0.0
    b = rhs_of(m)
    S = R.System(m, contrast_kappa(2, -4.0), NITSCHE, 0.0, 1.0, mean_of(m, terms))
    with pytest.raises((ArithmeticError, RuntimeError)):
        S.solve(b, rel_tol=1e-8, max_it=200)
    op = _op(2, n, terms)
    op.system_solve_setup()
    x = op.new_vector(local=False)
    its, res = ctypes.c_int(-1), ctypes.c_double(0.0)
    bd = _dev(b)
    rc = _capi.load().gdm_coef_solve(op.h, 0.0, 1.0, ctypes.c_void_p(bd.data_ptr()),
                                     ctypes.c_void_p(x.data_ptr()), 1e-8, 0.0, 200, ctypes.byref(its),
                                     ctypes.byref(res))
    print("breakdown: rc %d after %d iterations: %s" % (rc, its.value, _capi.last_error()))
    assert rc == ERR_STATE
    assert its.value >= 1
    torch.cuda.synchronize()
