"""gdm_density_solve (x = M[rho]^-1 rhs: direct for one term, preconditioned CG
for a sum), gdm_coef_solve with a density, and the drivers on top of them,
against dense numpy matrices from the restatements tests/varmass_ref.py and
tests/vardiff_ref.py.

Direct solve: b = M[rho] x_true; the bound is max(1e-12, 10 x the relative
error of numpy's dense solve of the same system) -- cond(M[rho]) grows with p
and the dimension, so the reference sets the bound, not the code under test.

CG: [0, 1]^dim, p = 3, 2D n = 24 and 3D n = 12, rho = 1 + 9 b(x) b(y) [b(z)],
b(t) = exp(-((t - 1/2) / 0.15)^2): contrast 10, rel_tol 1e-8.  The GPU count is
within 1 of the numpy PCG with the same preconditioner; the numpy count is not
borderline (no residual within 1e-6 relative of the threshold, the same count
under a 1e-12 perturbation of b).  numpy counts: tests/test_varmass_cpu.py.
"""
import ctypes
import functools

import numpy as np
import pytest

import cut1d
import oracle as O
import vardiff_ref as RD
import varmass_ref as R
from varmass_ref import MAX_IT, bump_terms

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

P = 3
NITSCHE = 6.0 * P * P
DT = 0.01
ERR_STATE = -5
LO3, HI3 = (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)
ONE = [[lambda x: 1 + 0.5 * np.sin(3 * x), np.exp, lambda z: 1 + z * z]]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _op(dim, p, n, lo=0.0, hi=1.0, density=None, coefficient=None, nitsche=None):
    import gdm_amd

    nitsche = 6.0 * p * p if nitsche is None else nitsche
    op = gdm_amd.GdmOperator(dim, p, n, lo, hi, "wave", params=(nitsche,) if nitsche else ())
    if density is not None:
        op.set_density(density)
    if coefficient is not None:
        op.set_coefficient(coefficient)
    return op


def _direct_meshes():
    """p cells per direction at every degree and dimension; one tile plus one
    node in 2D; a long 1D line"""
    from gdm_amd import _capi

    tx, ty, zc = _capi.density_tile(5, 3)
    out = [(dim, p, (p,) * dim) for p in (1, 3, 5, 7, 9) for dim in (1, 2, 3)]
    out += [(2, p, (tx, ty)) for p in (3, 5)] + [(1, p, (2 * zc + 2,)) for p in (3, 5)] + [(3, 3, (9, 5, 7))]
    return out


def test_direct_solve_one_term():
    """its == 0, out of place and in place, every mesh of _direct_meshes"""
    worst = 0.0
    for dim, p, n in _direct_meshes():
        m = O.Mesh(dim, p, list(n), list(LO3[:dim]), list(HI3[:dim]))
        terms = [ONE[0][:dim]]
        A = R.kron_dense(m, terms)
        x_true = np.random.default_rng(p + 10 * dim).uniform(-1, 1, m.n_dofs)
        b = A @ x_true
        ref_err = _rel(np.linalg.solve(A, b), x_true)
        tol = max(1e-12, 10.0 * ref_err)
        op = _op(dim, p, n, LO3[:dim], HI3[:dim], density=terms, nitsche=0.0)
        bd, x = _dev(b), op.new_vector(False)
        its, res = op.density_solve(bd, x)
        e = _rel(_host(x), x_true)
        print("direct %dD p=%d n=%s: error %.2e, numpy dense solve %.2e, bound %.2e" % (dim, p, n, e, ref_err, tol))
        assert its == 0
        assert e <= tol
        its, _ = op.density_solve(bd, bd)  # in place
        assert its == 0 and torch.equal(bd, x)
        worst = max(worst, e / tol)
    print("largest error / bound: %.2f" % worst)


def rhs_of(m):
    """M applied to a smooth function plus a rough part: every mode is present"""
    X = m.vertex_coords()
    rng = np.random.default_rng(m.n_dofs)
    f = np.prod([np.sin(2.3 * X[d] + 0.4 * d) for d in range(m.dim)], axis=0) + 0.3 * rng.uniform(-1, 1, m.n_dofs)
    M = [m.matrices_1d(d)[0] for d in range(m.dim)]
    return m.kron_apply([tuple(M)], f)


def _stable(solve, b, rel_tol=1e-8):
    """numpy PCG whose count is not borderline: (x, its)"""
    x, its, hist = solve(b)
    tol = rel_tol * hist[0]
    assert min(abs(h - tol) / tol for h in hist) > 1e-6, (its, hist[-2:], tol)
    rng = np.random.default_rng(1)
    _, its2, _ = solve(b * (1.0 + 1e-12 * rng.uniform(-1, 1, b.size)))
    assert its2 == its
    return x, its


@functools.lru_cache(maxsize=None)
def cpu_mass_solve(dim, n):
    m = O.Mesh(dim, P, n)
    S = R.MassSystem(m, bump_terms(dim))
    b = rhs_of(m)
    x, its = _stable(lambda v: S.solve(v, rel_tol=1e-8, max_it=MAX_IT), b)
    return m, S, b, x, its


@pytest.mark.parametrize("dim,n", [(2, 24), (3, 12)], ids=["2d-n24", "3d-n12"])
def test_cg_residual_and_iterations(dim, n):
    m, S, b, x_cpu, its_cpu = cpu_mass_solve(dim, n)
    op = _op(dim, P, n, density=bump_terms(dim))
    x = op.new_vector(False)
    its, res = op.density_solve(_dev(b), x, rel_tol=1e-8, max_it=MAX_IT)
    xh = _host(x)
    true_res = float(np.linalg.norm(b - S.A @ xh) / np.linalg.norm(b))
    print("density CG %dD n=%d: GPU %d iterations (CPU %d), recurrence residual %.3e, true residual / |b| %.3e, "
          "vs CPU solution %.2e" % (dim, n, its, its_cpu, res, true_res, _rel(xh, x_cpu)))
    assert true_res <= 2e-8
    assert abs(its - its_cpu) <= 1
    # from the solution: the first residual is already below an absolute tolerance of 1e-6 |b|
    its2, res2 = op.density_solve(_dev(b), x, rel_tol=1e-8, abs_tol=1e-6 * float(np.linalg.norm(b)))
    assert its2 == 0 and res2 <= 2e-8 * float(np.linalg.norm(b))


def test_breakdown_and_max_it_are_error_returns():
    """rho = 1 - 4 b(x) b(y) is negative at the centre: p^T M[rho] p <= 0 shows
    up, GDM_ERR_STATE; so does max_it = 1 on the positive density"""
    from gdm_amd import _capi

    n = 24
    m = O.Mesh(2, P, n)
    b = rhs_of(m)
    A = R.kron_dense(m, bump_terms(2, -3.0))
    assert np.linalg.eigvalsh(A)[0] < 0.0
    lib = _capi.load()
    for terms, max_it in ((bump_terms(2, -3.0), 200), (bump_terms(2), 1)):
        op = _op(2, P, n, density=terms)
        x, bd = op.new_vector(False), _dev(b)
        its, res = ctypes.c_int(-1), ctypes.c_double(0.0)
        rc = lib.gdm_density_solve(op.h, ctypes.c_void_p(bd.data_ptr()), ctypes.c_void_p(x.data_ptr()), 1e-8, 0.0,
                                   max_it, ctypes.byref(its), ctypes.byref(res))
        print("rc %d after %d iterations: %s" % (rc, its.value, _capi.last_error()))
        assert rc == ERR_STATE and its.value >= 1
        assert ("breakdown" if max_it > 1 else "max_it") in _capi.last_error()
    torch.cuda.synchronize()


def bump_kappa(dim, amp=9.0, width=0.2):
    def kappa(x):
        return 1.0 + amp * np.prod([np.exp(-((x[:, d] - 0.5) / width) ** 2) for d in range(dim)], axis=0)

    return kappa


def kappa_terms(dim, amp=9.0, width=0.2):
    b = lambda s: np.exp(-((s - 0.5) / width) ** 2)  # noqa: E731
    return [[None] * dim, [lambda s: amp * b(s)] + [b] * (dim - 1)]


@functools.lru_cache(maxsize=None)
def cpu_system_solve(dim, n, with_kappa):
    """numpy PCG of (M[rho] - dt K) x = b preconditioned by the exact inverse of
    rho-bar M - dt kappa-bar K_0"""
    m = O.Mesh(dim, P, n)
    rho = bump_terms(dim)
    Mrho = R.kron_dense(m, rho)
    M, K0 = RD.homogeneous_matrices(m, NITSCHE)
    kbar = R.gauss_mean(m, kappa_terms(dim)) if with_kappa else 1.0
    Pinv = np.linalg.inv(R.gauss_mean(m, rho) * M - DT * kbar * K0)
    if with_kappa:
        kap = bump_kappa(dim)
        apply = lambda x: Mrho @ x - DT * RD.wave_rhs(m, kap, x, NITSCHE)  # noqa: E731
    else:
        apply = lambda x: Mrho @ x - DT * (K0 @ x)  # noqa: E731
    b = rhs_of(m)
    x, its = _stable(lambda v: RD.pcg(apply, lambda r: Pinv @ r, v, rel_tol=1e-8), b)
    return apply, b, x, its


@pytest.mark.parametrize("with_kappa", [False, True], ids=["density", "density+kappa"])
@pytest.mark.parametrize("dim,n", [(2, 24), (3, 12)], ids=["2d-n24", "3d-n12"])
def test_system_solve_with_a_density(dim, n, with_kappa):
    """heat-implicit, tau = 0.01: coef_solve with a density alone (K = K_0) and
    with a coefficient too"""
    apply, b, x_cpu, its_cpu = cpu_system_solve(dim, n, with_kappa)
    op = _op(dim, P, n, density=bump_terms(dim), coefficient=kappa_terms(dim) if with_kappa else None)
    op.system_solve_setup()
    x = op.new_vector(False)
    its, res = op.coef_solve(1.0, DT, _dev(b), x, rel_tol=1e-8)
    xh = _host(x)
    true_res = float(np.linalg.norm(b - apply(xh)) / np.linalg.norm(b))
    print("system %dD n=%d kappa=%s: GPU %d iterations (CPU %d), true residual / |b| %.3e, vs CPU solution %.2e"
          % (dim, n, with_kappa, its, its_cpu, true_res, _rel(xh, x_cpu)))
    assert true_res <= 2e-8
    assert abs(its - its_cpu) <= 1
    # alpha != 1 scales the mass part: the same solution for (2 M[rho] - 2 dt K) x = 2 b
    x2 = op.new_vector(False)
    op.coef_solve(2.0, 2.0 * DT, _dev(2.0 * b), x2, rel_tol=1e-8)
    assert _rel(_host(x2), xh) <= 1e-6


# ---- drivers: a two-term rho and a one-term kappa, 2D p = 3 n = 12 ------------
RHO2 = [[lambda x: 1 + 0.5 * np.sin(3 * x), np.exp], [lambda x: 0.3 * (2 + x), lambda y: 1 + y]]
KAP1 = [[lambda x: 1 + x, lambda y: 1 + y * y]]


@functools.lru_cache(maxsize=None)
def driver_setup():
    n, lo, hi = (12, 12), (0.0, -0.2), (1.0, 0.6)
    m = O.Mesh(2, P, list(n), list(lo), list(hi))
    Mrho = R.kron_dense(m, RHO2)
    K = RD.dense_matrix(m, lambda x: (1 + x[:, 0]) * (1 + x[:, 1] ** 2), NITSCHE)
    X = m.vertex_coords()
    u0 = np.cos(2.0 * X[0]) * np.sin(3.0 * X[1] + 0.2)
    return n, lo, hi, m, Mrho, K, u0


def _driver_op():
    n, lo, hi = driver_setup()[:3]
    return _op(2, P, n, lo, hi, density=RHO2, coefficient=KAP1)


def test_wave_problem_rk4():
    """two RK4 steps of rho u_tt = div(kappa grad u) against the same scheme with
    dense matrices; the CG runs to rel_tol 1e-13, so its error is far below 1e-9"""
    import gdm_amd

    n, lo, hi, m, Mrho, K, u0 = driver_setup()
    N = m.n_dofs
    h = 0.05 * min(m.h)
    A = np.linalg.solve(Mrho, K)
    y = np.concatenate([u0, np.zeros(N)])
    for s in range(2):
        y = cut1d.rk4_step(lambda t, y: np.concatenate([y[N:], A @ y[:N]]), s * h, h, y)
    prob = gdm_amd.WaveProblem(_driver_op(), rel_tol=1e-13, max_it=100)
    prob.u.copy_(_dev(u0))
    for s in range(2):
        prob.step(s * h, h)
    ru, rv = _rel(_host(prob.u), y[:N]), _rel(_host(prob.v), y[N:])
    print("WaveProblem with rho: u %.2e v %.2e, iterations %s" % (ru, rv, prob.iterations))
    assert len(prob.iterations) == 8 and all(i > 0 for i in prob.iterations)
    assert ru < 1e-9 and rv < 1e-9


def test_heat_problem_rk4():
    import gdm_amd

    n, lo, hi, m, Mrho, K, u0 = driver_setup()
    h = 0.02 * min(m.h) ** 2
    A = np.linalg.solve(Mrho, K)
    u = u0.copy()
    for s in range(2):
        u = cut1d.rk4_step(lambda t, y: A @ y, s * h, h, u)
    prob = gdm_amd.HeatProblem(_driver_op(), scheme="rk", rel_tol=1e-13, max_it=100)
    prob.u.copy_(_dev(u0))
    for s in range(2):
        prob.step(s * h, h)
    r = _rel(_host(prob.u), u)
    print("HeatProblem rk with rho: %.2e, iterations %s" % (r, prob.iterations))
    assert len(prob.iterations) == 8 and all(i > 0 for i in prob.iterations)
    assert r < 1e-9


def test_heat_problem_implicit():
    import gdm_amd

    n, lo, hi, m, Mrho, K, u0 = driver_setup()
    u = u0.copy()
    for _ in range(2):
        u = np.linalg.solve(Mrho - DT * K, Mrho @ u)
    prob = gdm_amd.HeatProblem(_driver_op(), scheme="impl", rel_tol=1e-13)
    prob.u.copy_(_dev(u0))
    prob.step(0.0, DT)
    prob.step(DT, DT)
    r = _rel(_host(prob.u), u)
    print("HeatProblem impl with rho: %.2e, iterations %s" % (r, prob.iterations))
    assert len(prob.iterations) == 2 and all(i > 0 for i in prob.iterations)
    assert r < 1e-9


# ---- manufactured solution: layered rho(x), rho u_tt = lap u + f ---------------
def _layer(x):
    return np.where(x < 0.5, 1.0, 4.0)


def _exact(x, y, t):
    return np.cos(t) * np.sin(np.pi * x + 0.3) * np.cos(np.pi * y)


def _forcing(x, y, t):
    """f = rho u_tt - lap u = (2 pi^2 - rho) u"""
    return (2 * np.pi ** 2 - _layer(x)) * _exact(x, y, t)


def test_manufactured_layered_density():
    """u = cos t sin(pi x + 0.3) cos(pi y) on [0, 1]^2 with rho = 1 (x < 1/2), 4
    (x > 1/2) -- the layer sits on a cell boundary -- forcing through add_load,
    u on the boundary through the Nitsche data; 4 RK4 steps.  The L2 error at
    the end is within 1 % of the same scheme over the restatement's matrices."""
    import gdm_amd

    n, steps = 12, 4
    m = O.Mesh(2, P, n)
    h = 0.05 * float(min(m.h))
    terms = [[_layer, None]]
    Mrho = R.kron_dense(m, terms)
    q, bp = m.cell_qpoints(), m.boundary_points()
    N = m.n_dofs

    def f_cpu(t, y):
        r = m.wave_rhs(y[:N], fq=_forcing(q[:, 0], q[:, 1], t), nitsche=NITSCHE, gbc=_exact(bp[:, 0], bp[:, 1], t))
        return np.concatenate([y[N:], np.linalg.solve(Mrho, r)])

    X = m.vertex_coords()
    y = np.concatenate([_exact(X[0], X[1], 0.0), np.zeros(N)])
    for s in range(steps):
        y = cut1d.rk4_step(f_cpu, s * h, h, y)
    T = steps * h
    e_cpu = m.l2_error(y[:N], _exact(q[:, 0], q[:, 1], T))

    op = _op(2, P, n, density=terms)
    xq, yq = op.quadrature_points()
    XQ, YQ = np.meshgrid(xq, yq, indexing="xy")  # fq[qy Q_x + qx]
    bpd = op.bc_points()
    prob = gdm_amd.WaveProblem(op, forcing=lambda t: _dev(_forcing(XQ, YQ, t).reshape(-1)),
                               dirichlet=lambda t: _dev(_exact(bpd[:, 0], bpd[:, 1], t)))
    prob.u.copy_(_dev(_exact(X[0], X[1], 0.0)))
    for s in range(steps):
        prob.step(s * h, h)
    e_gpu = op.error_norms_grid(prob.u, _dev(_exact(XQ, YQ, T).reshape(-1)))[2]
    print("layered rho: L2 error %.6e (restatement %.6e), vs CPU solution %.2e" % (e_gpu, e_cpu,
                                                                                  _rel(_host(prob.u), y[:N])))
    assert prob.iterations == [0] * (4 * steps)
    assert e_cpu > 0.0 and abs(e_gpu - e_cpu) <= 1e-2 * e_cpu
