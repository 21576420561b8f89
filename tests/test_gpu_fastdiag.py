"""Direct heat-implicit / Poisson solve on uncut boxes by fast diagonalisation
(gdm_system_solve, csrc/gdm_fastdiag.hip) on the device.

Node counts sit around the 16 x 16 x 4 tile of the FP64 matrix instruction;
every box is anisotropic in h:

    tiny    n_sub (1, 1, 1), N = 2                p = 1
    small   n_sub (p, p + 2, p + 3)               p = 1 .. 9
    exact   n_sub 15 each, N = 16                 p = 3
    ragged  nodes 17 x 19 x 33                    p = 3, 5
    large   nodes 37 x 35 x 67                    p = 5
    2d      nodes 17 x 35                         p = 7
    1d      67 nodes                              p = 3

References: np.linalg.solve on the dense Kronecker system (tiny, small) and
the numpy / scipy helper tests/fastdiag_ref.py (pinned to the dense solve by
tests/test_fastdiag_cpu.py); err_ref, the helper's own error against the dense
solve, is computed here per case, not hard-coded.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

import fastdiag_ref as F
import load_ref as R
import oracle as O
import stencil_ref as SR

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GAMMA = 15.0
FN_SINE = 2
BOX2 = ((0.0, -1.0), (1.5, 0.2))
BOX1 = ((-0.3,), (1.1,))

MESHES = {"tiny-p1": (3, 1, (1, 1, 1)), "exact-p3": (3, 3, (15, 15, 15)), "ragged-p3": (3, 3, (16, 18, 32)),
          "ragged-p5": (3, 5, (16, 18, 32)), "large-p5": (3, 5, (36, 34, 66)), "2d-p7": (2, 7, (16, 34)),
          "1d-p3": (1, 3, (66,))}
MESHES.update({"small-p%d" % p: (3, p, F.small_n_sub(p)) for p in (1, 3, 5, 7, 9)})
DENSE = ["tiny-p1"] + ["small-p%d" % p for p in (1, 3, 5, 7, 9)]
HELPER = ["exact-p3", "ragged-p3", "ragged-p5", "large-p5", "2d-p7", "1d-p3"]
GAMMA_CASES = [c for c in F.DENSE_CASES if c[0] > 0.0]


def _box(dim):
    return {3: (F.BOX_LO, F.BOX_HI), 2: BOX2, 1: BOX1}[dim]


@functools.lru_cache(maxsize=None)
def _mesh(name):
    dim, p, n_sub = MESHES[name]
    lo, hi = _box(dim)
    return O.Mesh(dim, p, list(n_sub), list(lo), list(hi))


def _op(name, gamma=GAMMA, setup=True):
    import gdm_amd

    dim, p, n_sub = MESHES[name]
    lo, hi = _box(dim)
    op = gdm_amd.GdmOperator(dim, p, n_sub, lo, hi, "wave", params=(gamma,) if gamma > 0.0 else ())
    if setup:
        op.system_solve_setup()
    return op


@functools.lru_cache(maxsize=None)
def _pairs(name, gamma=GAMMA):
    return F.eigenpairs(_mesh(name), gamma)


@functools.lru_cache(maxsize=None)
def _dense(name, case):
    """(b, x_dense, err_ref) of a dense case, computed once"""
    gamma, alpha, tau = case
    return F.dense_reference(_mesh(name), gamma, alpha, tau, seed=MESHES[name][1])


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# -- single pass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MESHES))
def test_single_pass_equals_einsum(name):
    """every axis, both transposes, integer and random src against np.einsum
    with the tables the library exports"""
    m, op = _mesh(name), _op(name)
    rng = np.random.default_rng(1)
    srcs = [rng.integers(-8, 9, m.n_dofs).astype(np.float64), rng.uniform(-1, 1, m.n_dofs)]
    dst = op.new_vector(local=False)
    for axis in range(m.dim):
        S, _ = op.fastdiag_tables(axis)
        for tr in (0, 1):
            for src in srcs:
                dst.fill_(float("nan"))
                op.fastdiag_transform(axis, tr, _dev(src), dst)
                ref = F.transform(m, S.T if tr else S, axis, src)
                err = F.rel(_host(dst), ref)
                print("%s axis %d transpose %d: %.2e" % (name, axis, tr, err))
                assert err <= 1e-13


@pytest.mark.parametrize("name", sorted(MESHES))
def test_round_trip(name):
    """S (S^T M_d u) = u along every axis"""
    m, op = _mesh(name), _op(name)
    u = np.random.default_rng(2).uniform(-1, 1, m.n_dofs)
    a, b = op.new_vector(local=False), op.new_vector(local=False)
    for axis, (_, M) in enumerate(F.matrices(m, GAMMA)):
        op.fastdiag_transform(axis, 1, _dev(F.transform(m, M, axis, u)), a)
        op.fastdiag_transform(axis, 0, a, b)
        err = F.rel(_host(b), u)
        print("%s axis %d round trip: %.2e" % (name, axis, err))
        assert err <= 1e-11


# -- the solve -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DENSE)
def test_solve_against_the_dense_system(name):
    for case in F.DENSE_CASES:
        gamma, alpha, tau = case
        op = _op(name, gamma)
        b, x_dense, err_ref = _dense(name, case)
        x = op.system_solve(alpha, tau, _dev(b))
        err = F.rel(_host(x), x_dense)
        print("%s gamma %g alpha %g tau %g: device %.2e, helper (err_ref) %.2e" % (name, gamma, alpha, tau, err, err_ref))
        assert err <= max(1e-12, 20.0 * err_ref)


@pytest.mark.parametrize("name", HELPER)
def test_solve_against_the_helper(name):
    """rel-L2 <= 1e-11 at p <= 5 and <= 20 err_ref(small, same p) at p = 7,
    where both sides carry the eigenbasis' own error: measured on 2d-p7 1.0e-13
    / 5.3e-13 / 5.3e-13 against bounds of 2.5e-13 / 6.2e-13 / 5.6e-13"""
    m, op = _mesh(name), _op(name)
    p = m.p
    b = np.random.default_rng(3).uniform(-1, 1, m.n_dofs)
    bd = _dev(b)
    Mx, Kx = op.new_vector(local=False), op.new_vector(local=False)
    for case in GAMMA_CASES:
        gamma, alpha, tau = case
        bound = 1e-11 if p <= 5 else 20.0 * _dense("small-p%d" % p, case)[2]
        xh = F.solve(m, gamma, alpha, tau, b, _pairs(name))
        x = op.system_solve(alpha, tau, bd)
        err = F.rel(_host(x), xh)
        # residual through the device's own operators against the helper's through the Kronecker restatement
        op.mass_apply(x, Mx)
        op.apply(x, Kx)
        res = F.rel(alpha * _host(Mx) - tau * _host(Kx), b)
        res_h = F.rel(alpha * SR.apply(m, "mass", (), xh) - tau * SR.apply(m, "wave", (gamma,), xh), b)
        print("%s alpha %g tau %g: x %.2e (bound %.1e), residual %.2e (helper %.2e)" % (name, alpha, tau, err, bound,
                                                                                       res, res_h))
        assert err <= bound
        assert res <= 50.0 * res_h


@pytest.mark.parametrize("name", ["small-p3", "ragged-p5", "2d-p7", "1d-p3"])
def test_aliasing_and_repeatability(name):
    m, op = _mesh(name), _op(name)
    b = np.random.default_rng(4).uniform(-1, 1, m.n_dofs)
    rhs = _dev(b)
    ref = op.system_solve(1.0, 0.01, rhs)
    torch.cuda.synchronize()
    assert np.array_equal(_host(rhs), b)  # rhs untouched out of place
    assert float(ref.abs().max()) > 0.0
    inplace = _dev(b)
    op.system_solve(1.0, 0.01, inplace, inplace)
    assert torch.equal(inplace, ref)
    again = op.system_solve(1.0, 0.01, rhs)
    assert torch.equal(again, ref)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op.use_torch_stream()
        other = op.system_solve(1.0, 0.01, rhs)
    torch.cuda.synchronize()
    op.use_torch_stream()
    assert torch.equal(other, ref)


# -- Poisson, manufactured -----------------------------------------------------------------------------------------
PK, PPHI = (1.0, 0.75, 1.25), (0.1, 0.4, -0.3)
PPRM = [0.0, 0.0, 0.0] + list(PK) + list(PPHI)
PSCALE = (2.0 * math.pi) ** 2 * sum(k * k for k in PK)


def test_poisson_manufactured_solution():
    """-Laplace u = f with u = prod sin(2 pi k_d x_d + phi_d), g_D = u, gamma =
    15, p = 3 at 12^3 and 24^3 cells: the device's L2 error equals the
    helper's (same discrete problem) and falls by >= 12 (the helper: 16.3)"""
    import gdm_amd

    lo, hi = F.BOX_LO, F.BOX_HI
    exact = R.fn_sine_product((0.0,) * 3, PK, PPHI, 0.0, 3)
    errs = []
    for n in (12, 24):
        m = O.Mesh(3, 3, [n] * 3, list(lo), list(hi))
        op = gdm_amd.GdmOperator(3, 3, n, lo, hi, "wave", params=(GAMMA,))
        u = gdm_amd.solve_poisson(op, forcing=(FN_SINE, PPRM, PSCALE), dirichlet=(FN_SINE, PPRM))
        err = op.error_norms(u, FN_SINE, PPRM, 0.0)[2]
        bx = m.boundary_points()
        rhs = R.load_vector(m, PSCALE * R.grid_values(m, exact)) + R.dirichlet_data(
            m, GAMMA, exact(bx[:, 0], bx[:, 1], bx[:, 2]))
        uh = F.solve(m, GAMMA, 0.0, 1.0, rhs)
        xq = m.cell_qpoints()
        err_h = m.error_norms(uh, exact(xq[:, 0], xq[:, 1], xq[:, 2]))[2]
        print("poisson %d^3: device L2 %.6e, helper L2 %.6e, solution rel-L2 %.2e" % (n, err, err_h,
                                                                                    F.rel(_host(u), uh)))
        assert abs(err - err_h) <= 1e-8 * err_h
        errs.append(err)
    print("poisson L2 ratio 12^3 / 24^3: %.2f" % (errs[0] / errs[1]))
    assert errs[0] / errs[1] >= 12.0


# -- heat ----------------------------------------------------------------------------------------------------------
# data of the heat tests: the moving sine product w, forcing 3 w, g_D = w
HA, HK, HPHI = (0.8, 0.0, 0.0), (1.0, 0.5, 0.75), (0.3, 0.5, 0.2)
HPRM = list(HA) + list(HK) + list(HPHI)


def _heat_data(m, t):
    w = R.fn_sine_product(HA, HK, HPHI, t, m.dim)
    bx = m.boundary_points()
    return R.load_vector(m, 3.0 * R.grid_values(m, w)) + R.dirichlet_data(m, GAMMA, w(bx[:, 0], bx[:, 1], bx[:, 2]))


@pytest.mark.parametrize("name", ["small-p3", "small-p5", "ragged-p3"])
def test_heat_impl_equals_the_numpy_recursion(name):
    """5 backward-Euler steps, the last one shorter than dt (a changed tau)"""
    import gdm_amd
    from gdm_amd.problem import DiscreteTime

    m, op = _mesh(name), _op(name, setup=False)
    prob = gdm_amd.HeatProblem(op, forcing=(FN_SINE, HPRM, 3.0), dirichlet=(FN_SINE, HPRM), scheme="impl")
    u = R.fn_sine_product(HA, HK, HPHI, 0.0, 3)(*m.vertex_coords())
    prob.u.copy_(_dev(u))
    steps = []
    assert prob.run(0.0, 0.046, 0.01, callback=lambda t, pr: steps.append(t)) == 5
    time = DiscreteTime(0.0, 0.046, 0.01)
    hs = []
    while not time.is_at_end():
        h = time.next_step_size()
        hs.append(h)
        rhs = SR.apply(m, "mass", (), u) + h * _heat_data(m, time.t + h)
        u = F.solve(m, GAMMA, 1.0, h, rhs, _pairs(name))
        time.advance()
    assert len(hs) == 5 and hs[-1] < 0.7 * hs[0]
    err = F.rel(_host(prob.u), u)
    print("%s heat-impl, steps %s: %.2e" % (name, ["%.4g" % h for h in hs], err))
    assert err <= 1e-11


def test_heat_rk_equals_the_numpy_rk4():
    import gdm_amd
    import cut1d

    name = "small-p3"
    m, op = _mesh(name), _op(name, setup=False)
    prob = gdm_amd.HeatProblem(op, forcing=(FN_SINE, HPRM, 3.0), dirichlet=(FN_SINE, HPRM), scheme="rk")
    u = R.fn_sine_product(HA, HK, HPHI, 0.0, 3)(*m.vertex_coords())
    prob.u.copy_(_dev(u))
    Minv = np.linalg.inv(F.dense_system(m, GAMMA, 1.0, 0.0))
    f = lambda t, y: Minv @ (SR.apply(m, "wave", (GAMMA,), y) + _heat_data(m, t))  # noqa: E731
    h = 1e-4
    assert prob.run(0.0, 3 * h, h) == 3
    for s in range(3):
        u = cut1d.rk4_step(f, s * h, h, u)
    err = F.rel(_host(prob.u), u)
    print("heat-rk, 3 steps: %.2e" % err)
    assert err <= 1e-12


# -- refusals ------------------------------------------------------------------------------------------------------
def _solve_rc(op, alpha, tau, rhs, x):
    return op.lib.gdm_system_solve(op.h, ctypes.c_double(alpha), ctypes.c_double(tau), ctypes.c_void_p(rhs.data_ptr()),
                                   ctypes.c_void_p(x.data_ptr()))


def _valid_solve_works(name="small-p3"):
    op = _op(name)
    b, x_dense, err_ref = _dense(name, F.DENSE_CASES[0])
    assert F.rel(_host(op.system_solve(1.0, 0.01, _dev(b))), x_dense) <= max(1e-12, 20.0 * err_ref)


def test_refusals():
    import gdm_amd
    from gdm_amd import _capi

    lo, hi = F.BOX_LO, F.BOX_HI
    adv = gdm_amd.GdmOperator(3, 3, (3, 5, 6), lo, hi, "advection", params=(1.0, 0.2, -0.1))
    assert adv.lib.gdm_system_solve_setup(adv.h) == -3 and "wave" in _capi.last_error()
    two = gdm_amd.GdmOperator(3, 3, (3, 5, 8), lo, hi, "wave", params=(GAMMA,), rank=0, n_ranks=2)
    assert two.lib.gdm_system_solve_setup(two.h) == -3 and "rank" in _capi.last_error()
    per = gdm_amd.GdmOperator(3, 3, (3, 5, 6), lo, hi, "wave", periodic=1)
    assert per.lib.gdm_system_solve_setup(per.h) == -3 and "periodic" in _capi.last_error()
    _valid_solve_works()

    op = _op("small-p3", setup=False)
    rhs, x = op.new_vector(local=False), op.new_vector(local=False)
    assert _solve_rc(op, 1.0, 0.01, rhs, x) == -5 and "setup" in _capi.last_error()
    assert op.lib.gdm_fastdiag_transform(op.h, 0, 0, ctypes.c_void_p(rhs.data_ptr()),
                                         ctypes.c_void_p(x.data_ptr())) == -5
    op.system_solve_setup()
    op.system_solve_setup()  # idempotent
    assert op.lib.gdm_system_solve(op.h, ctypes.c_double(1.0), ctypes.c_double(0.01), None,
                                   ctypes.c_void_p(x.data_ptr())) == -1
    assert _solve_rc(op, float("nan"), 0.01, rhs, x) == -1
    assert _solve_rc(op, 1.0, float("inf"), rhs, x) == -1
    for axis in (-1, 3):
        assert op.lib.gdm_fastdiag_transform(op.h, axis, 0, ctypes.c_void_p(rhs.data_ptr()),
                                             ctypes.c_void_p(x.data_ptr())) == -1
    assert _solve_rc(op, 1.0, 0.01, rhs, x) == 0
    _valid_solve_works()

    # pure Neumann Poisson: singular
    neu = _op("small-p3", gamma=0.0)
    assert _solve_rc(neu, 0.0, 1.0, rhs, x) == -1 and "singular" in _capi.last_error()
    assert _solve_rc(neu, 1.0, 0.01, rhs, x) == 0
    # gamma = 4 at p = 5: the penalty is too small, the operator indefinite
    weak = _op("small-p5", gamma=4.0)
    v = weak.new_vector(local=False)
    assert _solve_rc(weak, 1.0, 0.01, v, v) == -1 and "penalty" in _capi.last_error()
    assert _solve_rc(weak, 0.0, 1.0, v, v) == -1 and "penalty" in _capi.last_error()
    _valid_solve_works()
