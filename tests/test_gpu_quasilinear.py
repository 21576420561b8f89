"""QuasilinearHeatProblem (gdm_amd/problem.py): u_t = M^-1 (K[kappa(u)] u +
data(t)) with kappa(u) = 1 + u^2 re-evaluated from every stage vector on the
device (eval_grid / eval_trace -> torch -> the borrowed kq / kbc), against a
numpy RK4 built from tests/evalgrid_ref.py (values, trace, wave_rhs_grid),
tests/load_ref.py and Mesh.kron_mass_inverse.

2D and 3D at p = 3 on the middle mesh of tests/test_gpu_evalgrid.py; 3 steps at
a tenth of the explicit limit of the constant operator at kappa_max: RK4's
real-axis stability bound 2.785 over kappa_max sum_d max lambda_d, the
generalised eigenvalues of (A_d, M_d) from tests/fastdiag_ref.py.

Tolerance: rel-L2 < 1e-10 after the steps, the bound of tests/test_gpu_rk.py
(mass solves and operator applications accumulate over the stages).
"""
import numpy as np
import pytest

import cut1d
import evalgrid_ref as E
import fastdiag_ref as FD
import load_ref as L
import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LO3, HI3 = (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)
FN_SINE_PRODUCT = 2
SINE = dict(a=(0.3, -0.2, 0.1), k=(0.5, 0.75, 0.4), phi=(0.1, 0.4, -0.3))


def _nsub(p, dim):
    """the middle mesh: one work item / tile plus one cell per extent"""
    from gdm_amd import _capi

    ex, ey, ez = _capi.eval_grid_tile(p, dim)
    tx, ty, zc = _capi.load_tile(p, dim)
    ext = (max(ex + 1, tx), max(ey + 1, ty), max(ez + 1, zc))
    return ext if dim == 3 else ext[:2]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float64).reshape(-1)).cuda()


def kappa(u):
    """works on device tensors and on numpy arrays"""
    return 1.0 + u * u


def _setup(dim, p):
    n_sub = _nsub(p, dim)
    m = O.Mesh(dim, p, list(n_sub), list(LO3[:dim]), list(HI3[:dim]))
    xv = m.vertex_coords()
    u0 = 0.8 * np.prod([np.cos(2.0 * (d + 1) * xv[d] + 0.3 * d) for d in range(dim)], axis=0)
    return n_sub, m, u0


def _dt(m, nitsche, kappa_max):
    lam_max = sum(float(lam.max()) for _, lam in FD.eigenpairs(m, nitsche))
    return 0.1 * 2.785 / (kappa_max * lam_max)


@pytest.mark.parametrize("data", [False, True], ids=["homogeneous", "nitsche-data"])
@pytest.mark.parametrize("dim", [2, 3])
def test_quasilinear_heat_rk4(dim, data):
    import gdm_amd

    p = 3
    n_sub, m, u0 = _setup(dim, p)
    nitsche = 6.0 * p * p if data else 0.0
    h = _dt(m, nitsche, float(kappa(np.abs(u0).max())))
    op = gdm_amd.GdmOperator(dim, p, n_sub, LO3[:dim], HI3[:dim], "wave", params=(nitsche,) if data else ())

    forcing = dirichlet = None
    f0 = g_ref = None
    if data:
        f0 = L.grid_values(m, lambda x, y, z: np.sin(2 * x + y) * np.cos(1.5 * z + 0.2) + 0.5)
        f0_dev = _dev(f0)
        forcing = lambda t: (1.0 + t) * f0_dev  # noqa: E731
        prm = list(SINE["a"]) + list(SINE["k"]) + list(SINE["phi"])
        dirichlet = (FN_SINE_PRODUCT, prm)
        xb = m.boundary_points()
        g_ref = lambda t: L.fn_sine_product(SINE["a"], SINE["k"], SINE["phi"], t, dim)(xb[:, 0], xb[:, 1], xb[:, 2])  # noqa: E731

    def f(t, u):
        kq = kappa(E.values(m, u))
        kbc = kappa(E.trace(m, u)[0]) if data else None
        r = E.wave_rhs_grid(m, kq, kbc, u, nitsche, g_ref(t) if data else None)
        if data:
            r = r + L.load_vector(m, (1.0 + t) * f0)
        return m.kron_mass_inverse(r)

    steps = 3
    y = u0.copy()
    for n in range(steps):
        y = cut1d.rk4_step(f, n * h, h, y)

    prob = gdm_amd.QuasilinearHeatProblem(op, kappa, forcing=forcing, dirichlet=dirichlet)
    prob.u.copy_(_dev(u0))
    for n in range(steps):
        prob.step(n * h, h)
        # the borrowed array holds kappa of the last stage vector, bit for bit
        assert torch.equal(prob.kq, kappa(op.eval_grid(prob.last_stage, gradients=False)))
        if data:
            assert torch.equal(prob.kbc, kappa(op.eval_trace(prob.last_stage, dn_bc=False)))
    torch.cuda.synchronize()
    got = prob.u.cpu().numpy()
    r = _rel(got, y)
    moved = _rel(u0, y)
    print("quasilinear heat %dD p=%d data=%s: dt %.3e, rel %.2e (the solution moved by %.2e)" % (dim, p, data, h, r,
                                                                                                moved))
    assert moved > 1e-6  # the steps do something
    assert r < 1e-10


def test_constructor_checks():
    import gdm_amd

    op = gdm_amd.GdmOperator(2, 3, (6, 5), 0.0, 1.0, "mass")
    with pytest.raises(gdm_amd.GdmError):
        gdm_amd.QuasilinearHeatProblem(op, kappa)
    op = gdm_amd.GdmOperator(2, 3, (6, 5), 0.0, 1.0, "wave")
    with pytest.raises(gdm_amd.GdmError):
        gdm_amd.QuasilinearHeatProblem(op, 1.0)
    with pytest.raises(gdm_amd.GdmError):  # Dirichlet data without Nitsche terms
        gdm_amd.QuasilinearHeatProblem(op, kappa, dirichlet=(FN_SINE_PRODUCT, [0.0] * 9))
