"""The C++ host mirror of the wave application's simulation types that solve
with the stiffness matrix (dealii-galerkin-difference-methods_amd/host,
gdm/hip/wave.h: Parameters::simulation_type = "poisson", "heat-impl",
"heat-rk"; applications/wave/include/gdm/wave/problem.h:46-128, 210-279),
driven through wave_app, against the Python drivers (gdm_amd.solve_poisson,
gdm_amd.HeatProblem) with the same data as host-evaluated arrays.  Both run
the same engine calls, so the values agree to round-off: rel-L2 1e-12.
"""
import os
import subprocess

import numpy as np
import pytest

import load_ref as R
import oracle as O

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE_APP = os.path.join(ROOT, "dealii-galerkin-difference-methods_amd", "lib", "host", "wave_app")
GAMMA = 15.0
LO, HI = -1.21, 1.21
# wave_app DATA = 1: function_rhs = 3 w, function_domain_dbc = w, u0 = w(., 0)
A, K, PHI = (0.8, 0.0, 0.0), (0.4, 0.3, 0.35), (0.3, 0.5, 0.2)
DIM, P, N = 2, 3, 9


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _app(tmp_path, steps, cfl, sim):
    out = tmp_path / "uv.bin"
    r = subprocess.run([WAVE_APP, str(DIM), str(P), str(N), str(steps), str(cfl), str(out), str(GAMMA), "0", "1", sim],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    uv = np.fromfile(out, dtype=np.float64)
    n = (N + 1) ** DIM
    assert uv.size == 2 * n
    assert not uv[n:].any()  # no velocity block in these simulation types
    return uv[:n]


def _setup():
    import gdm_amd

    m = O.Mesh(DIM, P, N, LO, HI)
    op = gdm_amd.GdmOperator(DIM, P, N, LO, HI, "wave", params=(GAMMA,))
    bxyz = op.bc_points()
    w = lambda t: R.fn_sine_product(A, K, PHI, t, DIM)  # noqa: E731
    forcing = lambda t: _dev(3.0 * R.grid_values(m, w(t)))  # noqa: E731
    dirichlet = lambda t: _dev(w(t)(bxyz[:, 0], bxyz[:, 1], bxyz[:, 2]))  # noqa: E731
    u0 = w(0.0)(*(list(m.vertex_coords()) + [0.0] * (3 - DIM)))
    return gdm_amd, op, forcing, dirichlet, u0


def test_wave_app_poisson(tmp_path):
    u_app = _app(tmp_path, 0, 0.05, "poisson")
    gdm_amd, op, forcing, dirichlet, _ = _setup()
    u = _host(gdm_amd.solve_poisson(op, forcing, dirichlet, 0.0))
    err = _rel(u_app, u)
    print("wave_app poisson against solve_poisson: %.2e" % err)
    assert np.linalg.norm(u) > 0.0 and err <= 1e-12


@pytest.mark.parametrize("sim,scheme,cfl", [("heat-impl", "impl", 0.05), ("heat-rk", "rk", 0.0005)])
def test_wave_app_heat(tmp_path, sim, scheme, cfl):
    steps = 3
    u_app = _app(tmp_path, steps, cfl, sim)
    gdm_amd, op, forcing, dirichlet, u0 = _setup()
    prob = gdm_amd.HeatProblem(op, forcing, dirichlet, scheme=scheme)
    prob.u.copy_(_dev(u0))
    assert prob.run(0.0, 1e9, cfl * (HI - LO) / N, max_steps=steps) == steps
    u = _host(prob.u)
    err = _rel(u_app, u)
    print("wave_app %s against HeatProblem(%s): %.2e, moved %.2e" % (sim, scheme, err, _rel(u, u0)))
    assert _rel(u, u0) > 1e-6 and err <= 1e-12


def test_wave_app_default_is_wave_rk(tmp_path):
    """the trailing argument left out, and given as wave-rk: the same bytes"""
    outs = []
    for extra in ([], ["wave-rk"]):
        out = tmp_path / ("uv%d.bin" % len(extra))
        r = subprocess.run([WAVE_APP, str(DIM), str(P), str(N), "2", "0.05", str(out), str(GAMMA), "0", "1"] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append((r.stdout, out.read_bytes()))
    assert outs[0] == outs[1]
    bad = subprocess.run([WAVE_APP, str(DIM), str(P), str(N), "2", "0.05", str(tmp_path / "x.bin"), str(GAMMA), "0", "1",
                          "heat"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "simulation_type" in bad.stderr
