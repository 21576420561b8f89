"""Forcing and Dirichlet data of the uncut wave / heat operator on the device
(gdm_add_load_fn, gdm_add_load, gdm_add_dirichlet_data; csrc/gdm_load.hip)
against the numpy restatement of the reference's two data terms
(tests/load_ref.py, pinned to the oracle in tests/test_load_cpu.py).

Tolerance: rel-L2 1e-12 against the helper, the project's bound for fp64
summation-order differences (tests/test_gpu_v8_inflow.py); 1e-13 between the
rank-1 path and the general kernel on the same function.

Meshes, derived from the general kernel's tile (gdm_load_tile: 16 x 16 nodes,
z chunk 32 planes; kernel axes 3D (x, y, z), 2D (x, y), 1D z):
  small   every extent p cells (the smallest the operator accepts): every node
          is a wall node;
  middle  each extent one tile / chunk plus 1 node: 17 x 17 x 33 nodes;
  large   two tiles plus a remainder in x and y, two z chunks plus a
          remainder: 37 x 35 x 67 nodes.
The boxes are anisotropic in h.  p in {1, 3, 5, 7, 9} on small (dim 1, 2, 3),
p in {3, 5} on middle and large, p = 7 on the 2D middle mesh.
"""
import ctypes
import functools
import json
import math
import os
import subprocess

import numpy as np
import pytest

import cut1d
import load_ref as R
import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LO3, HI3 = (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)
GAMMA = 15.0
FN_CONSTANT, FN_CONE, FN_SINE = 0, 1, 2
# GDM_FN_SINE_PRODUCT: a[3], k[3], phi[3] -- every k_d != 0, one a_d = 0
SINE_A, SINE_K, SINE_PHI = (0.3, 0.0, -0.2), (1.0, 0.75, 1.25), (0.1, 0.4, -0.3)
SINE = list(SINE_A) + list(SINE_K) + list(SINE_PHI)
T0 = 0.37


def _tile(p, dim):
    from gdm_amd import _capi

    return _capi.load_tile(p, dim)


def _nsub(kind, p, dim=3):
    """cells per direction of the small / middle / large mesh (kernel axes -> reference directions)"""
    tx, ty, zc = _tile(p, dim)
    ext = {"small": (p, p, p), "middle": (tx, ty, zc), "large": (2 * tx + 4, 2 * ty + 2, 2 * zc + 2)}[kind]
    if dim == 3:
        return ext
    return ext[:2] if dim == 2 else (ext[2],)


MESHES = ([("small", p, dim) for dim in (1, 2, 3) for p in (1, 3, 5, 7, 9)] + [("middle", 7, 2), ("large", 3, 1)] +
          [(k, p, 3) for k in ("middle", "large") for p in (3, 5)])
MESH_IDS = ["%s-p%d-%dd" % kp for kp in MESHES]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(-1)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _mesh(kind, p, dim):
    return O.Mesh(dim, p, list(_nsub(kind, p, dim)), list(LO3[:dim]), list(HI3[:dim]))


def _op(kind, p, dim, op_kind="wave", params=(GAMMA,)):
    import gdm_amd

    return gdm_amd.GdmOperator(dim, p, _nsub(kind, p, dim), LO3[:dim], HI3[:dim], op_kind, params=params)


def _prefilled(op, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(op.n_owned, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1


def _added(op, call, mag, seed=5):
    """after - before of a call that adds into a randomly prefilled vector.  The prefilled entries are
    uniform in [-mag, mag], mag the size of the entries the call adds, so that the rounding of the
    sum (relative to dst) stays relative to the added vector as well."""
    dst = _prefilled(op, seed) * mag
    before = _host(dst).copy()
    call(dst)
    return _host(dst) - before


def _cone_params(dim, outside=False):
    """support crossing the tile borders of every mesh (radius about half the box), or wholly outside the box"""
    if outside:
        return [0.3] + [HI3[d] + 1.0 for d in range(dim)]
    return [0.55] + [0.5 * (LO3[d] + HI3[d]) + 0.07 * (d + 1) for d in range(dim)]


def test_quadrature_points_are_the_gauss_entries_of_field_points():
    op = _op("small", 3, 3)
    m = _mesh("small", 3, 3)
    for d, (got, want) in enumerate(zip(op.quadrature_points(), R.quadrature_points(m))):
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-15
    assert op.load_tile() == _tile(3, 3)


@pytest.mark.parametrize("kind,p,dim", MESHES, ids=MESH_IDS)
def test_add_load_random_samples(kind, p, dim):
    """gdm_add_load with random fq, into a prefilled vector, with a scale"""
    m, op = _mesh(kind, p, dim), _op(kind, p, dim)
    rng = np.random.default_rng(100 * dim + p)
    fgrid = rng.uniform(-1, 1, [int(m.nsub[d]) * (p + 1) for d in reversed(range(dim))])
    want = R.load_vector(m, fgrid)
    fq = _dev(fgrid)
    mag = float(np.abs(want).max())
    e1 = _rel(_added(op, lambda dst: op.add_load(fq, dst), mag), want)
    e2 = _rel(_added(op, lambda dst: op.add_load(fq, dst, scale=-0.75), mag), -0.75 * want)
    dst = op.new_vector(local=False)
    op.add_load(fq, dst)
    e0 = _rel(_host(dst), want)
    print("add_load %s p %d dim %d: rel-L2 %.2e, scaled %.2e, into zeros %.2e" % (kind, p, dim, e1, e2, e0))
    assert e1 <= 1e-12 and e2 <= 1e-12 and e0 <= 1e-12


@pytest.mark.parametrize("kind,p,dim", MESHES, ids=MESH_IDS)
def test_add_load_fn_against_point_values(kind, p, dim):
    """constant, sine product (value and d/dt), cone (support crossing tile
    borders, and wholly outside the box): each against the helper fed with the
    same function's values from numpy"""
    m, op = _mesh(kind, p, dim), _op(kind, p, dim)
    cone = _cone_params(dim)
    cases = [
        ("constant", FN_CONSTANT, [1.7], 0, R.fn_constant(1.7)),
        ("sine", FN_SINE, SINE, 0, R.fn_sine_product(SINE_A, SINE_K, SINE_PHI, T0, dim)),
        ("sine d/dt", FN_SINE, SINE, 1, R.fn_sine_product(SINE_A, SINE_K, SINE_PHI, T0, dim, 1)),
        ("cone", FN_CONE, cone, 0, R.fn_cone(cone[0], cone[1:], dim)),
    ]
    for name, fn, prm, der, f in cases:
        want = R.load_vector(m, R.grid_values(m, f))
        assert np.linalg.norm(want) > 0.0
        dst = op.new_vector(local=False)
        op.add_load_fn(fn, prm, T0, dst, der, 1.0)
        e = _rel(_host(dst), want)
        got = _added(op, lambda d_: op.add_load_fn(fn, prm, T0, d_, der, -1.25), float(np.abs(want).max()))
        e2 = _rel(got, -1.25 * want)
        print("add_load_fn %s %s p %d dim %d: rel-L2 %.2e (prefilled, scaled: %.2e)" % (name, kind, p, dim, e, e2))
        assert e <= 1e-12 and e2 <= 1e-12
    # a cone wholly outside the box, and the d/dt of the constant and of the cone: dst keeps its bits
    dst = _prefilled(op, 9)
    keep = dst.clone()
    op.add_load_fn(FN_CONE, _cone_params(dim, outside=True), T0, dst)
    op.add_load_fn(FN_CONE, cone, T0, dst, 1)
    op.add_load_fn(FN_CONSTANT, [1.7], T0, dst, 1)
    torch.cuda.synchronize()
    assert torch.equal(dst, keep)


@pytest.mark.parametrize("kind,p,dim", [c for c in MESHES if c[0] != "small" or c[1] in (1, 9)],
                         ids=[i for c, i in zip(MESHES, MESH_IDS) if c[0] != "small" or c[1] in (1, 9)])
def test_rank1_path_equals_general_kernel(kind, p, dim):
    m, op = _mesh(kind, p, dim), _op(kind, p, dim)
    for der in (0, 1):
        fq = _dev(R.grid_values(m, R.fn_sine_product(SINE_A, SINE_K, SINE_PHI, T0, dim, der)))
        a, b = op.new_vector(local=False), op.new_vector(local=False)
        op.add_load_fn(FN_SINE, SINE, T0, a, der, 1.0)
        op.add_load(fq, b)
        e = _rel(_host(a), _host(b))
        print("rank-1 vs general %s p %d dim %d derivative %d: %.2e" % (kind, p, dim, der, e))
        assert e <= 1e-13


def test_scale_zero_leaves_dst_bit_for_bit():
    op = _op("middle", 3, 3)
    m = _mesh("middle", 3, 3)
    fq = _dev(np.random.default_rng(1).uniform(-1, 1, int(np.prod([int(m.nsub[d]) * 4 for d in range(3)]))))
    dst = _prefilled(op, 2)
    keep = dst.clone()
    op.add_load(fq, dst, scale=0.0)
    op.add_load_fn(FN_SINE, SINE, T0, dst, 0, 0.0)
    op.add_load_fn(FN_CONE, _cone_params(3), T0, dst, 0, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(dst, keep)


# -- Dirichlet data ------------------------------------------------------------------------------------------------
def _g_dev(op, g_ref):
    out = np.zeros(op.n_bc_points)
    out[op.bc_reference_order()] = g_ref
    return _dev(out)


@pytest.mark.parametrize("gamma", [15.0, 4.0])
@pytest.mark.parametrize("kind,p,dim", MESHES, ids=MESH_IDS)
def test_dirichlet_data_random_g(kind, p, dim, gamma):
    """random g in the reference's order against Mesh.wave_rhs(0, impl=False,
    nitsche, gbc) (small meshes: the oracle's cell loop itself) or the helper
    pinned to it (middle, large: the oracle's loop is too slow there)"""
    m, op = _mesh(kind, p, dim), _op(kind, p, dim, params=(gamma,))
    assert op.n_bc_points == op.n_bc_points_ref == m.n_boundary_points()
    g_ref = np.random.default_rng(p + dim).uniform(-1, 1, m.n_boundary_points())
    if kind == "small":
        want = m.wave_rhs(np.zeros(m.n_dofs), impl=False, nitsche=gamma, gbc=g_ref)
    else:
        want = R.dirichlet_data(m, gamma, g_ref)
    g = _g_dev(op, g_ref)
    dst = op.new_vector(local=False)
    op.add_dirichlet_data(g, dst)
    e = _rel(_host(dst), want)
    e2 = _rel(_added(op, lambda d_: op.add_dirichlet_data(g, d_), float(np.abs(want).max())), want)
    print("dirichlet data %s p %d dim %d gamma %g: rel-L2 %.2e (prefilled %.2e)" % (kind, p, dim, gamma, e, e2))
    assert e <= 1e-12 and e2 <= 1e-12


@pytest.mark.parametrize("dim,p,n_sub", [(3, 3, (6, 5, 7)), (2, 5, (8, 7)), (1, 3, (9,))])
def test_dirichlet_data_of_one_face_fills_the_planes_behind_it(dim, p, n_sub):
    import gdm_amd

    op = gdm_amd.GdmOperator(dim, p, n_sub, LO3[:dim], HI3[:dim], "wave", params=(GAMMA,))
    m = O.Mesh(dim, p, list(n_sub), list(LO3[:dim]), list(HI3[:dim]))
    xyz = op.bc_points()
    N = [n + 1 for n in n_sub]
    idx = np.unravel_index(np.arange(m.n_dofs), N[::-1])[::-1]  # idx[d] = node index along d
    for d in range(dim):
        for side in (0, 1):
            on_face = np.abs(xyz[:, d] - (HI3[d] if side else LO3[d])) < 1e-12
            for e in range(dim):  # the face's points lie strictly inside it along the other directions
                if e != d:
                    on_face &= (xyz[:, e] > LO3[e] + 1e-12) & (xyz[:, e] < HI3[e] - 1e-12)
            assert on_face.sum() == np.prod([n_sub[e] * (p + 1) for e in range(dim) if e != d])
            g = np.where(on_face, 1.0 + np.random.default_rng(d).uniform(0, 1, xyz.shape[0]), 0.0)
            dst = op.new_vector(local=False)
            op.add_dirichlet_data(_dev(g), dst)
            behind = idx[d] >= N[d] - 1 - p if side else idx[d] <= p
            assert np.array_equal(_host(dst) != 0.0, behind)


def test_dirichlet_data_needs_a_nitsche_wave_operator():
    import gdm_amd

    for op in (gdm_amd.GdmOperator(2, 3, (5, 4), LO3[:2], HI3[:2], "wave"),
               gdm_amd.GdmOperator(2, 3, (5, 4), LO3[:2], HI3[:2], "advection", params=(1.0, 0.5))):
        g = torch.zeros(max(op.n_bc_points, 1), dtype=torch.float64, device="cuda")
        dst = op.new_vector(local=False)
        rc = op.lib.gdm_add_dirichlet_data(op.h, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(dst.data_ptr()))
        assert rc == -3  # GDM_ERR_UNSUPPORTED
        assert "nitsche" in gdm_amd._capi.last_error()
        # the load itself does not depend on the operator kind
        op.add_load_fn(FN_CONSTANT, [1.0], 0.0, dst)
        assert float(dst.sum()) == pytest.approx((HI3[0] - LO3[0]) * (HI3[1] - LO3[1]), rel=1e-13)


def test_error_codes():
    import gdm_amd

    L = gdm_amd._capi.load()
    prm = (ctypes.c_double * 9)(*SINE)
    ops = [gdm_amd.GdmOperator(3, 3, (5, 4, 8), LO3, HI3, "wave", params=(GAMMA,), rank=0, n_ranks=2),
           gdm_amd.GdmOperator(2, 3, (5, 4), LO3[:2], HI3[:2], "wave", periodic=1)]
    for op in ops:
        dst = op.new_vector(local=False)
        buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
        dp, bp = ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(buf.data_ptr())
        assert L.gdm_add_load_fn(op.h, FN_SINE, prm, 9, 0.0, 0, 1.0, dp) == -3
        assert L.gdm_add_load(op.h, bp, 1.0, dp) == -3
        assert L.gdm_add_dirichlet_data(op.h, bp, dp) == -3
    op = _op("small", 3, 2)
    dst = op.new_vector(local=False)
    dp = ctypes.c_void_p(dst.data_ptr())
    assert L.gdm_add_load_fn(op.h, FN_SINE, prm, 9, 0.0, 0, 1.0, None) == -1   # NULL vector
    assert L.gdm_add_load_fn(op.h, FN_SINE, prm, 9, 0.0, 2, 1.0, dp) == -1     # derivative outside {0, 1}
    assert L.gdm_add_load_fn(op.h, FN_SINE, prm, 9, 0.0, -1, 1.0, dp) == -1
    assert L.gdm_add_load_fn(op.h, FN_SINE, prm, 8, 0.0, 0, 1.0, dp) == -1     # too few parameters
    assert L.gdm_add_load_fn(op.h, 3, prm, 9, 0.0, 0, 1.0, dp) == -1           # unknown kind
    assert L.gdm_add_load_fn(op.h, FN_CONE, prm, 2, 0.0, 0, 1.0, dp) == -1     # cone needs 1 + dim
    assert L.gdm_add_load_fn(None, FN_SINE, prm, 9, 0.0, 0, 1.0, dp) == -1
    assert L.gdm_add_load(op.h, None, 1.0, dp) == -1
    assert L.gdm_add_load(op.h, dp, 1.0, None) == -1
    assert L.gdm_add_dirichlet_data(op.h, None, dp) == -1
    assert L.gdm_add_dirichlet_data(op.h, dp, None) == -1
    torch.cuda.synchronize()
    assert float(dst.abs().max()) == 0.0


# -- repeatability -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [3, 5])
def test_bitwise_repeatable_runs_streams_and_graph_replay(p):
    """the three calls in a row ten times, on two alternating ordered streams,
    and in a captured graph replayed three times -- the graph is captured on a
    fresh operator, so its first calls are the captured ones -- all give the
    bits of the first run"""
    kind, dim = "middle", 3
    m = _mesh(kind, p, dim)
    rng = np.random.default_rng(p)
    fq = _dev(rng.uniform(-1, 1, int(np.prod([int(m.nsub[d]) * (p + 1) for d in range(dim)]))))
    cone = _cone_params(dim)

    def run(op, g, y):
        op.add_load(fq, y, 0.5)
        op.add_load_fn(FN_SINE, SINE, T0, y, 0, 1.5)
        op.add_load_fn(FN_SINE, SINE, T0, y, 1, -0.5)
        op.add_load_fn(FN_CONE, cone, T0, y)
        op.add_dirichlet_data(g, y)

    op = _op(kind, p, dim)
    g = _dev(rng.uniform(-1, 1, op.n_bc_points))
    ref = op.new_vector(local=False)
    run(op, g, ref)
    torch.cuda.synchronize()
    assert float(ref.abs().max()) > 0.0
    outs = [op.new_vector(local=False) for _ in range(10)]
    for y in outs:
        run(op, g, y)
    torch.cuda.synchronize()
    for y in outs:
        assert torch.equal(y, ref)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i, y in enumerate(outs):
        y.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[i % 2]):
            op.use_torch_stream()
            run(op, g, y)
        torch.cuda.synchronize()
    op.use_torch_stream()
    for y in outs:
        assert torch.equal(y, ref)
    op2 = _op(kind, p, dim)
    y = op2.new_vector(local=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op2.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            run(op2, g, y)
    torch.cuda.synchronize()
    for _ in range(3):
        y.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, ref)
    op2.use_torch_stream()


# -- golden pin: tests/mass_01_gdm.cc on the device ---------------------------------------------------------------
def test_mass_01_projection_on_the_device():
    """2D L2 projection of f = x, p = 3, n = 40: add_load, then SolverCG +
    Jacobi (rel 1e-8, abs 1e-10, 100 iterations at most).  The L2 error equals
    the reference's printed value to rtol 1e-4 (the bound of the oracle's own
    test, tests/test_oracle_golden.py) and the iteration count the oracle's 18;
    with the exact mass inverse the projection error of x is <= 1e-13."""
    import gdm_amd

    ref = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_outputs.json")))
    p, n = 3, 40
    m = O.Mesh(2, p, n)
    op = gdm_amd.GdmOperator(2, p, n, 0.0, 1.0, "mass")
    fq = _dev(R.grid_values(m, lambda x, y, z: x))
    rhs, x = op.new_vector(local=False), op.new_vector(local=False)
    op.add_load(fq, rhs)
    its, _ = op.mass_solve_cg(rhs, x, rel_tol=1e-8, abs_tol=1e-10, max_it=100, precond=1)
    xq = m.cell_qpoints()
    err = m.l2_error(_host(x), xq[:, 0])
    print("mass_01 on the device: %d iterations, L2 error %.6e (reference %.6e)" % (its, err,
                                                                                   ref["mass_01"]["error"]))
    assert its == 18
    np.testing.assert_allclose(err, ref["mass_01"]["error"], rtol=1e-4)
    op.mass_solve(rhs, x)
    err_exact = m.l2_error(_host(x), xq[:, 0])
    print("mass_01 with the exact mass inverse: L2 error %.3e" % err_exact)
    assert err_exact <= 1e-13


# -- end to end ----------------------------------------------------------------------------------------------------
# u = sin(2 pi k0 (x - a0 t) + phi0) sin(2 pi k1 y + phi1) sin(2 pi k2 z + phi2):
# u_tt - Laplace u = (2 pi)^2 (sum k_d^2 - k0^2 a0^2) u, a scaled sine product
E2E_A, E2E_K, E2E_PHI = (0.8, 0.0, 0.0), (1.0, 0.5, 0.75), (0.3, 0.5, 0.2)
E2E = list(E2E_A) + list(E2E_K) + list(E2E_PHI)
E2E_SCALE = (2.0 * math.pi) ** 2 * (sum(k * k for k in E2E_K) - (E2E_K[0] * E2E_A[0]) ** 2)


def _initial(prob, m):
    X = m.vertex_coords()
    u0 = R.fn_sine_product(E2E_A, E2E_K, E2E_PHI, 0.0, 3)(*X)
    v0 = R.fn_sine_product(E2E_A, E2E_K, E2E_PHI, 0.0, 3, 1)(*X)
    prob.u.copy_(_dev(u0))
    prob.v.copy_(_dev(v0))
    return u0, v0


def test_wave_problem_with_forcing_and_data_equals_the_oracle_rk4():
    import gdm_amd

    n_sub, h = (6, 5, 7), 0.004
    m = O.Mesh(3, 3, list(n_sub), list(LO3), list(HI3))
    op = gdm_amd.GdmOperator(3, 3, n_sub, LO3, HI3, "wave", params=(GAMMA,))
    prob = gdm_amd.WaveProblem(op, forcing=(FN_SINE, E2E, E2E_SCALE), dirichlet=(FN_SINE, E2E))
    u0, v0 = _initial(prob, m)
    N = m.n_dofs
    bxyz = m.boundary_points()

    def f(t, y):
        fq = E2E_SCALE * R.cell_major(m, R.grid_values(m, R.fn_sine_product(E2E_A, E2E_K, E2E_PHI, t, 3)))
        gbc = R.fn_sine_product(E2E_A, E2E_K, E2E_PHI, t, 3)(bxyz[:, 0], bxyz[:, 1], bxyz[:, 2])
        return np.concatenate([y[N:], m.kron_mass_inverse(m.wave_rhs(y[:N], True, fq, GAMMA, gbc))])

    y = np.concatenate([u0, v0])
    for s in range(3):
        y = cut1d.rk4_step(f, s * h, h, y)
        prob.step(s * h, h)
    eu, ev = _rel(_host(prob.u), y[:N]), _rel(_host(prob.v), y[N:])
    print("3 forced RK4 steps against the oracle: u %.2e v %.2e" % (eu, ev))
    assert eu <= 1e-10 and ev <= 1e-10
    # rhs(t, .) is the same function of t
    out = op.new_vector(local=False)
    prob.rhs(0.011, _dev(y[:N]), out)
    assert _rel(_host(out), f(0.011, y)[N:]) <= 1e-10


def test_wave_problem_converges_to_the_manufactured_solution():
    """the same problem on the unit cube at 12^3 and 24^3 cells, p = 3, to a
    fixed end time: the L2 error falls by at least 2^p (one order below the
    nominal p + 1, as slack for the time error)"""
    import gdm_amd

    errs = []
    for n in (12, 24):
        m = O.Mesh(3, 3, n)
        op = gdm_amd.GdmOperator(3, 3, n, 0.0, 1.0, "wave", params=(GAMMA,))
        prob = gdm_amd.WaveProblem(op, forcing=(FN_SINE, E2E, E2E_SCALE), dirichlet=(FN_SINE, E2E))
        _initial(prob, m)
        prob.run(0.0, 0.04, 0.002)
        errs.append(op.error_norms(prob.u, FN_SINE, E2E, 0.04)[2])
    print("manufactured wave solution, L2 error at 12^3: %.4e, at 24^3: %.4e, ratio %.2f" % (errs[0], errs[1],
                                                                                           errs[0] / errs[1]))
    assert errs[1] * 2 ** 3 <= errs[0]


# -- the C++ host mirror (host/include/gdm/hip/wave.h) ------------------------------------------------------------
WAVE_APP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "dealii-galerkin-difference-methods_amd", "lib", "host", "wave_app")


@pytest.mark.parametrize("dim,p,n", [(2, 3, 9), (3, 3, 6)])
def test_host_mirror_function_rhs_and_domain_dbc(dim, p, n, tmp_path):
    """wave_app DATA = 1: Parameters::function_rhs / function_domain_dbc through
    compute_rhs(dst, src, true, time) of the C++ mirror equal gdm_amd.WaveProblem
    with the same data as host-evaluated arrays (add_load, add_dirichlet_data)"""
    import gdm_amd

    steps, cfl, lo, hi = 3, 0.05, -1.21, 1.21
    a, k, phi = (0.8, 0.0, 0.0), (0.4, 0.3, 0.35), (0.3, 0.5, 0.2)
    out = tmp_path / "uv.bin"
    r = subprocess.run([WAVE_APP, str(dim), str(p), str(n), str(steps), str(cfl), str(out), str(GAMMA), "0", "1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    uv = np.fromfile(out, dtype=np.float64)
    m = O.Mesh(dim, p, n, lo, hi)
    op = gdm_amd.GdmOperator(dim, p, n, lo, hi, "wave", params=(GAMMA,))
    bxyz = op.bc_points()
    w = lambda t: R.fn_sine_product(a, k, phi, t, dim)  # noqa: E731
    prob = gdm_amd.WaveProblem(op, forcing=lambda t: _dev(3.0 * R.grid_values(m, w(t))),
                               dirichlet=lambda t: _dev(w(t)(bxyz[:, 0], bxyz[:, 1], bxyz[:, 2])))
    X = list(m.vertex_coords()) + [0.0] * (3 - dim)
    prob.u.copy_(_dev(w(0.0)(*X)))
    assert prob.run(0.0, 1e9, cfl * (hi - lo) / n, max_steps=steps) == steps
    N = m.n_dofs
    assert uv.size == 2 * N
    eu, ev = _rel(uv[:N], _host(prob.u)), _rel(uv[N:], _host(prob.v))
    print("host mirror with data, dim %d: u %.2e v %.2e" % (dim, eu, ev))
    assert eu <= 1e-12 and ev <= 1e-12
