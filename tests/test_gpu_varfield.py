"""Advection with a separable, spatially varying velocity field
(gdm_op_set_advection_field, csrc/gdm_varstencil.hip) against the numpy
restatement of the reference's cell loop for a pointwise field
(tests/varfield_ref.py, pinned to the oracle in tests/test_varfield_cpu.py).

Tolerance: rel-L2 1e-12 against the helper, the project's bound for fp64
summation-order differences (tests/test_gpu_v8_inflow.py).

Meshes, derived from the volume kernel's tile (T_x, T_y) = (32, 8) nodes and z
chunk 16 planes (gdm_field_tile; kernel axes: 3D (x, y, z), 2D (x, y), 1D z):
  small   every extent p cells (the smallest the operator accepts): every row
          is a wall row;
  middle  each extent one tile / chunk plus 1 node: 33 x 9 x 17 nodes, so a
          tile of a single column, one of a single row and a chunk of one
          plane exist;
  large   two tiles plus a remainder in x and y, two z chunks plus a
          remainder: 69 x 19 x 35 nodes.
The boxes are anisotropic in h.  p in {3, 5} on all three, p in {1, 7, 9} on
the small mesh (the helper's cell loop is the time limit, not the GPU).
"""
import ctypes
import functools
import math

import numpy as np
import pytest

import cut1d
import oracle as O
import varfield_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LO3, HI3 = (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)


def _tile():
    from gdm_amd import _capi

    return _capi.field_tile(5)


def _nsub(kind, p, dim=3):
    """cells per direction of the small / middle / large mesh (kernel axes -> reference directions)"""
    tx, ty, zc = _tile()
    ext = {"small": (p, p, p), "middle": (tx, ty, zc), "large": (2 * tx + 4, 2 * ty + 2, 2 * zc + 2)}[kind]
    if dim == 3:
        return ext
    return ext[:2] if dim == 2 else (ext[2],)


MESHES = [("small", p) for p in (1, 3, 5, 7, 9)] + [(k, p) for k in ("middle", "large") for p in (3, 5)]
MESH_IDS = ["%s-p%d" % kp for kp in MESHES]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _bc_dev(op, bc_ref):
    out = np.zeros(op.n_bc_points)
    out[op.bc_reference_order()] = bc_ref
    return out


def _apply(op, u, bc=None):
    y = op.new_vector(local=False)
    op.apply(u, y, bc)
    return y


# rotation about the off-centre axis (XC, YC) parallel to z plus a constant drift W along it
XC, YC, W = 0.25, 0.3, 0.35


def _rotation_terms():
    return [(0, [None, lambda y: -(y - YC), None]), (1, [lambda x: x - XC, None, None]),
            (2, [None, None, lambda z: W])]


def _rotation_field(x):
    return np.stack([-(x[:, 1] - YC), x[:, 0] - XC, np.full(x.shape[0], W)], axis=1)


@functools.lru_cache(maxsize=None)
def _mesh3(kind, p):
    return O.Mesh(3, p, list(_nsub(kind, p)), list(LO3), list(HI3))


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
@pytest.mark.parametrize("a", [(0.8, -0.45, 0.3), (-0.6, 0.2, -0.9)], ids=["+-+", "-+-"])
def test_constant_field_through_the_field_path(kind, p, a):
    """dim terms with constant factors: equals the constant operator to 1e-13
    (same operator, other summation order) and the helper to 1e-12; with the
    field removed again the plain operator's bits come back."""
    import gdm_amd

    n = _nsub(kind, p)
    m = _mesh3(kind, p)
    rng = np.random.default_rng(p)
    u = rng.uniform(-1, 1, m.n_dofs)
    bc_ref = rng.uniform(-1, 1, m.n_boundary_points())
    plain = gdm_amd.GdmOperator(3, p, n, LO3, HI3, "advection", params=a)
    op = gdm_amd.GdmOperator(3, p, n, LO3, HI3, "advection", params=(9.0, 9.0, 9.0))
    ud, bd = _dev(u), _dev(_bc_dev(op, bc_ref))
    want_plain = _apply(plain, ud, bd)
    # unit factors, the constants as the time scales
    op.set_advection_field([(d, [None, None, None]) for d in range(3)])
    op.set_field_scale(a)
    got = _host(_apply(op, ud, bd))
    r_plain = _rel(got, _host(want_plain))
    r_ref = _rel(got, R.advection_rhs(m, lambda x: np.tile(np.asarray(a), (x.shape[0], 1)), u, bc_ref))
    print("constant field %s p=%d a=%s: vs constant operator %.2e, vs helper %.2e" % (kind, p, a, r_plain, r_ref))
    assert r_plain < 1e-13
    assert r_ref < 1e-12
    # back to the constant path of an operator created with a: bit for bit
    plain2 = gdm_amd.GdmOperator(3, p, n, LO3, HI3, "advection", params=a)
    plain2.set_advection_field([(0, [None, None, None])])
    plain2.set_advection_field([])
    assert torch.equal(_apply(plain2, ud, bd), want_plain)


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
def test_rotation_with_drift_3d(kind, p):
    """3 terms; the lateral faces have inflow and outflow points, the z faces
    one of each: apply(u, bc), apply(u) and add_boundary_data(bc)."""
    import gdm_amd

    n = _nsub(kind, p)
    m = _mesh3(kind, p)
    rng = np.random.default_rng(100 + p)
    u = rng.uniform(-1, 1, m.n_dofs)
    bc_ref = rng.uniform(-1, 1, m.n_boundary_points())
    op = gdm_amd.GdmOperator(3, p, n, LO3, HI3, "advection", params=(1.0, 1.0, 1.0))
    op.set_advection_field(_rotation_terms())
    ud, bd = _dev(u), _dev(_bc_dev(op, bc_ref))
    vol = R.advection_rhs(m, _rotation_field, u, faces=False)
    f_ubc = R.advection_rhs(m, _rotation_field, u, bc_ref, volume=False)
    f_u = R.advection_rhs(m, _rotation_field, u, None, volume=False)
    f_bc = R.advection_rhs(m, _rotation_field, np.zeros_like(u), bc_ref, volume=False)
    # both kinds of points on the lateral faces
    pts = m.boundary_points()
    lateral = np.abs(pts[:, 0] - LO3[0]) < 1e-14
    an = -_rotation_field(pts[lateral])[:, 0]
    assert (an > 0).any() and (an < 0).any()
    r = [_rel(_host(_apply(op, ud, bd)), vol + f_ubc), _rel(_host(_apply(op, ud)), vol + f_u)]
    z = op.new_vector(local=False)
    op.add_boundary_data(bd, z)
    r.append(_rel(_host(z), f_bc))
    print("rotation %s p=%d: apply(u, bc) %.2e, apply(u) %.2e, add_boundary_data %.2e" % (kind, p, *r))
    assert max(r) < 1e-12


def _swirl_terms():
    return [(0, [lambda x: math.sin(math.pi * x) ** 2, lambda y: math.sin(2 * math.pi * y)]),
            (1, [lambda x: -math.sin(2 * math.pi * x), lambda y: math.sin(math.pi * y) ** 2])]


def _swirl_field(x):
    return np.stack([np.sin(np.pi * x[:, 0]) ** 2 * np.sin(2 * np.pi * x[:, 1]),
                     -np.sin(np.pi * x[:, 1]) ** 2 * np.sin(2 * np.pi * x[:, 0])], axis=1)


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
def test_swirl_2d_and_field_scale(kind, p):
    """LeVeque's swirl on the unit square: a.n = 0 on the whole boundary, so
    the face term vanishes (to 1e-12 of the volume term); the time factor
    through set_field_scale."""
    import gdm_amd

    n = _nsub(kind, p, 2)
    m = O.Mesh(2, p, list(n), [0.0, 0.0], [1.0, 1.0])
    rng = np.random.default_rng(200 + p)
    u = rng.uniform(-1, 1, m.n_dofs)
    bc_ref = rng.uniform(-1, 1, m.n_boundary_points())
    op = gdm_amd.GdmOperator(2, p, n, 0.0, 1.0, "advection", params=(1.0, 1.0))
    op.set_advection_field(_swirl_terms())
    ud, bd = _dev(u), _dev(_bc_dev(op, bc_ref))
    vol = R.advection_rhs(m, _swirl_field, u, faces=False)
    y1 = _host(_apply(op, ud, bd))
    assert _rel(y1, R.advection_rhs(m, _swirl_field, u, bc_ref)) < 1e-12
    assert _rel(y1, vol) < 1e-12
    z = op.new_vector(local=False)
    op.add_boundary_data(bd, z)
    assert np.linalg.norm(_host(z)) < 1e-12 * np.linalg.norm(vol)
    s = -0.37
    op.set_field_scale([s, s])
    ys = _host(_apply(op, ud, bd))
    print("swirl %s p=%d: scaled vs s * unscaled %.2e" % (kind, p, _rel(ys, s * y1)))
    assert _rel(ys, s * y1) < 1e-14
    assert _rel(ys, R.advection_rhs(m, lambda x: s * _swirl_field(x), u, bc_ref)) < 1e-12
    op.set_field_scale([1.0, 1.0])
    assert np.array_equal(_host(_apply(op, ud, bd)), y1)


def test_terms_sharing_a_factor_array_give_the_same_bits():
    """one factor array object used by several terms (shared tables and
    sweeps) against equal, separately allocated arrays"""
    import gdm_amd

    p = 3
    n = _nsub("middle", p)
    op = gdm_amd.GdmOperator(3, p, n, LO3, HI3, "advection", params=(1.0, 1.0, 1.0))
    fx = np.cos(1.3 * op.field_points(0))
    fy = 1.0 + 0.5 * np.sin(2.0 * op.field_points(1))
    fz = np.exp(-op.field_points(2))
    rng = np.random.default_rng(7)
    ud = _dev(rng.uniform(-1, 1, op.n_owned))
    bd = _dev(rng.uniform(-1, 1, op.n_bc_points))
    op.set_advection_field([(0, [fx, fy, fz]), (1, [fx, fy, fz]), (2, [fx, fy, None]), (0, [fx, None, fz])])
    shared = _apply(op, ud, bd)
    c = np.copy
    op.set_advection_field([(0, [c(fx), c(fy), c(fz)]), (1, [c(fx), c(fy), c(fz)]), (2, [c(fx), c(fy), None]),
                            (0, [c(fx), None, c(fz)])])
    separate = _apply(op, ud, bd)
    torch.cuda.synchronize()
    assert torch.equal(shared, separate)
    assert float(shared.abs().max()) > 0.0


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
def test_one_dimensional_field(kind, p):
    import gdm_amd

    n = _nsub(kind, p, 1)
    lo, hi = -0.4, 1.7
    m = O.Mesh(1, p, list(n), [lo], [hi])
    rng = np.random.default_rng(300 + p)
    u = rng.uniform(-1, 1, m.n_dofs)
    bc_ref = rng.uniform(-1, 1, m.n_boundary_points())
    for sign in (1.0, -1.0):  # outflow / inflow at the right end
        op = gdm_amd.GdmOperator(1, p, n, lo, hi, "advection", params=(1.0,))
        op.set_advection_field([(0, [lambda x: sign * (1.0 + 0.5 * math.sin(3.0 * x))])])
        field = lambda x: (sign * (1.0 + 0.5 * np.sin(3.0 * x[:, 0])))[:, None]  # noqa: E731
        got = _host(_apply(op, _dev(u), _dev(_bc_dev(op, bc_ref))))
        assert _rel(got, R.advection_rhs(m, field, u, bc_ref)) < 1e-12


@pytest.mark.parametrize("p", [3, 5])
def test_bitwise_repeatable_runs_streams_and_graph_replay(p):
    """ten applies in a row, applies on two alternating ordered streams and a
    captured graph replayed three times (no warm-up call on the capture
    stream) all give the bits of the first call"""
    import gdm_amd

    n = _nsub("middle", p)
    op = gdm_amd.GdmOperator(3, p, n, LO3, HI3, "advection", params=(1.0, 1.0, 1.0))
    op.set_advection_field(_rotation_terms())
    gen = torch.Generator(device="cuda").manual_seed(3)
    u = torch.rand(op.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    bc = torch.rand(op.n_bc_points, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    ref = _apply(op, u, bc)
    torch.cuda.synchronize()
    assert float(ref.abs().max()) > 0.0
    outs = [op.new_vector(local=False) for _ in range(10)]
    for y in outs:
        op.apply(u, y, bc)
    torch.cuda.synchronize()
    for y in outs:
        assert torch.equal(y, ref)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i, y in enumerate(outs):
        y.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[i % 2]):
            op.use_torch_stream()
            op.apply(u, y, bc)
        torch.cuda.synchronize()
    op.use_torch_stream()
    for y in outs:
        assert torch.equal(y, ref)
    y = op.new_vector(local=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            op.apply(u, y, bc)
    torch.cuda.synchronize()
    for _ in range(3):
        y.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, ref)
    op.use_torch_stream()


SINE = [1.0, 0.15, -0.05, 1.0, 2.0, 1.0, 0.3, 0.0, 0.7]


def _sine(pts, t, prm, dim, derivative):
    a, k, ph = prm[0:3], prm[3:6], prm[6:9]
    s = [np.sin(2 * np.pi * k[d] * (pts[:, d] - a[d] * t) + ph[d]) for d in range(dim)]
    c = [np.cos(2 * np.pi * k[d] * (pts[:, d] - a[d] * t) + ph[d]) for d in range(dim)]
    if not derivative:
        return np.prod(s, axis=0)
    r = np.zeros(len(pts))
    for d in range(dim):
        v = -2 * np.pi * k[d] * a[d] * c[d]
        for e in range(dim):
            if e != d:
                v = v * s[e]
        r += v
    return r


@pytest.mark.parametrize("carry_bc", [False, True], ids=["engine-bc", "carry-bc"])
def test_advection_problem_with_time_dependent_rotation(carry_bc):
    """AdvectionProblem with field_scale(t) (advection->set_time before every
    stage's compute_rhs): 3 RK4 steps of a 2D rotation whose angular velocity
    varies in time, against numpy RK4 over the helper and the exact mass inverse"""
    import gdm_amd

    p, n = 3, (20, 16)
    lo, hi = (0.0, 0.0), (1.0, 0.8)
    xc, yc = 0.45, 0.35
    m = O.Mesh(2, p, list(n), list(lo), list(hi))
    op = gdm_amd.GdmOperator(2, p, n, lo, hi, "advection", params=(1.0, 1.0))
    op.set_advection_field([(0, [None, lambda y: -(y - yc)]), (1, [lambda x: x - xc, None])])
    scale = lambda t: (math.cos(7.0 * t), 0.5 + math.cos(7.0 * t) ** 2)  # noqa: E731
    X = np.stack(m.vertex_coords(), axis=1)
    u0 = _sine(np.pad(X, ((0, 0), (0, 1))), 0.0, SINE, 2, 0)
    h, steps = min(m.h) * 0.1, 3
    pts = m.boundary_points()
    u = u0.copy()
    time = cut1d.DiscreteTime(0.0, h * steps, h)
    while not time.is_at_end():
        bc = _sine(pts, time.t, SINE, 2, 0)
        nb = len(bc)

        def f(tt, y):
            s = scale(tt)
            field = lambda x: np.stack([-s[0] * (x[:, 1] - yc), s[1] * (x[:, 0] - xc)], axis=1)  # noqa: E731
            r = R.advection_rhs(m, field, y[nb:], y[:nb])
            return np.concatenate([_sine(pts, tt, SINE, 2, 1), m.kron_mass_inverse(r)])

        u = cut1d.rk4_step(f, time.t, time.next_step_size(), np.concatenate([bc, u]))[nb:]
        time.advance()
    prob = gdm_amd.AdvectionProblem(op, op.FN_SINE_PRODUCT, SINE, carry_bc=carry_bc, field_scale=scale)
    prob.u.copy_(_dev(u0))
    assert prob.run(0.0, h * steps, h) == steps
    r = _rel(_host(prob.u), u)
    print("AdvectionProblem carry_bc=%s: %.2e" % (carry_bc, r))
    assert r < 1e-11


def test_errors():
    """the documented statuses, each with a message from gdm_last_error"""
    import gdm_amd
    from gdm_amd import _capi

    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    lib = _capi.load()
    unit = _capi.FieldTerm()
    unit.component = 0

    def set_field(op, n_terms, terms):
        rc = lib.gdm_op_set_advection_field(op.h, n_terms, terms)
        return rc, _capi.last_error()

    # n_ranks = 2
    op2 = gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "advection", params=(1.0, 0.5, 0.2), rank=0, n_ranks=2)
    rc, msg = set_field(op2, 1, ctypes.byref(unit))
    assert rc == ERR_UNSUPPORTED and "rank" in msg
    # a non-advection kind
    opw = gdm_amd.GdmOperator(2, 3, (6, 5), 0.0, 1.0, "wave")
    rc, msg = set_field(opw, 1, ctypes.byref(unit))
    assert rc == ERR_UNSUPPORTED and "advection" in msg
    op = gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "advection", params=(1.0, 0.5, 0.2))
    # n_terms = 9
    nine = (_capi.FieldTerm * 9)()
    rc, msg = set_field(op, 9, nine)
    assert rc == ERR_ARG and "n_terms" in msg
    # component >= dim
    bad = _capi.FieldTerm()
    bad.component = 3
    rc, msg = set_field(op, 1, ctypes.byref(bad))
    assert rc == ERR_ARG and "component" in msg
    op2d = gdm_amd.GdmOperator(2, 3, (6, 5), 0.0, 1.0, "advection", params=(1.0, 0.5))
    bad.component = 2
    rc, msg = set_field(op2d, 1, ctypes.byref(bad))
    assert rc == ERR_ARG and "component" in msg
    # apply_planes with a field
    op.set_advection_field([(0, [None, None, None])])
    u, y = op.new_vector(), op.new_vector(local=False)
    rc = lib.gdm_apply_planes(op.h, ctypes.c_void_p(u.data_ptr()), ctypes.c_void_p(y.data_ptr()), 0, 4)
    assert rc == ERR_UNSUPPORTED and "field" in _capi.last_error()
    rc = lib.gdm_apply_planes2(op.h, ctypes.c_void_p(u.data_ptr()), ctypes.c_void_p(y.data_ptr()), 0, 2, 4, 6)
    assert rc == ERR_UNSUPPORTED and "field" in _capi.last_error()
    with pytest.raises(gdm_amd.GdmError):
        op.apply_planes(u, y, 0, 4)
    # without the field the planes work again
    op.set_advection_field([])
    op.apply_planes(u, y, 0, 4)
    # the inner operator of a cut-advection handle keeps its constant field
    cut = gdm_amd.CutAdvection(3, 12, 0.0, 1.0, lambda x, y: np.hypot(x - 0.5, y - 0.5) - 0.31, (1.0, 0.5))
    rc = lib.gdm_op_set_advection_field(cut._op, 1, ctypes.byref(unit))
    assert rc == ERR_UNSUPPORTED and "cut" in _capi.last_error()
