"""The wave / heat / Poisson operator with a separable coefficient
(gdm_op_set_coefficient, csrc/gdm_vardiff.hip) against the numpy restatement of
the reference's cell loop for a pointwise kappa (tests/vardiff_ref.py, pinned
to the oracle in tests/test_vardiff_cpu.py).

Tolerance: rel-L2 1e-12 against the restatement, the project's bound for fp64
summation-order differences (tests/test_gpu_varfield.py).

Meshes, derived from the kernel's tile (T_x, T_y) and z chunk (gdm_coef_tile;
kernel axes: 3D (x, y, z), 2D (x, y), 1D z):
  small   every extent p cells (the smallest the operator accepts): every row
          is a wall row;
  middle  each extent one tile / chunk plus 1 node, so a tile of a single
          column, one of a single row and a chunk of one plane exist;
  large   two tiles plus a remainder in x and y, two z chunks plus a remainder.
The boxes are anisotropic in h.  p in {3, 5} on all three, p in {1, 7, 9} on
the small mesh (the restatement's cell loop is the time limit, not the GPU).

Coefficients on the box (-0.5, 0, 0.2) - (0.7, 0.9, 1.5):
  one   (1 + 0.5 sin 3x) e^y (1 + z^2)
  four  2 + 0.5 sin 3x + 0.4 z cos 2y + 0.3 x y z; the variable part is bounded
        by 0.5 + 0.6 + 0.28 = 1.38 < 2 there
(in 2D the z factors are dropped, in 1D the y factors too).
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle as O
import vardiff_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LO3, HI3 = (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -3, -5


def _tile():
    from gdm_amd import _capi

    return _capi.coef_tile(5, 3)


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


def _apply(op, u):
    y = op.new_vector(local=False)
    op.apply(u, y)
    return y


def _terms(which, dim):
    """the separable terms of a coefficient: a list of per-direction callables / None"""
    if which == "one":
        t = [[lambda x: 1 + 0.5 * np.sin(3 * x), np.exp, lambda z: 1 + z * z]]
    else:
        t = [[lambda x: 2.0, None, None],
             [lambda x: 0.5 * np.sin(3 * x), None, None],
             [None, lambda y: 0.4 * np.cos(2 * y), lambda z: z],
             [lambda x: 0.3 * x, lambda y: y, lambda z: z]]
    return [f[:dim] for f in t]


def _kappa(which, dim):
    terms = _terms(which, dim)

    def kappa(x):
        s = 0.0
        for t in terms:
            v = np.ones(x.shape[0])
            for d in range(dim):
                if t[d] is not None:
                    v = v * t[d](x[:, d])
            s = s + v
        return s

    return kappa


def _nitsche(p):
    return 6.0 * p * p


@functools.lru_cache(maxsize=None)
def _mesh(dim, kind, p):
    return O.Mesh(dim, p, list(_nsub(kind, p, dim)), list(LO3[:dim]), list(HI3[:dim]))


def _op(dim, kind, p, nitsche, which=None):
    import gdm_amd

    op = gdm_amd.GdmOperator(dim, p, _nsub(kind, p, dim), LO3[:dim], HI3[:dim], "wave",
                             params=(nitsche,) if nitsche else ())
    if which is not None:
        op.set_coefficient(_terms(which, dim))
    return op


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
def test_apply_3d(kind, p):
    """K[kappa] u: one term without Nitsche terms, four terms with them (the
    large mesh: the four-term case alone; small-p9 is the largest LDS plan)"""
    m = _mesh(3, kind, p)
    rng = np.random.default_rng(p)
    u = rng.uniform(-1, 1, m.n_dofs)
    cases = [("four", _nitsche(p))] if kind == "large" else [("one", 0.0), ("four", _nitsche(p)), ("one", _nitsche(p))]
    if kind == "middle":
        cases = cases[:2]
    for which, nit in cases:
        got = _host(_apply(_op(3, kind, p, nit, which), _dev(u)))
        r = _rel(got, R.wave_rhs(m, _kappa(which, 3), u, nit))
        print("apply 3D %s p=%d %s nitsche=%g: %.2e" % (kind, p, which, nit, r))
        assert r < 1e-12


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
@pytest.mark.parametrize("dim", [1, 2])
def test_apply_1d_2d(dim, kind, p):
    m = _mesh(dim, kind, p)
    rng = np.random.default_rng(10 * dim + p)
    u = rng.uniform(-1, 1, m.n_dofs)
    for which in ("one", "four"):
        for nit in (0.0, _nitsche(p)):
            got = _host(_apply(_op(dim, kind, p, nit, which), _dev(u)))
            r = _rel(got, R.wave_rhs(m, _kappa(which, dim), u, nit))
            print("apply %dD %s p=%d %s nitsche=%g: %.2e" % (dim, kind, p, which, nit, r))
            assert r < 1e-12


@pytest.mark.parametrize("kind,p", [("small", p) for p in (1, 3, 5, 7, 9)] + [("middle", 3), ("middle", 5)])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_unit_coefficient_equals_the_constant_stencil(dim, kind, p):
    """kappa = 1 as one term of unit factors: the constant wave stencil to 1e-13
    (same operator, other summation order); n_terms = 0 brings the constant
    path's bits back"""
    for nit in (0.0, _nitsche(p)):
        plain = _op(dim, kind, p, nit)
        gen = torch.Generator(device="cuda").manual_seed(p)
        u = torch.rand(plain.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        want = _apply(plain, u)
        op = _op(dim, kind, p, nit)
        op.set_coefficient([[lambda s: 1.0] * dim])
        r = _rel(_host(_apply(op, u)), _host(want))
        print("unit coefficient %dD %s p=%d nitsche=%g: %.2e" % (dim, kind, p, nit, r))
        assert r < 1e-13
        op.set_coefficient([[None] * dim])
        assert _rel(_host(_apply(op, u)), _host(want)) < 1e-13
        op.set_coefficient([])
        assert torch.equal(_apply(op, u), want)


@pytest.mark.parametrize("dim,kind,p", [(3, "middle", 3), (3, "small", 5), (2, "large", 5), (1, "large", 3)])
def test_symmetry(dim, kind, p):
    """v^T K u = u^T K v to 1e-13 of |v| |K u|"""
    op = _op(dim, kind, p, _nitsche(p), "four")
    gen = torch.Generator(device="cuda").manual_seed(7)
    u = torch.rand(op.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    v = torch.rand(op.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    Ku, Kv = _apply(op, u), _apply(op, v)
    a, b = float(torch.dot(v, Ku)), float(torch.dot(u, Kv))
    scale = float(torch.linalg.norm(v) * torch.linalg.norm(Ku))
    print("symmetry %dD %s p=%d: %.16e %.16e" % (dim, kind, p, a, b))
    assert abs(a - b) <= 1e-13 * scale


def test_shared_factor_arrays_give_the_bits_of_copies():
    p = 3
    op = _op(3, "middle", p, _nitsche(p))
    fx = np.array([1 + 0.5 * np.sin(3 * x) for x in op.field_points(0)])
    fy = np.exp(op.field_points(1))
    fz = 1 + op.field_points(2) ** 2
    gen = torch.Generator(device="cuda").manual_seed(11)
    u = torch.rand(op.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    op.set_coefficient([[fx, fy, fz], [fx, None, fz], [fx, fy, None]])
    shared = _apply(op, u)
    op.set_coefficient([[fx.copy(), fy.copy(), fz.copy()], [fx.copy(), None, fz.copy()], [fx.copy(), fy.copy(), None]])
    assert torch.equal(_apply(op, u), shared)
    assert float(shared.abs().max()) > 0.0


@pytest.mark.parametrize("p", [3, 5])
def test_bitwise_repeatable_runs_streams_and_graph_replay(p):
    """a second run, an apply on a second stream and a captured graph replayed
    after one warm-up give the bits of the first call"""
    op = _op(3, "middle", p, _nitsche(p), "four")
    gen = torch.Generator(device="cuda").manual_seed(3)
    u = torch.rand(op.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    ref = _apply(op, u)
    torch.cuda.synchronize()
    assert float(ref.abs().max()) > 0.0
    assert torch.equal(_apply(op, u), ref)
    y = op.new_vector(local=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op.use_torch_stream()
        op.apply(u, y)
    torch.cuda.synchronize()
    assert torch.equal(y, ref)
    with torch.cuda.stream(s):
        op.use_torch_stream()
        op.apply(u, y)  # warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            op.apply(u, y)
    torch.cuda.synchronize()
    for _ in range(2):
        y.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, ref)
    op.use_torch_stream()


@pytest.mark.parametrize("dim,kind,p", [(1, "small", 3), (2, "middle", 3), (3, "small", 5), (3, "middle", 3)])
def test_dirichlet_data_uses_kappa_g(dim, kind, p):
    m = _mesh(dim, kind, p)
    nit = _nitsche(p)
    rng = np.random.default_rng(p + dim)
    g = rng.uniform(-1, 1, m.n_boundary_points())
    for which in ("one", "four"):
        op = _op(dim, kind, p, nit, which)
        gd = _dev(_bc_dev(op, g))
        keep = gd.clone()
        y = op.new_vector(local=False)
        op.add_dirichlet_data(gd, y)
        r = _rel(_host(y), R.wave_rhs(m, _kappa(which, dim), None, nit, g))
        print("dirichlet data %dD %s p=%d %s: %.2e" % (dim, kind, p, which, r))
        assert r < 1e-12
        assert torch.equal(gd, keep)  # g_bc is not modified
        # without the coefficient the homogeneous data term comes back
        op.set_coefficient([])
        y.zero_()
        op.add_dirichlet_data(gd, y)
        assert _rel(_host(y), m.wave_rhs(np.zeros(m.n_dofs), impl=False, nitsche=nit, gbc=g)) < 1e-12


def test_time_op_and_bc_values():
    import gdm_amd

    op = _op(3, "small", 3, 0.0, "one")
    u, y = op.new_vector(), op.new_vector(local=False)
    assert op.time_op(0, u, y, None, 2) > 0.0
    bc = torch.zeros(max(op.n_bc_points, 1), dtype=torch.float64, device="cuda")[:op.n_bc_points]
    with pytest.raises(gdm_amd.GdmError):
        op.apply(u, y, bc)


def test_errors():
    """the documented statuses, each with a message from gdm_last_error"""
    import gdm_amd
    from gdm_amd import _capi
    from gdm_amd.cut_wave import CutWave, preset

    lib = _capi.load()
    unit = _capi.CoefTerm()

    def set_coef(op, n_terms, terms):
        h = op.h if hasattr(op, "h") else op
        rc = lib.gdm_op_set_coefficient(h, n_terms, terms)
        return rc, _capi.last_error()

    # another operator kind
    opa = gdm_amd.GdmOperator(2, 3, (6, 5), 0.0, 1.0, "advection", params=(1.0, 0.5))
    rc, msg = set_coef(opa, 1, ctypes.byref(unit))
    assert rc == ERR_UNSUPPORTED and "wave" in msg
    # n_ranks = 2
    op2 = gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "wave", rank=0, n_ranks=2)
    rc, msg = set_coef(op2, 1, ctypes.byref(unit))
    assert rc == ERR_UNSUPPORTED and "rank" in msg
    # a periodic mesh
    per = gdm_amd.GdmOperator(3, 3, (3, 5, 6), 0.0, 1.0, "wave", periodic=1)
    rc, msg = set_coef(per, 1, ctypes.byref(unit))
    assert rc == ERR_UNSUPPORTED and "periodic" in msg
    # the inner operator of a cut handle
    P = preset("wave", dim=2)
    cw = CutWave(P["p"], P["n"], P["left"], P["right"], P["level_set"], ghost_parameter_M=P["gamma_M"],
                 ghost_parameter_A=P["gamma_A"], nitsche=P["nitsche"], dim=2)
    rc, msg = set_coef(cw._op, 1, ctypes.byref(unit))
    assert rc == ERR_UNSUPPORTED and "cut" in msg

    op = gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "wave", params=(20.0,))
    # n_terms outside [0, 4]
    five = (_capi.CoefTerm * 5)()
    rc, msg = set_coef(op, 5, five)
    assert rc == ERR_ARG and "n_terms" in msg
    rc, msg = set_coef(op, -1, five)
    assert rc == ERR_ARG and "n_terms" in msg
    rc, msg = set_coef(op, 1, None)
    assert rc == ERR_ARG
    with pytest.raises(gdm_amd.GdmError):
        op.set_coefficient([[None] * 3] * 5)
    # a non-finite sample
    bad = np.ones_like(op.field_points(1))
    bad[3] = np.inf
    with pytest.raises(gdm_amd.GdmError, match="finite"):
        op.set_coefficient([[None, bad, None]])
    bad[3] = np.nan
    with pytest.raises(gdm_amd.GdmError, match="finite"):
        op.set_coefficient([[None, None, None], [None, bad, None]])
    # one term: a factor that vanishes or changes sign
    x = op.field_points(0)
    with pytest.raises(gdm_amd.GdmError, match="sign"):
        op.set_coefficient([[x - 0.5, None, None]])
    zero = np.ones_like(x)
    zero[-1] = 0.0
    with pytest.raises(gdm_amd.GdmError, match="vanishes"):
        op.set_coefficient([[zero, None, None]])
    op.set_coefficient([[-np.ones_like(x), -np.ones_like(op.field_points(1)), None]])  # two negative factors: kappa = 1
    # in a sum a factor may change sign
    op.set_coefficient([[None, None, None], [0.5 * (x - 0.5), None, None]])

    # apply_planes with a coefficient
    u, y = op.new_vector(), op.new_vector(local=False)
    rc = lib.gdm_apply_planes(op.h, ctypes.c_void_p(u.data_ptr()), ctypes.c_void_p(y.data_ptr()), 0, 4)
    assert rc == ERR_UNSUPPORTED and "coefficient" in _capi.last_error()
    rc = lib.gdm_apply_planes2(op.h, ctypes.c_void_p(u.data_ptr()), ctypes.c_void_p(y.data_ptr()), 0, 2, 4, 6)
    assert rc == ERR_UNSUPPORTED and "coefficient" in _capi.last_error()
    # the solvers' states
    rhs, sol = op.new_vector(local=False), op.new_vector(local=False)
    with pytest.raises(gdm_amd.GdmError, match="gdm_system_solve_setup"):
        op.coef_solve(1.0, 0.1, rhs, sol)
    op.system_solve_setup()  # stays legal with a coefficient
    with pytest.raises(gdm_amd.GdmError, match="gdm_coef_solve"):
        op.system_solve(1.0, 0.1, rhs, sol)
    rc = lib.gdm_system_solve(op.h, 1.0, 0.1, ctypes.c_void_p(rhs.data_ptr()), ctypes.c_void_p(sol.data_ptr()))
    assert rc == ERR_STATE
    # without the coefficient the planes and the direct solve work again, coef_solve does not
    op.set_coefficient([])
    op.apply_planes(u, y, 0, 4)
    op.system_solve(1.0, 0.1, rhs, sol)
    with pytest.raises(gdm_amd.GdmError, match="no coefficient"):
        op.coef_solve(1.0, 0.1, rhs, sol)
