"""The wave / heat / Poisson operator with a general coefficient on the Gauss
grid (gdm_op_set_coefficient_grid, csrc/gdm_coefgrid.hip) against the numpy
restatement of the reference's cell loop for a pointwise kappa
(tests/vardiff_ref.py, pinned to the oracle in tests/test_vardiff_cpu.py).

Tolerance: rel-L2 1e-12 against the restatement, the project's bound for fp64
summation-order differences (tests/test_gpu_vardiff.py).

Meshes on the box (-0.5, 0, 0.2) - (0.7, 0.9, 1.5), derived from the kernel's
node tile (T_x, T_y) and z chunk of the degree (gdm_coef_grid_tile; kernel axes:
3D (x, y, z), 2D (x, y), 1D z):
  small   every extent p cells: every row is a wall row;
  middle  one tile / chunk plus one node per extent;
  large   two tiles plus a remainder in x and y, two z chunks plus a remainder.
p in {3, 5} on all three, p in {1, 7, 9} on the small mesh.

Coefficient: kappa = 2 + sin(3xy + 2z) + 0.5 cos(5(x - yz)), not a finite
separable sum, in [0.5, 3.5]; in 2D z is dropped, in 1D 2 + sin 3x + 0.5 cos 5x.
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


def _nsub(kind, p, dim=3):
    """cells per direction (kernel axes -> reference directions); nodes = cells + 1"""
    from gdm_amd import _capi

    tx, ty, zc = _capi.coef_grid_tile(p, dim)
    ext = {"small": (p, p, p), "middle": (tx, ty, zc), "large": (2 * tx + 4, 2 * ty + 2, 2 * zc + 2)}[kind]
    ext = tuple(max(e, p) for e in ext)  # the operator needs n_sub >= p
    if dim == 3:
        return ext
    return ext[:2] if dim == 2 else (ext[2],)


MESHES = [("small", p) for p in (1, 3, 5, 7, 9)] + [(k, p) for k in ("middle", "large") for p in (3, 5)]
MESH_IDS = ["%s-p%d" % kp for kp in MESHES]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float64)).cuda()  # a copy: the cached inputs are read-only


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


def _kappa(dim):
    if dim == 3:
        return lambda x: 2 + np.sin(3 * x[:, 0] * x[:, 1] + 2 * x[:, 2]) + 0.5 * np.cos(5 * (x[:, 0] - x[:, 1] * x[:, 2]))
    if dim == 2:
        return lambda x: 2 + np.sin(3 * x[:, 0] * x[:, 1]) + 0.5 * np.cos(5 * x[:, 0])
    return lambda x: 2 + np.sin(3 * x[:, 0]) + 0.5 * np.cos(5 * x[:, 0])


def _kappa2(dim):
    """a second coefficient for the in-place overwrite"""
    return lambda x: 1.5 + 0.8 * np.cos(2 * x[:, 0] + x[:, :dim].sum(axis=1) ** 2)


def _nitsche(p):
    return 6.0 * p * p


@functools.lru_cache(maxsize=None)
def _mesh(dim, kind, p):
    return O.Mesh(dim, p, list(_nsub(kind, p, dim)), list(LO3[:dim]), list(HI3[:dim]))


def _op(dim, kind, p, nitsche):
    import gdm_amd

    return gdm_amd.GdmOperator(dim, p, _nsub(kind, p, dim), LO3[:dim], HI3[:dim], "wave",
                               params=(nitsche,) if nitsche else ())


def _grid_points(op):
    """the Gauss grid as (n, 3), x fastest (add_load's layout)"""
    xq = op.quadrature_points() + [np.zeros(1)] * (3 - op.dim)
    x = np.zeros((xq[2].size, xq[1].size, xq[0].size, 3))
    x[..., 0] = xq[0][None, None, :]
    x[..., 1] = xq[1][None, :, None]
    x[..., 2] = xq[2][:, None, None]
    return x.reshape(-1, 3)


def _samples(op, m, kappa):
    """(kq, kbc) device tensors; kbc through the reference's boundary points and
    bc_reference_order (None without boundary points)"""
    kq = _dev(kappa(_grid_points(op)))
    kbc = _dev(_bc_dev(op, kappa(m.boundary_points()))) if op.n_bc_points else None
    return kq, kbc


@functools.lru_cache(maxsize=None)
def _u(dim, kind, p):
    m = _mesh(dim, kind, p)
    u = np.random.default_rng(100 * dim + p).uniform(-1, 1, m.n_dofs)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def _ref(dim, kind, p, nitsche):
    """the restatement's K[kappa] u, computed once per mesh"""
    r = R.wave_rhs(_mesh(dim, kind, p), _kappa(dim), _u(dim, kind, p), nitsche)
    r.setflags(write=False)
    return r


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
def test_apply_3d(kind, p):
    """K[kappa] u with and without the box-face terms (the large mesh: with them only)"""
    m = _mesh(3, kind, p)
    for nit in ((_nitsche(p),) if kind == "large" else (0.0, _nitsche(p))):
        op = _op(3, kind, p, nit)
        op.set_coefficient_grid(*_samples(op, m, _kappa(3)))
        r = _rel(_host(_apply(op, _dev(_u(3, kind, p)))), _ref(3, kind, p, nit))
        print("grid apply 3D %s p=%d nitsche=%g: %.2e" % (kind, p, nit, r))
        assert r <= 1e-12


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
@pytest.mark.parametrize("dim", [1, 2])
def test_apply_1d_2d(dim, kind, p):
    m = _mesh(dim, kind, p)
    for nit in (0.0, _nitsche(p)):
        op = _op(dim, kind, p, nit)
        op.set_coefficient_grid(*_samples(op, m, _kappa(dim)))
        r = _rel(_host(_apply(op, _dev(_u(dim, kind, p)))), _ref(dim, kind, p, nit))
        print("grid apply %dD %s p=%d nitsche=%g: %.2e" % (dim, kind, p, nit, r))
        assert r <= 1e-12


def test_callable_equals_sampled_tensors():
    p, dim = 3, 3
    m = _mesh(dim, "small", p)
    op = _op(dim, "small", p, _nitsche(p))
    op.set_coefficient_grid(_kappa(dim))
    assert op.has_coefficient
    r = _rel(_host(_apply(op, _dev(_u(dim, "small", p)))), _ref(dim, "small", p, _nitsche(p)))
    assert r <= 1e-12
    op.set_coefficient_grid(None)
    assert not op.has_coefficient


def _four_terms(dim):
    t = [[lambda x: 2.0, None, None],
         [lambda x: 0.5 * np.sin(3 * x), None, None],
         [None, lambda y: 0.4 * np.cos(2 * y), lambda z: z],
         [lambda x: 0.3 * x, lambda y: y, lambda z: z]]
    return [f[:dim] for f in t]


def _four_kappa(dim):
    terms = _four_terms(dim)

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


@pytest.mark.parametrize("dim,kind,p", [(3, "middle", 3), (3, "small", 5), (2, "middle", 5), (1, "middle", 3)])
def test_separable_kappa_agrees_with_the_separable_path(dim, kind, p):
    """the "four" coefficient of test_gpu_vardiff.py sampled on the grid"""
    m = _mesh(dim, kind, p)
    for nit in (0.0, _nitsche(p)):
        op = _op(dim, kind, p, nit)
        u = _dev(_u(dim, kind, p))
        op.set_coefficient(_four_terms(dim))
        want = _host(_apply(op, u))
        op.set_coefficient_grid(*_samples(op, m, _four_kappa(dim)))
        r = _rel(_host(_apply(op, u)), want)
        print("separable on the grid %dD %s p=%d nitsche=%g: %.2e" % (dim, kind, p, nit, r))
        assert r <= 1e-12


@pytest.mark.parametrize("kind,p", [("small", p) for p in (1, 3, 5, 7, 9)] + [("middle", 3), ("middle", 5)])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_unit_coefficient_equals_the_constant_stencil(dim, kind, p):
    for nit in (0.0, _nitsche(p)):
        op = _op(dim, kind, p, nit)
        u = _dev(_u(dim, kind, p))
        want = _apply(op, u)
        op.set_coefficient_grid(lambda x: np.ones(x.shape[0]))
        r = _rel(_host(_apply(op, u)), _host(want))
        print("unit grid coefficient %dD %s p=%d nitsche=%g: %.2e" % (dim, kind, p, nit, r))
        assert r <= 1e-12
        op.set_coefficient_grid(None)
        assert torch.equal(_apply(op, u), want)


@pytest.mark.parametrize("dim,kind,p", [(3, "middle", 3), (3, "small", 5), (2, "large", 5), (1, "large", 3)])
def test_symmetry(dim, kind, p):
    """|v . K u - u . K v| <= 1e-12 |u| |K v|"""
    op = _op(dim, kind, p, _nitsche(p))
    op.set_coefficient_grid(_kappa(dim))
    gen = torch.Generator(device="cuda").manual_seed(7)
    u = torch.rand(op.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    v = torch.rand(op.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    Ku, Kv = _apply(op, u), _apply(op, v)
    a, b = float(torch.dot(v, Ku)), float(torch.dot(u, Kv))
    scale = float(torch.linalg.norm(u) * torch.linalg.norm(Kv))
    print("symmetry %dD %s p=%d: %.16e %.16e" % (dim, kind, p, a, b))
    assert abs(a - b) <= 1e-12 * scale


@pytest.mark.parametrize("p", [3, 5])
def test_bitwise_repeatable_runs_streams_and_graph_replay(p):
    """a second run, an apply on a second stream and the replay of a captured
    FIRST apply (no warm-up of the operator before the capture) give the same bits"""
    m = _mesh(3, "middle", p)
    u = _dev(_u(3, "middle", p))
    # the captured operator has never applied before: nothing may allocate in the apply
    cap = _op(3, "middle", p, _nitsche(p))
    cap.set_coefficient_grid(*_samples(cap, m, _kappa(3)))
    yc = cap.new_vector(local=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        cap.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            cap.apply(u, yc)
    torch.cuda.synchronize()
    cap.use_torch_stream()

    op = _op(3, "middle", p, _nitsche(p))
    op.set_coefficient_grid(*_samples(op, m, _kappa(3)))
    ref = _apply(op, u)
    torch.cuda.synchronize()
    assert float(ref.abs().max()) > 0.0
    assert torch.equal(_apply(op, u), ref)
    y = op.new_vector(local=False)
    with torch.cuda.stream(s):
        op.use_torch_stream()
        op.apply(u, y)
    torch.cuda.synchronize()
    op.use_torch_stream()
    assert torch.equal(y, ref)
    for _ in range(2):
        yc.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(yc, ref)


@pytest.mark.parametrize("dim,kind,p", [(3, "middle", 3), (2, "middle", 5), (1, "small", 3)])
def test_borrowed_arrays(dim, kind, p):
    m = _mesh(dim, kind, p)
    nit = _nitsche(p)
    op = _op(dim, kind, p, nit)
    u = _dev(_u(dim, kind, p))
    plain = _apply(op, u)
    kq, kbc = _samples(op, m, _kappa(dim))
    op.set_coefficient_grid(kq, kbc)
    assert _rel(_host(_apply(op, u)), _ref(dim, kind, p, nit)) <= 1e-12
    # overwrite in place, no set call: the next apply sees the second kappa
    kq2, kbc2 = _samples(op, m, _kappa2(dim))
    kq.copy_(kq2)
    kbc.copy_(kbc2)
    r = _rel(_host(_apply(op, u)), R.wave_rhs(m, _kappa2(dim), _u(dim, kind, p), nit))
    print("borrowed arrays %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= 1e-12
    # removing the coefficient: the constant operator's bits from before
    op.set_coefficient_grid(None)
    assert torch.equal(_apply(op, u), plain)
    # separable -> grid -> separable reproduces the separable bits
    op.set_coefficient(_four_terms(dim))
    sep = _apply(op, u)
    op.set_coefficient_grid(kq, kbc)
    assert not torch.equal(_apply(op, u), sep)
    op.set_coefficient(_four_terms(dim))
    assert torch.equal(_apply(op, u), sep)


@pytest.mark.parametrize("dim,kind,p", [(1, "small", 3), (2, "middle", 3), (3, "small", 5), (3, "middle", 3)])
def test_dirichlet_data_uses_kbc_g(dim, kind, p):
    m = _mesh(dim, kind, p)
    nit = _nitsche(p)
    g = np.random.default_rng(p + dim).uniform(-1, 1, m.n_boundary_points())
    op = _op(dim, kind, p, nit)
    op.set_coefficient_grid(*_samples(op, m, _kappa(dim)))
    gd = _dev(_bc_dev(op, g))
    keep = gd.clone()
    y = op.new_vector(local=False)
    op.add_dirichlet_data(gd, y)
    r = _rel(_host(y), R.wave_rhs(m, _kappa(dim), None, nit, g))
    print("grid dirichlet data %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= 1e-12
    assert torch.equal(gd, keep)  # g_bc is not modified


def test_errors():
    """the documented statuses, each with a message from gdm_last_error"""
    import gdm_amd
    from gdm_amd import _capi

    lib = _capi.load()
    one = torch.ones(8, dtype=torch.float64, device="cuda")

    def set_grid(op, kq, kbc):
        rc = lib.gdm_op_set_coefficient_grid(op.h, ctypes.c_void_p(kq.data_ptr()) if kq is not None else None,
                                             ctypes.c_void_p(kbc.data_ptr()) if kbc is not None else None)
        return rc, _capi.last_error()

    # another operator kind, n_ranks = 2, a periodic mesh
    opa = gdm_amd.GdmOperator(2, 3, (6, 5), 0.0, 1.0, "advection", params=(1.0, 0.5))
    rc, msg = set_grid(opa, one, one)
    assert rc == ERR_UNSUPPORTED and "wave" in msg
    op2 = gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "wave", rank=0, n_ranks=2)
    rc, msg = set_grid(op2, one, one)
    assert rc == ERR_UNSUPPORTED and "rank" in msg
    per = gdm_amd.GdmOperator(3, 3, (3, 5, 6), 0.0, 1.0, "wave", periodic=1)
    rc, msg = set_grid(per, one, one)
    assert rc == ERR_UNSUPPORTED and "periodic" in msg

    op = gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "wave", params=(20.0,))
    nq = 6 * 5 * 8 * 64
    kq = torch.full((nq,), 1.5, dtype=torch.float64, device="cuda")
    kbc = torch.full((op.n_bc_points,), 1.5, dtype=torch.float64, device="cuda")
    u, y = op.new_vector(), op.new_vector(local=False)
    plain = _apply(op, u + 1.0)
    # kbc = NULL on a Nitsche operator
    rc, msg = set_grid(op, kq, None)
    assert rc == ERR_ARG and "kbc" in msg
    # a NaN or a non-positive sample in kq or kbc; the operator stays as it was
    for arr, idx, bad in ((kq, 777, float("nan")), (kq, nq - 1, 0.0), (kq, 0, -1.0), (kq, 5, float("inf")),
                          (kbc, 3, float("nan")), (kbc, op.n_bc_points - 1, -2.0)):
        arr[idx] = bad
        rc, msg = set_grid(op, kq, kbc)
        assert rc == ERR_ARG and "positive" in msg
        arr[idx] = 1.5
        assert torch.equal(_apply(op, u + 1.0), plain)
    op.set_coefficient_grid(kq, kbc)
    # bc_values != NULL in apply
    bc = torch.zeros(op.n_bc_points, dtype=torch.float64, device="cuda")
    with pytest.raises(gdm_amd.GdmError):
        op.apply(u, y, bc)
    rc = lib.gdm_apply(op.h, ctypes.c_void_p(u.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(bc.data_ptr()))
    assert rc == ERR_ARG
    # apply_planes with a coefficient
    rc = lib.gdm_apply_planes(op.h, ctypes.c_void_p(u.data_ptr()), ctypes.c_void_p(y.data_ptr()), 0, 4)
    assert rc == ERR_UNSUPPORTED and "coefficient" in _capi.last_error()
    rc = lib.gdm_apply_planes2(op.h, ctypes.c_void_p(u.data_ptr()), ctypes.c_void_p(y.data_ptr()), 0, 2, 4, 6)
    assert rc == ERR_UNSUPPORTED and "coefficient" in _capi.last_error()
    # the direct solve
    rhs, sol = op.new_vector(local=False), op.new_vector(local=False)
    op.system_solve_setup()
    rc = lib.gdm_system_solve(op.h, 1.0, 0.1, ctypes.c_void_p(rhs.data_ptr()), ctypes.c_void_p(sol.data_ptr()))
    assert rc == ERR_STATE
    # time_op
    assert op.time_op(0, u, y, None, 2) > 0.0
    # an operator without Nitsche terms ignores kbc
    op0 = gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "wave")
    rc, msg = set_grid(op0, kq, None)
    assert rc == 0
    # without the coefficient the planes and the direct solve work again
    op.set_coefficient_grid(None)
    op.apply_planes(u, y, 0, 4)
    op.system_solve(1.0, 0.1, rhs, sol)
