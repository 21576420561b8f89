"""The mass matrix weighted by a general density on the Gauss grid
(gdm_op_set_density_grid, csrc/gdm_massgrid.hip) against the numpy restatement
of the reference's cell loop for a pointwise rho (tests/varmass_ref.py, pinned
to the oracle in tests/test_varmass_cpu.py).

Tolerance: rel-L2 1e-12 against the restatement, the project's bound for fp64
summation-order differences (tests/test_gpu_varmass.py).

Meshes on the box (-0.5, 0, 0.2) - (0.7, 0.9, 1.5), derived from the kernel's
node tile (T_x, T_y) and z chunk of the degree (gdm_density_grid_tile; kernel
axes: 3D (x, y, z), 2D (x, y), 1D z):
  small   every extent p cells: every row is a wall row;
  middle  one tile / chunk plus one node per extent;
  large   two tiles plus a remainder in x and y, two z chunks plus a remainder.
p in {3, 5} on all three, p in {1, 7, 9} on the small mesh.

Density: rho = 2 + sin(3xy + 2z) + 0.5 cos(5(x - yz)) (massgrid_ref.osc), not a
finite separable sum, in [0.5, 3.5].
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle as O
import varmass_ref as R
from massgrid_ref import mass_diag, osc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LO3, HI3 = (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -3, -5


def _nsub(kind, p, dim=3):
    """cells per direction (kernel axes -> reference directions); nodes = cells + 1"""
    from gdm_amd import _capi

    tx, ty, zc = _capi.density_grid_tile(p, dim)
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


def _rho2(dim):
    """a second density for the in-place overwrite"""
    return lambda x: 1.5 + 0.8 * np.cos(2 * x[:, 0] + x[:, :dim].sum(axis=1) ** 2)


@functools.lru_cache(maxsize=None)
def _mesh(dim, kind, p):
    return O.Mesh(dim, p, list(_nsub(kind, p, dim)), list(LO3[:dim]), list(HI3[:dim]))


def _op(dim, kind, p, nitsche=0.0):
    import gdm_amd

    return gdm_amd.GdmOperator(dim, p, _nsub(kind, p, dim), LO3[:dim], HI3[:dim], "wave",
                               params=(nitsche,) if nitsche else ())


def _samples(op, rho):
    return _dev(rho(op.gauss_grid_points()))


@functools.lru_cache(maxsize=None)
def _u(dim, kind, p):
    m = _mesh(dim, kind, p)
    u = np.random.default_rng(100 * dim + p).uniform(-1, 1, m.n_dofs)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def _ref(dim, kind, p):
    """the restatement's M[rho] u, computed once per mesh"""
    r = R.mass_apply(_mesh(dim, kind, p), osc(dim), _u(dim, kind, p))
    r.setflags(write=False)
    return r


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_apply(dim, kind, p):
    op = _op(dim, kind, p)
    op.set_density_grid(_samples(op, osc(dim)))
    assert op.has_density
    r = _rel(_host(op.density_apply(_dev(_u(dim, kind, p)))), _ref(dim, kind, p))
    print("grid density apply %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= 1e-12


@pytest.mark.parametrize("dim,kind,p", [(3, "middle", 3), (3, "small", 5), (2, "large", 5), (1, "large", 3),
                                        (3, "small", 9), (2, "small", 7), (1, "small", 1)])
def test_apply_add(dim, kind, p):
    """dst = M[rho] u + c * add in the same launch"""
    op = _op(dim, kind, p)
    op.set_density_grid(_samples(op, osc(dim)))
    add = np.random.default_rng(p).uniform(-1, 1, op.n_local)
    c = -0.37
    want = _ref(dim, kind, p) + c * add
    r = _rel(_host(op.density_apply(_dev(_u(dim, kind, p)), c=c, add=_dev(add))), want)
    print("grid density apply_add %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= 1e-12


def test_callable_equals_sampled_tensor():
    p, dim = 3, 3
    op = _op(dim, "small", p)
    u = _dev(_u(dim, "small", p))
    op.set_density_grid(osc(dim))
    assert op.has_density
    y = op.density_apply(u)
    assert _rel(_host(y), _ref(dim, "small", p)) <= 1e-12
    op.set_density_grid(_samples(op, osc(dim)))
    assert torch.equal(op.density_apply(u), y)


def _four_terms(dim):
    """positive on the box: 2.5 + 0.5 sin 3x + 0.4 cos 2y z + 0.3 x y z >= 1.2"""
    t = [[lambda x: 2.5 + 0.0 * x, None, None],
         [lambda x: 0.5 * np.sin(3 * x), None, None],
         [None, lambda y: 0.4 * np.cos(2 * y), lambda z: z],
         [lambda x: 0.3 * x, lambda y: y, lambda z: z]]
    return [f[:dim] for f in t]


@pytest.mark.parametrize("dim,kind,p", [(3, "middle", 3), (3, "small", 5), (2, "middle", 5), (1, "middle", 3)])
def test_separable_rho_agrees_with_the_separable_path(dim, kind, p):
    op = _op(dim, kind, p)
    u = _dev(_u(dim, kind, p))
    op.set_density(_four_terms(dim))
    want = _host(op.density_apply(u))
    op.set_density_grid(_samples(op, R.pointwise(_four_terms(dim), dim)))
    r = _rel(_host(op.density_apply(u)), want)
    print("separable on the grid %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= 1e-12


@pytest.mark.parametrize("kind,p", [("small", p) for p in (1, 3, 5, 7, 9)] + [("middle", 3), ("middle", 5)])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_unit_density_equals_mass_apply(dim, kind, p):
    op = _op(dim, kind, p)
    u = _dev(_u(dim, kind, p))
    want = op.new_vector(local=False)
    op.mass_apply(u, want)
    op.set_density_grid(lambda x: np.ones(x.shape[0]))
    r = _rel(_host(op.density_apply(u)), _host(want))
    print("unit grid density %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= 1e-12


@pytest.mark.parametrize("dim,kind,p", [(3, "middle", 3), (3, "small", 5), (2, "large", 5), (1, "large", 3)])
def test_symmetry_and_positivity(dim, kind, p):
    """|v . M u - u . M v| <= 1e-12 |u| |M v|, u . M u > 0"""
    op = _op(dim, kind, p)
    op.set_density_grid(osc(dim))
    gen = torch.Generator(device="cuda").manual_seed(7)
    u = torch.rand(op.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    v = torch.rand(op.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    Mu, Mv = op.density_apply(u), op.density_apply(v)
    a, b = float(torch.dot(v, Mu)), float(torch.dot(u, Mv))
    scale = float(torch.linalg.norm(u) * torch.linalg.norm(Mv))
    print("symmetry %dD %s p=%d: %.16e %.16e" % (dim, kind, p, a, b))
    assert abs(a - b) <= 1e-12 * scale
    assert float(torch.dot(u, Mu)) > 0.0 and float(torch.dot(v, Mv)) > 0.0


# the dense matrix costs one restatement apply per DoF: 3D p = 7 and 9 (512 and 1000 DoFs) take the direct
# diagonal of massgrid_ref.mass_diag instead, which tests/test_massgrid_cpu.py pins to the dense diagonal
@pytest.mark.parametrize("p", [1, 3, 5, 7, 9])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_density_diag_against_the_dense_matrix(dim, p):
    m = _mesh(dim, "small", p)
    op = _op(dim, "small", p)
    op.set_density_grid(osc(dim))
    direct = mass_diag(m, osc(dim))
    want = direct if dim == 3 and p >= 7 else np.diag(R.dense_matrix(m, osc(dim)))
    assert _rel(direct, want) <= 1e-13
    r = _rel(_host(op.density_diag()), want)
    print("grid density diag %dD small p=%d: %.2e" % (dim, p, r))
    assert r <= 1e-12


@pytest.mark.parametrize("dim,kind,p", [(3, "middle", 3), (3, "large", 5), (2, "large", 5), (1, "large", 3)])
def test_density_diag_on_more_than_one_tile(dim, kind, p):
    """the diagonal mode across tiles and z chunks, against massgrid_ref.mass_diag"""
    op = _op(dim, kind, p)
    op.set_density_grid(osc(dim))
    r = _rel(_host(op.density_diag()), mass_diag(_mesh(dim, kind, p), osc(dim)))
    print("grid density diag %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= 1e-12


@pytest.mark.parametrize("dim,kind,p", [(3, "middle", 3), (3, "small", 5), (2, "large", 5), (1, "large", 3),
                                        (3, "small", 7), (3, "small", 9)])
def test_density_diag_of_a_separable_density(dim, kind, p):
    """grid and separable form against diag_ratio * diag(M) of the restatement"""
    m = _mesh(dim, kind, p)
    terms = _four_terms(dim)
    one = np.ones(1)
    for d in range(dim):
        one = np.kron(np.diag(R.mass_1d(m, d, None)), one)
    want = R.diag_ratio(m, terms) * one
    op = _op(dim, kind, p)
    op.set_density(terms)
    r_sep = _rel(_host(op.density_diag()), want)
    op.set_density_grid(_samples(op, R.pointwise(terms, dim)))
    dst = op.new_vector(local=False)
    assert op.density_diag(dst) is dst
    r_grid = _rel(_host(dst), want)
    print("separable density diag %dD %s p=%d: separable %.2e, grid %.2e" % (dim, kind, p, r_sep, r_grid))
    assert r_sep <= 1e-12 and r_grid <= 1e-12


@pytest.mark.parametrize("p", [3, 5])
def test_bitwise_repeatable_runs_streams_and_graph_replay(p):
    """a second run, an apply on a second stream and the replay of a captured
    FIRST apply (no warm-up of the operator before the capture) give the same bits"""
    u = _dev(_u(3, "middle", p))
    # the captured operator has never applied before: nothing may allocate in the apply
    cap = _op(3, "middle", p)
    cap.set_density_grid(_samples(cap, osc(3)))
    yc = cap.new_vector(local=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        cap.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            cap.density_apply(u, yc)
    torch.cuda.synchronize()
    cap.use_torch_stream()

    op = _op(3, "middle", p)
    op.set_density_grid(_samples(op, osc(3)))
    ref = op.density_apply(u)
    torch.cuda.synchronize()
    assert float(ref.abs().max()) > 0.0
    assert torch.equal(op.density_apply(u), ref)
    y = op.new_vector(local=False)
    with torch.cuda.stream(s):
        op.use_torch_stream()
        op.density_apply(u, y)
    torch.cuda.synchronize()
    op.use_torch_stream()
    assert torch.equal(y, ref)
    for _ in range(2):
        yc.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(yc, ref)


@pytest.mark.parametrize("dim,kind,p", [(3, "large", 3), (3, "large", 5), (3, "middle", 5), (1, "large", 3),
                                        (3, "small", 7), (3, "small", 9)])
def test_bits_do_not_depend_on_the_z_chunk(dim, kind, p):
    """the automatic choice shrinks the chunk on meshes this small; the whole chunk
    of gdm_density_grid_tile (what a large mesh runs with), the half and single
    planes give the same bits, for the apply, apply_add and the diagonal"""
    import gdm_amd
    from gdm_amd import _capi

    op = _op(dim, kind, p)
    with pytest.raises(gdm_amd.GdmError):  # no grid density yet
        op.set_density_grid_z_chunk(1)
    op.set_density_grid(osc(dim))
    u = _dev(_u(dim, kind, p))
    add = torch.linspace(-1.0, 1.0, op.n_owned, dtype=torch.float64, device="cuda")
    ref = (op.density_apply(u), op.density_apply(u, c=0.3, add=add), op.density_diag())
    assert _rel(_host(ref[0]), _ref(dim, kind, p)) <= 1e-12
    zc = op.density_grid_tile()[2]
    for z in (zc, zc // 2, 1, -1):
        op.set_density_grid_z_chunk(z)
        got = (op.density_apply(u), op.density_apply(u, c=0.3, add=add), op.density_diag())
        assert all(torch.equal(g, r) for g, r in zip(got, ref)), z
    for z in (0, -2, zc + 1):
        rc = _capi.load().gdm_op_set_density_grid_z_chunk(op.h, z)
        assert rc == ERR_ARG and "z_chunk" in _capi.last_error()


@pytest.mark.parametrize("dim,kind,p", [(3, "middle", 3), (2, "middle", 5), (1, "small", 3)])
def test_borrowed_array_removal_and_replacement(dim, kind, p):
    import gdm_amd

    m = _mesh(dim, kind, p)
    op = _op(dim, kind, p, 6.0 * p * p)
    u = _dev(_u(dim, kind, p))
    # gdm_apply and gdm_mass_apply before any density
    k_plain, m_plain = op.new_vector(local=False), op.new_vector(local=False)
    op.apply(u, k_plain)
    op.mass_apply(u, m_plain)
    rq = _samples(op, osc(dim))
    op.set_density_grid(rq)
    assert _rel(_host(op.density_apply(u)), _ref(dim, kind, p)) <= 1e-12
    # overwrite in place, no set call: the next apply sees the second rho
    rq.copy_(_samples(op, _rho2(dim)))
    r = _rel(_host(op.density_apply(u)), R.mass_apply(m, _rho2(dim), _u(dim, kind, p)))
    print("borrowed array %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= 1e-12
    # the stiffness and the unweighted mass keep their bits while a grid density is set
    k2, m2 = op.new_vector(local=False), op.new_vector(local=False)
    op.apply(u, k2)
    op.mass_apply(u, m2)
    assert torch.equal(k2, k_plain) and torch.equal(m2, m_plain)
    # None removes the density
    op.set_density_grid(None)
    assert not op.has_density
    with pytest.raises(gdm_amd.GdmError):
        op.density_apply(u)
    # separable -> grid -> separable reproduces the separable bits
    op.set_density(_four_terms(dim))
    sep = op.density_apply(u)
    x_sep = op.new_vector(local=False)
    its_sep, _ = op.density_solve(sep, x_sep, rel_tol=1e-10)
    op.set_density_grid(rq)
    assert op.has_density and not torch.equal(op.density_apply(u), sep)
    op.set_density(_four_terms(dim))
    assert torch.equal(op.density_apply(u), sep)
    x2 = op.new_vector(local=False)
    its2, _ = op.density_solve(sep, x2, rel_tol=1e-10)
    assert its2 == its_sep and torch.equal(x2, x_sep)


def test_errors():
    """the documented statuses, each with a message from gdm_last_error"""
    import gdm_amd
    from gdm_amd import _capi

    lib = _capi.load()
    one = torch.ones(8, dtype=torch.float64, device="cuda")

    def set_grid(op, rq):
        rc = lib.gdm_op_set_density_grid(getattr(op, "h", op),  # a CutWave keeps the raw handle of its inner operator
                                         ctypes.c_void_p(rq.data_ptr()) if rq is not None else None)
        return rc, _capi.last_error()

    # another operator kind, n_ranks = 2, a periodic mesh
    opa = gdm_amd.GdmOperator(2, 3, (6, 5), 0.0, 1.0, "advection", params=(1.0, 0.5))
    rc, msg = set_grid(opa, one)
    assert rc == ERR_UNSUPPORTED and "wave" in msg
    op2 = gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "wave", rank=0, n_ranks=2)
    rc, msg = set_grid(op2, one)
    assert rc == ERR_UNSUPPORTED and "rank" in msg
    per = gdm_amd.GdmOperator(3, 3, (3, 5, 6), 0.0, 1.0, "wave", periodic=1)
    rc, msg = set_grid(per, one)
    assert rc == ERR_UNSUPPORTED and "periodic" in msg

    # the inner operator of a cut handle
    from gdm_amd.cut_wave import CutWave, preset

    P = preset("wave", dim=2)
    cw = CutWave(P["p"], P["n"], P["left"], P["right"], P["level_set"], ghost_parameter_M=P["gamma_M"],
                 ghost_parameter_A=P["gamma_A"], nitsche=P["nitsche"], dim=2)
    rc, msg = set_grid(cw._op, one)
    assert rc == ERR_UNSUPPORTED and "cut" in msg

    op = gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "wave", params=(20.0,))
    nq = 6 * 5 * 8 * 64
    u, y = op.new_vector() + 1.0, op.new_vector(local=False)
    # no density: apply, solve and diag are state errors
    rc = lib.gdm_density_diag(op.h, ctypes.c_void_p(y.data_ptr()))
    assert rc == ERR_STATE and "density" in _capi.last_error()
    rc = lib.gdm_density_apply(op.h, ctypes.c_void_p(u.data_ptr()), ctypes.c_void_p(y.data_ptr()))
    assert rc == ERR_STATE
    # a wrong size is refused by the Python layer
    with pytest.raises(gdm_amd.GdmError):
        op.set_density_grid(one)
    # a previous state, separable or on the grid, survives every refused sample
    rq = torch.full((nq,), 1.5, dtype=torch.float64, device="cuda")
    prev = torch.linspace(1.0, 2.0, nq, dtype=torch.float64, device="cuda")
    for state in ("separable", "grid"):
        if state == "separable":
            op.set_density([[lambda x: 1 + x, None, lambda z: 2 - z], [None, np.exp, None]])
        else:
            op.set_density_grid(prev)
        before = op.density_apply(u)
        for idx, bad in ((777, float("nan")), (nq - 1, 0.0), (0, -1.0), (5, float("inf")), (9, float("-inf"))):
            rq[idx] = bad
            rc, msg = set_grid(op, rq)
            assert rc == ERR_ARG and "positive" in msg
            rq[idx] = 1.5
            assert torch.equal(op.density_apply(u), before)
    # a refresh (the same pointer) with a bad sample is refused too and leaves the mean and W alone
    keep = float(prev[3])
    prev[3] = float("nan")
    rc, msg = set_grid(op, prev)
    assert rc == ERR_ARG and "positive" in msg
    prev[3] = keep
    assert torch.equal(op.density_apply(u), before)
    rc, msg = set_grid(op, prev)
    assert rc == 0
    # rhs == x in the solve, NULL vectors
    rc = lib.gdm_density_solve(op.h, ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(y.data_ptr()), 1e-8, 0.0, 10,
                               None, None)
    assert rc == ERR_ARG and "rhs != x" in _capi.last_error()
    rc = lib.gdm_density_diag(op.h, None)
    assert rc == ERR_ARG
    # time_op(which = 3) times the grid kernel
    assert op.time_op(3, u, y, None, 2) > 0.0
