"""Grid evaluation on the device (gdm_eval_grid, gdm_add_load_grad,
gdm_eval_trace; csrc/gdm_evalgrid.hip) against the numpy restatement
tests/evalgrid_ref.py (pinned to the oracle in tests/test_evalgrid_cpu.py).

Tolerance: rel-L2 1e-12 against the restatement, the project's bound for fp64
summation-order differences (tests/test_gpu_vardiff.py).

Meshes on the box (-0.5, 0, 0.2) - (0.7, 0.9, 1.5), derived from the cells of
one work item of the evaluation kernel (gdm_eval_grid_tile) and from the node
tile and z chunk of the flux load (gdm_load_tile); kernel axes: 3D (x, y, z),
2D (x, y), 1D z:
  small   every extent p cells: every cell is a wall category;
  middle  one work item / tile plus one cell per extent;
  large   two work items / tiles plus a remainder in x and y, two z blocks plus
          a remainder.
3D on all three (p in {3, 5}; p in {1, 7, 9} on the small mesh), 2D and 1D on
small and middle.  u is uniform random.
"""
import ctypes
import functools

import numpy as np
import pytest

import evalgrid_ref as E
import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LO3, HI3 = (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)
ERR_ARG, ERR_UNSUPPORTED = -1, -3
TOL = 1e-12


def _nsub(kind, p, dim=3):
    """cells per direction (kernel axes -> reference directions)"""
    from gdm_amd import _capi

    ex, ey, ez = _capi.eval_grid_tile(p, dim)  # cells
    tx, ty, zc = _capi.load_tile(p, dim)       # nodes: a tile plus one node is `tile` cells
    ext = {"small": (p, p, p),
           "middle": (max(ex + 1, tx), max(ey + 1, ty), max(ez + 1, zc)),
           "large": (max(2 * ex + 3, 2 * tx + 4), max(2 * ey + 1, 2 * ty + 2), max(2 * ez + 1, 2 * zc + 2))}[kind]
    ext = tuple(max(e, p) for e in ext)  # the operator needs n_sub >= p
    if dim == 3:
        return ext
    return ext[:2] if dim == 2 else (ext[2],)


MESHES = [("small", p) for p in (1, 3, 5, 7, 9)] + [(k, p) for k in ("middle", "large") for p in (3, 5)]
MESH_IDS = ["%s-p%d" % kp for kp in MESHES]
LOW = [("small", p) for p in (1, 3, 5, 7, 9)] + [("middle", p) for p in (3, 5)]
LOW_IDS = ["%s-p%d" % kp for kp in LOW]


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(b), 1e-300))


def _dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float64).reshape(-1)).cuda()  # a copy: the cached inputs are read-only


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _mesh(dim, kind, p):
    return O.Mesh(dim, p, list(_nsub(kind, p, dim)), list(LO3[:dim]), list(HI3[:dim]))


def _op(dim, kind, p, nitsche=0.0, what="wave"):
    import gdm_amd

    return gdm_amd.GdmOperator(dim, p, _nsub(kind, p, dim), LO3[:dim], HI3[:dim], what,
                               params=(nitsche,) if nitsche else ())


@functools.lru_cache(maxsize=None)
def _u(dim, kind, p):
    m = _mesh(dim, kind, p)
    u = np.random.default_rng(100 * dim + p).uniform(-1, 1, m.n_dofs)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def _flux(dim, kind, p):
    """(a random F on the grid, the restatement's flux load of it), computed once per mesh"""
    m = _mesh(dim, kind, p)
    F = np.random.default_rng(7 * dim + p).uniform(-1, 1, (dim,) + E.grid_shape(m))
    ref = E.flux_load(m, F)
    F.setflags(write=False)
    ref.setflags(write=False)
    return F, ref


def _check_eval(dim, kind, p):
    m = _mesh(dim, kind, p)
    op = _op(dim, kind, p)
    u = _dev(_u(dim, kind, p))
    nq = op.n_grid_points
    uq, gq = op.eval_grid(u)
    assert uq.numel() == nq and gq.numel() == dim * nq
    r = _rel(_host(uq), E.values(m, _u(dim, kind, p)))
    print("eval values %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= TOL
    g = _host(gq).reshape(dim, nq)
    for e in range(dim):
        r = _rel(g[e], E._eval(m, _u(dim, kind, p), e))
        print("eval d/dx_%d %dD %s p=%d: %.2e" % (e, dim, kind, p, r))
        assert r <= TOL
    # a NULL output: the other one has the combined call's bits
    only_v = op.eval_grid(u, gradients=False)
    only_g = op.eval_grid(u, values=False)
    assert torch.equal(only_v, uq) and torch.equal(only_g, gq)


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
def test_eval_3d(kind, p):
    _check_eval(3, kind, p)


@pytest.mark.parametrize("kind,p", LOW, ids=LOW_IDS)
@pytest.mark.parametrize("dim", [1, 2])
def test_eval_1d_2d(dim, kind, p):
    _check_eval(dim, kind, p)


def _check_flux(dim, kind, p):
    op = _op(dim, kind, p)
    F, ref = _flux(dim, kind, p)
    Fd = _dev(F)
    # add_load before and after the flux load on the same operator: the flux call leaves add_load's tables and
    # bits alone.  (That the bits equal those of earlier builds holds by construction: the flux load is a kernel
    # of its own and gdm_load.hip's load_kernel is unchanged.)
    fq = _dev(F[0])
    load0 = op.add_load(fq, op.new_vector(False))
    y = op.add_load_grad(Fd, op.new_vector(False))
    r = _rel(_host(y), ref)
    print("flux load %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= TOL
    # scale, adding into a non-zero dst
    d0 = np.random.default_rng(p).uniform(-1, 1, op.n_owned) * np.abs(ref).max()
    y = op.add_load_grad(Fd, _dev(d0), scale=-2.5)
    r = _rel(_host(y), d0 - 2.5 * ref)
    print("flux load, scale -2.5 into dst %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= TOL
    # scale 0 launches nothing
    y0 = _dev(d0)
    op.add_load_grad(Fd, y0, scale=0.0)
    assert np.array_equal(_host(y0), d0)
    assert torch.equal(op.add_load(fq, op.new_vector(False)), load0)


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
def test_flux_load_3d(kind, p):
    _check_flux(3, kind, p)


@pytest.mark.parametrize("kind,p", LOW, ids=LOW_IDS)
@pytest.mark.parametrize("dim", [1, 2])
def test_flux_load_1d_2d(dim, kind, p):
    _check_flux(dim, kind, p)


def _check_trace(dim, kind, p):
    m = _mesh(dim, kind, p)
    U, Dn = E.trace(m, _u(dim, kind, p))
    for nit in (0.0, 6.0 * p * p):  # the trace does not depend on the operator's Nitsche terms
        op = _op(dim, kind, p, nit)
        perm = op.bc_reference_order()
        u = _dev(_u(dim, kind, p))
        ub, db = op.eval_trace(u)
        assert ub.numel() == op.n_bc_points == U.size
        ru, rd = _rel(_host(ub)[perm], U), _rel(_host(db)[perm], Dn)
        print("trace %dD %s p=%d nitsche=%g: %.2e %.2e" % (dim, kind, p, nit, ru, rd))
        assert ru <= TOL and rd <= TOL
        assert torch.equal(op.eval_trace(u, dn_bc=False), ub)
        assert torch.equal(op.eval_trace(u, u_bc=False), db)


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
def test_trace_3d(kind, p):
    _check_trace(3, kind, p)


@pytest.mark.parametrize("kind,p", LOW, ids=LOW_IDS)
@pytest.mark.parametrize("dim", [1, 2])
def test_trace_1d_2d(dim, kind, p):
    _check_trace(dim, kind, p)


def _kappa(dim):
    """the coefficient of test_gpu_coefgrid.py"""
    if dim == 3:
        return lambda x: 2 + np.sin(3 * x[:, 0] * x[:, 1] + 2 * x[:, 2]) + 0.5 * np.cos(5 * (x[:, 0] - x[:, 1] * x[:, 2]))
    if dim == 2:
        return lambda x: 2 + np.sin(3 * x[:, 0] * x[:, 1]) + 0.5 * np.cos(5 * x[:, 0])
    return lambda x: 2 + np.sin(3 * x[:, 0]) + 0.5 * np.cos(5 * x[:, 0])


@pytest.mark.parametrize("dim,kind,p", [(3, "middle", 3), (3, "small", 5), (3, "middle", 5), (2, "middle", 5),
                                        (2, "small", 9), (1, "middle", 3), (3, "small", 7)])
def test_device_identities(dim, kind, p):
    """add_load(eval values) = M u; -add_load_grad(kq grad u) = K[kappa] u at nitsche = 0"""
    op = _op(dim, kind, p)
    u = _dev(_u(dim, kind, p))
    uq, gq = op.eval_grid(u)
    Mu = op.mass_apply(u, op.new_vector(False))
    r = _rel(_host(op.add_load(uq, op.new_vector(False))), _host(Mu))
    print("add_load(values) vs mass_apply %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= TOL
    kq = _dev(_kappa(dim)(op.gauss_grid_points()))
    op.set_coefficient_grid(kq)
    Ku = op.apply(u, op.new_vector(False))
    flux = (gq.view(dim, -1) * kq[None, :]).reshape(-1).contiguous()
    r = _rel(_host(op.add_load_grad(flux, op.new_vector(False), scale=-1.0)), _host(Ku))
    print("-add_load_grad(kq grad u) vs grid apply %dD %s p=%d: %.2e" % (dim, kind, p, r))
    assert r <= TOL


@pytest.mark.parametrize("p", [3, 5])
def test_bitwise_repeatable_runs_streams_and_graph_replay(p):
    """a second run, a run on a second stream and the replay of captured FIRST
    calls (no warm-up of the operator before the capture) give the same bits"""
    dim, kind = 3, "middle"
    nit = 6.0 * p * p
    u = _dev(_u(dim, kind, p))
    F = _dev(_flux(dim, kind, p)[0])

    def run(op, out):
        op.eval_grid(u, out[0], out[1])
        op.add_load_grad(F, out[2], scale=1.5)
        op.eval_trace(u, out[3], out[4])

    def outputs(op):
        nq, nb = op.n_grid_points, op.n_bc_points
        z = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")  # noqa: E731
        return [z(nq), z(dim * nq), z(op.n_owned), z(nb), z(nb)]

    # the captured operator has never run before: nothing may allocate or synchronise in the calls
    cap = _op(dim, kind, p, nit)
    oc = outputs(cap)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        cap.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            run(cap, oc)
    torch.cuda.synchronize()
    cap.use_torch_stream()

    op = _op(dim, kind, p, nit)
    ref = outputs(op)
    run(op, ref)
    torch.cuda.synchronize()
    assert all(float(r.abs().max()) > 0.0 for r in ref)
    again = outputs(op)
    run(op, again)
    assert all(torch.equal(a, r) for a, r in zip(again, ref))
    other = outputs(op)
    with torch.cuda.stream(s):
        op.use_torch_stream()
        run(op, other)
    torch.cuda.synchronize()
    op.use_torch_stream()
    assert all(torch.equal(a, r) for a, r in zip(other, ref))
    for _ in range(2):
        for o in oc:
            o.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, r) for a, r in zip(oc, ref))


def test_elasticity_components():
    """on an elasticity operator every entry point takes one component's block"""
    import gdm_amd

    dim, kind, p = 2, "middle", 3
    m = _mesh(dim, kind, p)
    op = gdm_amd.GdmOperator(dim, p, _nsub(kind, p, dim), LO3[:dim], HI3[:dim], "elasticity", params=(1.0, 2.0))
    rng = np.random.default_rng(3)
    uh = rng.uniform(-1, 1, (dim, m.n_dofs))
    u = _dev(uh)
    nq = op.n_grid_points
    for c in range(dim):
        uq, gq = op.eval_grid(op.component(u, c))
        assert _rel(_host(uq), E.values(m, uh[c])) <= TOL
        g = _host(gq).reshape(dim, nq)
        ref = E.gradients(m, uh[c])
        for e in range(dim):
            assert _rel(g[e], ref[e]) <= TOL
        ub, db = op.eval_trace(op.component(u, c))
        U, Dn = E.trace(m, uh[c])
        perm = op.bc_reference_order()
        assert _rel(_host(ub)[perm], U) <= TOL and _rel(_host(db)[perm], Dn) <= TOL
    F, ref = _flux(dim, kind, p)
    y = op.new_vector_field()
    op.add_load_grad(_dev(F), op.component(y, 1))
    assert _rel(_host(op.component(y, 1)), ref) <= TOL
    assert float(op.component(y, 0).abs().max()) == 0.0


def test_errors():
    """the documented statuses, each with a message from gdm_last_error"""
    import gdm_amd
    from gdm_amd import _capi

    lib = _capi.load()
    big = torch.ones(3 * 6 * 5 * 8 * 64, dtype=torch.float64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    op = gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "wave", params=(20.0,))
    u = op.new_vector()
    assert lib.gdm_eval_grid(op.h, P(u), None, None) == ERR_ARG
    assert "NULL" in _capi.last_error()
    assert lib.gdm_eval_grid(op.h, None, P(big), None) == ERR_ARG
    assert lib.gdm_eval_grid(op.h, P(big), P(big), None) == ERR_ARG  # an output overlaps u
    assert "overlap" in _capi.last_error()
    assert lib.gdm_eval_trace(op.h, P(u), None, None) == ERR_ARG
    assert lib.gdm_add_load_grad(op.h, None, 1.0, P(u)) == ERR_ARG
    assert lib.gdm_eval_grid(None, P(u), P(big), None) == ERR_ARG
    with pytest.raises(gdm_amd.GdmError):
        op.eval_grid(u, values=big)  # wrong size
    with pytest.raises(gdm_amd.GdmError):
        op.add_load_grad(big[:7], op.new_vector(False))
    # n_ranks = 2, a periodic mesh
    for other, word in ((gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "wave", rank=0, n_ranks=2), "rank"),
                        (gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "wave", periodic=1), "periodic")):
        v = other.new_vector()
        assert lib.gdm_eval_grid(other.h, P(v), P(big), P(big)) == ERR_UNSUPPORTED and word in _capi.last_error()
        assert lib.gdm_add_load_grad(other.h, P(big), 1.0, P(v)) == ERR_UNSUPPORTED and word in _capi.last_error()
        assert lib.gdm_eval_trace(other.h, P(v), P(big), P(big)) == ERR_UNSUPPORTED and word in _capi.last_error()
    # every operator kind evaluates
    adv = gdm_amd.GdmOperator(2, 3, (6, 5), 0.0, 1.0, "advection", params=(1.0, 0.5))
    m = O.Mesh(2, 3, [6, 5], 0.0, 1.0)
    uh = np.random.default_rng(1).uniform(-1, 1, m.n_dofs)
    assert _rel(_host(adv.eval_grid(_dev(uh), gradients=False)), E.values(m, uh)) <= TOL
