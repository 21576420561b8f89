"""The mass matrix weighted by a separable density (gdm_op_set_density,
csrc/gdm_varmass.hip) against the numpy restatement of the reference's cell
loop for a pointwise rho (tests/varmass_ref.py, pinned to the oracle in
tests/test_varmass_cpu.py).

Tolerance: rel-L2 1e-12 against the restatement, the project's bound for fp64
summation-order differences (tests/test_gpu_vardiff.py).

Meshes, derived from the kernel's tile (T_x, T_y) and z chunk
(gdm_density_tile; kernel axes: 3D (x, y, z), 2D (x, y), 1D z):
  small   every extent p cells (the smallest the operator accepts): every row
          is a wall row;
  middle  each extent one tile / chunk plus 1 node, so a tile of a single
          column, one of a single row and a chunk of one plane exist;
  large   two tiles plus a remainder in x and y, two z chunks plus a remainder.
The boxes are anisotropic in h.  p in {3, 5} on all three, p in {1, 7, 9} on
the small mesh.

Densities on the box (-0.5, 0, 0.2) - (0.7, 0.9, 1.5), the families of
tests/test_gpu_vardiff.py:
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
import varmass_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LO3, HI3 = (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -3, -5


def _tile():
    from gdm_amd import _capi

    return _capi.density_tile(5, 3)


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


def _terms(which, dim):
    """the separable terms of a density: a list of per-direction callables / None"""
    if which == "one":
        t = [[lambda x: 1 + 0.5 * np.sin(3 * x), np.exp, lambda z: 1 + z * z]]
    else:
        t = [[lambda x: 2.0, None, None],
             [lambda x: 0.5 * np.sin(3 * x), None, None],
             [None, lambda y: 0.4 * np.cos(2 * y), lambda z: z],
             [lambda x: 0.3 * x, lambda y: y, lambda z: z]]
    return [f[:dim] for f in t]


@functools.lru_cache(maxsize=None)
def _mesh(dim, kind, p):
    return O.Mesh(dim, p, list(_nsub(kind, p, dim)), list(LO3[:dim]), list(HI3[:dim]))


def _op(dim, kind, p, which=None, nitsche=0.0):
    import gdm_amd

    op = gdm_amd.GdmOperator(dim, p, _nsub(kind, p, dim), LO3[:dim], HI3[:dim], "wave",
                             params=(nitsche,) if nitsche else ())
    if which is not None:
        op.set_density(_terms(which, dim))
    return op


def _check_apply(dim, kind, p, cases, seed):
    """density_apply against the restatement; the fused `+ c add` against apply
    then axpby; a second apply gives the same bits"""
    m = _mesh(dim, kind, p)
    u = np.random.default_rng(seed).uniform(-1, 1, m.n_dofs)
    ud = _dev(u)
    for which in cases:
        op = _op(dim, kind, p, which)
        got = op.density_apply(ud)
        r = _rel(_host(got), R.mass_apply(m, R.pointwise(_terms(which, dim), dim), u))
        print("density apply %dD %s p=%d %s: %.2e" % (dim, kind, p, which, r))
        assert r < 1e-12
        assert float(got.abs().max()) > 0.0
        assert torch.equal(op.density_apply(ud), got)
        gen = torch.Generator(device="cuda").manual_seed(seed)
        add = torch.rand(op.n_owned, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        fused = op.density_apply(ud, c=-0.37, add=add)
        want = got - 0.37 * add
        e = float(torch.linalg.norm(fused - want) / torch.linalg.norm(want))
        print("  fused epilogue: %.2e" % e)
        assert e <= 1e-14
        assert torch.equal(op.density_apply(ud, c=-0.37, add=add), fused)


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
def test_apply_3d(kind, p):
    """M[rho] u (the large mesh: the four-term case alone; small-p9 with four
    terms is the largest LDS plan, above the default 64 KiB limit)"""
    _check_apply(3, kind, p, ["four"] if kind == "large" else ["one", "four"], p)


@pytest.mark.parametrize("kind,p", MESHES, ids=MESH_IDS)
@pytest.mark.parametrize("dim", [1, 2])
def test_apply_1d_2d(dim, kind, p):
    _check_apply(dim, kind, p, ["one", "four"], 10 * dim + p)


@pytest.mark.parametrize("kind,p", [("small", p) for p in (1, 3, 5, 7, 9)] + [("middle", 3), ("middle", 5)])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_constant_density_and_removal(dim, kind, p):
    """rho = 2 (one term, and 1 + 1 as two terms) gives 2 mass_apply to 1e-14;
    set_density([]) leaves mass_apply, apply and mass_solve with the bits they
    had before a density was ever set"""
    op = _op(dim, kind, p, nitsche=6.0 * p * p)
    gen = torch.Generator(device="cuda").manual_seed(p)
    u = torch.rand(op.n_local, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    before = [op.mass_apply(u, op.new_vector(False)).clone(), op.apply(u, op.new_vector(False)).clone(),
              op.mass_solve(u, op.new_vector(False)).clone()]
    want = 2.0 * before[0]
    for terms in ([[lambda s: 2.0] + [None] * (dim - 1)], [[None] * dim, [None] * dim]):
        op.set_density(terms)
        assert op.has_density
        got = op.density_apply(u)
        e = float(torch.linalg.norm(got - want) / torch.linalg.norm(want))
        print("rho = 2, %dD %s p=%d, %d term(s): %.2e" % (dim, kind, p, len(terms), e))
        assert e <= 1e-14
        # the unweighted entry points do not change while a density is set
        assert torch.equal(op.mass_apply(u, op.new_vector(False)), before[0])
        assert torch.equal(op.apply(u, op.new_vector(False)), before[1])
        assert torch.equal(op.mass_solve(u, op.new_vector(False)), before[2])
    op.set_density([])
    assert not op.has_density
    assert torch.equal(op.mass_apply(u, op.new_vector(False)), before[0])
    assert torch.equal(op.apply(u, op.new_vector(False)), before[1])
    assert torch.equal(op.mass_solve(u, op.new_vector(False)), before[2])
    import gdm_amd

    with pytest.raises(gdm_amd.GdmError, match="no density"):
        op.density_apply(u)


def test_replacing_the_density_and_shared_arrays():
    """a second set_density replaces the first; terms that share an array
    object give the bits of copies"""
    p = 3
    op = _op(3, "middle", p, "four")
    m = _mesh(3, "middle", p)
    u = np.random.default_rng(5).uniform(-1, 1, m.n_dofs)
    op.set_density(_terms("one", 3))
    assert _rel(_host(op.density_apply(_dev(u))), R.mass_apply(m, R.pointwise(_terms("one", 3), 3), u)) < 1e-12
    fx = np.array([1 + 0.5 * np.sin(3 * x) for x in op.field_points(0)])
    fy = np.exp(op.field_points(1))
    fz = 1 + op.field_points(2) ** 2
    op.set_density([[fx, fy, fz], [fx, None, fz], [fx, fy, None]])
    shared = op.density_apply(_dev(u))
    op.set_density([[fx.copy(), fy.copy(), fz.copy()], [fx.copy(), None, fz.copy()], [fx.copy(), fy.copy(), None]])
    assert torch.equal(op.density_apply(_dev(u)), shared)
    assert float(shared.abs().max()) > 0.0


def test_time_op():
    op = _op(3, "small", 3, "one")
    u, y = op.new_vector(), op.new_vector(local=False)
    assert op.time_op(3, u, y, None, 2) > 0.0


def test_errors():
    """the documented statuses, each with a message from gdm_last_error"""
    import gdm_amd
    from gdm_amd import _capi
    from gdm_amd.cut_wave import CutWave, preset

    lib = _capi.load()
    unit = _capi.CoefTerm()

    def set_density(op, n_terms, terms):
        rc = lib.gdm_op_set_density(op.h if hasattr(op, "h") else op, n_terms, terms)
        return rc, _capi.last_error()

    # another operator kind
    opa = gdm_amd.GdmOperator(2, 3, (6, 5), 0.0, 1.0, "advection", params=(1.0, 0.5))
    rc, msg = set_density(opa, 1, ctypes.byref(unit))
    assert rc == ERR_UNSUPPORTED and "wave" in msg
    # n_ranks = 2
    op2 = gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "wave", rank=0, n_ranks=2)
    rc, msg = set_density(op2, 1, ctypes.byref(unit))
    assert rc == ERR_UNSUPPORTED and "rank" in msg
    # a periodic mesh
    per = gdm_amd.GdmOperator(3, 3, (3, 5, 6), 0.0, 1.0, "wave", periodic=1)
    rc, msg = set_density(per, 1, ctypes.byref(unit))
    assert rc == ERR_UNSUPPORTED and "periodic" in msg
    # the inner operator of a cut handle
    P = preset("wave", dim=2)
    cw = CutWave(P["p"], P["n"], P["left"], P["right"], P["level_set"], ghost_parameter_M=P["gamma_M"],
                 ghost_parameter_A=P["gamma_A"], nitsche=P["nitsche"], dim=2)
    rc, msg = set_density(cw._op, 1, ctypes.byref(unit))
    assert rc == ERR_UNSUPPORTED and "cut" in msg

    op = gdm_amd.GdmOperator(3, 3, (6, 5, 8), 0.0, 1.0, "wave", params=(20.0,))
    # n_terms outside [0, 4]
    five = (_capi.CoefTerm * 5)()
    rc, msg = set_density(op, 5, five)
    assert rc == ERR_ARG and "n_terms" in msg
    rc, msg = set_density(op, -1, five)
    assert rc == ERR_ARG and "n_terms" in msg
    rc, msg = set_density(op, 1, None)
    assert rc == ERR_ARG
    with pytest.raises(gdm_amd.GdmError):
        op.set_density([[None] * 3] * 5)
    # a non-finite sample
    bad = np.ones_like(op.field_points(1))
    bad[3] = np.inf
    with pytest.raises(gdm_amd.GdmError, match="finite"):
        op.set_density([[None, bad, None]])
    bad[3] = np.nan
    with pytest.raises(gdm_amd.GdmError, match="finite"):
        op.set_density([[None, None, None], [None, bad, None]])
    # one term: a factor that vanishes or changes sign
    x = op.field_points(0)
    with pytest.raises(gdm_amd.GdmError, match="sign"):
        op.set_density([[x - 0.5, None, None]])
    zero = np.ones_like(x)
    zero[-1] = 0.0
    with pytest.raises(gdm_amd.GdmError, match="vanishes"):
        op.set_density([[zero, None, None]])
    assert not op.has_density  # the failed calls left no density behind
    u, y = op.new_vector(), op.new_vector(local=False)
    with pytest.raises(gdm_amd.GdmError, match="no density"):
        op.density_apply(u, y)
    with pytest.raises(gdm_amd.GdmError, match="no density"):
        op.density_solve(u, y)
    # two negative factors: rho = 1; in a sum a factor may change sign
    op.set_density([[-np.ones_like(x), -np.ones_like(op.field_points(1)), None]])
    u.copy_(_dev(np.random.default_rng(1).uniform(-1, 1, op.n_local)))
    assert _rel(_host(op.density_apply(u, y)), _host(op.mass_apply(u, op.new_vector(False)))) < 1e-14
    op.set_density([[None, None, None], [0.5 * (x - 0.5), None, None]])
    # src = dst
    rc = lib.gdm_density_apply(op.h, ctypes.c_void_p(u.data_ptr()), ctypes.c_void_p(u.data_ptr()))
    assert rc == ERR_ARG
    rc = lib.gdm_density_apply(op.h, None, ctypes.c_void_p(u.data_ptr()))
    assert rc == ERR_ARG
