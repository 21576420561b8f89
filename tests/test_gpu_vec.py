"""The vector, reduction and constraint entry points, called directly.

gdm_vec_axpby, gdm_vec_dot, gdm_vec_pointwise_mult, gdm_vec_rk_update (scalar
path), gdm_mass_diagonal and gdm_constraints_distribute otherwise run only
inside the CG loops and RK drivers, at a few hundred entries.  Here each is
compared with a plain reference (tests/vec_ref.py, numpy, the oracle's 1D
matrices, tests/periodic_mass_ref.py) at the lengths where its kernel changes
behaviour: 1 .. 3 entries, around two blocks of 256, and one length past the
launcher's block cap, where the grid-stride loop takes a second trip.

Operands are views that start 0 or 1 doubles past a 16-byte boundary; each
test asserts data_ptr() % 16.  Alignment is the only input of the launchers'
choice between the pair (double2) and the entry-by-entry kernels (al16 in
gdmk_launch_rk_update / gdmk_launch_axpby), so that assertion is the path
assertion of DESIGN §3.  Outputs that alias no input start as NaN, and one
sentinel double on each side of every output must survive.

Tolerances (none is measured on the device):
  axpby   |got - ref| <= 2 * 2^-53 (|a x| + |b y|) per entry: the kernel rounds
          b * y (2^-53 |b y|) and then the fma (2^-53 |result| <= 2^-53 (|a x|
          + |b y|) to first order); ref is a x + b y in np.longdouble.
  dot     vec_ref.dot_bound, derived in its docstring; tests/
          test_vec_ref_cpu.py shows the kernel's summation order meets it.
  vmul    bitwise numpy's w * x (one rounding).
  rk      rtol 1e-14, atol 1e-15 against numpy: the tolerances of
          tests/test_gpu_rk.py::test_rk_update_matches_numpy (numpy rounds
          beta * k before the addition, the kernel's fma does not: with
          operands in [-1, 1] that is below 1.25 * 2^-53 < atol); and bitwise
          against the same call on aligned copies (gdm_hip.h: same bits).
  mass_diagonal  rel 1e-14 against the Kronecker product of the oracle's 1D
          diagonals, periodic or not (dim factors, each a sum of a few
          positive quadrature terms assembled independently by the library
          and the oracle, and dim - 1 multiplications: some tens of 2^-53);
          against the assembled condensed cell-loop matrix rel 4 K 2^-53,
          K = 2^dim (p+1)^dim: a diagonal entry there is a sum of up to
          2^dim (4^dim when periodic images fold onto it, which the factor
          4 covers with the few roundings of each term) cell contributions
          of (p+1)^dim positive quadrature terms, so its relative error is
          at most the number of additions times 2^-53; bitwise across
          ranks.
  distribute  bitwise (copies).
"""
import numpy as np
import pytest

import oracle as O
import periodic_mass_ref as R
import vec_ref as V
from test_gpu_mass_dispatch import MODES

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7.25e33
BETA, ALPHA = 0.37, -1.25  # as tests/test_gpu_rk.py

L_SMALL = [1, 2, 3, 511, 512, 513]
# one length past each launcher's cap of 4096 blocks of 256 lanes, where the grid-stride loop wraps:
L_AXPBY_WRAP = 2 * 4096 * 256 + 3  # gdmk_launch_axpby: min(.., 4096) blocks of pairs, and an odd tail
L_VMUL_WRAP = 4096 * 256 + 5  # gdmk_launch_vmul: min(.., 4096) blocks
L_RK_WRAP = 4096 * 256 + 5  # gdmk_launch_rk_update, scalar path: min(.., 256 * 16) blocks
L_DOT_WRAP = [262144, 262145, 1000003]  # gdm_op::n_dot_partial = 1024 blocks: exactly full, one more, four trips
L_DOT = L_SMALL + [63, 64, 65, 255, 256, 257] + L_DOT_WRAP


@pytest.fixture(scope="module")
def op():
    import gdm_amd

    return gdm_amd.GdmOperator(1, 1, 4, 0.0, 1.0, "mass")


class Vec:
    """n doubles on the device starting `shift` (0 / 1) doubles past a 16-byte
    boundary, NaN unless values are given, with a sentinel on each side"""

    def __init__(self, n, shift, values=None):
        self.n, self.lo = n, 2 + int(shift)
        self.buf = torch.full((n + 4,), NAN, dtype=torch.float64, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[self.lo - 1] = SENTINEL
        self.buf[self.lo + n] = SENTINEL
        self.t = self.buf[self.lo:self.lo + n]
        if values is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)))
        assert self.t.data_ptr() % 16 == 8 * int(shift)

    def host(self):
        """the values, after checking that the sentinels survived"""
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert b[self.lo - 1] == SENTINEL and b[self.lo + self.n] == SENTINEL, "sentinel overwritten"
        return b[self.lo:self.lo + self.n].copy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def first_mismatch(got, ref):
    bad = np.flatnonzero(bits(got) != bits(ref))
    return "no mismatch" if bad.size == 0 else "%d of %d differ, first at %d: got %r, expected %r" % (
        bad.size, got.size, bad[0], got[bad[0]], ref[bad[0]])


def assert_bitwise(got, ref, what):
    assert np.array_equal(bits(got), bits(ref)), (what, first_mismatch(got, ref))


SHIFTS2 = [(0, 0), (1, 0), (0, 1), (1, 1)]


# ---- axpby -------------------------------------------------------------------------------------------------------
def _assert_axpby_bound(got, a, x, b, y, what):
    ref, mag = V.axpby_ref(a, x, b, y)
    err = np.abs(got.astype(np.longdouble) - ref)
    bad = np.flatnonzero(~(err <= 2 * np.longdouble(V.U) * mag))
    assert bad.size == 0, (what, "%d entries, first %d: got %r ref %r" % (bad.size, bad[0], got[bad[0]],
                                                                           float(ref[bad[0]])))


@pytest.mark.parametrize("n", L_SMALL + [L_AXPBY_WRAP])
@pytest.mark.parametrize("a,b", [(0.37, -1.25), (-0.6, 1.0)])
def test_axpby_general(op, n, a, b):
    rng = np.random.default_rng(n)
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    for sx, sy in SHIFTS2:
        xv, yv = Vec(n, sx, x), Vec(n, sy, y)
        op.axpby(a, xv.t, b, yv.t)
        _assert_axpby_bound(yv.host(), a, x, b, y, (n, a, b, sx, sy))
        assert_bitwise(xv.host(), x, "x is only read")


@pytest.mark.parametrize("n", L_SMALL + [L_AXPBY_WRAP])
def test_axpby_zero_factor_does_not_read_its_operand(op, n):
    """b == 0: y = a x whatever y held; a == 0: y = b y whatever x holds; both:
    y = 0 -- the `v = 0`, `r = b`, `p = z` calls of DeviceVector::operator= and
    MassMatrixOperator::solve_distributed on memory that was never written"""
    rng = np.random.default_rng(n + 1)
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    poison = np.full(n, NAN)
    poison[1::3] = np.inf
    poison[2::3] = -np.inf
    for sx, sy in SHIFTS2:
        xv, yv = Vec(n, sx, x), Vec(n, sy, poison)
        op.axpby(1.0, xv.t, 0.0, yv.t)
        assert_bitwise(yv.host(), x, ("(1, 0): y = x", n, sx, sy))
        xv, yv = Vec(n, sx, x), Vec(n, sy, poison)
        op.axpby(0.37, xv.t, 0.0, yv.t)
        assert_bitwise(yv.host(), 0.37 * x, ("(0.37, 0): y = 0.37 x, one rounding", n, sx, sy))
        xv, yv = Vec(n, sx, poison), Vec(n, sy, y)
        op.axpby(0.0, xv.t, 2.0, yv.t)
        assert_bitwise(yv.host(), 2.0 * y, ("(0, 2): y = 2 y", n, sx, sy))
        xv, yv = Vec(n, sx, poison), Vec(n, sy, poison)
        op.axpby(0.0, xv.t, 0.0, yv.t)
        assert_bitwise(yv.host(), np.zeros(n), ("(0, 0): y = 0", n, sx, sy))
    for s in (0, 1):
        v = Vec(n, s, poison)
        op.axpby(0.0, v.t, 0.0, v.t)
        assert_bitwise(v.host(), np.zeros(n), ("(0, 0), x is y: v = 0", n, s))


@pytest.mark.parametrize("n", L_SMALL + [L_AXPBY_WRAP])
def test_axpby_x_is_y(op, n):
    x = np.random.default_rng(n + 2).uniform(-1, 1, n)
    for s in (0, 1):
        for a, b in [(0.5, 0.5), (0.37, -1.25)]:
            v = Vec(n, s, x)
            op.axpby(a, v.t, b, v.t)
            got = v.host()
            _assert_axpby_bound(got, a, x, b, x, (n, s, a, b))
            if (a, b) == (0.5, 0.5):
                assert_bitwise(got, x, "0.5 x + 0.5 x is exact")


# ---- dot ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["uniform", "same", "cancel"])
def test_dot(op, case):
    """against math.fsum of the float64 products within vec_ref.dot_bound (an
    absolute bound in terms of sum |x_i y_i|: the "cancel" inputs sum to ~ 0);
    a second call returns the same bits"""
    for n in L_DOT:
        x, y = V.dot_inputs(case, n)
        ref, sum_abs = V.dot_ref(x, y)
        bound = V.dot_bound(n, sum_abs)
        for sx, sy in SHIFTS2:
            xv = Vec(n, sx, x)
            if case == "same":
                if sy != sx:
                    continue
                yv = xv
            else:
                yv = Vec(n, sy, y)
            got = op.dot(xv.t, yv.t)
            assert abs(got - ref) <= bound, (case, n, sx, sy, got, ref, abs(got - ref), bound)
            again = op.dot(xv.t, yv.t)
            assert bits([got])[0] == bits([again])[0], (case, n, got, again)
            assert_bitwise(xv.host(), x, "x is only read")


def test_dot_of_nothing_is_zero(op):
    e = torch.empty(0, dtype=torch.float64, device="cuda")
    assert op.dot(e, e) == 0.0
    v = Vec(4, 0, np.ones(4))
    assert op.dot(v.t[:0], v.t[:0]) == 0.0


# ---- pointwise_mult ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", L_SMALL + [L_VMUL_WRAP])
def test_pointwise_mult(op, n):
    rng = np.random.default_rng(n + 3)
    w, x = rng.uniform(-2, 2, n), rng.uniform(-1, 1, n)
    ref = w * x
    for sw in (0, 1):
        for sx in (0, 1):
            for sy in (0, 1):
                wv, xv, yv = Vec(n, sw, w), Vec(n, sx, x), Vec(n, sy)
                op.pointwise_mult(wv.t, xv.t, yv.t)
                assert_bitwise(yv.host(), ref, (n, sw, sx, sy))
                assert_bitwise(wv.host(), w, "w is only read")
                assert_bitwise(xv.host(), x, "x is only read")
            wv, xv = Vec(n, sw, w), Vec(n, sx, x)
            op.pointwise_mult(wv.t, xv.t, xv.t)
            assert_bitwise(xv.host(), ref, ("y is x", n, sw, sx))
            wv, xv = Vec(n, sw, w), Vec(n, sx, x)
            op.pointwise_mult(wv.t, xv.t, wv.t)
            assert_bitwise(wv.host(), ref, ("y is w", n, sw, sx))


# ---- rk_update, scalar path ----------------------------------------------------------------------------------------
def _rk_call(op, mode, k, acc, y, shifted):
    """one gdm_vec_rk_update in alias mode `mode` on fresh copies; the operand
    named `shifted` (or none) starts one double past a 16-byte boundary.
    Returns (acc_out values, Y values or None)."""
    has_Y, y_is_acc, acc_alias, Y_alias = mode
    n = k.size
    kv = Vec(n, shifted == "k", k)
    acc_in = Vec(n, shifted == "acc_in", acc)
    y_in = acc_in if y_is_acc else Vec(n, shifted == "y", y)
    acc_out = acc_in if acc_alias else Vec(n, shifted == "acc_out")
    Y = (y_in if Y_alias else Vec(n, shifted == "Y")) if has_Y else None
    used = [kv, acc_in, acc_out] + ([y_in, Y] if has_Y else [])
    # the dispatch's only input: every operand 16-byte aligned <=> the pair kernel
    assert all(v.t.data_ptr() % 16 == 0 for v in used) == (shifted is None)
    op.rk_update(BETA, kv.t, acc_in.t, acc_out.t, ALPHA, y_in.t if has_Y else None, Y.t if has_Y else None)
    assert_bitwise(kv.host(), k, "k is only read")
    return acc_out.host(), (Y.host() if has_Y else None)


def _distinct_operands(mode):
    has_Y, y_is_acc, acc_alias, Y_alias = mode
    names = ["k", "acc_in"]
    if not acc_alias:
        names.append("acc_out")
    if has_Y and not y_is_acc:
        names.append("y")
    if has_Y and not Y_alias:
        names.append("Y")
    return names


@pytest.mark.parametrize("n", L_SMALL + [L_RK_WRAP])
@pytest.mark.parametrize("name", list(MODES))
def test_rk_update_scalar_path_every_alias_mode(op, name, n):
    mode = MODES[name][0]
    has_Y, y_is_acc = mode[0], mode[1]
    rng = np.random.default_rng(n + 4)
    k, acc, y = (rng.uniform(-1, 1, n) for _ in range(3))
    acc_ref = acc + BETA * k
    Y_ref = (acc if y_is_acc else y) + ALPHA * k
    acc_al, Y_al = _rk_call(op, mode, k, acc, y, None)
    for shifted in _distinct_operands(mode):
        acc_got, Y_got = _rk_call(op, mode, k, acc, y, shifted)
        np.testing.assert_allclose(acc_got, acc_ref, rtol=1e-14, atol=1e-15, err_msg=str((name, n, shifted)))
        assert_bitwise(acc_got, acc_al, ("acc_out vs aligned", name, n, shifted))
        if has_Y:
            np.testing.assert_allclose(Y_got, Y_ref, rtol=1e-14, atol=1e-15, err_msg=str((name, n, shifted)))
            assert_bitwise(Y_got, Y_al, ("Y vs aligned", name, n, shifted))
    np.testing.assert_allclose(acc_al, acc_ref, rtol=1e-14, atol=1e-15)
    if has_Y:
        np.testing.assert_allclose(Y_al, Y_ref, rtol=1e-14, atol=1e-15)


# ---- mass_diagonal -------------------------------------------------------------------------------------------------
LO, HI = (-0.3, 0.1, 0.0), (1.1, 0.8, 1.3)
DIAG_CASES = [(dim, p) for dim in (1, 2, 3) for p in (1, 3, 5, 7, 9)]


def _mesh(dim, p):
    n = (p, p + 1, p + 2)[:dim]
    return n, O.Mesh(dim, p, list(n), LO[:dim], HI[:dim])


def _kron_diagonal(m):
    d = [m.matrices_1d(a)[0][:, m.p] for a in range(m.dim)]  # band form: column p is the diagonal
    out = d[0]
    for a in range(1, m.dim):
        out = np.multiply.outer(d[a], out)
    return out.reshape(-1)


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("dim,p", DIAG_CASES)
def test_mass_diagonal_is_the_kronecker_product_of_the_1d_diagonals(dim, p):
    import gdm_amd
    from gdm_amd.distributed import slab

    n, m = _mesh(dim, p)
    one = gdm_amd.GdmOperator(dim, p, n, LO[:dim], HI[:dim], "mass")
    out = Vec(one.n_owned, 1)
    one.mass_diagonal(out.t)
    got = out.host()
    assert got.size == m.n_dofs
    np.testing.assert_allclose(got, _kron_diagonal(m), rtol=1e-14, atol=0)
    assert_bitwise(_host(one.mass_diagonal()), got, "the wrapper's own vector")
    # the slabs of 2 and 3 ranks tile the one-rank diagonal
    for n_ranks in (2, 3):
        tiled = 0
        for r in range(n_ranks):
            pb, pe, _, _ = slab(n[-1], n_ranks, r)
            if pe == pb:  # p + dim - 1 cells do not always fill 3 slabs; a rank without planes has no diagonal
                continue
            opr = gdm_amd.GdmOperator(dim, p, n, LO[:dim], HI[:dim], "mass", n_ranks=n_ranks, rank=r)
            L = opr.layout
            assert (L["owned_plane_begin"], L["owned_plane_end"]) == (pb, pe)
            b = pb * L["plane_size"]
            assert opr.n_owned == (pe - pb) * L["plane_size"] and b == tiled
            assert_bitwise(_host(opr.mass_diagonal()), got[b:b + opr.n_owned], (n_ranks, r))
            tiled += opr.n_owned
        assert tiled == m.n_dofs


@pytest.mark.parametrize("dim,p", DIAG_CASES)
def test_mass_diagonal_periodic_is_the_condensed_diagonal(dim, p):
    import gdm_amd

    n, m = _mesh(dim, p)
    for mask in range(1, 2 ** dim):
        ref = R.PeriodicMassRef(m, mask)
        opp = gdm_amd.GdmOperator(dim, p, n, LO[:dim], HI[:dim], "mass", periodic=mask)
        got = _host(opp.mass_diagonal())
        assert np.array_equal(got == 1.0, ref.constrained), (dim, p, mask)
        # the Kronecker product of the reference's condensed 1D factors (constrained vertices 1)
        d = []
        for a in range(dim):
            f = np.diag(ref.factor[a])
            d.append(np.append(f, 1.0) if mask & (1 << a) else f)
        kron = d[0]
        for a in range(1, dim):
            kron = np.multiply.outer(d[a], kron)
        kron = np.where(ref.constrained, 1.0, kron.reshape(-1))
        np.testing.assert_allclose(got, kron, rtol=1e-14, atol=0, err_msg=str((dim, p, mask)))
        # the assembled condensed cell-loop matrix, where the oracle assembles it in well under a second
        # (3D p = 7 takes 3 s and p = 9 50 s per matrix: there the factors above, which
        # tests/test_periodic_mass_cpu.py pins to this matrix, stand alone)
        if dim < 3 or p <= 5:
            np.testing.assert_allclose(got, ref.sparse_condensed().diagonal(),
                                       rtol=4 * 2 ** dim * (p + 1) ** dim * V.U, atol=0, err_msg=str((dim, p, mask)))


# ---- distribute ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(2, (9, 6)), (3, (5, 4, 6))])
def test_distribute_every_periodic_mask(dim, n):
    import gdm_amd

    p = 3
    m = O.Mesh(dim, p, list(n))
    u = np.random.default_rng(dim).uniform(-1, 1, m.n_dofs)
    for mask in range(0, 2 ** dim):
        opp = gdm_amd.GdmOperator(dim, p, n, 0.0, 1.0, "mass", periodic=mask)
        v = Vec(m.n_dofs, 1, u)
        opp.distribute(v.t)
        ref = R.PeriodicMassRef(m, mask).distribute(u) if mask else u  # no constraints: unchanged
        assert_bitwise(v.host(), ref, (dim, mask))


def test_distribute_wraps_the_grid_stride_loop():
    """periodic in z on 1030 x 1030 x 1 cells, p = 1: the face z = 0 has 1031^2
    vertices, more than the 4096 blocks of 256 lanes gdmk_launch_periodic
    caps its grid at (the operator takes 0.03 s to create)"""
    import gdm_amd

    face = 1031 * 1031
    assert face > 4096 * 256
    opp = gdm_amd.GdmOperator(3, 1, (1030, 1030, 1), 0.0, 1.0, "mass", periodic=4)
    assert opp.n_owned == 2 * face
    u = np.random.default_rng(9).uniform(-1, 1, 2 * face)
    ref = u.copy()
    ref[face:] = u[:face]  # vertex plane z = 1 := plane z = 0
    for shift in (0, 1):
        v = Vec(2 * face, shift, u)
        opp.distribute(v.t)
        assert_bitwise(v.host(), ref, shift)
