"""Every dispatch path of the exact mass inverse, reached from small meshes.

Which kernels gdm_mass_solve / gdm_mass_solve_rk launch depends on the number
of lines per pass (a pass with fewer waves of 64 lines than the segment
threshold, 1024 by default, splits its lines into segments) and on the line
length, parity and alignment.  The path the headline benchmark takes -- every
pass unsegmented, the RK update fused into the x pass (mass3_rows_kernel<P,
false, RKM = 1 | 2 | 3>) -- needs a 256^3 mesh at the default threshold.
gdm_op_set_mass_seg_waves lowers the threshold per operator, gdm_op_mass_path
reports what the last solve launched.

Every case asserts the reported path first, so none of them can pass on a
kernel it did not mean to run.  The numbers are then checked against the CPU
reference (oracle.Mesh.kron_mass_inverse followed by numpy acc + beta k and
y + alpha k) at rel-L2 1e-12, and, where include/gdm_hip.h promises the same
bits, bitwise against mass_solve + rk_update."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402

RTOL = 1e-12
BETA, ALPHA = 0.37, -1.25
NAN = float("nan")
CHUNK = {3: 48, 5: 48, 7: 56}  # gdmk_mass3_chunk(p): positions per chunk of the v3 kernels


def _gdm():
    import gdm_amd

    return gdm_amd


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def test_chunk_sizes_and_threshold_range():
    """the shapes below are chosen from C = 48 / 48 / 56; the threshold accepts
    [0, default] and -1 only"""
    g = _gdm()
    lib = g.load()
    assert {p: lib.gdmk_mass3_chunk(p) for p in (1, 3, 5, 7, 9)} == {1: 0, 9: 0, **CHUNK}
    default = lib.gdmk_mass3_seg_waves()
    assert default == 1024
    op = g.GdmOperator(2, 3, 8, 0.0, 1.0, "mass")
    assert op.mass_path() == {"rk_mode": 0, "passes": []}
    for w in (0, 1, default, -1):
        op.set_mass_seg_waves(w)
    for w in (-2, default + 1):
        with pytest.raises(g.GdmError):
            op.set_mass_seg_waves(w)


# ---- the RK operands of one stage ------------------------------------------------------------------------------
# mode: (Y given, y is acc_in, acc_out is acc_in, Y is y) -> the fused kernel's variant RKM
MODES = {
    "noY": ((False, False, False, False), 1),
    "noY-acc_alias": ((False, False, True, False), 1),
    "Y": ((True, False, False, False), 2),
    "Y-acc_alias": ((True, False, True, False), 2),
    "Y-Y_alias": ((True, False, False, True), 2),
    "y_is_acc": ((True, True, False, False), 3),
    "y_is_acc-acc_alias": ((True, True, True, False), 3),
    "y_is_acc-Y_alias": ((True, True, False, True), 3),
}


def _nan(n, shift):
    """n NaNs on the device, starting `shift` (0 / 1) doubles past a 16-byte boundary"""
    buf = torch.full((n + 2,), NAN, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf[int(shift):int(shift) + n]


def _shifted(t, shift):
    """a copy of t that starts `shift` (0 / 1) doubles past a 16-byte boundary"""
    v = _nan(t.numel(), shift)
    v.copy_(t)
    return v


def _stage(op, fused, rhs, acc, y, mode, shift=()):
    """One RK stage's solve + update, fused (mass_solve_rk) or separate
    (mass_solve in place + rk_update) on fresh copies of the operands; outputs
    that alias no input start as NaN.  shift: names of the operands placed one
    double past a 16-byte boundary.  Returns (acc_out, Y or None, path)."""
    has_Y, y_is_acc, acc_alias, Y_alias = mode
    k = _shifted(rhs, "rhs" in shift)
    acc_in = _shifted(acc, "acc_in" in shift)
    y_in = acc_in if y_is_acc else _shifted(y, "y" in shift)
    acc_out = acc_in if acc_alias else _nan(acc.numel(), "acc_out" in shift)
    Y = None
    if has_Y:
        Y = y_in if Y_alias else _nan(acc.numel(), "Y" in shift)
    if fused:
        op.mass_solve_rk(k, BETA, acc_in, acc_out, ALPHA, y_in if has_Y else None, Y)
        path = op.mass_path()
    else:
        op.mass_solve(k, k)
        path = op.mass_path()
        op.rk_update(BETA, k, acc_in, acc_out, ALPHA, y_in if has_Y else None, Y)
    return acc_out, Y, path


def _stage_ref(k_ref, acc, y, mode):
    has_Y, y_is_acc = mode[0], mode[1]
    return acc + BETA * k_ref, ((acc if y_is_acc else y) + ALPHA * k_ref) if has_Y else None


class _Case:
    """operator, operands and CPU reference of one mesh (vertices per axis)"""

    def __init__(self, p, vertices, seed):
        g = _gdm()
        dim = len(vertices)
        n = [v - 1 for v in vertices]
        lo, hi = (0.0,) * dim, (1.0, 0.7, 1.3)[:dim]
        self.op = g.GdmOperator(dim, p, n, lo, hi, "mass")
        self.mesh = O.Mesh(dim, p, n, lo, hi)
        rng = np.random.default_rng(seed)
        self.rhs, self.acc, self.y = (rng.uniform(-1, 1, self.mesh.n_dofs) for _ in range(3))
        self.k_ref = self.mesh.kron_mass_inverse(self.rhs)
        self.d = tuple(dev(v) for v in (self.rhs, self.acc, self.y))

    def check_stage(self, name, fused_expected, x_v3_expected=True, shift=()):
        """the fused call's path, then its numbers: CPU reference, then the
        bits of the separate kernels"""
        mode, rkm = MODES[name]
        acc_f, Y_f, path = _stage(self.op, True, *self.d, mode, shift)
        last = path["passes"][-1]
        assert path["rk_mode"] == (rkm if fused_expected else 0), (name, path)
        assert last["axis"] == 0 and last["v3"] == x_v3_expected and last["segments"] == 1, (name, path)
        if fused_expected:
            assert not last["in_place"], (name, path)
        acc_ref, Y_ref = _stage_ref(self.k_ref, self.acc, self.y, mode)
        assert rel(host(acc_f), acc_ref) < RTOL, name
        if Y_ref is not None:
            assert rel(host(Y_f), Y_ref) < RTOL, name
        acc_s, Y_s, path_s = _stage(self.op, False, *self.d, mode, shift)
        assert path_s["rk_mode"] == 0, (name, path_s)
        assert torch.equal(acc_f, acc_s), (name, float((acc_f - acc_s).abs().max()))
        if Y_ref is not None:
            assert torch.equal(Y_f, Y_s), (name, float((Y_f - Y_s).abs().max()))


# ---- 1. the fused x pass at small shapes -----------------------------------------------------------------------
# x lengths in vertices (even) from the chunk size C: below one chunk, exactly one, a 2-vertex last chunk, both
# parities of the chunk count (the march loop handles two chunks per iteration and leaves it from either half),
# a partial last chunk
X_LENGTHS = {"C-8": lambda C: C - 8, "C": lambda C: C, "C+2": lambda C: C + 2, "2C": lambda C: 2 * C,
             "3C-2": lambda C: 3 * C - 2, "4C+18": lambda C: 4 * C + 18, "5C": lambda C: 5 * C}
# the other axes' vertices: 72 / 35 / 128 / 40 / 70 x lines (a ragged last wave of 8 / 35 / - / 40 / 6 lines; 35 and
# 40 lines are one partial wave).  A mesh has at least p + 1 vertices per direction: 5 x 7 exists for p = 3 only
LINES = {"9x8": (9, 8), "5x7": (5, 7), "16x8": (16, 8), "2d-40": (40,), "2d-70": (70,)}
FUSED_CASES = [(p, xl, ln) for p in (3, 5, 7) for xl in X_LENGTHS for ln in LINES if min(LINES[ln]) >= p + 1]


@pytest.mark.parametrize("p,xlen,lines", FUSED_CASES)
def test_fused_x_pass_small_shapes(p, xlen, lines):
    X = X_LENGTHS[xlen](CHUNK[p])
    assert X % 2 == 0
    c = _Case(p, (X,) + LINES[lines], seed=1000 * p + X)
    assert c.mesh.n_dofs < 1e5
    c.op.set_mass_seg_waves(0)
    for name in MODES:
        c.check_stage(name, fused_expected=True)


# ---- 2. fallbacks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [3, 5, 7])
@pytest.mark.parametrize("lines", ["9x8", "2d-40"])
def test_odd_x_length_is_not_fused(p, lines):
    """the v3 x kernel moves pairs: an odd line length runs the two-sweep x
    kernel and the separate update"""
    c = _Case(p, (2 * CHUNK[p] + 1,) + LINES[lines], seed=7 + p)
    c.op.set_mass_seg_waves(0)
    for name in MODES:
        c.check_stage(name, fused_expected=False, x_v3_expected=False)


@pytest.mark.parametrize("p", [3, 5, 7])
@pytest.mark.parametrize("operand", ["rhs", "acc_in", "acc_out", "y", "Y"])
def test_unaligned_operand_is_not_fused(p, operand):
    """an operand one double past a 16-byte boundary: the fused kernel's pair
    loads and stores cannot run, the separate kernels do (an unaligned rhs also
    takes the x pass to the two-sweep kernel)"""
    c = _Case(p, (2 * CHUNK[p] + 2, 9, 8), seed=70 + p)
    c.op.set_mass_seg_waves(0)
    c.check_stage("Y", fused_expected=False, x_v3_expected=operand != "rhs", shift=(operand,))
    if operand in ("rhs", "acc_in", "acc_out"):
        c.check_stage("noY", fused_expected=False, x_v3_expected=operand != "rhs", shift=(operand,))
    # the same operands aligned: fused (the shifted cases above fell back for the shift alone)
    c.check_stage("Y", fused_expected=True)


@pytest.mark.parametrize("p", [1, 9])
@pytest.mark.parametrize("vertices", [(96, 10, 11), (96, 40)])
def test_degrees_without_v3_kernel_are_not_fused(p, vertices):
    c = _Case(p, vertices, seed=90 + p)
    c.op.set_mass_seg_waves(0)
    for name in ("noY", "Y", "y_is_acc"):
        mode = MODES[name][0]
        acc_f, Y_f, path = _stage(c.op, True, *c.d, mode)
        assert path["rk_mode"] == 0 and not any(q["v3"] for q in path["passes"]), path
        assert [q["axis"] for q in path["passes"]] == list(range(len(vertices)))[::-1], path
        acc_ref, Y_ref = _stage_ref(c.k_ref, c.acc, c.y, mode)
        assert rel(host(acc_f), acc_ref) < RTOL
        if Y_ref is not None:
            assert rel(host(Y_f), Y_ref) < RTOL
        acc_s, Y_s, _ = _stage(c.op, False, *c.d, mode)
        assert torch.equal(acc_f, acc_s) and (Y_f is None or torch.equal(Y_f, Y_s))


# ---- 3. whole-line v3 kernels on long lines with few lines -----------------------------------------------------
# (dim, n_subdivisions, p): the shapes of test_gpu_mass_segments.py::test_segmented_solve_vs_kronecker and of
# test_gpu_parity.py::test_mass_solve_v3_long_lines.  Three of the former have an odd number of x vertices (401, 501,
# 251), which the v3 x kernel does not take: their long pass runs the two-sweep kernel at either threshold.  The
# same shapes with one subdivision less (an even x length) follow them, so every one has a case that reaches the
# v3 kernels.  (A 1D mesh's one direction is kernel axis 2, strided lines of either parity.)
LONG = [(2, (400, 30), 5), (2, (30, 400), 5), (1, (2000,), 3), (2, (500, 20), 7), (3, (250, 12, 9), 5)]
LONG += [(2, (399, 30), 5), (2, (499, 20), 7), (3, (249, 12, 9), 5)]
LONG += [(len(s), s, p) for s in [(499, 7, 8), (7, 433, 8), (7, 8, 601), (239, 190), (1023, 7), (8, 7, 145)]
         for p in (3, 5, 7)]


def _kernel_axes(dim):
    """kernel axes in launch order: 3D z, y, x; 2D y, x; the one direction of a 1D mesh is kernel axis 2"""
    return [2] if dim == 1 else [ax for ax in (2, 1, 0) if ax < dim]


def _expected_pass(axis, vertices, p, default_threshold):
    """(v3, segmented) of the pass along kernel axis `axis` as
    include/gdm_hip.h and csrc/gdm_mass.hip document the dispatch: x lines
    (kernel axis 0, contiguous) need an even length, strided lines more than
    one chunk; a pass of these few lines is segmented at the default threshold
    when its lines hold at least 4 chunks"""
    L, C = vertices[0 if len(vertices) == 1 else axis], CHUNK[p]
    v3 = L % 2 == 0 if axis == 0 else L > C
    return v3, v3 and default_threshold and -(-L // C) >= 4


@pytest.mark.parametrize("dim,n,p", LONG)
def test_whole_line_and_segmented_v3_on_long_lines(dim, n, p):
    g = _gdm()
    vertices = tuple(s + 1 for s in n)
    assert int(np.prod(vertices)) // min(vertices) < 64 * 1024  # every pass is below the default threshold
    op = g.GdmOperator(dim, p, n, -0.3, 1.1, "mass")
    m = O.Mesh(dim, p, list(n), -0.3, 1.1)
    r = np.random.default_rng(dim * 10 + p).uniform(-1, 1, m.n_dofs)
    ref = m.kron_mass_inverse(r)
    axes = _kernel_axes(dim)
    seg_counts = {}
    for waves in (0, -1):
        op.set_mass_seg_waves(waves)
        x = torch.full((m.n_dofs,), NAN, dtype=torch.float64, device="cuda")
        op.mass_solve(dev(r), x)
        path = op.mass_path()
        assert path["rk_mode"] == 0 and [q["axis"] for q in path["passes"]] == axes, path
        for q in path["passes"]:
            v3, segmented = _expected_pass(q["axis"], vertices, p, waves == -1)
            assert q["v3"] == v3 and (q["segments"] > 1) == bool(segmented), (waves, path)
            assert not (q["segments"] > 1 and q["in_place"]), path  # segments read their neighbours' input
        assert not path["passes"][0]["in_place"], path
        if waves == 0:  # rhs -> x, then in place
            assert all(q["in_place"] for q in path["passes"][1:]), path
        seg_counts[waves] = [q["segments"] for q in path["passes"]]
        got = host(x)
        assert rel(got, ref) < RTOL
        assert np.max(np.abs(got - ref)) < 1e-13 * np.max(np.abs(ref))
        y = dev(r)
        op.mass_solve(y, y)
        path = op.mass_path()
        if waves == 0:  # nothing is segmented: every pass runs in place, whole lines
            assert all(q["in_place"] and q["segments"] == 1 for q in path["passes"]), path
            assert [q["v3"] for q in path["passes"]] == [_expected_pass(ax, vertices, p, False)[0] for ax in axes]
            assert rel(host(y), ref) < RTOL
        else:  # rhs aliases the result: the first pass's input is moved aside, then the same launches
            assert [q["segments"] for q in path["passes"]] == seg_counts[-1], path
            assert np.array_equal(host(y), got)
    reaches_v3 = any(_expected_pass(ax, vertices, p, True)[1] for ax in axes)
    assert (seg_counts[0] != seg_counts[-1]) == reaches_v3, seg_counts
    # the shapes whose long pass cannot run the v3 kernel, exactly (see LONG)
    assert reaches_v3 == ((dim, n, p) not in [(2, (400, 30), 5), (2, (500, 20), 7), (3, (250, 12, 9), 5),
                                              (3, (8, 7, 145), 7)])


# ---- 4. the default dispatch at the smallest natural size ------------------------------------------------------
@pytest.fixture(scope="module")
def ops256():
    g = _gdm()
    ops = {}

    def get(p):
        if p not in ops:
            ops.clear()  # one 256^3 operator alive at a time
            ops[p] = g.GdmOperator(3, p, 255, 0.0, 1.0, "advection", params=(1.0, 0.15, -0.05))
        return ops[p]

    yield get
    ops.clear()


@pytest.mark.parametrize("p,name", [(3, "Y"), (5, "Y"), (5, "noY"), (5, "y_is_acc"), (7, "Y")])
def test_default_dispatch_256_cubed_is_fused(ops256, p, name):
    """256^3 vertices: 65536 lines = 1024 waves per pass, the smallest cube the
    default threshold leaves unsegmented -- the path of the headline benchmark.
    Bitwise against the separate kernels (no CPU reference at this size)."""
    op = ops256(p)
    mode, rkm = MODES[name]
    gen = torch.Generator(device="cuda").manual_seed(11)
    rhs, acc, y = (torch.rand(op.n_owned, dtype=torch.float64, device="cuda", generator=gen) - 0.5 for _ in range(3))
    acc_f, Y_f, path = _stage(op, True, rhs, acc, y, mode)
    assert path["rk_mode"] == rkm, path
    assert [(q["axis"], q["v3"], q["segments"]) for q in path["passes"]] == [(2, True, 1), (1, True, 1), (0, True, 1)]
    acc_s, Y_s, path_s = _stage(op, False, rhs, acc, y, mode)
    assert path_s["rk_mode"] == 0 and all(q["in_place"] and q["segments"] == 1 for q in path_s["passes"]), path_s
    assert torch.equal(acc_f, acc_s), float((acc_f - acc_s).abs().max())
    assert not bool(torch.isnan(acc_f).any())
    if Y_f is not None:
        assert torch.equal(Y_f, Y_s), float((Y_f - Y_s).abs().max())
        assert not bool(torch.isnan(Y_f).any())


# ---- 5. the CG's guards ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,p,n", [(1, 1, 4), (2, 3, 4)])
@pytest.mark.parametrize("precond", [0, 1])
def test_mass_solve_cg_stops_at_once_on_a_nan_rhs(dim, p, n, precond):
    """one NaN in rhs: the residual is not finite, gdm_mass_solve_cg returns
    GDM_ERR_STATE with its == 0 instead of iterating max_it = 50 times"""
    import ctypes

    from gdm_amd import _capi

    op = _gdm().GdmOperator(dim, p, n, 0.0, 1.0, "mass")
    b = np.ones(op.n_owned)
    b[op.n_owned // 2] = NAN
    rhs, x = dev(b), op.new_vector(local=False)
    its, res = ctypes.c_int(-1), ctypes.c_double(0.0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = op.lib.gdm_mass_solve_cg(op.h, ptr(rhs), ptr(x), 1e-8, 1e-10, 50, precond, ctypes.byref(its),
                                  ctypes.byref(res))
    assert rc == -5  # GDM_ERR_STATE
    assert its.value == 0
    assert "gdm_mass_solve_cg" in _capi.last_error() and "not finite" in _capi.last_error()
    assert np.isnan(res.value)
