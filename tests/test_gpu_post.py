"""Device postprocess: gdm_error_norms vs the oracle.

Oracle: oracle/gdm_oracle.c gdmo_error_norms -- the cell loop of
integrate_difference (include/gdm/vector_tools.h:25-86) and of the volume part
of the advection postprocess (applications/advection/include/gdm/advection/
problem.h:330-425), whose L2 branch is pinned by the poisson_01 / mass_01
goldens (tests/test_oracle_golden.py).  The exact function is evaluated in
numpy at the oracle's cell quadrature points.

Tolerances: Linf, L1, L2 rel <= 1e-11 (summation order differs); per-cell L2
errors <= 1e-11 * max.  Multi-rank: the per-rank norms reduced as the
reference does (max, sum, sqrt of the sum of squares) equal the one-rank
norms to 1e-12.

The cases from test_error_norms_wraps_the_grid_stride_loop on reach what the
ones above leave out: a second trip through the kernel's grid-stride loop
(its LDS is reused across __syncthreads), every x-chunk edge, the largest LDS
launch, every function kind at every odd degree on a box with a different lo /
hi per direction, the grid kind on slabs, and a rank without cells.  Same
scheme and tolerances; their inputs and references come from
tests/post_ref.py, which reads the oracle's numbers for the 3D high-degree
meshes from tests/golden/error_norms_oracle.npz (the oracle's cell loop takes
up to a minute there) and calls the oracle for the rest.
"""
import numpy as np
import pytest

import oracle as O
import post_ref as PR
from post_ref import SINE, exact, field, reference  # noqa: F401  (tests/post_ref.py: shared with the recorded references)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


CASES = [
    (1, 3, 37, 2, SINE), (1, 9, 23, 1, [0.3, 0.4]), (2, 5, (19, 13), 2, SINE), (2, 1, 17, 0, [0.25]),
    (3, 3, (9, 7, 8), 2, SINE), (3, 5, (11, 9, 10), 1, [0.4, 0.1, 0.2, -0.3]), (3, 7, 9, 2, SINE),
    (3, 5, (70, 6, 6), 2, SINE),  # two x chunks of 64 cells
]


@pytest.mark.parametrize("dim,p,n,kind,prm", CASES)
def test_error_norms_vs_oracle(dim, p, n, kind, prm):
    import gdm_amd

    m = O.Mesh(dim, p, n, -0.5, 1.25)
    op = gdm_amd.GdmOperator(dim, p, n, -0.5, 1.25, "mass")
    t = 0.37
    u = field(m, kind, prm, t, seed=dim * 10 + p)
    (ref, ref_cells) = reference(m, u, kind, prm, t)
    cells = torch.zeros(op.n_owned_cells, dtype=torch.float64, device="cuda")
    got = op.error_norms(dev(u), kind, prm, t, cells)
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-11 * abs(r), (got, ref)
    c = host(cells)
    assert np.max(np.abs(c - ref_cells)) <= 1e-11 * np.max(ref_cells)


@pytest.mark.parametrize("dim,p,n,n_ranks", [(3, 5, (12, 10, 23), 3), (2, 3, (20, 17), 2), (1, 5, 41, 2)])
def test_error_norms_multi_rank(dim, p, n, n_ranks):
    """owned-cell norms of each rank's slab, reduced max / sum / sqrt(sum sq)
    (problem.h:410-425), reproduce the one-rank norms; cell errors tile."""
    import gdm_amd

    m = O.Mesh(dim, p, n)
    u = field(m, 2, SINE, 0.1, seed=7)
    one = gdm_amd.GdmOperator(dim, p, n, 0.0, 1.0, "mass")
    ref = one.error_norms(dev(u), 2, SINE, 0.1)
    ref_cells = torch.zeros(one.n_owned_cells, dtype=torch.float64, device="cuda")
    one.error_norms(dev(u), 2, SINE, 0.1, ref_cells)
    linf, l1, l2sq, cells = 0.0, 0.0, 0.0, []
    for r in range(n_ranks):
        op = gdm_amd.GdmOperator(dim, p, n, 0.0, 1.0, "mass", n_ranks=n_ranks, rank=r)
        L = op.layout
        first = (L["owned_plane_begin"] - L["ghost_planes_below"]) * L["plane_size"]
        loc = dev(u[first:first + op.n_local])
        c = torch.zeros(max(op.n_owned_cells, 1), dtype=torch.float64, device="cuda")
        e = op.error_norms(loc, 2, SINE, 0.1, c if op.n_owned_cells else None)
        linf, l1, l2sq = max(linf, e[0]), l1 + e[1], l2sq + e[2] ** 2
        cells.append(host(c)[:op.n_owned_cells])
    assert abs(linf - ref[0]) <= 1e-14 * ref[0]
    assert abs(l1 - ref[1]) <= 1e-12 * ref[1]
    assert abs(np.sqrt(l2sq) - ref[2]) <= 1e-12 * ref[2]
    np.testing.assert_allclose(np.concatenate(cells), host(ref_cells), rtol=0, atol=1e-15 * float(ref[0]) + 1e-300)


def test_error_norms_convergence_full_size():
    """Size-independent property at a C3-class size: the GDM vertex interpolant
    of a smooth function converges at O(h^(p+1)) in L2 (p = 5: factor ~64 per
    halving); the device evaluation sees it on 64^3 -> 128^3 -> 256^3 cells."""
    import gdm_amd

    prm = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.3, 0.1, 0.2]
    errs = []
    for n in (32, 64, 128):
        op = gdm_amd.GdmOperator(3, 5, n, 0.0, 1.0, "mass")
        x = torch.linspace(0.0, 1.0, n + 1, dtype=torch.float64, device="cuda")
        sx = torch.sin(2 * np.pi * x + 0.3)
        sy = torch.sin(2 * np.pi * x + 0.1)
        sz = torch.sin(2 * np.pi * x + 0.2)
        u = (sz[:, None, None] * sy[None, :, None] * sx[None, None, :]).reshape(-1).contiguous()
        errs.append(op.error_norms(u, 2, prm, 0.0))
    for a, b in zip(errs, errs[1:]):
        assert 40.0 < a[2] / b[2] < 90.0, errs
        assert 40.0 < a[1] / b[1] < 90.0, errs


# ---- where the kernel can go wrong ----------------------------------------------------------------------------
def _check_case(dim, p, n, kind, with_and_without_cells=False):
    """one case of tests/post_ref.py against the oracle: the three norms rel
    1e-11, the cell errors 1e-11 * max (the tolerances of
    test_error_norms_vs_oracle).  Returns the operator and the device field."""
    import gdm_amd

    m, u, ref, ref_cells = PR.case_reference(dim, p, n, kind)
    op = gdm_amd.GdmOperator(dim, p, n, PR.LO[:dim], PR.HI[:dim], "mass")
    assert op.n_owned_cells == m.n_cells
    prm = PR.kind_params(kind, dim)
    ud = dev(u)
    cells = torch.full((m.n_cells,), float("nan"), dtype=torch.float64, device="cuda")
    if kind == PR.KIND_GRID:
        xq = m.cell_qpoints()
        # the reordering itself: in the grid layout, coordinate d varies along grid axis d only
        n1 = p + 1
        Q = [int(m.nsub[d]) * n1 if d < dim else 1 for d in range(3)]
        for d in range(dim):
            X = PR.grid_layout(m, xq[:, d]).reshape(Q[2], Q[1], Q[0])
            line = np.moveaxis(X, 2 - d, 0).reshape(Q[d], -1)
            assert np.all(line == line[:, :1]) and np.all(np.diff(line[:, 0]) > 0)
        exq = dev(PR.grid_layout(m, exact(kind, prm, xq, PR.T, dim)))
        call = lambda c: op.error_norms_grid(ud, exq, c)  # noqa: E731
    else:
        call = lambda c: op.error_norms(ud, kind, prm, PR.T, c)  # noqa: E731
    got = call(cells)
    print("%dD p %d n %s kind %d: device %s oracle %s" % (dim, p, n, kind, got, ref))
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-11 * abs(r), (got, ref)
    assert np.max(np.abs(host(cells) - ref_cells)) <= 1e-11 * np.max(ref_cells)
    if with_and_without_cells:
        # the kernel has one more barrier per work item when it stores the cell errors: the norms do not depend on it
        assert call(None) == got
    return op, ud


@pytest.mark.parametrize("dim,p,n", PR.WRAP_CASES)
def test_error_norms_wraps_the_grid_stride_loop(dim, p, n):
    """more than 2 * 1024 work items (gdm_op::n_err_partial = 1024 workgroups):
    every workgroup takes a second or third trip through the item loop and
    reuses its LDS; with and without cell errors, the same bits"""
    assert -(-n[0] // 64) * int(np.prod(n[1:])) > 2 * 1024
    _check_case(dim, p, n, 2, with_and_without_cells=True)


@pytest.mark.parametrize("dim,p,n", PR.CHUNK_CASES)
def test_error_norms_x_chunk_edges(dim, p, n):
    """63 / 64 / 65 / 128 / 129 cells along x: a chunk of 64 cells short by
    one, full, followed by a single cell; the same for two chunks"""
    _check_case(dim, p, n, 2, with_and_without_cells=True)


def test_error_norms_largest_lds_launch():
    """3D p = 9: about 131 KB of dynamic LDS, the largest launch"""
    import ctypes

    import gdm_amd

    dim, p, n = PR.LARGEST_LDS
    lds_bytes = gdm_amd.load().gdmk_error_norms_lds_bytes
    lds_bytes.restype, lds_bytes.argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]
    assert 128 * 1024 < lds_bytes(p, dim) <= 160 * 1024
    assert lds_bytes(7, 3) > 64 * 1024 >= lds_bytes(5, 3)  # the wrap cases sit on both sides of the attribute path
    _check_case(dim, p, n, 2, with_and_without_cells=True)


@pytest.mark.parametrize("dim,p,n,kind", PR.KIND_CASES)
def test_error_norms_every_kind_at_every_degree(dim, p, n, kind):
    """constant, cone (rim inside cells, centre off the grid), sine product and
    the grid kind (gdm_error_norms_grid) at p = 1 .. 9 on a non-cubic mesh of
    a box with a different lo / hi per direction"""
    _check_case(dim, p, n, kind)


@pytest.mark.parametrize("dim,p,n,n_ranks", [(3, 5, (12, 10, 23), 3), (2, 3, (20, 17), 2), (1, 5, 41, 2)])
def test_error_norms_grid_multi_rank(dim, p, n, n_ranks):
    """gdm_error_norms_grid on slabs (the partitions of
    test_error_norms_multi_rank): every rank takes the whole mesh's exact_q
    and its own local field; the reduced norms equal the one-rank call to the
    1e-14 (max) / 1e-12 (sums) of that test, the cell errors tile"""
    import gdm_amd

    m = O.Mesh(dim, p, n)
    u = field(m, PR.KIND_GRID, [], 0.0, seed=7)
    exq = dev(PR.grid_layout(m, exact(PR.KIND_GRID, [], m.cell_qpoints(), 0.0, dim)))
    one = gdm_amd.GdmOperator(dim, p, n, 0.0, 1.0, "mass")
    ref_cells = torch.zeros(one.n_owned_cells, dtype=torch.float64, device="cuda")
    ref = one.error_norms_grid(dev(u), exq, ref_cells)
    assert all(v > 0.0 for v in ref)
    linf, l1, l2sq, cells = 0.0, 0.0, 0.0, []
    for r in range(n_ranks):
        op = gdm_amd.GdmOperator(dim, p, n, 0.0, 1.0, "mass", n_ranks=n_ranks, rank=r)
        L = op.layout
        first = (L["owned_plane_begin"] - L["ghost_planes_below"]) * L["plane_size"]
        c = torch.zeros(op.n_owned_cells, dtype=torch.float64, device="cuda")
        e = op.error_norms_grid(dev(u[first:first + op.n_local]), exq, c)
        linf, l1, l2sq = max(linf, e[0]), l1 + e[1], l2sq + e[2] ** 2
        cells.append(host(c))
    assert abs(linf - ref[0]) <= 1e-14 * ref[0]
    assert abs(l1 - ref[1]) <= 1e-12 * ref[1]
    assert abs(np.sqrt(l2sq) - ref[2]) <= 1e-12 * ref[2]
    np.testing.assert_allclose(np.concatenate(cells), host(ref_cells), rtol=0, atol=1e-15 * float(ref[0]) + 1e-300)


def test_error_norms_on_a_rank_without_cells():
    """5 cell planes on 4 ranks: distributed.slab gives rank 3 no cell and no
    plane.  Its norms are (0, 0, 0) -- the neutral elements of the reduction --
    and nothing is written, for the built-in and the grid kind"""
    import gdm_amd
    from gdm_amd.distributed import slab

    dim, p, n, n_ranks, r = 2, 3, (20, 5), 4, 3
    assert slab(n[-1], n_ranks, r) == (6, 6, 5, 5)
    op = gdm_amd.GdmOperator(dim, p, n, 0.0, 1.0, "mass", n_ranks=n_ranks, rank=r)
    assert op.n_owned_cells == 0 and op.n_local == 0 and op.n_owned == 0
    guard = torch.full((4,), -7.25e33, dtype=torch.float64, device="cuda")
    u, cells = guard[1:1], guard[3:3]
    m = O.Mesh(dim, p, n)
    exq = dev(PR.grid_layout(m, exact(PR.KIND_GRID, [], m.cell_qpoints(), 0.0, dim)))
    assert op.error_norms(u, 2, SINE, 0.1, cells) == (0.0, 0.0, 0.0)
    assert op.error_norms(u, 2, SINE, 0.1) == (0.0, 0.0, 0.0)
    assert op.error_norms_grid(u, exq, cells) == (0.0, 0.0, 0.0)
    assert np.all(host(guard) == -7.25e33)
