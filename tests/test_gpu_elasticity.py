"""Linear elasticity on uncut boxes on the device (GDM_OP_ELASTICITY,
csrc/gdm_elasticity.hip) against tests/elasticity_ref.py, which
tests/test_elasticity_cpu.py pins to a dense assembly of the bilinear form and
to the reference's golden output.

Apply parity, p = 1 .. 9 in 2D and 3D, (mu, lambda) in {(1, 0), (0.7, 2.5)},
anisotropic boxes, random source (constrained entries included: those rows
must return the source value).  Meshes from the kernel's tile (T_x, T_y) and z
chunk Z_c of gdm_elasticity_tile:
    small   n_sub (p, p + 2, p + 3): all-wall, no Toeplitz interior;
    edges   nodes max(T + 1, 2p + 3) in x and y and max(Z_c + 2p + 1, 2p + 3) in
            z: one node more than a tile / than a chunk plus its 2p ring warm-up
            (33 x 9 x 19 at p = 1, 33 x 21 x 35 at p = 9);
    fit     the smallest multiples of (T_x, T_y, Z_c) the degree admits (n_sub
            >= p): 32 x 8 x 16 nodes up to p = 7, 32 x 16 x 16 at p = 9.
Bounds: rel-L2 <= 1e-12 and max-norm <= 1e-13 max|ref|, the project's stencil
bounds.
"""
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

import elasticity_ref as E
import fastdiag_ref as FR
import load_ref as LR
import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEGREES = (1, 3, 5, 7, 9)
PARAMS = ((1.0, 0.0), (0.7, 2.5))
BOX = {3: (FR.BOX_LO, FR.BOX_HI), 2: ((0.0, -1.0), (1.5, 0.2))}


def _tile(p, dim):
    from gdm_amd import _capi

    return _capi.elasticity_tile(p, dim)


def _nodes(kind, p, dim):
    tx, ty, zc = _tile(p, dim)
    if kind == "small":
        n = (p + 1, p + 3, p + 4)
    elif kind == "edges":
        n = (max(tx + 1, 2 * p + 3), max(ty + 1, 2 * p + 3), max(zc + 2 * p + 1, 2 * p + 3))
    else:
        n = tuple(t * -(-(p + 1) // t) for t in (tx, ty, zc))
    return n[:dim]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _mesh(dim, p, nodes):
    lo, hi = BOX[dim]
    return O.Mesh(dim, p, [n - 1 for n in nodes], list(lo), list(hi))


def _op(m, mu, lam):
    import gdm_amd

    dim = m.dim
    return gdm_amd.GdmOperator(dim, m.p, [int(m.nsub[d]) for d in range(dim)], [float(m.lo[d]) for d in range(dim)],
                               [float(m.hi[d]) for d in range(dim)], "elasticity", params=(mu, lam))


def test_mesh_extents():
    """the meshes sit where the docstring says, below ~50 x 30 x 50 nodes"""
    assert _tile(3, 3) == (32, 8, 16) and _tile(3, 2)[2] == 1
    assert _nodes("edges", 1, 3) == (33, 9, 19) and _nodes("edges", 9, 3) == (33, 21, 35)
    assert _nodes("fit", 7, 3) == (32, 8, 16) and _nodes("fit", 9, 3) == (32, 16, 16)
    for p in DEGREES:
        for kind in ("small", "edges", "fit"):
            n = _nodes(kind, p, 3)
            assert n[0] <= 50 and n[1] <= 30 and n[2] <= 50 and min(n) >= p + 1


@pytest.mark.parametrize("kind", ["small", "edges", "fit"])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("p", DEGREES)
def test_apply_parity(p, dim, kind):
    m = _mesh(dim, p, _nodes(kind, p, dim))
    n = m.n_dofs
    u = np.random.default_rng(10 * p + dim).uniform(-1, 1, dim * n)
    ud = _dev(u)
    constrained = np.tile(E.free_mask(m), dim) == 0
    for mu, lam in PARAMS:
        op = _op(m, mu, lam)
        y = op.new_vector_field()
        y.fill_(float("nan"))
        op.apply(ud, y)
        got = _host(y)
        ref = E.Operator(m, mu, lam)(u)
        rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        mx = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("%s %dD p %d nodes %s mu %g lambda %g: rel-L2 %.2e, max %.2e" % (kind, dim, p, _nodes(kind, p, dim), mu,
                                                                                lam, rel, mx))
        assert rel <= 1e-12
        assert mx <= 1e-13
        assert np.array_equal(got[constrained], u[constrained])
        y2 = op.new_vector_field()
        op.apply(ud, y2)
        assert torch.equal(y2, y)


@pytest.mark.parametrize("dim,p", [(2, 5), (3, 3)])
def test_bitwise_on_a_second_stream_and_in_a_graph_replay(dim, p):
    m = _mesh(dim, p, _nodes("edges", p, dim))
    op = _op(m, 0.7, 2.5)
    gen = torch.Generator(device="cuda").manual_seed(3)
    u = torch.rand(dim * m.n_dofs, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    ref = op.apply(u, op.new_vector_field())
    torch.cuda.synchronize()
    assert float(ref.abs().max()) > 0.0
    y = op.new_vector_field()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op.use_torch_stream()
        op.apply(u, y)
    torch.cuda.synchronize()
    assert torch.equal(y, ref)
    y.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
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


@pytest.mark.parametrize("dim,p,kind", [(2, 3, "edges"), (3, 5, "small"), (3, 1, "fit")])
def test_diagonal(dim, p, kind):
    m = _mesh(dim, p, _nodes(kind, p, dim))
    for mu, lam in PARAMS:
        got = _host(_op(m, mu, lam).elasticity_diagonal())
        ref = E.Operator(m, mu, lam).diagonal()
        err = float(np.abs(got / ref - 1.0).max())
        print("diagonal %dD p %d %s mu %g lambda %g: %.2e" % (dim, p, kind, mu, lam, err))
        assert err <= 1e-14


def _block_diagonal_sparse(m, mu, lam):
    """B = blockdiag_c(P A_cc P + I - P), sparse, from the helper's reduced 1D bands"""
    dim, p = m.dim, m.p
    w = E.weights(dim, mu, lam)
    bands = [E.bands_1d(m, d, reduced=True) for d in range(dim)]
    M = [scipy.sparse.csr_matrix(FR.dense_band(bands[d][0], p)) for d in range(dim)]
    L = [scipy.sparse.csr_matrix(FR.dense_band(bands[d][3], p)) for d in range(dim)]
    mask = E.free_mask(m)
    blocks = []
    for c in range(dim):
        B = scipy.sparse.diags(1.0 - mask)
        for d in range(dim):
            t = scipy.sparse.identity(1)
            for a in reversed(range(dim)):  # x fastest = the last Kronecker factor
                t = scipy.sparse.kron(t, L[a] if a == d else M[a])
            B = B + w[c][d] * t
        blocks.append(B)
    return scipy.sparse.block_diag(blocks, format="csc")


@pytest.mark.parametrize("dim,p,kind", [(2, 3, "edges"), (3, 3, "small"), (3, 5, "small"), (2, 7, "small")])
def test_preconditioner(dim, p, kind):
    """gdm_elasticity_precond against the helper; the bound is 20 x the helper's
    own error against a sparse direct solve of B on the same case"""
    m = _mesh(dim, p, _nodes(kind, p, dim))
    mask = np.tile(E.free_mask(m), dim)
    r = np.random.default_rng(p).uniform(-1, 1, dim * m.n_dofs) * mask
    for mu, lam in PARAMS:
        direct = scipy.sparse.linalg.spsolve(_block_diagonal_sparse(m, mu, lam), r)
        helper = E.BlockPreconditioner(m, mu, lam)(r)
        err_ref = FR.rel(helper, direct)
        op = _op(m, mu, lam)
        with pytest.raises(Exception, match="precond_setup"):
            op.elasticity_precond(_dev(r))
        op.elasticity_precond_setup()
        op.elasticity_precond_setup()
        z = op.elasticity_precond(_dev(r))
        got = _host(z)
        err = FR.rel(got, helper)
        print("precond %dD p %d %s mu %g lambda %g: device vs helper %.2e, helper vs direct (err_ref) %.2e, device vs "
              "direct %.2e" % (dim, p, kind, mu, lam, err, err_ref, FR.rel(got, direct)))
        assert err <= 20.0 * err_ref
        assert np.all(got[mask == 0] == 0.0)
        assert torch.equal(op.elasticity_precond(_dev(r)), z)


def _golden_line():
    with open(os.path.join(HERE, "golden", "elasticity_01.json")) as f:
        return json.load(f)["line"]


@functools.lru_cache(maxsize=None)
def _solve_reference(name):
    """(mesh, operator, b, {precond: its}) of a CG case, computed once"""
    case = [c for c in E.SOLVE_CASES if c[0] == name][0]
    _, dim, p, n, lo, hi, mu, lam, seed = case
    m = O.Mesh(dim, p, n, lo, hi)
    A = E.Operator(m, mu, lam)
    b = E.solve_case_rhs(m, seed)
    its = {pc: E.pcg(A, b, E.preconditioner(A, pc))[1] for pc in ("jacobi", "fastdiag")}
    return m, A, b, its


@pytest.mark.parametrize("name", [c[0] for c in E.SOLVE_CASES])
def test_solve(name):
    """iteration counts equal the helper's (its residuals are >= 1 % away from
    the threshold, tests/test_elasticity_cpu.py), and the true residual of the
    device's solution, through the numpy operator, is within 1.1 x threshold:
    the recursive residual drifts by O(eps cond its) ~ 1e-12 |b|, four orders
    below the threshold"""
    m, A, b, its_ref = _solve_reference(name)
    op = _op(m, A.mu, A.lam)
    tol = max(E.ABS_TOL, E.REL_TOL * np.linalg.norm(b))
    # a right-hand side with garbage on the constrained entries: they count as 0
    b_dirty = b + (1.0 - A.mask) * 3.0
    for pc in ("jacobi", "fastdiag"):
        x = op.new_vector_field()
        its, res = op.elasticity_solve(_dev(b_dirty), x, pc, E.REL_TOL, E.ABS_TOL, 1000)
        true_res = float(np.linalg.norm(b - A(_host(x))))
        print("%s %s: %d iterations (helper %d), |r| %.3e, true residual %.3e, threshold %.3e"
              % (name, pc, its, its_ref[pc], res, true_res, tol))
        assert its == its_ref[pc]
        assert true_res <= 1.1 * tol
        assert res <= tol


@pytest.mark.parametrize("precond", [0, 1, 2])
def test_solve_stops_at_once_on_a_nan_rhs(precond):
    """one NaN in rhs (on a free DoF): the residual is not finite, the solve
    returns GDM_ERR_STATE with its == 0 instead of iterating max_it = 50 times"""
    import ctypes

    from gdm_amd import _capi

    op = _op(_mesh(2, 1, (4, 4)), 1.0, 0.5)
    if precond == 2:
        op.elasticity_precond_setup()
    b = np.ones(2 * 16)
    b[5] = float("nan")  # vertex (1, 1) of component 0: interior
    rhs, x = _dev(b), op.new_vector_field()
    its, res = ctypes.c_int(-1), ctypes.c_double(0.0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = op.lib.gdm_elasticity_solve(op.h, ptr(rhs), ptr(x), precond, 1e-8, 1e-10, 50, ctypes.byref(its),
                                     ctypes.byref(res))
    assert rc == -5  # GDM_ERR_STATE
    assert its.value == 0
    assert "gdm_elasticity_solve" in _capi.last_error() and "not finite" in _capi.last_error()
    assert np.isnan(res.value)


def test_golden_case_end_to_end():
    """tests/elasticity_01_gdm.cc on the device: the right-hand side through
    gdm_add_load per component, the solve, gdm_error_norms_grid per component;
    the combined L2 error prints as the reference's line"""
    import gdm_amd

    g = E.GOLDEN
    m = O.Mesh(g["dim"], g["p"], g["n"])
    f, ex = E.golden_data(m)
    for pc, its_expected in (("jacobi", 73), ("fastdiag", 12)):
        op = _op(m, g["mu"], g["lam"])
        x, its, err = gdm_amd.solve_elasticity(op, f, exact=ex, precond=pc)
        line = "error : %g" % err
        print("golden %s: %d iterations, %s" % (pc, its, line))
        assert its == its_expected
        assert line == _golden_line()


@pytest.mark.parametrize("dim,p,nodes", [(2, 3, (33, 9)), (3, 1, (5, 4, 7))])
def test_interleave(dim, p, nodes):
    m = _mesh(dim, p, nodes)
    op = _op(m, 1.0, 0.0)
    u = np.random.default_rng(5).uniform(-1, 1, dim * m.n_dofs)
    ref = _host(op.interleave(_dev(u)))
    assert np.array_equal(ref, u.reshape(dim, -1).T.reshape(-1))
    back = _host(op.interleave(_dev(ref), to_reference=False))
    assert np.array_equal(back, u)
    assert np.array_equal(back, ref.reshape(-1, dim).T.reshape(-1))


@pytest.mark.parametrize("dim,p,n_sub", [(3, 3, (5, 4, 6)), (2, 5, (9, 7)), (1, 3, (11,))])
def test_error_norms_grid_equals_error_norms(dim, p, n_sub):
    """a sine product sampled on the Gauss grid against the built-in function on
    a wave operator: the same quadrature, so the three norms differ by the
    round-off of the function evaluation only"""
    import gdm_amd

    lo, hi = (-0.5, 0.0, 0.2)[:dim], (0.7, 0.9, 1.5)[:dim]
    m = O.Mesh(dim, p, list(n_sub), list(lo), list(hi))
    op = gdm_amd.GdmOperator(dim, p, n_sub, lo, hi, "wave")
    prm = [0.0, 0.0, 0.0, 1.0, 0.75, 1.25, 0.1, 0.4, -0.3]
    u = np.random.default_rng(6).uniform(-1, 1, m.n_dofs)
    ud = _dev(u)
    exq = LR.grid_values(m, LR.fn_sine_product(prm[0:3], prm[3:6], prm[6:9], 0.0, dim))
    ncell = int(np.prod(n_sub))
    ce1 = torch.zeros(ncell, dtype=torch.float64, device="cuda")
    ce2 = torch.zeros(ncell, dtype=torch.float64, device="cuda")
    a = op.error_norms(ud, op.FN_SINE_PRODUCT, prm, 0.0, ce1)
    b = op.error_norms_grid(ud, _dev(exq.reshape(-1)), ce2)
    print("%dD p %d: built-in %s, grid %s" % (dim, p, a, b))
    for va, vb in zip(a, b):
        assert abs(va - vb) <= 1e-13 * abs(va)
    assert float((ce1 - ce2).abs().max()) <= 1e-13 * float(ce1.abs().max())
