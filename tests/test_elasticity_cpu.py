"""Linear elasticity with zero boundary constraints, host side (no GPU):

(a) the Kronecker form of tests/elasticity_ref.py against a dense assembly
    written directly from the bilinear form 2 mu (eps(u), eps(v)) + lambda
    (div u, div v) by cell quadrature (oracle.basis_value, oracle.gauss); both
    use QGauss(p+1), so they differ by round-off only (~1e-15 measured);
(b) symmetry of the operator;
(c) the host tables behind the ABI (gdm_elasticity_tables_1d) against the
    helper: the bands entry-wise, the eigen tables through S diag(lambda) S^T M
    = L on the interior and S^T M S = I;
(d) the golden case of tests/elasticity_01_gdm.cc: the printed error and the
    iteration counts 73 (Jacobi) and 12 (block fast diagonalisation);
(e) every CG case of the GPU test keeps its residual at the stopping iteration
    and at the one before at least 1 % away from the threshold, and its history
    does not move under 1e-12 perturbations of the right-hand side, so that
    the device's iteration count cannot differ by round-off.
"""
import itertools
import json
import os

import numpy as np
import pytest

import elasticity_ref as E
import fastdiag_ref as FR
import oracle as O

from gdm_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))


def golden_line():
    with open(os.path.join(HERE, "golden", "elasticity_01.json")) as f:
        return json.load(f)


def dense_assembly(mesh, mu, lam):
    """A[(c, i), (e, j)] = a(phi_j e_e, phi_i e_c), component-major, by cell quadrature"""
    dim, p, n1 = mesh.dim, mesh.p, mesh.p + 1
    xq, wq = O.gauss(n1)
    n = mesh.n_dofs
    stride = [int(np.prod(mesh.N[:d])) for d in range(dim)]
    A = np.zeros((dim * n, dim * n))
    nsub = [int(mesh.nsub[d]) for d in range(dim)]
    for cell in itertools.product(*[range(nsub[d]) for d in reversed(range(dim))]):
        cidx = cell[::-1]  # by direction
        V, D, off = [], [], []
        for d in range(dim):
            cat = int(O.lib().gdmo_category(cidx[d], p, nsub[d]))
            off.append(int(O.lib().gdmo_offset(cidx[d], p, nsub[d])))
            V.append(np.array([[O.basis_value(p, cat, i, x, 0) for x in xq] for i in range(n1)]))
            D.append(np.array([[O.basis_value(p, cat, i, x, 1) for x in xq] for i in range(n1)]) / float(mesh.h[d]))
        # local functions / points as flat tensors, direction 0 fastest
        def tensor(fs):
            t = fs[0]
            for d in range(1, dim):
                t = np.einsum("iq,jr->jirq", t, fs[d]).reshape(t.shape[0] * n1, t.shape[1] * n1)
            return t
        G = [tensor([D[a] if a == d else V[a] for a in range(dim)]) for d in range(dim)]
        jxw = np.ones(1)
        for d in range(dim):
            jxw = np.multiply.outer(wq * float(mesh.h[d]), jxw).reshape(-1)
        dofs = np.zeros(1, dtype=np.int64)
        for d in range(dim):
            dofs = (np.add.outer((off[d] + np.arange(n1)) * stride[d], dofs)).reshape(-1)
        GG = [[(G[a] * jxw) @ G[b].T for b in range(dim)] for a in range(dim)]  # GG[a][b][I, J] = sum_q G_a[I] G_b[J] JxW
        for c in range(dim):
            for e in range(dim):
                blk = mu * GG[e][c] + lam * GG[c][e]
                if c == e:
                    blk = blk + mu * sum(GG[d][d] for d in range(dim))
                A[np.ix_(c * n + dofs, e * n + dofs)] += blk
    return A


DENSE_MESHES = [
    ("2d-p1", 2, 1, (1, 3), (-0.5, 0.0), (0.7, 0.9)),
    ("2d-p3", 2, 3, (3, 5), (-0.5, 0.0), (0.7, 0.9)),
    ("3d-p1", 3, 1, (1, 2, 3), (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)),
]


@pytest.mark.parametrize("name,dim,p,n_sub,lo,hi", DENSE_MESHES, ids=[c[0] for c in DENSE_MESHES])
@pytest.mark.parametrize("mu,lam", [(1.0, 0.0), (0.7, 2.5)])
def test_kronecker_form_equals_dense_assembly(name, dim, p, n_sub, lo, hi, mu, lam):
    m = O.Mesh(dim, p, list(n_sub), list(lo), list(hi))
    A = dense_assembly(m, mu, lam)
    K = E.Operator(m, mu, lam, reduced=False).dense()
    err = np.linalg.norm(K - A) / np.linalg.norm(A)
    # the constrained form: P A P + I - P of the same dense matrix
    mask = np.tile(E.free_mask(m), dim)
    Ar = mask[:, None] * A * mask[None, :] + np.diag(1.0 - mask)
    Kr = E.Operator(m, mu, lam, reduced=True).dense()
    err_r = np.linalg.norm(Kr - Ar) / np.linalg.norm(Ar)
    sym = np.linalg.norm(Kr - Kr.T) / np.linalg.norm(Kr)
    dg = np.abs(E.Operator(m, mu, lam).diagonal() - np.diag(Ar)).max() / np.abs(np.diag(Ar)).max()
    print("%s mu %g lambda %g: Kronecker vs dense %.2e, constrained %.2e, asymmetry %.2e, diagonal %.2e"
          % (name, mu, lam, err, err_r, sym, dg))
    assert err <= 1e-13
    assert err_r <= 1e-13
    assert sym <= 1e-14
    assert dg <= 1e-14


def test_operator_is_symmetric_and_definite_on_free_dofs():
    m = O.Mesh(3, 3, [3, 5, 6], [-0.5, 0.0, 0.2], [0.7, 0.9, 1.5])
    A = E.Operator(m, 0.7, 2.5)
    rng = np.random.default_rng(1)
    u, v = rng.uniform(-1, 1, (2, 3 * m.n_dofs))
    a, b = float(v @ A(u)), float(u @ A(v))
    print("v^T A u %.15e, u^T A v %.15e" % (a, b))
    assert abs(a - b) <= 1e-13 * max(abs(a), abs(b), np.linalg.norm(u) * np.linalg.norm(A(v)))
    assert float(u @ A(u)) > 0.0


def _desc(m):
    d = _capi.mesh_desc(m.dim, m.p, [int(m.nsub[e]) for e in range(m.dim)])
    for e in range(m.dim):
        d.lo[e], d.hi[e] = float(m.lo[e]), float(m.hi[e])
    return d


TABLE_MESHES = [("3d-p%d" % p, 3, p, FR.small_n_sub(p), FR.BOX_LO, FR.BOX_HI) for p in (1, 3, 5, 7, 9)] + [
    ("2d-p3-40", 2, 3, (40, 40), (0.0, 0.0), (1.0, 1.0)), ("2d-p1-1", 2, 1, (1, 2), (0.0, 0.0), (1.0, 1.0))]


@pytest.mark.parametrize("name,dim,p,n_sub,lo,hi", TABLE_MESHES, ids=[c[0] for c in TABLE_MESHES])
def test_host_tables_against_helper(name, dim, p, n_sub, lo, hi):
    m = O.Mesh(dim, p, list(n_sub), list(lo), list(hi))
    desc = _desc(m)
    for d in range(dim):
        bands, S, lam = _capi.elasticity_tables_1d(desc, d)
        bands2, S2, lam2 = _capi.elasticity_tables_1d(desc, d)
        assert bands.tobytes() == bands2.tobytes() and S.tobytes() == S2.tobytes() and lam.tobytes() == lam2.tobytes()
        ref = E.bands_1d(m, d, reduced=True)
        for f, name_f in enumerate(("M", "C", "C^T", "L")):
            scale = np.abs(ref[f]).max()
            e = np.abs(bands[f] - ref[f]).max() / (scale if scale > 0 else 1.0)
            print("%s axis %d band %s: %.2e" % (name, d, name_f, e))
            assert e <= 1e-14
        N = m.N[d]
        assert np.all(S[0] == 0.0) and np.all(S[-1] == 0.0) and np.all(S[:, 0] == 0.0) and np.all(S[:, -1] == 0.0)
        assert lam[0] == 1.0 and lam[-1] == 1.0
        if N <= 2:
            continue
        M = FR.dense_band(ref[0], p)[1:-1, 1:-1]
        L = FR.dense_band(ref[3], p)[1:-1, 1:-1]
        Si, li = S[1:-1, 1:-1], lam[1:-1]
        lmax = np.abs(li).max()
        orth = np.abs(Si.T @ M @ Si - np.eye(N - 2)).max()
        diag = np.abs(Si.T @ L @ Si - np.diag(li)).max() / lmax
        # S diag(lambda) S^T = M^-1 L M^-1, i.e. M S diag(lambda) S^T M = L
        recon = np.abs(M @ Si @ np.diag(li) @ Si.T @ M - L).max() / np.abs(L).max()
        lr = E.interior_eigenpairs(m)[d][1][1:-1]
        e_lam = np.abs(np.sort(li) - lr).max() / lmax
        print("%s axis %d N %d: lambda %.2e  S^T M S - I %.2e  S^T L S - Lambda %.2e  M S Lambda S^T M - L %.2e"
              % (name, d, N, e_lam, orth, diag, recon))
        assert np.all(li > 0.0)
        assert e_lam <= 1e-11 and orth <= 1e-11 and diag <= 1e-11 and recon <= 1e-11


def test_host_table_argument_checks():
    import ctypes

    lib = _capi.load()
    m = _desc(O.Mesh(2, 3, [3, 5]))
    b = np.zeros((4, 4, 7))
    pb = b.ctypes.data_as(ctypes.c_void_p)
    assert lib.gdm_elasticity_tables_1d(None, 0, pb, None, None) == -1
    assert lib.gdm_elasticity_tables_1d(ctypes.byref(m), 2, pb, None, None) == -1
    S = np.zeros((4, 4))
    assert lib.gdm_elasticity_tables_1d(ctypes.byref(m), 0, pb, S.ctypes.data_as(ctypes.c_void_p), None) == -1
    assert lib.gdm_elasticity_tables_1d(ctypes.byref(m), 0, pb, None, None) == _capi.GDM_OK
    t = [ctypes.c_int(0) for _ in range(3)]
    assert lib.gdm_elasticity_tile(3, 1, *[ctypes.byref(v) for v in t]) == -1
    assert lib.gdm_elasticity_tile(4, 3, *[ctypes.byref(v) for v in t]) == -3
    assert _capi.elasticity_tile(3, 2)[2] == 1


@pytest.fixture(scope="module")
def golden_case():
    g = E.GOLDEN
    m = O.Mesh(g["dim"], g["p"], g["n"])
    f, ex = E.golden_data(m)
    return m, E.Operator(m, g["mu"], g["lam"]), E.load_rhs(m, f), ex


@pytest.mark.parametrize("precond,its_expected", [("jacobi", 73), ("fastdiag", 12)])
def test_golden_case(golden_case, precond, its_expected):
    m, A, b, ex = golden_case
    x, its, hist, tol = E.pcg(A, b, E.preconditioner(A, precond))
    err = E.l2_error(m, x, ex)
    line = "error : %g" % err
    print("%s: %d iterations, %s, residual %.3e / threshold %.3e, margin %.1f %%"
          % (precond, its, line, hist[-1], tol, 100 * E.threshold_margin(hist, tol)))
    assert its == its_expected
    assert line == golden_line()["line"]


@pytest.mark.parametrize("case", E.SOLVE_CASES, ids=[c[0] for c in E.SOLVE_CASES])
@pytest.mark.parametrize("precond", ["jacobi", "fastdiag"])
def test_gpu_solve_cases_are_away_from_the_threshold(case, precond):
    name, dim, p, n, lo, hi, mu, lam, seed = case
    m = O.Mesh(dim, p, n, lo, hi)
    A = E.Operator(m, mu, lam)
    b = E.solve_case_rhs(m, seed)
    x, its, hist, tol = E.pcg(A, b, E.preconditioner(A, precond))
    margin = E.threshold_margin(hist, tol)
    true_res = np.linalg.norm(b - A(x))
    print("%s %s: %d iterations, |r| %.3e (true %.3e), threshold %.3e, margin %.1f %%"
          % (name, precond, its, hist[-1], true_res, tol, 100 * margin))
    assert margin >= 0.01
    assert true_res <= 1.1 * tol
    # round-off must not decide the count: 1e-12 relative perturbations of b (four orders above what a different
    # summation order does) leave the count and the last two residuals (to 1e-3) as they are
    for k in (1, 2):
        bp = b * (1.0 + 1e-12 * np.random.default_rng(100 + k).uniform(-1, 1, b.size))
        _, its_p, hist_p, _ = E.pcg(A, bp, E.preconditioner(A, precond))
        drift = max(abs(hist_p[-1] / hist[-1] - 1.0), abs(hist_p[-2] / hist[-2] - 1.0)) if its_p == its else np.inf
        print("  perturbed %d: %d iterations, last residuals moved by %.1e" % (k, its_p, drift))
        assert its_p == its and drift <= 1e-3
