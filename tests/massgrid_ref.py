"""TEST INFRASTRUCTURE ONLY: the numpy side of the grid-density solver tests
(tests/test_massgrid_cpu.py pins the counts, tests/test_gpu_massgrid_solve.py
compares the engine against them).  Dense M[rho] from tests/varmass_ref.py, dense
K[kappa] from tests/vardiff_ref.py, the engine's preconditioners restated with
numpy, and the restatement's PCG at rel_tol 1e-8.

Densities on [0, 1]^dim, p = 3:
  osc      2 + sin(3xy + 2z) + 0.5 cos(5(x - yz)) (the kappa of
           tests/test_gpu_coefgrid.py; 2D: z dropped), in [0.5, 3.5];
  ellipse  1 + 9 exp(-(|y|^2 + y_0 y_1) / 0.15^2), y = x - 1/2: contrast 10, a
           tilted ellipse, not separable.
"""
import functools

import numpy as np

import oracle as O
import vardiff_ref as RD
import varmass_ref as R
from varfield_ref import BATCH, _Cells, _tables
from varmass_ref import MAX_IT

P = 3
NITSCHE = 6.0 * P * P
ALPHA, TAU = 1.0, 0.01
MASS_CASES = [(2, 24), (3, 8)]
SYSTEM_CASES = [(2, 24), (3, 8)]
SYSTEM_KAPPAS = ("none", "separable", "grid")


def osc(dim):
    if dim == 3:
        return lambda x: 2 + np.sin(3 * x[:, 0] * x[:, 1] + 2 * x[:, 2]) + 0.5 * np.cos(5 * (x[:, 0] - x[:, 1] * x[:, 2]))
    if dim == 2:
        return lambda x: 2 + np.sin(3 * x[:, 0] * x[:, 1]) + 0.5 * np.cos(5 * x[:, 0])
    return lambda x: 2 + np.sin(3 * x[:, 0]) + 0.5 * np.cos(5 * x[:, 0])


def ellipse(dim):
    def rho(x):
        y = x[:, :dim] - 0.5
        return 1.0 + 9.0 * np.exp(-((y * y).sum(axis=1) + y[:, 0] * y[:, 1]) / 0.15 ** 2)

    return rho


DENSITIES = {"osc": osc, "ellipse": ellipse}


def kappa_terms(dim, amp=9.0, width=0.2):
    """the separable kappa of tests/test_gpu_varmass_solve.py: 1 + amp prod_d b(x_d)"""
    b = lambda s: np.exp(-((s - 0.5) / width) ** 2)  # noqa: E731
    return [[None] * dim, [lambda s: amp * b(s)] + [b] * (dim - 1)]


def rhs_of(m):
    """M applied to a smooth function plus a rough part: every mode is present
    (rhs_of of tests/test_gpu_varmass_solve.py)"""
    X = m.vertex_coords()
    rng = np.random.default_rng(m.n_dofs)
    f = np.prod([np.sin(2.3 * X[d] + 0.4 * d) for d in range(m.dim)], axis=0) + 0.3 * rng.uniform(-1, 1, m.n_dofs)
    M = [m.matrices_1d(d)[0] for d in range(m.dim)]
    return m.kron_apply([tuple(M)], f)


def stable(solve, b, rel_tol=1e-8):
    """numpy PCG whose count is not borderline (_stable of
    tests/test_gpu_varmass_solve.py): (x, its, margin), margin the smallest
    relative distance of a residual from the threshold"""
    x, its, hist = solve(b)
    tol = rel_tol * hist[0]
    margin = min(abs(h - tol) / tol for h in hist)
    assert margin > 1e-6, (its, hist[-2:], tol)
    rng = np.random.default_rng(1)
    _, its2, _ = solve(b * (1.0 + 1e-12 * rng.uniform(-1, 1, b.size)))
    assert its2 == its
    return x, its, margin


def gauss_mean(m, f):
    """the Gauss-weighted domain mean of a pointwise function: sum_q w_q f(x_q) /
    volume = 1^T M[f] 1 / volume (the basis is a partition of unity)"""
    vol = float(np.prod([float(m.hi[d]) - float(m.lo[d]) for d in range(m.dim)]))
    return float(R.mass_apply(m, f, np.ones(m.n_dofs)).sum()) / vol


def mass_diag(m, rho):
    """diag(M[rho])_i = sum_q w_q rho(x_q) prod_d phi_{i_d}(x_q)^2 by the cell loop
    of varmass_ref.mass_apply with the forward sweeps left out and the squared
    tables in the transposed ones (test_massgrid_cpu pins it to the diagonal of
    the dense matrix)"""
    dim, n1 = m.dim, m.p + 1
    xq, wq, V, _, _ = _tables(m.p)
    cells = _Cells(m)
    shape = (n1,) * dim
    w = np.ones(())
    for d in range(dim):
        w = np.multiply.outer(wq * float(m.h[d]), w) if d else wq * float(m.h[0])
    out = np.zeros(m.n_dofs)
    for b in range(0, m.n_cells, BATCH):
        sl = slice(b, min(m.n_cells, b + BATCH))
        n = sl.stop - sl.start
        f = np.asarray(rho(RD._qpoints(m, cells, sl, xq))).reshape((n,) + shape) * w
        for d in range(dim):
            f = RD._to_i(f, V[cells.cat[d][sl]] ** 2, d, dim)
        np.add.at(out, cells.dofs[sl].reshape(-1), f.reshape(-1))
    return out


@functools.lru_cache(maxsize=None)
def mesh(dim, n):
    return O.Mesh(dim, P, n)


@functools.lru_cache(maxsize=None)
def unit_mass(dim, n):
    """(M dense, M^-1)"""
    M = R.kron_dense(mesh(dim, n), [[None] * dim])
    return M, np.linalg.inv(M)


@functools.lru_cache(maxsize=None)
def dense_mass(dim, n, name):
    A = R.dense_matrix(mesh(dim, n), DENSITIES[name](dim))
    A.setflags(write=False)
    return A


def mass_precond(dim, n, name):
    """r -> W^-1/2 M^-1 W^-1/2 r, W = diag(M[rho]) / diag(M) from the dense diagonals"""
    M, Minv = unit_mass(dim, n)
    wis = 1.0 / np.sqrt(np.diag(dense_mass(dim, n, name)) / np.diag(M))
    return lambda r: wis * (Minv @ (wis * r))


@functools.lru_cache(maxsize=None)
def cpu_mass_solve(dim, n, name, precond_name=None):
    """(A, b, x, its, margin) of M[rho] x = b; precond_name: the density whose W
    the preconditioner uses (None: the density itself)"""
    A = dense_mass(dim, n, name)
    b = rhs_of(mesh(dim, n))
    Pinv = mass_precond(dim, n, precond_name or name)
    x, its, margin = stable(lambda v: RD.pcg(lambda y: A @ y, Pinv, v, rel_tol=1e-8, max_it=1000), b)
    return A, b, x, its, margin


def system_kappa(dim, kind):
    """(pointwise kappa or None, separable terms or None)"""
    if kind == "none":
        return None, None
    if kind == "separable":
        return R.pointwise(kappa_terms(dim), dim), kappa_terms(dim)
    return osc(dim), None


@functools.lru_cache(maxsize=None)
def cpu_system_solve(dim, n, kind):
    """(apply, b, x, its, margin) of (alpha M[rho] - tau K[kappa]) x = b, rho =
    ellipse on the grid, preconditioned by (alpha mean(rho) M - tau mean(kappa) K_0)^-1"""
    m = mesh(dim, n)
    Mrho = dense_mass(dim, n, "ellipse")
    M, K0 = RD.homogeneous_matrices(m, NITSCHE)
    kappa, _ = system_kappa(dim, kind)
    K = K0 if kappa is None else RD.dense_matrix(m, kappa, NITSCHE)
    kbar = 1.0 if kappa is None else gauss_mean(m, kappa)
    Pinv = np.linalg.inv(ALPHA * gauss_mean(m, ellipse(dim)) * M - TAU * kbar * K0)
    A = ALPHA * Mrho - TAU * K
    b = rhs_of(m)
    x, its, margin = stable(lambda v: RD.pcg(lambda y: A @ y, lambda r: Pinv @ r, v, rel_tol=1e-8), b)
    return (lambda y: A @ y), b, x, its, margin


# the counts of the recipe above (pinned by tests/test_massgrid_cpu.py)
MASS_ITS = {(2, 24, "osc"): 4, (2, 24, "ellipse"): 5, (3, 8, "osc"): 6, (3, 8, "ellipse"): 8}
assert max(MASS_ITS.values()) <= MAX_IT / 2
