"""TEST INFRASTRUCTURE ONLY: the mass matrix of the reference weighted by an
arbitrary pointwise density rho(x) -- a numpy restatement of the cell loop of
wave/mass.h:47-249 with every JxW(q) multiplied by rho at the quadrature point:

  (M[rho] u)_i = sum_cells sum_q w_q rho(x_q) phi_i(x_q) sum_j phi_j(x_q) u_j

Built like tests/vardiff_ref.py from what oracle/oracle.py exports: the cells
are processed in batches with the tensor-product shape functions applied
direction by direction.  tests/test_varmass_cpu.py pins it to the oracle's mass
matrix for rho = 1 and to the Kronecker sum of the engine's 1D bands.

A density is a callable rho(x): x of shape (n, 3) -> (n,).  A separable one is a
list of terms, each a list of per-direction callables of one coordinate / None.
"""
import numpy as np

import oracle as O
from varfield_ref import BATCH, _Cells, _tables
from vardiff_ref import _qpoints, _to_i, _to_q, kron_matrix, pcg  # noqa: F401  (pcg: re-exported)


def mass_apply(m, rho, u):
    """M[rho] u by the cell loop"""
    dim, n1 = m.dim, m.p + 1
    xq, wq, V, G, T = _tables(m.p)
    cells = _Cells(m)
    shape = (n1,) * dim
    h = [float(m.h[d]) for d in range(dim)]
    u = np.asarray(u, dtype=np.float64)
    w = np.ones(())
    for d in range(dim):  # w[q_{dim-1}, ..., q_0] = prod w_q h
        w = np.multiply.outer(wq * h[d], w) if d else wq * h[0]
    out = np.zeros(m.n_dofs)
    for b in range(0, m.n_cells, BATCH):
        sl = slice(b, min(m.n_cells, b + BATCH))
        n = sl.stop - sl.start
        rq = np.asarray(rho(_qpoints(m, cells, sl, xq))).reshape((n,) + shape)
        f = u[cells.dofs[sl]].reshape((n,) + shape)
        for d in range(dim):
            f = _to_q(f, V[cells.cat[d][sl]], d, dim)
        f = rq * f * w
        for d in range(dim):
            f = _to_i(f, V[cells.cat[d][sl]], d, dim)
        np.add.at(out, cells.dofs[sl].reshape(-1), f.reshape(-1))
    return out


def dense_matrix(m, rho):
    """M[rho] as a dense matrix, column by column (small meshes)"""
    A = np.zeros((m.n_dofs, m.n_dofs))
    e = np.zeros(m.n_dofs)
    for j in range(m.n_dofs):
        e[j] = 1.0
        A[:, j] = mass_apply(m, rho, e)
        e[j] = 0.0
    return A


def mass_1d(m, d, f):
    """dense M_d[f] from the restatement on the 1D mesh of direction d; f a
    callable of one coordinate (None: 1)"""
    m1 = O.Mesh(1, m.p, int(m.nsub[d]), float(m.lo[d]), float(m.hi[d]))
    return dense_matrix(m1, (lambda x: np.ones(x.shape[0])) if f is None else (lambda x: f(x[:, 0]) + 0.0 * x[:, 0]))


def pointwise(terms, dim):
    """rho(x) of a list of separable terms"""

    def rho(x):
        s = 0.0
        for t in terms:
            v = np.ones(x.shape[0])
            for d in range(dim):
                if t[d] is not None:
                    v = v * t[d](x[:, d])
            s = s + v
        return s

    return rho


def kron_dense(m, terms):
    """M[rho] = sum_t kron_d M_d[r_td] dense, every factor from the restatement
    (what mass_apply computes, by exactness of the tensor quadrature;
    test_varmass_cpu checks that)"""
    cache = {}

    def fac(d, f):
        key = (d, id(f))
        if key not in cache:
            cache[key] = mass_1d(m, d, f)
        return cache[key]

    return sum(kron_matrix([fac(d, t[d]) for d in range(m.dim)]) for t in terms)


def diag_ratio(m, terms):
    """W = diag(M[rho]) / diag(M) = sum_t prod_d diag(M_d[r_td]) / prod_d diag(M_d)"""
    one = [np.diag(mass_1d(m, d, None)) for d in range(m.dim)]
    W = 0.0
    for t in terms:
        v = np.ones(1)
        for d in range(m.dim):
            v = np.kron(np.diag(mass_1d(m, d, t[d])) / one[d], v)
        W = W + v
    return W


class MassSystem:
    """M[rho] (dense, from kron_dense) with the engine's preconditioner
    W^-1/2 M^-1 W^-1/2, W = diag_ratio"""

    def __init__(self, m, terms):
        self.A = kron_dense(m, terms)
        self.Minv = np.linalg.inv(kron_dense(m, [[None] * m.dim]))
        self.wis = 1.0 / np.sqrt(diag_ratio(m, terms))

    def precond(self, r):
        return self.wis * (self.Minv @ (self.wis * r))

    def solve(self, b, x0=None, rel_tol=1e-8, abs_tol=0.0, max_it=1000):
        return pcg(lambda x: self.A @ x, self.precond, b, x0, rel_tol, abs_tol, max_it)


def gauss_mean(m, terms):
    """sum_t prod_d mean(r_td), the means Gauss-weighted (the engine's rho-bar)"""
    xq, wq = O.gauss(m.p + 1)
    s = 0.0
    for t in terms:
        prod = 1.0
        for d in range(m.dim):
            if t[d] is None:
                continue
            x = float(m.lo[d]) + (np.arange(int(m.nsub[d]))[:, None] + np.asarray(xq)[None, :]) * float(m.h[d])
            prod *= float(np.sum(np.asarray(wq)[None, :] * t[d](x))) / int(m.nsub[d])
        s += prod
    return s


MAX_IT = 20  # max_it of the test solves: more than twice the numpy counts (tests/test_varmass_cpu.py)


def bump_terms(dim, contrast=10.0, width=0.15):
    """rho = 1 + (contrast - 1) prod_d b(x_d), b a Gaussian bump at 0.5"""
    b = lambda s: np.exp(-((s - 0.5) / width) ** 2)  # noqa: E731
    c = lambda s: (contrast - 1.0) * b(s)  # noqa: E731
    return [[None] * dim, [c] + [b] * (dim - 1)]
