"""TEST INFRASTRUCTURE ONLY: the exact mass inverse with periodicity constraints
(System::make_periodicity_constraints, system.h:427-463: vertex N_d - 1 :=
vertex 0 in every periodic direction d), numpy only and without Woodbury.

Per direction the dense condensed 1D matrix P_d^T M_d P_d on the N_d - 1 free
vertices (M_d from oracle.Mesh.matrices_1d; a non-periodic direction keeps
M_d) is solved with np.linalg.solve, direction by direction on the
unconstrained sub-grid (the condensed mass is the Kronecker product of these
factors); the result is distributed.  tests/test_periodic_mass_cpu.py pins it
to a sparse direct solve of the condensed cell-loop matrix.

`mask` has bit d set for a periodic direction d.
"""
import numpy as np
import scipy.sparse as sp


def dense_1d(m, d):
    """dense M_d from the band form of Mesh.matrices_1d"""
    B = m.matrices_1d(d)[0]
    N, p = m.N[d], m.p
    M = np.zeros((N, N))
    for i in range(N):
        for j in range(max(0, i - p), min(N - 1, i + p) + 1):
            M[i, j] = B[i, j - i + p]
    return M


def condensed_1d(M):
    """P^T M P on the free vertices 0 .. N-2 (vertex N-1 := vertex 0)"""
    N = M.shape[0]
    P = np.zeros((N, N - 1))
    P[np.arange(N - 1), np.arange(N - 1)] = 1.0
    P[N - 1, 0] = 1.0
    return P.T @ M @ P


class PeriodicMassRef:
    def __init__(self, m, mask):
        self.m, self.mask = m, mask
        self.shape = tuple(m.N[d] for d in range(m.dim))[::-1]  # (.., N1, N0): x fastest
        self.factor = []
        for d in range(m.dim):
            M = dense_1d(m, d)
            self.factor.append(condensed_1d(M) if mask & (1 << d) else M)
        idx = np.arange(m.n_dofs)
        Ns = m.N
        coords = [idx % Ns[0], (idx // Ns[0]) % Ns[1], idx // (Ns[0] * Ns[1])]
        stride = [1, Ns[0], Ns[0] * Ns[1]]
        master = idx.copy()
        self.constrained = np.zeros(m.n_dofs, dtype=bool)
        for d in range(m.dim):
            if mask & (1 << d):
                at_end = coords[d] == Ns[d] - 1
                master = np.where(at_end, master - (Ns[d] - 1) * stride[d], master)
                self.constrained |= at_end
        self.master = master
        self.P = sp.csr_matrix((np.ones(m.n_dofs), (idx, master)), shape=(m.n_dofs, m.n_dofs))

    def distribute(self, u):
        return np.asarray(u)[self.master]

    def condense(self, r):
        return self.P.T @ r

    def solve(self, rhs):
        """distribute((P^T M P)^-1 rhs); rhs entries on constrained DoFs are ignored"""
        dim = self.m.dim
        X = np.asarray(rhs, dtype=np.float64).reshape(self.shape)
        free = tuple(slice(0, self.shape[a] - 1) if self.mask & (1 << (dim - 1 - a)) else slice(None)
                     for a in range(dim))
        X = X[free].copy()
        for d in range(dim):
            a = dim - 1 - d
            Y = np.moveaxis(X, a, 0)
            sh = Y.shape
            Y = np.linalg.solve(self.factor[d], Y.reshape(sh[0], -1)).reshape(sh)
            X = np.moveaxis(Y, 0, a)
        for d in range(dim):
            if self.mask & (1 << d):
                a = dim - 1 - d
                X = np.concatenate([X, np.take(X, [0], axis=a)], axis=a)
        return np.ascontiguousarray(X).reshape(-1)

    def sparse_condensed(self):
        """the condensed cell-loop mass P^T M P with identity on the constrained rows (csr)"""
        n = self.m.n_dofs
        rp, cols, vals = self.m.matrix_csr(kind=0)
        M = sp.csr_matrix((vals, cols, rp), shape=(n, n))
        A = (self.P.T @ M @ self.P).tolil()
        for i in np.where(self.constrained)[0]:
            A[i, i] = 1.0
        return A.tocsc()
