"""TEST INFRASTRUCTURE ONLY: the wave / heat / Poisson right-hand side of the
reference for an arbitrary pointwise coefficient kappa(x) -- a numpy
restatement of wave/stiffness.h:151-330 with every JxW(q) of the operator part
(I, :171-181) and of the box-face part (IV, :296-327) multiplied by kappa at
the quadrature point:

  K[kappa] u = -(kappa grad v, grad u)
               - sum_faces (-<kappa dv/dn, u> - <kappa v, du/dn> + gamma/h_min <kappa v, u>)
  data       = sum_faces <gamma/h_min v - dv/dn, kappa g_D>

Built from what oracle/oracle.py exports only (Mesh.cell_dofs, boundary_points,
basis_value, gauss; the cell quadrature points are Mesh.cell_qpoints', formed
batch by batch from the Gauss abscissae); the cells
are processed in batches with the tensor-product shape functions applied
direction by direction, which is the cell loop's quadrature sum for each cell.
tests/test_vardiff_cpu.py pins it to Mesh.wave_rhs (itself pinned to the
reference goldens) for kappa = 1.

A coefficient is a callable kappa(x): x of shape (n, 3) -> (n,).
"""
import numpy as np

import oracle as O
from varfield_ref import BATCH, _Cells, _tables


def _contract(arr, tab, d, dim):
    """contract the array axis of direction d (axis dim - d) with tab[c, :, :]'s
    first index, cell by cell (batched matrix products)"""
    a = np.moveaxis(arr, dim - d, -1)
    out = np.matmul(a.reshape(a.shape[0], -1, a.shape[-1]), tab).reshape(a.shape[:-1] + (tab.shape[2],))
    return np.moveaxis(out, -1, dim - d)


def _to_q(arr, tab, d, dim):
    """local index i of direction d -> quadrature index q with tab[c, i, q]"""
    return _contract(arr, tab, d, dim)


def _to_i(arr, tab, d, dim):
    return _contract(arr, np.swapaxes(tab, 1, 2), d, dim)


def _qpoints(m, cells, sl, xq):
    """the quadrature points of the cells sl, (n (p+1)^dim, 3) in the order of
    Mesh.cell_qpoints (cell-major, q_0 fastest)"""
    dim, n1 = m.dim, m.p + 1
    n = sl.stop - sl.start
    x = np.zeros((n,) + (n1,) * dim + (3,))
    for d in range(dim):
        c = float(m.lo[d]) + (cells.cidx[d][sl][:, None] + xq[None, :]) * float(m.h[d])  # (n, n1)
        x[..., d] = c.reshape((n,) + tuple(n1 if ax == dim - d else 1 for ax in range(1, dim + 1)))
    return x.reshape(-1, 3)


def wave_rhs(m, kappa, u=None, nitsche=0.0, gbc=None, hmin=None):
    """K[kappa] u (u None: left out) + the data term of gbc (None: left out;
    reference block(0) order).  hmin overrides the mesh's smallest cell width
    (the 1D factors of a Kronecker form need the full mesh's)."""
    dim, p, n1 = m.dim, m.p, m.p + 1
    xq, wq, V, G, T = _tables(p)
    ncat = max(1, p)
    Tn = np.array([[[O.basis_value(p, c, i, s, 1) for i in range(n1)] for s in (0.0, 1.0)] for c in range(ncat)])
    cells = _Cells(m)
    nc, nq = m.n_cells, n1 ** dim
    rhs = np.zeros(m.n_dofs)
    shape = (n1,) * dim
    h = [float(m.h[d]) for d in range(dim)]
    hmin = min(h) if hmin is None else float(hmin)
    if u is not None:
        u = np.asarray(u, dtype=np.float64)
        w = np.ones(())
        for d in range(dim):  # w[q_{dim-1}, ..., q_0] = prod w_q h
            w = np.multiply.outer(wq * h[d], w) if d else wq * h[0]
        for b in range(0, nc, BATCH):
            sl = slice(b, min(nc, b + BATCH))
            n = sl.stop - sl.start
            kq = np.asarray(kappa(_qpoints(m, cells, sl, xq))).reshape((n,) + shape)
            ul = u[cells.dofs[sl]].reshape((n,) + shape)
            cv = np.zeros((n,) + shape)
            for e in range(dim):
                du = ul
                for d in range(dim):  # d u / d x_e at the quadrature points
                    du = _to_q(du, (G if d == e else V)[cells.cat[d][sl]] / (h[d] if d == e else 1.0), d, dim)
                f = -kq * du * w
                for d in range(dim):
                    f = _to_i(f, (G if d == e else V)[cells.cat[d][sl]] / (h[d] if d == e else 1.0), d, dim)
                cv += f
            np.add.at(rhs, cells.dofs[sl].reshape(-1), cv.reshape(-1))
    if not nitsche > 0.0:
        return rhs
    gamma = nitsche / hmin
    nfq = n1 ** (dim - 1)
    at = np.zeros((nc, 2 * dim), dtype=bool)
    for d in range(dim):
        at[:, 2 * d] = cells.cidx[d] == 0
        at[:, 2 * d + 1] = cells.cidx[d] == int(m.nsub[d]) - 1
    start = (np.cumsum(at.reshape(-1)) - at.reshape(-1)).reshape(nc, 2 * dim) * nfq  # point_counter
    bxyz = m.boundary_points()
    assert bxyz.shape[0] == int(at.sum()) * nfq
    g_all = None if gbc is None else np.asarray(gbc, dtype=np.float64)
    for f in range(2 * dim):
        d, side = f // 2, f % 2
        B = np.nonzero(at[:, f])[0]
        if B.size == 0:
            continue
        nrm = 1.0 if side else -1.0
        tang = [e for e in range(dim) if e != d]
        # reference point order (QProjector) -> natural order (higher tangential direction slowest)
        nat = np.arange(nfq)
        if dim == 3 and d == 1:
            nat = nat.reshape(n1, n1).T.reshape(-1)  # reference: z fastest, x slowest
        idx = start[B, f][:, None] + nat[None, :]
        kap = np.asarray(kappa(bxyz[idx.reshape(-1)])).reshape(B.size, nfq)
        tr = T[cells.cat[d][B], side]                    # (nb, n1) trace of the normal direction
        trn = Tn[cells.cat[d][B], side] / h[d] * nrm     # its normal derivative
        jxw = np.ones(())
        for k, e in enumerate(tang):
            jxw = np.multiply.outer(wq * h[e], jxw) if k else wq * h[e]
        jxw = np.reshape(jxw, -1)
        a_v = np.zeros((B.size, nfq))   # coefficient of v at the face points
        a_dv = np.zeros((B.size, nfq))  # coefficient of dv/dn
        if u is not None:
            ul = np.moveaxis(u[cells.dofs[B]].reshape((B.size,) + shape), dim - d, -1)
            uval = np.einsum("c...i,ci->c...", ul, tr)
            dun = np.einsum("c...i,ci->c...", ul, trn)
            for k, e in enumerate(tang):  # remaining axes: tangential directions, highest first
                uval = _to_q(uval, V[cells.cat[e][B]], k, dim - 1)
                dun = _to_q(dun, V[cells.cat[e][B]], k, dim - 1)
            uval, dun = uval.reshape(B.size, nfq), dun.reshape(B.size, nfq)
            # cv_i -= (-dphin u - dun phi + gamma phi u) kappa JxW
            a_v += kap * (dun - gamma * uval) * jxw
            a_dv += kap * uval * jxw
        if g_all is not None:
            # cv_i += kappa g (gamma phi - dphin) JxW
            a_v += kap * g_all[idx] * gamma * jxw
            a_dv -= kap * g_all[idx] * jxw
        cv = 0.0
        for a, t in ((a_v, tr), (a_dv, trn)):
            a = a.reshape((B.size,) + (n1,) * (dim - 1))
            for k, e in enumerate(tang):
                a = _to_i(a, V[cells.cat[e][B]], k, dim - 1)
            a = np.moveaxis(np.multiply.outer(a, np.ones(n1)), -1, dim - d)
            cv = cv + a * t.reshape((B.size,) + tuple(n1 if ax == dim - d else 1 for ax in range(1, dim + 1)))
        np.add.at(rhs, cells.dofs[B].reshape(-1), cv.reshape(-1))
    return rhs


def dense_matrix(m, kappa, nitsche=0.0, hmin=None):
    """K[kappa] as a dense matrix, column by column (small meshes)"""
    K = np.zeros((m.n_dofs, m.n_dofs))
    e = np.zeros(m.n_dofs)
    for j in range(m.n_dofs):
        e[j] = 1.0
        K[:, j] = wave_rhs(m, kappa, e, nitsche, hmin=hmin)
        e[j] = 0.0
    return K


def band_to_dense(band):
    n, W = band.shape
    p = (W - 1) // 2
    A = np.zeros((n, n))
    for i in range(n):
        for k in range(W):
            j = i - p + k
            if 0 <= j < n:
                A[i, j] = band[i, k]
    return A


def dense_to_band(A, p):
    n = A.shape[0]
    band = np.zeros((n, 2 * p + 1))
    for i in range(n):
        for k in range(2 * p + 1):
            j = i - p + k
            if 0 <= j < n:
                band[i, k] = A[i, j]
    return band


def factors_1d(m, d, f, nitsche=0.0):
    """dense (M[f], B[f]) along direction d from the restatement on the 1D mesh
    of that direction, f a callable of one coordinate; gamma / h_min is the
    full mesh's"""
    m1 = O.Mesh(1, m.p, int(m.nsub[d]), float(m.lo[d]), float(m.hi[d]))
    hmin = min(float(m.h[e]) for e in range(m.dim))
    B = dense_matrix(m1, lambda x: f(x[:, 0]), nitsche, hmin)
    # M[f]: the 1D quadrature sum of f phi_i phi_j, cell by cell
    n1 = m.p + 1
    xq, wq, V, G, T = _tables(m.p)
    cells = _Cells(m1)
    M = np.zeros((m1.n_dofs, m1.n_dofs))
    xyz = m1.cell_qpoints()
    for c in range(m1.n_cells):
        v = V[cells.cat[0][c]]
        fw = f(xyz[c * n1:(c + 1) * n1, 0]) * wq * float(m1.h[0])
        M[np.ix_(cells.dofs[c], cells.dofs[c])] += np.einsum("iq,jq,q->ij", v, v, fw)
    return M, B


def kron_matrix(mats):
    """kron over the directions, direction 0 fastest: mats[d] dense"""
    A = np.ones((1, 1))
    for Md in mats:
        A = np.kron(Md, A)
    return A


def homogeneous_matrices(m, nitsche):
    """(M, K_0) dense from the Kronecker form of the 1D restatement"""
    one = lambda x: np.ones_like(x)
    fac = [factors_1d(m, d, one, nitsche) for d in range(m.dim)]
    M = kron_matrix([f[0] for f in fac])
    K = sum(kron_matrix([fac[e][1 if e == d else 0] for e in range(m.dim)]) for d in range(m.dim))
    return M, K


# (elasticity_ref.pcg is a different function: zero start, no breakdown check, another return value)
def pcg(apply_A, apply_Pinv, b, x0=None, rel_tol=1e-8, abs_tol=0.0, max_it=1000):
    """deal.II's SolverCG with ReductionControl(max_it, abs_tol, rel_tol):
    returns (x, last_step, residual norms); raises on max_it or breakdown"""
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - apply_A(x)
    res = np.linalg.norm(r)
    hist = [res]
    tol = max(abs_tol, rel_tol * res)
    it = 0
    if res > tol:
        z = apply_Pinv(r)
        p = z.copy()
        rz = r @ z
        while True:
            if it >= max_it:
                raise RuntimeError("pcg: max_it reached")
            it += 1
            Ap = apply_A(p)
            pAp = p @ Ap
            if not pAp > 0.0:
                raise ArithmeticError("pcg: breakdown, p^T A p = %g" % pAp)
            step = rz / pAp
            x += step * p
            r -= step * Ap
            res = np.linalg.norm(r)
            hist.append(res)
            if res <= tol:
                break
            z = apply_Pinv(r)
            rz_new = r @ z
            p = z + (rz_new / rz) * p
            rz = rz_new
    return x, it, hist


class System:
    """A = alpha M - tau K[kappa] through the restatement, preconditioned by
    the exact dense inverse of alpha M - tau mean K_0"""

    def __init__(self, m, kappa, nitsche, alpha, tau, mean):
        self.m, self.kappa, self.nitsche, self.alpha, self.tau = m, kappa, nitsche, alpha, tau
        self.M, K0 = homogeneous_matrices(m, nitsche)
        self.P = np.linalg.inv(alpha * self.M - tau * mean * K0)

    def apply(self, x):
        return self.alpha * (self.M @ x) - self.tau * wave_rhs(self.m, self.kappa, x, self.nitsche)

    def solve(self, b, x0=None, rel_tol=1e-8, abs_tol=0.0, max_it=1000):
        return pcg(self.apply, lambda r: self.P @ r, b, x0, rel_tol, abs_tol, max_it)
