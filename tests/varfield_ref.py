"""TEST INFRASTRUCTURE ONLY: the advection right-hand side of the reference for
an arbitrary pointwise velocity field a(x), alpha = 0 -- a numpy restatement of
advection/stiffness.h:345-418 (cell term (a u, grad v)) and :473-532 (box-face
term <(a.n)(0 u - [a.n >= 0 ? u : u+]), v>), with advection->value(x_q, d)
evaluated at every cell and face quadrature point.

Built from what oracle/oracle.py exports only (Mesh.cell_dofs, cell_qpoints,
boundary_points, basis_value, gauss); the cells are processed in batches with
the tensor-product shape functions applied direction by direction, which is
the cell loop's quadrature sum for each cell.  tests/test_varfield_cpu.py pins
it to Mesh.advection_rhs (itself pinned to the reference goldens) for a
constant field.

A field is a callable a(x): x of shape (n, 3) -> (n, dim).
"""
import numpy as np

import oracle as O

BATCH = 4096


class _Cells:
    """per-cell data of a mesh: DoF indices, per-direction cell index and category"""

    def __init__(self, m):
        dim, n1 = m.dim, m.p + 1
        nc = m.n_cells
        self.dofs = np.empty((nc, n1 ** dim), dtype=np.int64)
        for c in range(nc):
            self.dofs[c] = m.cell_dofs(c)
        self.cidx, self.cat = [], []
        rem = np.arange(nc)
        first = self.dofs[:, 0].copy()  # the DoF box's lowest corner
        for d in range(dim):
            ns = int(m.nsub[d])
            self.cidx.append(rem % ns)
            rem = rem // ns
            self.cat.append(self.cidx[d] - first % m.N[d])  # category = cell - box offset
            first = first // m.N[d]


def _tables(p):
    n1 = p + 1
    xq, wq = O.gauss(n1)
    ncat = max(1, p)
    V = np.array([[[O.basis_value(p, c, i, x) for x in xq] for i in range(n1)] for c in range(ncat)])
    G = np.array([[[O.basis_value(p, c, i, x, 1) for x in xq] for i in range(n1)] for c in range(ncat)])
    T = np.array([[[O.basis_value(p, c, i, s) for i in range(n1)] for s in (0.0, 1.0)] for c in range(ncat)])
    return xq, wq, V, G, T


def _to_q(arr, tab, d, dim):
    """contract local index i of direction d with tab[c, i, q] (array axis dim - d)"""
    ax = dim - d
    return np.moveaxis(np.einsum("c...i,ciq->c...q", np.moveaxis(arr, ax, -1), tab), -1, ax)


def _to_i(arr, tab, d, dim):
    ax = dim - d
    return np.moveaxis(np.einsum("c...q,ciq->c...i", np.moveaxis(arr, ax, -1), tab), -1, ax)


def advection_rhs(m, a, u, stage_bc=None, volume=True, faces=True):
    """rhs of compute_rhs for the field a; stage_bc in the reference's block(0)
    order (None: u+ = 0); volume / faces select the two terms"""
    dim, p, n1 = m.dim, m.p, m.p + 1
    xq, wq, V, G, T = _tables(p)
    cells = _Cells(m)
    nc, nq = m.n_cells, n1 ** dim
    u = np.asarray(u, dtype=np.float64)
    rhs = np.zeros(m.n_dofs)
    shape = (n1,) * dim
    h = [float(m.h[d]) for d in range(dim)]
    if volume:
        xyz = m.cell_qpoints()
        w = np.ones(())
        for d in range(dim):  # w[q_{dim-1}, ..., q_0] = prod w_q h
            w = np.multiply.outer(wq * h[d], w) if d else wq * h[0]
        for b in range(0, nc, BATCH):
            sl = slice(b, min(nc, b + BATCH))
            n = sl.stop - sl.start
            aq = np.asarray(a(xyz[sl.start * nq:sl.stop * nq])).reshape((n,) + shape + (dim,))
            uq = u[cells.dofs[sl]].reshape((n,) + shape)
            for d in range(dim):
                uq = _to_q(uq, V[cells.cat[d][sl]], d, dim)
            cv = np.zeros((n,) + shape)
            for e in range(dim):
                f = aq[..., e] * uq * w
                for d in range(dim):
                    f = _to_i(f, (G if d == e else V)[cells.cat[d][sl]] / (h[d] if d == e else 1.0), d, dim)
                cv += f
            np.add.at(rhs, cells.dofs[sl].reshape(-1), cv.reshape(-1))
    if not faces:
        return rhs
    nfq = n1 ** (dim - 1)
    at = np.zeros((nc, 2 * dim), dtype=bool)
    for d in range(dim):
        at[:, 2 * d] = cells.cidx[d] == 0
        at[:, 2 * d + 1] = cells.cidx[d] == int(m.nsub[d]) - 1
    start = (np.cumsum(at.reshape(-1)) - at.reshape(-1)).reshape(nc, 2 * dim) * nfq  # point_counter
    bxyz = m.boundary_points()
    assert bxyz.shape[0] == int(at.sum()) * nfq
    bc = None if stage_bc is None else np.asarray(stage_bc, dtype=np.float64)
    for f in range(2 * dim):
        d, side = f // 2, f % 2
        B = np.nonzero(at[:, f])[0]
        if B.size == 0:
            continue
        tang = [e for e in range(dim) if e != d]
        # reference point order (QProjector) -> natural order (higher tangential direction slowest)
        nat = np.arange(nfq)
        if dim == 3 and d == 1:
            nat = nat.reshape(n1, n1).T.reshape(-1)  # reference: z fastest, x slowest
        idx = start[B, f][:, None] + nat[None, :]
        an = np.asarray(a(bxyz[idx.reshape(-1)]))[:, d].reshape(B.size, nfq) * (1.0 if side else -1.0)
        uplus = np.zeros_like(an) if bc is None else bc[idx]
        ul = u[cells.dofs[B]].reshape((B.size,) + shape)
        tr = T[cells.cat[d][B], side]  # (nb, n1) trace of the normal direction
        uval = np.einsum("c...i,ci->c...", np.moveaxis(ul, dim - d, -1), tr)
        for k, e in enumerate(tang):  # remaining axes: tangential directions, highest first
            uval = _to_q(uval, V[cells.cat[e][B]], k, dim - 1)
        jxw = np.ones(())
        for k, e in enumerate(tang):
            jxw = np.multiply.outer(wq * h[e], jxw) if k else wq * h[e]
        uval = uval.reshape(B.size, nfq)
        upw = np.where(an >= 0.0, uval, uplus)
        g = (an * (0.0 * uval - upw) * np.reshape(jxw, -1)).reshape((B.size,) + (n1,) * (dim - 1))
        for k, e in enumerate(tang):
            g = _to_i(g, V[cells.cat[e][B]], k, dim - 1)
        cv = np.moveaxis(np.multiply.outer(g, np.ones(n1)), -1, dim - d) if dim > 1 else np.multiply.outer(
            g.reshape(B.size), np.ones(n1))
        # the normal direction's trace values
        trs = tr.reshape((B.size,) + tuple(n1 if ax == dim - d else 1 for ax in range(1, dim + 1)))
        cv = cv * trs
        np.add.at(rhs, cells.dofs[B].reshape(-1), cv.reshape(-1))
    return rhs
