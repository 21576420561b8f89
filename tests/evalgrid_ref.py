"""TEST INFRASTRUCTURE ONLY: a GDM field on the tensor Gauss grid and back -- a
numpy restatement of what FEValues::get_function_values /
get_function_gradients give the reference's cell loops
(wave/stiffness.h:151-203, advection/problem.h:330-425), of the flux integral
(grad v, F) and of the wall trace and normal derivative at the box-face
quadrature points (wave/stiffness.h:296-310).

Built from what oracle/oracle.py exports and from the helpers of varfield_ref /
vardiff_ref / load_ref only; the cells are processed in batches with the
tensor-product shape functions applied direction by direction.
tests/test_evalgrid_cpu.py pins every function to the oracle.

Grid layout: arrays of shape (Q_{dim-1}, ..., Q_0), Q_d = n_sub_d (p + 1), x
fastest when flattened (gdm_add_load's fq); vector-valued grid arrays carry
the reference direction as their first axis (component-major).
"""
import numpy as np

import oracle as O
from load_ref import _cell_view, _cells
from vardiff_ref import _to_i, _to_q
from varfield_ref import BATCH, _tables


def grid_shape(m):
    return tuple(int(m.nsub[d]) * (m.p + 1) for d in reversed(range(m.dim)))


def _grid_from_cells(m, arr):
    """(n_cells, n1, ..., n1) cell-major, points [q_{dim-1}, ..., q_0] -> the grid layout (load_ref._cell_view's
    inverse)"""
    dim, n1 = m.dim, m.p + 1
    ns = [int(m.nsub[d]) for d in reversed(range(dim))]
    a = arr.reshape(ns + [n1] * dim)
    # axes (c_{dim-1}, ..., c_0, q_{dim-1}, ..., q_0) -> (c_{dim-1}, q_{dim-1}, ..., c_0, q_0)
    a = a.transpose([v for k in range(dim) for v in (k, dim + k)])
    return a.reshape(grid_shape(m))


def _tab(m, cells, sl, d, deriv):
    """[cell, i, q] table of direction d for the cells sl: values, or physical derivatives"""
    _, _, V, G, _ = _tables(m.p)
    return G[cells.cat[d][sl]] / float(m.h[d]) if deriv else V[cells.cat[d][sl]]


def _eval(m, u, e):
    """u (e None) or d u / d x_e at the Gauss points, grid layout"""
    dim, n1 = m.dim, m.p + 1
    cells = _cells(m)
    u = np.asarray(u, dtype=np.float64)
    out = np.empty((m.n_cells,) + (n1,) * dim)
    for b in range(0, m.n_cells, BATCH):
        sl = slice(b, min(m.n_cells, b + BATCH))
        a = u[cells.dofs[sl]].reshape((sl.stop - sl.start,) + (n1,) * dim)
        for d in range(dim):
            a = _to_q(a, _tab(m, cells, sl, d, d == e), d, dim)
        out[sl] = a
    return _grid_from_cells(m, out)


def values(m, u):
    """u at the Gauss points"""
    return _eval(m, u, None)


def gradients(m, u):
    """the physical gradient at the Gauss points, (dim, Q_{dim-1}, ..., Q_0)"""
    return np.stack([_eval(m, u, e) for e in range(m.dim)])


def _weights(m):
    _, wq, _, _, _ = _tables(m.p)
    w = np.ones(())
    for d in range(m.dim):  # w[q_{dim-1}, ..., q_0] = prod w_q h
        w = np.multiply.outer(wq * float(m.h[d]), w) if d else wq * float(m.h[0])
    return w


def flux_load(m, F):
    """sum_e (d_e v, F_e) over QGauss(p+1), F of shape (dim, grid)"""
    dim, n1 = m.dim, m.p + 1
    cells = _cells(m)
    w = _weights(m)
    F = np.asarray(F, dtype=np.float64).reshape((dim,) + grid_shape(m))
    Fc = [_cell_view(m, F[e]) for e in range(dim)]
    rhs = np.zeros(m.n_dofs)
    for b in range(0, m.n_cells, BATCH):
        sl = slice(b, min(m.n_cells, b + BATCH))
        cv = 0.0
        for e in range(dim):
            f = Fc[e][sl] * w
            for d in range(dim):
                f = _to_i(f, _tab(m, cells, sl, d, d == e), d, dim)
            cv = cv + f
        np.add.at(rhs, cells.dofs[sl].reshape(-1), cv.reshape(-1))
    return rhs


class _Faces:
    """the box faces as wave/stiffness.h:296-327 walks them (vardiff_ref.wave_rhs): per face the boundary cells,
    the reference block(0) index of every face point in natural order, the normal direction's trace tables"""

    def __init__(self, m):
        dim, p, n1 = m.dim, m.p, m.p + 1
        _, wq, _, _, T = _tables(p)
        ncat = max(1, p)
        Tn = np.array([[[O.basis_value(p, c, i, s, 1) for i in range(n1)] for s in (0.0, 1.0)] for c in range(ncat)])
        cells = _cells(m)
        nc, nfq = m.n_cells, n1 ** (dim - 1)
        at = np.zeros((nc, 2 * dim), dtype=bool)
        for d in range(dim):
            at[:, 2 * d] = cells.cidx[d] == 0
            at[:, 2 * d + 1] = cells.cidx[d] == int(m.nsub[d]) - 1
        start = (np.cumsum(at.reshape(-1)) - at.reshape(-1)).reshape(nc, 2 * dim) * nfq  # point_counter
        self.n_points = int(at.sum()) * nfq
        self.faces = []
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
            jxw = np.ones(())
            for k, e in enumerate(tang):
                jxw = np.multiply.outer(wq * float(m.h[e]), jxw) if k else wq * float(m.h[e])
            self.faces.append((d, B, tang, idx, T[cells.cat[d][B], side],
                               Tn[cells.cat[d][B], side] / float(m.h[d]) * nrm, np.reshape(jxw, -1)))


def _face_eval(m, u, d, B, tang, tr, trn):
    """(trace, outward normal derivative) of u at the face points of the boundary cells B, natural order"""
    dim, n1 = m.dim, m.p + 1
    cells = _cells(m)
    _, _, V, _, _ = _tables(m.p)
    ul = np.moveaxis(u[cells.dofs[B]].reshape((B.size,) + (n1,) * dim), dim - d, -1)
    uval = np.einsum("c...i,ci->c...", ul, tr)
    dun = np.einsum("c...i,ci->c...", ul, trn)
    for k, e in enumerate(tang):  # remaining axes: tangential directions, highest first
        uval = _to_q(uval, V[cells.cat[e][B]], k, dim - 1)
        dun = _to_q(dun, V[cells.cat[e][B]], k, dim - 1)
    nfq = n1 ** (dim - 1)
    return uval.reshape(B.size, nfq), dun.reshape(B.size, nfq)


def trace(m, u):
    """(U, Dn): the wall trace and the outward normal derivative of u at the boundary points, the reference's
    block(0) order (Mesh.boundary_points)"""
    u = np.asarray(u, dtype=np.float64)
    fc = _Faces(m)
    U, Dn = np.zeros(fc.n_points), np.zeros(fc.n_points)
    for d, B, tang, idx, tr, trn, _ in fc.faces:
        U[idx], Dn[idx] = _face_eval(m, u, d, B, tang, tr, trn)
    return U, Dn


def wave_rhs_grid(m, kq, kbc, u=None, nitsche=0.0, gbc=None):
    """vardiff_ref.wave_rhs with kappa given as arrays: kq on the Gauss grid, kbc at the boundary points in the
    reference's block(0) order (not read without nitsche)"""
    dim, n1 = m.dim, m.p + 1
    cells = _cells(m)
    _, _, V, _, _ = _tables(m.p)
    rhs = np.zeros(m.n_dofs)
    if u is not None:
        u = np.asarray(u, dtype=np.float64)
        rhs -= flux_load(m, np.asarray(kq, dtype=np.float64).reshape(grid_shape(m))[None] * gradients(m, u))
    if not nitsche > 0.0:
        return rhs
    gamma = nitsche / min(float(m.h[d]) for d in range(dim))
    kbc = np.asarray(kbc, dtype=np.float64)
    g_all = None if gbc is None else np.asarray(gbc, dtype=np.float64)
    for d, B, tang, idx, tr, trn, jxw in _Faces(m).faces:
        kap = kbc[idx]
        nfq = n1 ** (dim - 1)
        a_v, a_dv = np.zeros((B.size, nfq)), np.zeros((B.size, nfq))  # coefficients of v and dv/dn
        if u is not None:
            uval, dun = _face_eval(m, u, d, B, tang, tr, trn)
            a_v += kap * (dun - gamma * uval) * jxw
            a_dv += kap * uval * jxw
        if g_all is not None:
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


def factors_1d(m, d):
    """(val[Q][p+1], der[Q][p+1], first[Q]) of direction d: the restatement's tables per Gauss point, the layout
    of gdm_coef_grid_tables_1d"""
    n1 = m.p + 1
    m1 = O.Mesh(1, m.p, int(m.nsub[d]), float(m.lo[d]), float(m.hi[d]))
    cells = _cells(m1)
    sl = slice(0, m1.n_cells)
    val = np.swapaxes(_tab(m1, cells, sl, 0, False), 1, 2).reshape(-1, n1)  # [cell, q, i]
    der = np.swapaxes(_tab(m1, cells, sl, 0, True), 1, 2).reshape(-1, n1)
    first = np.repeat(cells.dofs[:, 0], n1)
    return val, der, first
