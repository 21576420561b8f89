"""TEST INFRASTRUCTURE ONLY: the two data terms of the reference's uncut wave
right-hand side -- a numpy sum-factorised restatement of
wave/stiffness.h:196-200 (the source term (v, f) over QGauss(p+1)) and
:320-326 (the Nitsche Dirichlet data <gamma / h_min v - dv/dn, g> on the box
faces).

Built from what oracle/oracle.py exports only (Mesh.cell_dofs, basis_value,
gauss); the cells are processed in batches with the tensor-product shape
functions applied direction by direction, which is the cell loop's quadrature
sum for each cell.  tests/test_load_cpu.py pins both terms to Mesh.wave_rhs
(itself pinned to the reference goldens) on small meshes; the helper then
serves the larger GPU meshes, where the oracle's (p+1)^(2 dim) cell loop is
too slow.

f lives on the tensor Gauss grid: an array of shape (Q_z, Q_y, Q_x) (trivial
axes dropped: (Q_y, Q_x) in 2D, (Q_x,) in 1D), Q_d = n_sub_d (p + 1), point
q_d = cell_d (p + 1) + point -- the layout of gdm_add_load, flattened x
fastest.
"""
import numpy as np

import oracle as O
from varfield_ref import BATCH, _Cells, _to_i


def _tables(p):
    n1 = p + 1
    xq, wq = O.gauss(n1)
    ncat = max(1, p)
    V = np.array([[[O.basis_value(p, c, i, x) for x in xq] for i in range(n1)] for c in range(ncat)])
    T = np.array([[[O.basis_value(p, c, i, s) for i in range(n1)] for s in (0.0, 1.0)] for c in range(ncat)])
    D = np.array([[[O.basis_value(p, c, i, s, 1) for i in range(n1)] for s in (0.0, 1.0)] for c in range(ncat)])
    return xq, wq, V, T, D


def _cells(m):
    """_Cells(m), built once per mesh object (its cell loop is Python)"""
    c = getattr(m, "_load_ref_cells", None)
    if c is None:
        c = m._load_ref_cells = _Cells(m)
    return c


def quadrature_points(m):
    """per-axis Gauss abscissae (Q_d values each)"""
    xq, _ = O.gauss(m.p + 1)
    return [(m.lo[d] + (np.arange(int(m.nsub[d]))[:, None] + xq[None, :]) * m.h[d]).reshape(-1)
            for d in range(m.dim)]


def grid_values(m, fn):
    """fn(x, y, z) (missing coordinates 0) on the tensor Gauss grid, shape (Q_{dim-1}, ..., Q_0)"""
    ax = quadrature_points(m)
    g = np.meshgrid(*ax[::-1], indexing="ij")[::-1]  # g[d] has shape (Q_{dim-1}, ..., Q_0)
    z = np.zeros_like(g[0])
    return fn(*(list(g) + [z] * (3 - m.dim)))


def _cell_view(m, fgrid):
    """(n_cells, n1, ..., n1) view of the grid: cells lexicographic (x fastest), points [q_{dim-1}, ..., q_0]"""
    dim, n1 = m.dim, m.p + 1
    ns = [int(m.nsub[d]) for d in range(dim)]
    a = np.asarray(fgrid, dtype=np.float64).reshape([v for d in reversed(range(dim)) for v in (ns[d], n1)])
    # axes: (c_{dim-1}, q_{dim-1}, ..., c_0, q_0) -> (c_{dim-1}, ..., c_0, q_{dim-1}, ..., q_0)
    a = a.transpose(list(range(0, 2 * dim, 2)) + list(range(1, 2 * dim, 2)))
    return a.reshape((m.n_cells,) + (n1,) * dim)


def cell_major(m, fgrid):
    """the grid in the oracle's fq order: fq[cell * (p+1)^dim + q], q x fastest"""
    return _cell_view(m, fgrid).reshape(-1)


def load_vector(m, fgrid):
    """(v, f) over QGauss(p+1): the source term of compute_rhs"""
    dim, p, n1 = m.dim, m.p, m.p + 1
    _, wq, V, _, _ = _tables(p)
    cells = _cells(m)
    h = [float(m.h[d]) for d in range(dim)]
    w = np.ones(())
    for d in range(dim):  # w[q_{dim-1}, ..., q_0] = prod w_q h
        w = np.multiply.outer(wq * h[d], w) if d else wq * h[0]
    fc = _cell_view(m, fgrid)
    rhs = np.zeros(m.n_dofs)
    for b in range(0, m.n_cells, BATCH):
        sl = slice(b, min(m.n_cells, b + BATCH))
        f = fc[sl] * w
        for d in range(dim):
            f = _to_i(f, V[cells.cat[d][sl]], d, dim)
        np.add.at(rhs, cells.dofs[sl].reshape(-1), f.reshape(-1))
    return rhs


def dirichlet_data(m, gamma, gbc):
    """sum_faces <gamma / h_min v - dv/dn, g>; gbc in the reference's block(0) order"""
    dim, p, n1 = m.dim, m.p, m.p + 1
    _, wq, V, T, D = _tables(p)
    cells = _cells(m)
    nc = m.n_cells
    h = [float(m.h[d]) for d in range(dim)]
    hmin = min(h)
    nfq = n1 ** (dim - 1)
    at = np.zeros((nc, 2 * dim), dtype=bool)
    for d in range(dim):
        at[:, 2 * d] = cells.cidx[d] == 0
        at[:, 2 * d + 1] = cells.cidx[d] == int(m.nsub[d]) - 1
    start = (np.cumsum(at.reshape(-1)) - at.reshape(-1)).reshape(nc, 2 * dim) * nfq  # point_counter
    gbc = np.asarray(gbc, dtype=np.float64)
    assert gbc.size == int(at.sum()) * nfq
    rhs = np.zeros(m.n_dofs)
    shape = (n1,) * dim
    for f in range(2 * dim):
        d, side = f // 2, f % 2
        B = np.nonzero(at[:, f])[0]
        if B.size == 0:
            continue
        tang = [e for e in range(dim) if e != d]
        nat = np.arange(nfq)
        if dim == 3 and d == 1:
            nat = nat.reshape(n1, n1).T.reshape(-1)  # reference: z fastest, x slowest
        idx = start[B, f][:, None] + nat[None, :]
        jxw = np.ones(())
        for k, e in enumerate(tang):
            jxw = np.multiply.outer(wq * h[e], jxw) if k else wq * h[e]
        g = (gbc[idx] * np.reshape(jxw, -1)).reshape((B.size,) + (n1,) * (dim - 1))
        for k, e in enumerate(tang):
            g = _to_i(g, V[cells.cat[e][B]], k, dim - 1)
        nrm = 1.0 if side else -1.0
        ck = gamma / hmin * T[cells.cat[d][B], side] - nrm * D[cells.cat[d][B], side] / h[d]  # (nb, n1)
        cv = np.moveaxis(np.multiply.outer(g, np.ones(n1)), -1, dim - d) if dim > 1 else np.multiply.outer(
            g.reshape(B.size), np.ones(n1))
        cks = ck.reshape((B.size,) + tuple(n1 if ax == dim - d else 1 for ax in range(1, dim + 1)))
        cv = cv.reshape((B.size,) + shape) * cks
        np.add.at(rhs, cells.dofs[B].reshape(-1), cv.reshape(-1))
    return rhs


# -- the built-in functions of gdm_fn_kind on arrays (include/gdm_hip.h) -----------------------------------------
def fn_constant(c):
    return lambda x, y, z: np.full_like(x, c)


def fn_cone(r0, center, dim):
    c = list(center) + [0.0] * (3 - len(center))

    def f(x, y, z):
        r2 = (x - c[0]) ** 2
        if dim > 1:
            r2 = r2 + (y - c[1]) ** 2
        if dim > 2:
            r2 = r2 + (z - c[2]) ** 2
        return np.maximum(0.0, r0 - np.sqrt(r2))
    return f


def fn_sine_product(a, k, phi, t, dim, derivative=0):
    """prod_d sin(2 pi k_d (x_d - a_d t) + phi_d) or its d/dt"""
    def f(x, y, z):
        X = (x, y, z)
        arg = [2.0 * np.pi * k[d] * (X[d] - a[d] * t) + phi[d] for d in range(dim)]
        if not derivative:
            return np.prod([np.sin(v) for v in arg], axis=0)
        out = np.zeros_like(x)
        for e in range(dim):
            term = -2.0 * np.pi * k[e] * a[e] * np.cos(arg[e])
            for d in range(dim):
                if d != e:
                    term = term * np.sin(arg[d])
            out = out + term
        return out
    return f
