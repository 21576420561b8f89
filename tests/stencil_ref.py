"""TEST INFRASTRUCTURE ONLY: the 1D band matrices B_d of every operator kind,
in the row form Mesh.kron_apply takes (A[i, k] = A(i, i - p + k)), so that

    rhs = sum_d  M_0 (x) .. B_d .. (x) M_{dim-1}  u

is available as a checker at 3D sizes where the oracle's cell loops (O((p+1)^6)
per cell) are out of reach.

  advection    B_d = a_d C_d - outflow traces (Mesh.advection_outflow_B;
               advection/stiffness.h:345-418, :473-532 with u+ = 0)
  convective   B_d = -a_d C_d^T (advection_01_gdm.cc:199-203, -(a . grad u, v))
  wave         B_d = -L_d (wave/stiffness.h:171-181) and, with Nitsche gamma > 0,
               minus the box-face terms of wave/stiffness.h:296-310
                   -dv/dn u - v du/dn + gamma / h_min v u
               on the first and last cell of direction d; h_min is the minimum
               vertex distance of a cell, i.e. the smallest cell width over all
               directions.  The tangential factors of a face integral are the
               1D mass matrices (QGauss(p+1) integrates degree 2p exactly).
  mass         B_d unused: the single term M (x) M (x) M

Built from what oracle/oracle.py exports only (matrices_1d,
advection_outflow_B, basis_value and the cell category / offset);
tests/test_stencil_ref_cpu.py pins it to the cell loops.
"""
import numpy as np

import oracle as O

KINDS = ("mass", "advection", "convective", "wave")


def band_transpose(A, p):
    """CT[i, k] = A[i - p + k, 2p - k], zero where the row lies outside"""
    n = A.shape[0]
    T = np.zeros_like(A)
    for k in range(2 * p + 1):
        j = np.arange(n) - p + k  # column of CT = row of A
        ok = (j >= 0) & (j < n)
        T[ok, k] = A[j[ok], 2 * p - k]
    return T


def h_min(mesh):
    return min(float(mesh.h[d]) for d in range(mesh.dim))


def nitsche_band_1d(mesh, d, gamma):
    """Band of  sum over the two ends of direction d of
    (-dv/dn u - v du/dn + gamma / h_min v u)  (rows v, columns u)."""
    p, n_sub, h = mesh.p, int(mesh.nsub[d]), float(mesh.h[d])
    N = np.zeros((mesh.N[d], 2 * p + 1))
    pen = gamma / h_min(mesh)
    for side, cell in ((0, 0), (1, n_sub - 1)):
        cat = int(O.lib().gdmo_category(cell, p, n_sub))
        off = int(O.lib().gdmo_offset(cell, p, n_sub))
        nrm = 1.0 if side else -1.0
        v = [O.basis_value(p, cat, i, float(side), 0) for i in range(p + 1)]
        dn = [O.basis_value(p, cat, i, float(side), 1) / h * nrm for i in range(p + 1)]
        for i in range(p + 1):
            for j in range(p + 1):
                N[off + i, (off + j) - (off + i) + p] += -dn[i] * v[j] - v[i] * dn[j] + pen * v[i] * v[j]
    return N


def band_1d(mesh, d, kind, params=()):
    """B_d of `kind` in kron_apply's row form.  params: the velocity a
    (advection, convective) or (gamma,) / () (wave)."""
    p = mesh.p
    M, C, L = mesh.matrices_1d(d)
    if kind == "mass":
        return M
    if kind == "advection":
        return mesh.advection_outflow_B(d, float(params[d]))
    if kind == "convective":
        return -float(params[d]) * band_transpose(C, p)
    if kind == "wave":
        B = -L
        gamma = float(params[0]) if len(params) else 0.0
        if gamma > 0.0:
            B = B - nitsche_band_1d(mesh, d, gamma)
        return B
    raise ValueError("unknown kind %r" % (kind,))


def kron_terms(mesh, kind, params=()):
    """Term list for Mesh.kron_apply (2D: the third factor is None)."""
    dim = mesh.dim
    M = [mesh.matrices_1d(d)[0] for d in range(dim)]
    pad = [None] * (3 - dim)
    if kind == "mass":
        return [tuple(M + pad)]
    B = [band_1d(mesh, d, kind, params) for d in range(dim)]
    return [tuple([B[e] if e == d else M[e] for e in range(dim)] + pad) for d in range(dim)]


def apply(mesh, kind, params, u):
    return mesh.kron_apply(kron_terms(mesh, kind, params), u)
