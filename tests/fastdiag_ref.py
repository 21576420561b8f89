"""TEST INFRASTRUCTURE ONLY: the fast-diagonalisation solve of the uncut wave /
heat system (alpha M + tau S) x = b in numpy / scipy.

S = -K with K the wave operator of tests/stencil_ref.py: S = sum_d M (x) ..
A_d .. (x) M, A_d = -band_1d(mesh, d, "wave", (gamma,)) = L_d + the box Nitsche
terms, symmetric.  With scipy.linalg.eigh(A_d, M_d) (A S = M S Lambda, S^T M S
= I)

    x = (S_z (x) S_y (x) S_x) diag(1 / (alpha + tau sum_d lambda_d)) (S_z (x) S_y (x) S_x)^T b.

dense_system builds alpha M + tau S by Kronecker products for small meshes:
np.linalg.solve on it is the independent check of the formula.
"""
import numpy as np
import scipy.linalg

import stencil_ref as SR


def dense_band(B, p):
    """row form B[i, k] = A(i, i - p + k) -> dense"""
    n = B.shape[0]
    A = np.zeros((n, n))
    for i in range(n):
        for k in range(2 * p + 1):
            j = i - p + k
            if 0 <= j < n:
                A[i, j] = B[i, k]
    return A


def matrices(mesh, gamma):
    """per direction the dense (A_d, M_d)"""
    p = mesh.p
    prm = (gamma,) if gamma > 0.0 else ()
    out = []
    for d in range(mesh.dim):
        M = dense_band(mesh.matrices_1d(d)[0], p)
        A = -dense_band(SR.band_1d(mesh, d, "wave", prm), p)
        out.append((0.5 * (A + A.T), M))
    return out


def eigenpairs(mesh, gamma):
    """per direction (S_d, lambda_d) from scipy.linalg.eigh(A_d, M_d)"""
    out = []
    for A, M in matrices(mesh, gamma):
        lam, S = scipy.linalg.eigh(A, M)
        out.append((S, lam))
    return out


def _shape(mesh):
    return [mesh.N[d] for d in reversed(range(mesh.dim))]  # (Nz, Ny, Nx)


def transform(mesh, T, axis, v):
    """dst[.., i, ..] = sum_j T[i, j] v[.., j, ..] along reference direction `axis`"""
    a = np.asarray(v, dtype=np.float64).reshape(_shape(mesh))
    ax = mesh.dim - 1 - axis
    return np.moveaxis(np.tensordot(T, a, axes=([1], [ax])), 0, ax).reshape(-1)


def solve(mesh, gamma, alpha, tau, b, pairs=None):
    pairs = eigenpairs(mesh, gamma) if pairs is None else pairs
    v = np.asarray(b, dtype=np.float64)
    for d in range(mesh.dim):
        v = transform(mesh, pairs[d][0].T, d, v)
    lam = np.zeros(())
    for d in range(mesh.dim):  # lam[.., iz, iy, ix]
        lam = np.add.outer(pairs[d][1], lam) if d else pairs[d][1].copy()
    v = v / (alpha + tau * lam.reshape(-1))
    for d in reversed(range(mesh.dim)):
        v = transform(mesh, pairs[d][0], d, v)
    return v


def dense_system(mesh, gamma, alpha, tau):
    """alpha M + tau S, dense (small meshes only), x fastest"""
    AM = matrices(mesh, gamma)

    def kron(fs):  # fs by reference direction; x is the fastest index = the last Kronecker factor
        out = np.ones((1, 1))
        for f in reversed(fs):
            out = np.kron(out, f)
        return out

    Ms = [M for _, M in AM]
    mass = kron(Ms)
    stiff = sum(kron([AM[e][0] if e == d else Ms[e] for e in range(mesh.dim)]) for d in range(mesh.dim))
    return alpha * mass + tau * stiff


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


# the cases of the dense check, shared by the CPU test (which records err_ref)
# and the GPU test (whose bound is 20 err_ref of the same case)
BOX_LO, BOX_HI = (-0.5, 0.0, 0.2), (0.7, 0.9, 1.5)
DENSE_CASES = [(15.0, 1.0, 0.01), (15.0, 0.0, 1.0), (15.0, 1.0, 10.0), (0.0, 1.0, 0.01)]


def small_n_sub(p):
    return (p, p + 2, p + 3)


def dense_reference(mesh, gamma, alpha, tau, seed=0):
    """(b, x_dense, err_ref): a random right-hand side, np.linalg.solve on the
    dense system and the rel-L2 error of the helper's solve against it"""
    rng = np.random.default_rng(seed)
    b = rng.uniform(-1, 1, mesh.n_dofs)
    x = np.linalg.solve(dense_system(mesh, gamma, alpha, tau), b)
    return b, x, rel(solve(mesh, gamma, alpha, tau, b), x)
