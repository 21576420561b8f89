"""TEST INFRASTRUCTURE ONLY: inputs and the oracle reference of the error-norm
tests (tests/test_gpu_post.py).

The reference is oracle.Mesh.error_norms(u, exact(cell_qpoints()), cells=True)
-- the cell loop of integrate_difference -- for a noisy vertex interpolant u of
the exact function.  That loop is not sum-factorised: a 3D mesh at p >= 7 costs
it from seconds to a minute.  For those cases (is_recorded) its inputs and
outputs are recorded once in tests/golden/error_norms_oracle.npz

    python3 tests/post_ref.py        # recompute and rewrite the file

and case_reference() reads them back; every other case calls the oracle.
tests/test_post_ref_cpu.py recomputes recorded cases and compares.
"""
import os
import sys

import numpy as np

try:
    import oracle as O
except ImportError:  # run as a script: the tests' conftest.py has not set the path
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "error_norms_oracle.npz")

SINE = [0.7, -0.3, 0.2, 1.0, 2.0, 1.5, 0.1, 0.4, -0.2]
KIND_GRID = 3  # not a gdm_fn_kind: a function that is not built in, given on the Gauss grid (gdm_error_norms_grid)


def exact(kind, prm, X, t, dim):
    """X: (n, 3) coordinates.  Same definitions as include/gdm_hip.h gdm_fn_kind."""
    if kind == 0:
        return np.full(len(X), prm[0])
    if kind == 1:
        r = np.sqrt(sum((X[:, d] - prm[1 + d]) ** 2 for d in range(dim)))
        return np.maximum(0.0, prm[0] - r)
    if kind == KIND_GRID:
        return np.cos(1.3 * X[:, 0] - 0.4) * np.exp(0.5 * X[:, 1]) * (1.0 + 0.3 * X[:, 2])
    v = np.ones(len(X))
    for d in range(dim):
        v = v * np.sin(2 * np.pi * prm[3 + d] * (X[:, d] - prm[d] * t) + prm[6 + d])
    return v


def field(m, kind, prm, t, seed):
    """vertex interpolant of the exact function plus noise (so errors are O(1e-2))"""
    V = m.vertex_coords()
    X = np.zeros((m.n_dofs, 3))
    for d in range(m.dim):
        X[:, d] = V[d]
    u = exact(kind, prm, X, t, m.dim)
    return u + 0.01 * np.random.default_rng(seed).standard_normal(m.n_dofs)


def reference(m, u, kind, prm, t):
    xq = m.cell_qpoints()
    return m.error_norms(u, exact(kind, prm, xq, t, m.dim), cells=True)


def grid_layout(m, values):
    """values at oracle.Mesh.cell_qpoints() (cell by cell, x fastest in both the
    cells and a cell's points) -> gdm_add_load's layout fq[(qz Q_y + qy) Q_x +
    qx] on the tensor Gauss grid, q_d = cell_d (p + 1) + point_d"""
    n1 = m.p + 1
    nc = [int(m.nsub[d]) if d < m.dim else 1 for d in range(3)]
    nq = [n1 if d < m.dim else 1 for d in range(3)]
    v = np.asarray(values).reshape(nc[2], nc[1], nc[0], nq[2], nq[1], nq[0])
    return np.ascontiguousarray(v.transpose(0, 3, 1, 4, 2, 5)).reshape(-1)


# ---- the new cases of tests/test_gpu_post.py: (dim, p, n, kind, prm) on the box LO .. HI --------------------------
LO, HI = (-0.5, 0.2, -1.0), (1.25, 0.9, 0.3)
T = 0.37


def cone(dim):
    """centre off every grid line and Gauss point, the rim r0 well inside the box: it cuts cells"""
    c = [LO[d] + (0.43, 0.57, 0.39)[d] * (HI[d] - LO[d]) for d in range(dim)]
    return [0.31] + c


def kind_params(kind, dim):
    return {0: [0.25], 1: cone(dim), 2: SINE, KIND_GRID: []}[kind]


# error_norms_kernel strides ceil(ncx / 64) * ncy * ncz work items over gdm_op::n_err_partial = 1024 workgroups:
# more than 2 * 1024 items, so that a moderate change of that constant still leaves a second trip
WRAP_CASES = [(3, 1, (1, 46, 46)), (3, 5, (5, 46, 46)), (3, 7, (7, 46, 46)),  # 2116 items; p = 7: > 64 KB of LDS
              (2, 3, (65, 1040)),  # 2080 items: two chunks per row, the second a single cell
              (1, 3, (65 * 2100,))]  # 2133 items
CHUNK_CASES = [(1, 9, (ncx,)) for ncx in (63, 64, 65, 128, 129)] + [(2, 5, (ncx, 5)) for ncx in (63, 64, 65, 128, 129)]
LARGEST_LDS = (3, 9, (9, 10, 9))  # about 131 KB of LDS
KIND_CASES = [(dim, p, ((p + 2, p), (p + 1, p, p + 2))[dim - 2], kind)
              for dim in (2, 3) for p in (1, 3, 5, 7, 9) for kind in (0, 1, 2, KIND_GRID)]


def all_cases():
    """(dim, p, n, kind) of every new single-rank case"""
    return ([c + (2,) for c in WRAP_CASES] + [c + (2,) for c in CHUNK_CASES] + [LARGEST_LDS + (2,)] + KIND_CASES)


def seed_of(dim, p, n, kind):
    return 1000 * dim + 10 * p + kind + sum(n)


def is_recorded(dim, p, n):
    """the oracle's cell loop costs n_cells (p + 1)^(2 dim) multiply-adds: above 5e7 (about a second) it is recorded"""
    return int(np.prod(n)) * (p + 1) ** (2 * dim) > 5e7


def key_of(dim, p, n, kind):
    return "d%d_p%d_n%s_k%d" % (dim, p, "x".join(str(v) for v in n), kind)


def mesh_of(dim, p, n):
    return O.Mesh(dim, p, list(n), list(LO[:dim]), list(HI[:dim]))


def compute(dim, p, n, kind):
    m = mesh_of(dim, p, n)
    prm = kind_params(kind, dim)
    u = field(m, kind, prm, T, seed_of(dim, p, n, kind))
    norms, cells = reference(m, u, kind, prm, T)
    return u, np.array(norms), cells


_golden = None


def case_reference(dim, p, n, kind):
    """(mesh, u, norms, cell errors) of one case: recorded, or from the oracle"""
    global _golden
    m = mesh_of(dim, p, n)
    if not is_recorded(dim, p, n):
        u, norms, cells = compute(dim, p, n, kind)
        return m, u, tuple(norms), cells
    if _golden is None:
        _golden = np.load(GOLDEN)
    k = key_of(dim, p, n, kind)
    if k + "_u" not in _golden:
        raise KeyError("%s is not recorded in %s: run python3 tests/post_ref.py" % (k, GOLDEN))
    u, norms, cells = _golden[k + "_u"], _golden[k + "_norms"], _golden[k + "_cells"]
    assert u.size == m.n_dofs and cells.size == m.n_cells
    return m, u, tuple(norms), cells


def record():
    out = {}
    for dim, p, n, kind in all_cases():
        if is_recorded(dim, p, n):
            u, norms, cells = compute(dim, p, n, kind)
            k = key_of(dim, p, n, kind)
            out[k + "_u"], out[k + "_norms"], out[k + "_cells"] = u, norms, cells
            print(k, norms, flush=True)
    np.savez(GOLDEN, **out)
    print("wrote %s: %d bytes" % (GOLDEN, os.path.getsize(GOLDEN)))


if __name__ == "__main__":
    record()
