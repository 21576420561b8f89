"""gdm_csr_vmult with a matrix that has more rows than columns: the
interpolation matrix (B_z (x) B_y (x) B_x) from the nodes to the Gauss grid,
assembled here with scipy (as tests/fastdiag_ref.py uses it) from
gdm_coef_grid_tables_1d: the matrix that tools/bench_evalgrid.py takes as its
SpMV yardstick.  The SpMV kernels used to read src[row] for every row even when
no dot-product partials were asked for, which lies outside src once n_rows >
n_cols.

The product equals scipy's (rel-L2 1e-13: the same sums in another order) and
the values of gdm_eval_grid (1e-12, the bound of tests/test_gpu_evalgrid.py).
"""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def interpolation_matrix(op):
    """(B_z (x) B_y (x) B_x) as scipy CSR, x fastest, from the kernel's 1D tables"""
    n1 = op.p + 1
    E = None
    for d in range(op.dim):
        val, _, first = op.coef_grid_tables_1d(d)
        val, first = np.asarray(val).reshape(-1, n1), np.asarray(first).reshape(-1)
        rows = np.repeat(np.arange(val.shape[0]), n1)
        cols = (first[:, None] + np.arange(n1)[None, :]).reshape(-1)
        B = sp.csr_matrix((val.reshape(-1), (rows, cols)), shape=(val.shape[0], op.mesh.n_subdivisions[d] + 1))
        E = B if E is None else sp.kron(B, E, format="csr")
    return E


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("dim,p,n_sub", [(3, 3, (12, 9, 10)), (2, 5, (9, 14)), (1, 1, (40,))])
def test_tall_matrix_vmult(dim, p, n_sub):
    import gdm_amd

    op = gdm_amd.GdmOperator(dim, p, n_sub, 0.0, 1.0, "wave")
    E = interpolation_matrix(op)
    assert E.shape == (op.n_grid_points, op.n_owned) and E.shape[0] > E.shape[1]
    M = gdm_amd.SparseMatrix.from_scipy(E)
    uh = np.random.default_rng(p).uniform(-1, 1, op.n_owned)
    u = torch.from_numpy(uh).cuda()
    y = torch.zeros(op.n_grid_points, dtype=torch.float64, device="cuda")
    M.vmult(y, u)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert _rel(got, E @ uh) <= 1e-13
    uq = op.eval_grid(u, gradients=False)
    torch.cuda.synchronize()
    r = _rel(uq.cpu().numpy(), got)
    print("eval_grid vs the assembled interpolation %dD p=%d: %.2e" % (dim, p, r))
    assert r <= 1e-12
