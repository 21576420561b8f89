"""tests/post_ref.py without a GPU: the recorded oracle references of
tests/test_gpu_post.py are complete and are what the oracle computes, and the
reordering of the oracle's cell quadrature points to gdm_add_load's grid layout
is the one the device documents."""
import numpy as np
import pytest

import post_ref as PR


def test_every_slow_case_is_recorded_and_no_other():
    g = np.load(PR.GOLDEN)
    want = {PR.key_of(*c) for c in PR.all_cases() if PR.is_recorded(*c[:3])}
    have = {k[:-2] for k in g.files if k.endswith("_u")}
    assert have == want
    for dim, p, n, kind in PR.all_cases():
        if PR.is_recorded(dim, p, n):
            m = PR.mesh_of(dim, p, n)
            k = PR.key_of(dim, p, n, kind)
            assert g[k + "_u"].shape == (m.n_dofs,) and g[k + "_cells"].shape == (m.n_cells,)
            assert g[k + "_norms"].shape == (3,) and np.all(g[k + "_norms"] > 0.0)
            # the recorded field is the one field() builds (numpy's Generator stream has not moved)
            u = PR.field(m, kind, PR.kind_params(kind, dim), PR.T, PR.seed_of(dim, p, n, kind))
            assert np.allclose(g[k + "_u"], u, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("kind", [1, PR.KIND_GRID])
def test_recorded_reference_is_the_oracle(kind):
    """the cheapest recorded mesh (2 s per call), recomputed from the recorded
    field: 1e-13, the oracle being compiled where the test runs"""
    dim, p, n = 3, 7, (8, 7, 9)
    assert PR.is_recorded(dim, p, n)
    m, u, norms, cells = PR.case_reference(dim, p, n, kind)
    ref, ref_cells = PR.reference(m, u, kind, PR.kind_params(kind, dim), PR.T)
    np.testing.assert_allclose(norms, ref, rtol=1e-13, atol=0)
    np.testing.assert_allclose(cells, ref_cells, rtol=1e-13, atol=0)


@pytest.mark.parametrize("dim,n", [(1, (4,)), (2, (3, 2)), (3, (2, 3, 4))])
def test_grid_layout(dim, n):
    p = 3
    m = PR.mesh_of(dim, p, n)
    xq = m.cell_qpoints()
    n1 = p + 1
    Q = [n[d] * n1 if d < dim else 1 for d in range(3)]
    for d in range(dim):
        X = PR.grid_layout(m, xq[:, d]).reshape(Q[2], Q[1], Q[0])
        line = np.moveaxis(X, 2 - d, 0).reshape(Q[d], -1)
        assert np.all(line == line[:, :1]) and np.all(np.diff(line[:, 0]) > 0)
        assert line[0, 0] > PR.LO[d] and line[-1, 0] < PR.HI[d]


def test_case_tables():
    """the shapes test_gpu_post.py relies on"""
    for dim, p, n in PR.WRAP_CASES:
        assert -(-n[0] // 64) * int(np.prod(n[1:])) > 2 * 1024
    assert len(PR.KIND_CASES) == 2 * 5 * 4 and all(min(n) >= p for _, p, n, _ in PR.KIND_CASES)
    # the cone's rim crosses cells of every kind mesh: some quadrature points are inside, some outside
    for dim, p, n, kind in PR.KIND_CASES:
        if kind == 1 and p <= 5:
            m = PR.mesh_of(dim, p, n)
            v = PR.exact(1, PR.cone(dim), m.cell_qpoints(), PR.T, dim).reshape(m.n_cells, -1)
            assert np.any((v > 0).any(axis=1) & (v == 0).any(axis=1))
