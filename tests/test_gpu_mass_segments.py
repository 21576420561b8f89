"""Segmented line solves of the exact mass inverse (gdm_mass.hip: a pass
with fewer than 1024 waves of lines splits every line into segments of >= 1
chunk, each with a forward warm-up chunk before and a backward warm-up chunk
after it, and the passes run out of place through a scratch vector).  The
warm-ups start the recurrences from zero C = 48 / 48 / 56 positions (p = 3 /
5 / 7) before the segment; the factors' homogeneous solutions decay below
1e-16 within that distance, so the segmented inverse agrees with the exact
one to rounding: test_segmented_error_level pins the achieved level.  Small
meshes take this path: BASELINE C2 (2D 1024^2: 16 waves per pass), long 1D
lines, thin 3D slabs.  Checked against the oracle's Kronecker inverse
(== CG rel 1e-14 of the reference's solve) and by M^-1 (M u) == u, in and
out of place."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402


def _gdm():
    import gdm_amd

    return gdm_amd


@pytest.mark.parametrize("dim,n,p", [(2, (400, 30), 5), (2, (30, 400), 5), (1, 2000, 3), (2, (500, 20), 7),
                                     (3, (250, 12, 9), 5)])
def test_segmented_solve_vs_kronecker(dim, n, p):
    g = _gdm()
    op = g.GdmOperator(dim, p, n, -0.3, 1.1, "mass")
    m = O.Mesh(dim, p, list(n) if dim > 1 else n, -0.3, 1.1)
    r = np.random.default_rng(dim * 10 + p).uniform(-1, 1, m.n_dofs)
    ref = m.kron_mass_inverse(r)
    x = op.new_vector(local=False)
    op.mass_solve(torch.from_numpy(r).cuda(), x)
    got = x.cpu().numpy()
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-12
    # in place (rhs aliases the result: the first pass's input is moved aside)
    y = torch.from_numpy(r).cuda()
    op.mass_solve(y, y)
    assert float(np.linalg.norm(y.cpu().numpy() - got)) == 0.0


def test_c2_mass_inverse_round_trip():
    """BASELINE C2: 2D advection mesh 1024^2, p = 5"""
    g = _gdm()
    op = g.GdmOperator(2, 5, 1023, 0.0, 1.0, "advection", params=(1.8126, 0.8452))
    gen = torch.Generator(device="cuda").manual_seed(11)
    u = torch.rand(op.n_owned, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    Mu, x = op.new_vector(local=False), op.new_vector(local=False)
    op.mass_apply(u, Mu)
    op.mass_solve(Mu, x)
    assert float(torch.linalg.norm(x - u) / torch.linalg.norm(u)) < 1e-12


@pytest.mark.parametrize("p", [3, 5, 7])
def test_segmented_error_level(p):
    """Achieved accuracy of the segmented path (1-chunk segments: the C2-like
    2D mesh with few lines per pass) against the oracle's exact Kronecker
    inverse, per p: at the level of fp64 rounding of the exact path (the
    whole-line kernels agree with the same reference to ~1e-16)."""
    g = _gdm()
    op = g.GdmOperator(2, p, (700, 40), 0.0, 1.0, "mass")
    m = O.Mesh(2, p, [700, 40], 0.0, 1.0)
    r = np.random.default_rng(100 + p).uniform(-1, 1, m.n_dofs)
    ref = m.kron_mass_inverse(r)
    x = op.new_vector(local=False)
    op.mass_solve(torch.from_numpy(r).cuda(), x)
    err = float(np.linalg.norm(x.cpu().numpy() - ref) / np.linalg.norm(ref))
    print("segmented mass inverse p=%d: rel-L2 %.3e" % (p, err))
    assert err < 2e-15
