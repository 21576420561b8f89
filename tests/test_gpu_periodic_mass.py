"""The exact, direct mass inverse with periodicity constraints on the device
(gdm_mass_solve_periodic / _rk, replacing the SolverCG of
prototypes/advection_01_gdm.cc:208-217) against the numpy reference of
tests/periodic_mass_ref.py (dense condensed 1D solves direction by direction,
pinned to a sparse solve of the condensed cell-loop matrix by
tests/test_periodic_mass_cpu.py).

Bound: relative L2 <= 1e-12, the bound of the exact non-periodic inverse
(tests/test_gpu_parity.py); the numpy restatement of the device arithmetic
stays at or below 1.2e-13 on these shapes.  Shapes are ragged (no two axes
alike), cover n = p + 1 (e_0 and m overlap, nothing skipped), lines with
skipped middle rows along x and along y, odd and even x lengths (v2 and v3 x
pass), every periodic mask in 3D, lines longer than one v3 chunk, and meshes
whose passes run the segmented and the whole-line kernels.
"""
import functools

import numpy as np
import pytest

import cut1d
import oracle as O
import periodic_mass_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-12


def dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float64, order="C")).cuda()  # a copy: the cached cases are read only


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@functools.lru_cache(maxsize=None)
def case(dim, p, n, mask):
    """mesh, reference, a condensed random rhs and its reference solution (computed once, read only)"""
    m = O.Mesh(dim, p, n)
    ref = R.PeriodicMassRef(m, mask)
    b = ref.condense(np.random.default_rng(11 + mask).uniform(-1, 1, m.n_dofs))
    x = ref.solve(b)
    b.setflags(write=False)
    x.setflags(write=False)
    return m, ref, b, x


def make_op(dim, p, n, mask, kind="mass", params=()):
    import gdm_amd

    return gdm_amd.GdmOperator(dim, p, n, 0.0, 1.0, kind, params=params, periodic=mask)


CASES = ([(1, 3, 30, 1), (1, 5, 6, 1), (1, 9, 200, 1)] +
         [(2, 5, (11, 13), k) for k in (1, 2, 3)] +
         [(2, 3, (200, 9), 3), (2, 3, (9, 200), 3), (2, 9, (19, 25), 3)] +
         [(3, 3, (6, 7, 8), k) for k in range(1, 8)] +
         [(3, 7, (9, 8, 60), 4), (3, 7, (9, 8, 60), 7)] +
         [(3, 3, (255, 255, 12), 7)])


@pytest.mark.parametrize("dim,p,n,mask", CASES)
def test_solve_vs_reference(dim, p, n, mask):
    """out of place and in place against the reference; garbage on the
    constrained rhs entries changes no bit; x[constrained] == x[master]
    exactly; M x reproduces the condensed rhs"""
    m, ref, b, x_ref = case(dim, p, n, mask)
    op = make_op(dim, p, n, mask)
    rhs = dev(b)
    x = op.new_vector(False)
    op.mass_solve_periodic(rhs, x)
    xh = host(x)
    err = rel(xh, x_ref)
    print("periodic mass solve %s p %d n %s mask %d: rel L2 %.3e" % (dim, p, n, mask, err))
    assert err <= TOL
    assert torch.equal(rhs, dev(b))  # the out-of-place solve leaves rhs alone
    assert np.array_equal(xh[ref.constrained], xh[ref.master[ref.constrained]])
    # in place
    y = dev(b)
    op.mass_solve_periodic(y, y)
    assert torch.equal(y, x)
    # garbage on the constrained entries
    g = b.copy()
    g[ref.constrained] = np.random.default_rng(3).uniform(-50, 50, int(ref.constrained.sum()))
    z = op.new_vector(False)
    op.mass_solve_periodic(dev(g), z)
    assert torch.equal(z, x)
    zi = dev(g)
    op.mass_solve_periodic(zi, zi)
    assert torch.equal(zi, x)
    # round trip
    r = op.new_vector(False)
    op.mass_apply(x, r)
    rh = host(r)
    free = ~ref.constrained
    back = rel(rh[free], b[free])
    print("  round trip %.3e" % back)
    assert back <= TOL
    assert np.all(rh[ref.constrained] == 0.0)


def test_whole_line_kernels_full_size_planes():
    """65536 lines in every pass: no pass is segmented, the whole-line kernels
    run in place (255^3 cells, all directions periodic; Kronecker reference),
    and the RK form on it"""
    dim, p, n, mask = 3, 3, (255, 255, 255), 7
    m = O.Mesh(dim, p, n)
    ref = R.PeriodicMassRef(m, mask)
    b = np.random.default_rng(5).uniform(-1, 1, m.n_dofs)
    x_ref = ref.solve(b)
    op = make_op(dim, p, n, mask)
    x = dev(b)
    op.mass_solve_periodic(x, x)
    xh = host(x)
    err = rel(xh, x_ref)
    print("periodic mass solve 255^3: rel L2 %.3e" % err)
    assert err <= TOL
    X = xh.reshape(256, 256, 256)
    assert np.array_equal(X[-1], X[0]) and np.array_equal(X[:, -1], X[:, 0]) and np.array_equal(X[..., -1], X[..., 0])
    _check_rk_bits(op, dev(b), x)


def _check_rk_bits(op, rhs, k):
    """the three argument patterns of the low-storage RK4 against solve + rk_update"""
    n = rhs.numel()
    g = torch.Generator(device="cpu").manual_seed(1)
    y = torch.rand(n, dtype=torch.float64, generator=g).cuda()
    acc = torch.rand(n, dtype=torch.float64, generator=g).cuda()
    beta, alpha = 0.0371, 0.0186
    # stage 0: acc_in == y, acc_out = acc, Y
    acc_ref, Y_ref = torch.empty_like(y), torch.empty_like(y)
    op.rk_update(beta, k, y, acc_ref, alpha, y, Y_ref)
    acc_o, Y_o, r = torch.empty_like(y), torch.empty_like(y), rhs.clone()
    op.mass_solve_periodic_rk(r, beta, y, acc_o, alpha, y, Y_o)
    assert torch.equal(acc_o, acc_ref) and torch.equal(Y_o, Y_ref)
    # middle stages: acc_in == acc_out, Y
    a_ref, a_o = acc.clone(), acc.clone()
    op.rk_update(beta, k, a_ref, a_ref, alpha, y, Y_ref)
    r = rhs.clone()
    op.mass_solve_periodic_rk(r, beta, a_o, a_o, alpha, y, Y_o)
    assert torch.equal(a_o, a_ref) and torch.equal(Y_o, Y_ref)
    # last stage: no Y, acc_out another vector
    out_ref, out_o = torch.empty_like(y), torch.empty_like(y)
    op.rk_update(beta, k, acc, out_ref)
    r = rhs.clone()
    op.mass_solve_periodic_rk(r, beta, acc, out_o)
    assert torch.equal(out_o, out_ref)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dim,p,n,mask", [(1, 3, 30, 1), (2, 5, (11, 13), 2), (2, 3, (200, 9), 3),
                                          (3, 7, (9, 8, 60), 7), (3, 3, (255, 255, 12), 7)])
def test_rk_form_bits(dim, p, n, mask):
    m, ref, b, _ = case(dim, p, n, mask)
    op = make_op(dim, p, n, mask)
    k = dev(b)
    op.mass_solve_periodic(k, k)
    _check_rk_bits(op, dev(b), k)
    import gdm_amd

    with pytest.raises(gdm_amd.GdmError):  # rhs must not alias an output
        v = dev(b)
        op.mass_solve_periodic_rk(v, 0.1, k, v)


def test_against_cg():
    import gdm_amd  # noqa: F401

    dim, p, n, mask = 2, 5, (11, 13), 3
    m, ref, b, x_ref = case(dim, p, n, mask)
    op = make_op(dim, p, n, mask)
    x = op.new_vector(False)
    op.mass_solve_cg(dev(b), x, rel_tol=1e-12, abs_tol=1e-20, max_it=1000, precond=1)
    op.distribute(x)
    d = op.new_vector(False)
    op.mass_solve_periodic(dev(b), d)
    assert rel(host(d), host(x)) <= 1e-10


@pytest.mark.parametrize("dim,p,n", [(2, 5, (11, 13)), (3, 3, (6, 7, 8)), (1, 9, 40)])
def test_nonperiodic_operator_gives_mass_solve_bits(dim, p, n):
    m = O.Mesh(dim, p, n)
    op = make_op(dim, p, n, 0)
    rng = np.random.default_rng(2)
    b, yv, av = (dev(rng.uniform(-1, 1, m.n_dofs)) for _ in range(3))
    x0, x1 = op.new_vector(False), op.new_vector(False)
    op.mass_solve(b, x0)
    op.mass_solve_periodic(b, x1)
    assert torch.equal(x0, x1)
    assert rel(host(x1), m.kron_mass_inverse(host(b))) <= TOL
    o0, o1, Y0, Y1 = (op.new_vector(False) for _ in range(4))
    op.mass_solve_rk(b.clone(), 0.3, av, o0, 0.2, yv, Y0)
    op.mass_solve_periodic_rk(b.clone(), 0.3, av, o1, 0.2, yv, Y1)
    assert torch.equal(o0, o1) and torch.equal(Y0, Y1)


@pytest.mark.parametrize("dim,p,n,mask", [(2, 5, (11, 13), 3), (3, 3, (6, 7, 8), 7), (2, 3, (200, 9), 3)])
def test_repeatable_across_runs_streams_and_graph(dim, p, n, mask):
    m, ref, b, x_ref = case(dim, p, n, mask)
    rhs = dev(b)
    # another operator's solve loads the kernels; the graph below is captured
    # as its operator's very first call (everything allocated at creation)
    other = make_op(dim, p, n, mask)
    other.mass_solve_periodic(rhs, other.new_vector(False))
    torch.cuda.synchronize()
    op = make_op(dim, p, n, mask)
    xg = op.new_vector(False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            op.mass_solve_periodic(rhs, xg)
    torch.cuda.synchronize()
    op.use_torch_stream()
    x = op.new_vector(False)
    op.mass_solve_periodic(rhs, x)
    assert rel(host(x), x_ref) <= TOL
    for _ in range(2):
        xg.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg, x)
    x2 = op.new_vector(False)
    op.mass_solve_periodic(rhs, x2)
    assert torch.equal(x2, x)
    x3 = op.new_vector(False)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        op.use_torch_stream()
        op.mass_solve_periodic(rhs, x3)
    torch.cuda.synchronize()
    op.use_torch_stream()
    assert torch.equal(x3, x)


def test_refusals():
    import gdm_amd

    op2 = gdm_amd.GdmOperator(2, 3, (9, 20), 0.0, 1.0, "mass", rank=0, n_ranks=2)
    v = op2.new_vector(False)
    with pytest.raises(gdm_amd.GdmError):
        op2.mass_solve_periodic(v, v.clone())
    with pytest.raises(gdm_amd.GdmError):
        op2.mass_solve_periodic_rk(v, 0.1, v.clone(), v.clone())
    op = make_op(2, 3, (9, 11), 3)
    w = op.new_vector(False)
    with pytest.raises(gdm_amd.GdmError, match="gdm_mass_solve_periodic"):
        op.mass_solve(w, w.clone())
    with pytest.raises(gdm_amd.GdmError):
        op.mass_solve_rk(w, 0.1, w.clone(), w.clone())


def _exact(m, t, a):
    X = m.vertex_coords()
    v = np.sin(2.0 * np.pi * (X[0] - a[0] * t))
    for d in range(1, m.dim):
        v = v * np.cos(2.0 * np.pi * (X[d] - a[d] * t))
    return v


@pytest.mark.parametrize("dim,p,n,steps", [(1, 5, 40, None), (2, 5, 12, 3)])
def test_advection_01_direct(dim, p, n, steps):
    """Advection01(mass_solver="direct") against the oracle's RK4 with the
    exact periodic inverse (<= 1e-11) and against the CG run (<= 1e-6: the
    CG's rel 1e-8 per solve)"""
    import gdm_amd

    a = (1.0, 0.15, -0.05)[:dim]
    mask = (1 << dim) - 1
    m = O.Mesh(dim, p, n)
    ref = R.PeriodicMassRef(m, mask)
    u0 = _exact(m, 0.0, a)
    dt = 1.0 / n * 0.5
    u = u0.copy()
    time = cut1d.DiscreteTime(0.0, 0.1, dt)
    k = 0
    f = lambda t, y: ref.solve(ref.condense(m.convective_rhs(a, ref.distribute(y))))  # noqa: E731
    while not time.is_at_end() and (steps is None or k < steps):
        u = ref.distribute(cut1d.rk4_step(f, time.t, time.next_step_size(), u))
        time.advance()
        k += 1
    res = {}
    for solver in ("direct", "cg"):
        op = make_op(dim, p, n, mask, "convective", a)
        prob = gdm_amd.Advection01(op, mass_solver=solver)
        prob.u.copy_(dev(u0))
        assert prob.run(0.0, 0.1, dt, max_steps=steps) == k
        res[solver] = (host(prob.u).copy(), list(prob.cg_iterations))
    err = rel(res["direct"][0], u)
    diff = rel(res["direct"][0], res["cg"][0])
    print("Advection01 direct vs oracle RK4 %.3e, vs cg run %.3e" % (err, diff))
    assert err <= 1e-11
    assert diff <= 1e-6
    assert res["direct"][1] == []
    assert len(res["cg"][1]) == 4 * k
