"""Device-resident time integration: the RK drivers of the reference's
problems over the C ABI, every vector in HBM.

  AdvectionProblem   applications/advection/include/gdm/advection/problem.h:31-102
                     (non-composite branch): y = (block(0) boundary values,
                     block(1) u); f(t, y) = (dg/dt, M^-1 (K u + inflow data))
  WaveProblem        applications/wave/include/gdm/wave/problem.h:280-346
                     (wave-rk): y = (u, v); f(t, y) = (v, M^-1 K u)

Both use TimeStepping::ExplicitRungeKutta with RK_CLASSIC_FOURTH_ORDER and
DiscreteTime, restated in low-storage form: the b-weighted sum of the stages
is accumulated as each stage is produced (gdm_vec_rk_update: one pass writes
the accumulator and the next stage vector), in the same order as deal.II's
final y.sadd loop, so no per-stage BlockVector is allocated (problem.h:64-65)
and nothing crosses PCIe inside the loop.  Block(0) of the advection problem
is g(t_n) at the start of every step (initialize_time_step,
advection/stiffness.h:181-194) and dg/dt at the stage times
(stiffness.h:286-289), both evaluated on the device for the built-in
boundary functions.  By default block(0) is not stored at all: stage s reads
y0 + h a_{s,s-1} k_{s-1} = g(t_n) + h a dg/dt(t_n + c_{s-1} h), which the
engine computes per stage itself (gdm_apply_bc_fn, the same bits as
gdm_eval_boundary + gdm_vec_rk_update); block(0) after a step is never read
by the reference (initialize_time_step overwrites it, problem.h:88-90).
carry_bc=True keeps the explicit block(0) vectors (gdm_eval_boundary).
"""
from ._capi import GdmError

# RK_CLASSIC_FOURTH_ORDER (deal.II TimeStepping): c, a_{i,i-1}, b
RK4_C = (0.0, 0.5, 0.5, 1.0)
RK4_A = (0.5, 0.5, 1.0)
RK4_B = (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)


class DiscreteTime:
    """deal.II DiscreteTime (base/discrete_time.cc): the next time is the
    current one plus the last step, the step recomputed as the difference of
    the two times (round-off accumulates as in the reference), snapped to the
    end time when within 5 % of a step of it."""

    def __init__(self, start, end, dt):
        self.t, self.end, self.step = float(start), float(end), 0
        self._next = self._next_time(self.t, float(dt))

    def _next_time(self, current, step):
        n = current + step
        if step > 0.0 and n > self.end - 0.05 * step:
            n = self.end
        return n

    def is_at_end(self):
        return self.t == self.end

    def next_step_size(self):
        return self._next - self.t

    def advance(self):
        step = self._next - self.t
        self.t = self._next
        self._next = self._next_time(self.t, step)
        self.step += 1

class WaveProblem:
    """wave-rk on one rank: du/dt = v, dv/dt = M^-1 (K u + (v, f(t)) + Nitsche
    data of g_D(t)) with K the wave operator of `op` (kind "wave": -(grad v,
    grad u) [+ box Nitsche]) -- compute_rhs(dst, src, true, time),
    wave/stiffness.h:409-420.

    forcing: None, (fn_kind, params, scale) for scale * a built-in function
    (GdmOperator.add_load_fn), or a callable t -> device array on the
    quadrature grid (add_load).  dirichlet: None, (fn_kind, params) for a
    built-in g_D (eval_boundary), or a callable t -> device array of
    n_bc_points values in device order (add_dirichlet_data; needs an operator
    with nitsche > 0).  Both are taken at the stage times t + c_s h.  With both
    None the launches are those of the homogeneous problem.

    With a density set on `op` (GdmOperator.set_density) the mass is M[rho]:
    every stage's k comes from GdmOperator.density_solve (direct for one term;
    a sum by CG from a zero guess with rel_tol / abs_tol / max_it, the counts
    appended to `iterations`), then rk_update."""

    def __init__(self, op, forcing=None, dirichlet=None, rel_tol=1e-8, abs_tol=1e-30, max_it=1000):
        if op.mesh.n_ranks != 1:
            raise GdmError("WaveProblem: single-rank driver (multi-rank: gdm_amd.distributed)")
        self.op = op
        self.rel_tol, self.abs_tol, self.max_it = rel_tol, abs_tol, max_it
        self.iterations = []
        self._ks = None
        n = op.n_owned
        self.u, self.v = op.new_vector(False), op.new_vector(False)
        self._acc = [op.new_vector(False) for _ in range(2)]
        self._Y = [op.new_vector(False) for _ in range(2)]
        self._kv = op.new_vector(False)
        self.n = n
        self.forcing, self.dirichlet = forcing, dirichlet
        self._g = None
        if dirichlet is not None and not callable(dirichlet):
            import torch

            self._g = torch.zeros(max(op.n_bc_points, 1), dtype=torch.float64, device="cuda:%d" % op.device)
            self._g = self._g[:op.n_bc_points]

    def add_data(self, t, out):
        """out += (v, f(t)) + the Nitsche data of g_D(t) (stiffness.h:196-200, 320-326)"""
        op = self.op
        if self.forcing is not None:
            if callable(self.forcing):
                op.add_load(self.forcing(t), out)
            else:
                fn, prm, scale = self.forcing
                op.add_load_fn(fn, prm, t, out, 0, scale)
        if self.dirichlet is not None:
            if callable(self.dirichlet):
                op.add_dirichlet_data(self.dirichlet(t), out)
            else:
                fn, prm = self.dirichlet
                op.eval_boundary(fn, prm, t, 0, self._g)
                op.add_dirichlet_data(self._g, out)
        return out

    def rhs(self, t, U, out):
        """dv/dt = M^-1 compute_rhs(U, t) (wave/problem.h:313-317)"""
        self.op.apply(U, out)
        self.add_data(t, out)
        if self._density():
            out.copy_(self._density_stage(out))
        else:
            self.op.mass_solve(out, out)
        return out

    def _density(self):
        """whether the operator carries a density (GdmOperator.set_density)"""
        return getattr(self.op, "has_density", False) is True

    def _density_stage(self, rhs):
        """k = M[rho]^-1 rhs: direct for one term, else CG from a zero guess"""
        if self._ks is None:
            self._ks = self.op.new_vector(False)
        self._ks.zero_()
        its, _ = self.op.density_solve(rhs, self._ks, self.rel_tol, self.abs_tol, self.max_it)
        self.iterations.append(its)
        return self._ks

    def step(self, t, h):
        op, y = self.op, (self.u, self.v)
        acc, Y, kv = self._acc, self._Y, self._kv
        stage = y
        data = self.forcing is not None or self.dirichlet is not None
        for s in range(4):
            # k = (stage_v, M^-1 (K stage_u + data(t + c_s h)))
            op.apply(stage[0], kv)
            if data:
                self.add_data(t + RK4_C[s] * h, kv)
            ku = stage[1]
            last = s == 3
            acc_in = y if s == 0 else acc
            acc_out = y if last else acc
            a_next = 0.0 if last else h * RK4_A[s]
            # u block first (stage_u is consumed): it reads ku = stage_v before
            # the v block overwrites Y_v
            op.rk_update(h * RK4_B[s], ku, acc_in[0], acc_out[0], a_next, None if last else y[0],
                         None if last else Y[0])
            if self._density():
                op.rk_update(h * RK4_B[s], self._density_stage(kv), acc_in[1], acc_out[1], a_next,
                             None if last else y[1], None if last else Y[1])
            else:
                # v block: the mass solve with the update fused into its last pass
                op.mass_solve_rk(kv, h * RK4_B[s], acc_in[1], acc_out[1], a_next, None if last else y[1],
                                 None if last else Y[1])
            stage = Y

    def run(self, start_t, end_t, dt, max_steps=None, callback=None):
        time = DiscreteTime(start_t, end_t, dt)
        n = 0
        while not time.is_at_end() and (max_steps is None or n < max_steps):
            h = time.next_step_size()
            self.step(time.t, h)
            n += 1
            if callback is not None:
                callback(time.t + h, self)
            time.advance()
        return n


class HeatProblem(WaveProblem):
    """heat-impl and heat-rk on one rank and an uncut box (wave/problem.h:
    210-279 and 72-128): M du/dt = K u + data(t), K the wave operator of `op`,
    data(t) = (v, f(t)) + the Nitsche data of g_D(t) (WaveProblem.add_data;
    forcing / dirichlet as there).

    scheme "impl": backward Euler, (M + h S) u_new = M u + h data(t + h) with
    S = -K, solved directly (GdmOperator.system_solve(1, h)); h is the
    DiscreteTime step of every step, so a shorter last step needs no new setup.
    scheme "rk": classic RK4 of du/dt = M^-1 (K u + data(t)) through apply +
    mass_solve_rk.

    With a coefficient set on `op` (GdmOperator.set_coefficient) scheme "impl"
    solves by GdmOperator.coef_solve(1, h) from the previous step's solution
    with rel_tol / abs_tol / max_it; `iterations` lists the CG counts of the
    steps taken.  With a density set (GdmOperator.set_density) the mass is
    M[rho]: scheme "impl" takes its right-hand side from density_apply and
    solves (M[rho] + h S[kappa]) by coef_solve, scheme "rk" takes every stage
    from density_solve (see WaveProblem)."""

    def __init__(self, op, forcing=None, dirichlet=None, scheme="impl", rel_tol=1e-8, abs_tol=1e-30, max_it=1000):
        if scheme not in ("impl", "rk"):
            raise GdmError("HeatProblem: scheme is 'impl' or 'rk'")
        WaveProblem.__init__(self, op, forcing, dirichlet, rel_tol, abs_tol, max_it)
        self.scheme = scheme
        if scheme == "impl":
            op.system_solve_setup()

    def step(self, t, h):
        op, u, k = self.op, self.u, self._kv
        if self.scheme == "impl":
            if self._density():
                op.density_apply(u, k)
            else:
                op.mass_apply(u, k)
            if self.forcing is not None or self.dirichlet is not None:
                data = self._Y[0]
                data.zero_()
                self.add_data(t + h, data)
                op.axpby(h, data, 1.0, k)
            if op.has_coefficient or self._density():
                its, _ = op.coef_solve(1.0, h, k, u, self.rel_tol, self.abs_tol, self.max_it)
                self.iterations.append(its)
            else:
                op.system_solve(1.0, h, k, u)
            return
        acc, Y = self._acc[0], self._Y[0]
        stage = u
        for s in range(4):
            op.apply(stage, k)
            self.add_data(t + RK4_C[s] * h, k)
            last = s == 3
            if self._density():
                op.rk_update(h * RK4_B[s], self._density_stage(k), u if s == 0 else acc, u if last else acc,
                             0.0 if last else h * RK4_A[s], None if last else u, None if last else Y)
            else:
                op.mass_solve_rk(k, h * RK4_B[s], u if s == 0 else acc, u if last else acc,
                                 0.0 if last else h * RK4_A[s], None if last else u, None if last else Y)
            stage = Y


class QuasilinearHeatProblem:
    """Quasi-linear heat conduction u_t = M^-1 (K[kappa(u)] u + data(t)) on one
    rank and an uncut box by classic RK4: K[kappa] the wave operator of `op`
    (kind "wave") with the coefficient on the Gauss grid
    (GdmOperator.set_coefficient_grid), kappa re-evaluated from the stage
    vector before every stage's apply.

    kappa: a callable on device tensors, elementwise, with values > 0 (for
    instance lambda u: 1 + u * u).  The problem owns the grid arrays kq and kbc
    that the engine borrows.  They are set once, from the initial u, by the
    first step (the only set call, with its check that kappa > 0); after that
    every stage refreshes them in place, kq.copy_(kappa(eval_grid(stage))) and,
    with nitsche > 0, kbc.copy_(kappa(eval_trace(stage))): no set call, no
    reduction and no host synchronisation per stage.  Positivity of kappa at
    the later stages is therefore the caller's responsibility: a sample that
    is not positive is not reported, the step is then not parabolic.

    forcing / dirichlet as in WaveProblem (add_data); the Dirichlet data term
    uses the refreshed kbc."""

    def __init__(self, op, kappa, forcing=None, dirichlet=None):
        import torch

        from .operator import KINDS

        if op.mesh.n_ranks != 1:
            raise GdmError("QuasilinearHeatProblem: single-rank driver")
        if op.kind != KINDS["wave"]:
            raise GdmError("QuasilinearHeatProblem: a 'wave' operator is needed")
        if not callable(kappa):
            raise GdmError("QuasilinearHeatProblem: kappa is a callable on device tensors")
        if dirichlet is not None and not op.nitsche > 0.0:
            raise GdmError("QuasilinearHeatProblem: Dirichlet data needs an operator with nitsche > 0")
        self.op, self.kappa = op, kappa
        self.forcing, self.dirichlet = forcing, dirichlet
        dev = "cuda:%d" % op.device
        # the boundary values of a built-in g_D (add_data)
        self._g = None
        if dirichlet is not None and not callable(dirichlet):
            self._g = torch.zeros(op.n_bc_points, dtype=torch.float64, device=dev)
        self.u = op.new_vector(False)
        self._acc, self._Y, self._k = (op.new_vector(False) for _ in range(3))
        self.kq = torch.empty(op.n_grid_points, dtype=torch.float64, device=dev)
        self._uq = torch.empty_like(self.kq)
        self._face = op.nitsche > 0.0 and op.n_bc_points > 0
        self.kbc = torch.empty(op.n_bc_points, dtype=torch.float64, device=dev) if self._face else None
        self._ubc = torch.empty_like(self.kbc) if self._face else None
        self._set = False
        self.last_stage = None

    def refresh(self, stage):
        """kq (and kbc) = kappa of the stage vector at the Gauss points (the boundary points), in place"""
        op = self.op
        self.kq.copy_(self.kappa(op.eval_grid(stage, self._uq, False)))
        if self._face:
            self.kbc.copy_(self.kappa(op.eval_trace(stage, self._ubc, False)))

    def rhs(self, t, stage, out):
        """out = K[kappa(stage)] stage + data(t)"""
        self.refresh(stage)
        if not self._set:
            self.op.set_coefficient_grid(self.kq, self.kbc)
            self._set = True
        self.op.apply(stage, out)
        self.add_data(t, out)
        return out

    add_data = WaveProblem.add_data

    def step(self, t, h):
        op, u, k = self.op, self.u, self._k
        acc, Y = self._acc, self._Y
        stage = u
        for s in range(4):
            self.last_stage = stage  # kq / kbc hold kappa of this vector until the next refresh
            self.rhs(t + RK4_C[s] * h, stage, k)
            last = s == 3
            op.mass_solve_rk(k, h * RK4_B[s], u if s == 0 else acc, u if last else acc,
                             0.0 if last else h * RK4_A[s], None if last else u, None if last else Y)
            stage = Y

    def run(self, start_t, end_t, dt, max_steps=None, callback=None):
        time = DiscreteTime(start_t, end_t, dt)
        n = 0
        while not time.is_at_end() and (max_steps is None or n < max_steps):
            h = time.next_step_size()
            self.step(time.t, h)
            n += 1
            if callback is not None:
                callback(time.t + h, self)
            time.advance()
        return n


def solve_poisson(op, forcing=None, dirichlet=None, t=0.0, rel_tol=1e-8, abs_tol=1e-30, max_it=1000, info=None):
    """The "poisson" simulation type (wave/problem.h:46-71) on an uncut box:
    the device solution of S u = data(t), S = -K of the wave operator `op`
    (created with nitsche > 0: without the box Nitsche terms S is singular),
    data as in WaveProblem (forcing / dirichlet).  With a coefficient set on
    `op` the solve is GdmOperator.coef_solve(0, 1) from a zero guess with
    rel_tol / abs_tol / max_it; a dict passed as `info` receives "iterations"
    and "residual"."""
    prob = WaveProblem(op, forcing, dirichlet)
    op.system_solve_setup()
    rhs = prob._kv
    rhs.zero_()
    prob.add_data(t, rhs)
    if op.has_coefficient:
        its, res = op.coef_solve(0.0, 1.0, rhs, prob.u, rel_tol, abs_tol, max_it)
        if info is not None:
            info["iterations"], info["residual"] = its, res
        return prob.u
    return op.system_solve(0.0, 1.0, rhs, prob.u)


def solve_elasticity(op, f_components, exact=None, precond="fastdiag", rel_tol=1e-8, abs_tol=1e-10, max_it=1000):
    """tests/elasticity_01_gdm.cc on the device: the right-hand side (v_c, f_c)
    per component through add_load, preconditioned CG from a zero start on the
    elasticity operator `op`, and, when `exact` is given, the L2 error
    sqrt(sum_c e_c^2) through error_norms_grid.  f_components / exact: one
    array per component on the tensor Gauss grid (op.quadrature_points(), x
    fastest; numpy or device).  Returns (x, iterations) or (x, iterations,
    error), x component-major on the device."""
    import numpy as np
    import torch

    def dev(a):
        if isinstance(a, torch.Tensor):
            return a.reshape(-1)
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).cuda(op.device)

    if len(f_components) != op.n_components:
        raise GdmError("solve_elasticity: %d right-hand sides for %d components" % (len(f_components),
                                                                                 op.n_components))
    rhs, x = op.new_vector_field(), op.new_vector_field()
    for c, f in enumerate(f_components):
        op.add_load(dev(f), op.component(rhs, c))
    its, _ = op.elasticity_solve(rhs, x, precond, rel_tol, abs_tol, max_it)
    if exact is None:
        return x, its
    err2 = 0.0
    for c, e in enumerate(exact):
        err2 += op.error_norms_grid(op.component(x, c), dev(e))[2] ** 2
    return x, its, float(np.sqrt(err2))


class AdvectionProblem:
    """advection problem.h:31-102 on one rank with a built-in boundary
    function (gdm_fn_kind) for g and dg/dt."""

    def __init__(self, op, fn_kind, fn_params, carry_bc=False, field_scale=None):
        if op.mesh.n_ranks != 1:
            raise GdmError("AdvectionProblem: single-rank driver")
        self.op, self.fn, self.prm = op, int(fn_kind), list(fn_params)
        self.carry_bc = bool(carry_bc)
        # field_scale(t) -> the time factors s_t of the operator's separable field
        # at time t: the reference's advection->set_time(time) before every
        # compute_rhs (stiffness.h:339)
        self.field_scale = field_scale
        import torch

        dev = "cuda:%d" % op.device
        # block(0) (the boundary points, ~28 M at C3) exists only on the explicit
        # path: with carry_bc=False the engine computes the stage values itself
        nb = max(op.n_bc_points, 1) if self.carry_bc else 0
        z = lambda m: torch.zeros(m, dtype=torch.float64, device=dev) if m else None  # noqa: E731
        self.u = op.new_vector(False)
        self._bc = z(nb)
        self._acc = [z(nb), op.new_vector(False)]
        self._Y = [z(nb), op.new_vector(False)]
        self._k = [z(nb), op.new_vector(False)]

    @property
    def bc(self):
        """block(0) = g at the boundary points; kept only with carry_bc=True"""
        if not self.carry_bc:
            raise GdmError("AdvectionProblem.bc: block(0) is not kept (carry_bc=False computes the stage "
                           "boundary values on the device)")
        return self._bc

    def initialize_time_step(self, t):
        """block(0) = g(t_n) at the boundary points (stiffness.h:181-194).
        With carry_bc=False there is no block(0) to fill: step() has the
        engine evaluate g(t_n) (+ the stage terms) right before each stencil,
        so this is a no-op and returns False; True when block(0)
        was written."""
        if not self.carry_bc:
            return False
        if self.op.n_bc_points:
            self.op.eval_boundary(self.fn, self.prm, t, 0, self.bc)
        return True

    def _set_time(self, t):
        if self.field_scale is not None:
            self.op.set_field_scale(self.field_scale(t))

    def rhs(self, t, BC, U, kbc, ku):
        op = self.op
        self._set_time(t)
        if op.n_bc_points:
            op.eval_boundary(self.fn, self.prm, t, 1, kbc)  # block(0) = dg/dt (stiffness.h:286-289)
        op.apply(U, ku, BC if op.n_bc_points else None)
        op.mass_solve(ku, ku)

    def step(self, t, h):
        op = self.op
        if not self.carry_bc:
            # block(0) computed by the engine: stage s reads g(t) + alpha dg/dt(t_k)
            y, acc, Y, k = self.u, self._acc[1], self._Y[1], self._k[1]
            stage = y
            for s in range(4):
                alpha, t_k = (0.0, t) if s == 0 else (h * RK4_A[s - 1], t + RK4_C[s - 1] * h)
                self._set_time(t + RK4_C[s] * h)
                op.apply_bc_fn(stage, k, self.fn, self.prm, t, alpha, t_k)
                last = s == 3
                op.mass_solve_rk(k, h * RK4_B[s], y if s == 0 else acc, y if last else acc,
                                 0.0 if last else h * RK4_A[s], None if last else y, None if last else Y)
                stage = Y
            return
        self.initialize_time_step(t)
        y = (self.bc, self.u)
        acc, Y, k = self._acc, self._Y, self._k
        stage = y
        blocks = (0, 1) if op.n_bc_points else (1,)
        for s in range(4):
            self.rhs(t + RK4_C[s] * h, stage[0], stage[1], k[0], k[1])
            last = s == 3
            a_next = 0.0 if last else h * RK4_A[s]
            for b in blocks:
                op.rk_update(h * RK4_B[s], k[b], (y if s == 0 else acc)[b], (y if last else acc)[b], a_next,
                             None if last else y[b], None if last else Y[b])
            stage = Y

    def run(self, start_t, end_t, dt, max_steps=None):
        time = DiscreteTime(start_t, end_t, dt)
        n = 0
        while not time.is_at_end() and (max_steps is None or n < max_steps):
            self.step(time.t, time.next_step_size())
            n += 1
            time.advance()
        return n


class Advection01:
    """prototypes/advection_01_gdm.cc:62-282 (use_mass_lumping = false) on the
    device: periodicity constraints in every direction (:107-110), the
    convective form cell_i -= (a . grad u_q) phi_i JxW (:164-206) on the
    distributed stage vector, SolverCG + PreconditionJacobi with
    ReductionControl(100, 1e-10, 1e-8) from a zero initial guess (:208-217),
    RK_CLASSIC_FOURTH_ORDER + DiscreteTime, constraints.distribute after
    every step (:268).  `op` is a "convective" operator with periodic = all
    directions.

    mass_solver="cg" is the reference's solve.  mass_solver="direct" replaces
    it by the exact periodic mass inverse fused with the stage update
    (GdmOperator.mass_solve_periodic_rk): no CG, cg_iterations stays empty."""

    def __init__(self, op, mass_solver="cg"):
        if op.mesh.n_ranks != 1:
            raise GdmError("Advection01: single rank")
        if mass_solver not in ("cg", "direct"):
            raise GdmError("Advection01: mass_solver is 'cg' or 'direct'")
        self.mass_solver = mass_solver
        self.op = op
        self.u = op.new_vector(False)
        self._acc, self._Y, self._k = (op.new_vector(False) for _ in range(3))
        self.cg_iterations = []

    def rhs(self, U, out):
        op = self.op
        op.apply(U, self._r_tmp())  # distributes a copy of U, condenses the result
        out.zero_()
        its, _ = op.mass_solve_cg(self._r, out, rel_tol=1e-8, abs_tol=1e-10, max_it=100, precond=1)
        self.cg_iterations.append(its)
        return out

    def _r_tmp(self):
        if not hasattr(self, "_r"):
            self._r = self.op.new_vector(False)
        return self._r

    def step(self, t, h):
        op, y = self.op, self.u
        acc, Y, k = self._acc, self._Y, self._k
        stage = y
        direct = self.mass_solver == "direct"
        for s in range(4):
            last = s == 3
            upd = (h * RK4_B[s], y if s == 0 else acc, y if last else acc, 0.0 if last else h * RK4_A[s],
                   None if last else y, None if last else Y)
            if direct:
                op.apply(stage, self._r_tmp())
                op.mass_solve_periodic_rk(self._r, *upd)
            else:
                self.rhs(stage, k)
                op.rk_update(upd[0], k, *upd[1:])
            stage = Y
        op.distribute(y)

    def run(self, start_t, end_t, dt, max_steps=None):
        time = DiscreteTime(start_t, end_t, dt)
        n = 0
        while not time.is_at_end() and (max_steps is None or n < max_steps):
            self.step(time.t, time.next_step_size())
            n += 1
            time.advance()
        return n
