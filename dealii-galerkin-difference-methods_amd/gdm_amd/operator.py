"""Device operator handle over the C ABI (include/gdm_hip.h).

`GdmOperator` owns one `gdm_op`: the uncut structured-mesh GDM operator of
one rank (mass, advection, wave, convective or elasticity) with its slab layout.  Vectors
are torch CUDA tensors (fp64); torch is only the allocator / stream provider.
"""
import ctypes

import numpy as np

from . import _capi
from ._capi import GdmError, check

KINDS = {
    "mass": _capi.GDM_OP_MASS,
    "advection": _capi.GDM_OP_ADVECTION,
    "wave": _capi.GDM_OP_WAVE,
    "convective": _capi.GDM_OP_CONVECTIVE,
    "elasticity": _capi.GDM_OP_ELASTICITY,
}

PRECONDS = {"none": 0, "jacobi": 1, "fastdiag": 2}


def _ptr(t):
    if t is None:
        return None
    import torch

    if not t.is_cuda or t.dtype != torch.float64:
        raise GdmError("device fp64 tensor expected")
    if not t.is_contiguous():
        raise GdmError("contiguous tensor expected")
    return ctypes.c_void_p(t.data_ptr())


class GdmOperator:
    """One rank's operator.  Local vectors are laid out
    [ghost planes below | owned planes | ghost planes above] along the last
    coordinate, each plane in the reference's lexicographic DoF order."""

    def __init__(self, dim, fe_degree, n_subdivisions, lo, hi, kind, params=(), rank=0, n_ranks=1, device=0,
                 periodic=0):
        import torch

        self._torch = torch
        self.lib = _capi.load()
        if not torch.cuda.is_available():
            raise GdmError("no GPU visible: the GDM operator engine has no CPU path")
        m = _capi.MeshDesc()
        m.dim = dim
        m.fe_degree = fe_degree
        ns = list(n_subdivisions) if hasattr(n_subdivisions, "__len__") else [n_subdivisions] * dim
        los = list(lo) if hasattr(lo, "__len__") else [lo] * dim
        his = list(hi) if hasattr(hi, "__len__") else [hi] * dim
        for d in range(3):
            m.n_subdivisions[d] = int(ns[d]) if d < dim else 1
            m.lo[d] = float(los[d]) if d < dim else 0.0
            m.hi[d] = float(his[d]) if d < dim else 1.0
        m.n_ranks, m.rank, m.periodic = n_ranks, rank, periodic
        self.mesh = m
        self.dim, self.p = dim, fe_degree
        self.kind = KINDS[kind] if isinstance(kind, str) else kind
        # elasticity: apply() acts on component-major vectors [u_0 | u_1 | (u_2)] of dim blocks
        self.n_components = dim if self.kind == _capi.GDM_OP_ELASTICITY else 1
        self.device = device
        self._params = tuple(float(v) for v in params)
        arr = (ctypes.c_double * max(1, len(params)))(*params) if len(params) else None
        h = ctypes.c_void_p()
        torch.cuda.set_device(device)
        check(self.lib.gdm_op_create(ctypes.byref(m), self.kind, arr, len(params), device, ctypes.byref(h)),
              "gdm_op_create")
        self.h = h
        lay = _capi.Layout()
        check(self.lib.gdm_op_layout(self.h, ctypes.byref(lay)), "gdm_op_layout")
        self.layout = lay.as_dict()
        self.use_torch_stream()

    # -- lifetime -----------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.gdm_op_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_torch_stream(self):
        """Order the operator's launches on torch's current stream."""
        s = self._torch.cuda.current_stream(self.device).cuda_stream
        check(self.lib.gdm_op_set_stream(self.h, ctypes.c_void_p(s)), "gdm_op_set_stream")

    # -- layout helpers --------------------------------------------------------
    @property
    def n_local(self):
        return self.layout["n_local"]

    @property
    def n_owned(self):
        return self.layout["n_owned"]

    @property
    def n_bc_points(self):
        return self.layout["n_bc_points"]

    def owned_view(self, local):
        lay = self.layout
        b = lay["ghost_planes_below"] * lay["plane_size"]
        return local[b:b + lay["n_owned"]]

    def new_vector(self, local=True):
        n = self.n_local if local else self.n_owned
        return self._torch.zeros(n, dtype=self._torch.float64, device="cuda:%d" % self.device)

    def _check_sizes(self, src_local, dst_owned, n_components=1):
        if src_local is not None and src_local.numel() != self.n_local * n_components:
            raise GdmError("src has %d entries, local layout needs %d" % (src_local.numel(),
                                                                          self.n_local * n_components))
        if dst_owned is not None and dst_owned.numel() != self.n_owned * n_components:
            raise GdmError("dst has %d entries, owned layout needs %d" % (dst_owned.numel(),
                                                                          self.n_owned * n_components))

    # -- operator applications -------------------------------------------------
    def apply(self, src_local, dst_owned, bc_values=None):
        self._check_sizes(src_local, dst_owned, self.n_components)
        if bc_values is not None and bc_values.numel() != self.n_bc_points:
            raise GdmError("bc_values has %d entries, expected %d" % (bc_values.numel(), self.n_bc_points))
        check(self.lib.gdm_apply(self.h, _ptr(src_local), _ptr(dst_owned), _ptr(bc_values)), "gdm_apply")
        return dst_owned

    def apply_planes(self, src_local, dst_owned, plane_begin, plane_end):
        """Volume term for the owned output planes [plane_begin, plane_end) only."""
        self._check_sizes(src_local, dst_owned)
        check(self.lib.gdm_apply_planes(self.h, _ptr(src_local), _ptr(dst_owned), int(plane_begin), int(plane_end)),
              "gdm_apply_planes")
        return dst_owned

    def apply_planes2(self, src_local, dst_owned, b0, e0, b1, e1):
        """apply_planes of two plane ranges in one launch (gdm_apply_planes2)"""
        self._check_sizes(src_local, dst_owned)
        check(self.lib.gdm_apply_planes2(self.h, _ptr(src_local), _ptr(dst_owned), int(b0), int(e0), int(b1),
                                         int(e1)), "gdm_apply_planes2")
        return dst_owned

    def add_boundary_data(self, bc_values, dst_owned):
        self._check_sizes(None, dst_owned)
        check(self.lib.gdm_add_boundary_data(self.h, _ptr(bc_values), _ptr(dst_owned)), "gdm_add_boundary_data")
        return dst_owned

    # -- separable advection field --------------------------------------------
    def field_points(self, axis):
        """Abscissae at which a field factor along `axis` is sampled
        (gdm_field_points): lo, the Gauss points cell by cell, hi."""
        return _capi.field_points(self.mesh, axis)

    def set_advection_field(self, terms):
        """a_d(x) = sum of the terms (component d, [f0, f1, f2]) of products
        f0(x_0) f1(x_1) f2(x_2) (gdm_op_set_advection_field).  A factor is an
        array sampled at field_points(axis), a callable evaluated there, or
        None (= 1).  Terms that pass the same array object share its tables
        and sweeps.  An empty list restores the constant field of the
        constructor."""
        terms = list(terms)
        arr = (_capi.FieldTerm * max(len(terms), 1))()
        keep = {}  # id(factor object) -> sampled array: object identity becomes pointer identity
        for t, (comp, factors) in enumerate(terms):
            arr[t].component = int(comp)
            factors = list(factors) + [None] * (3 - len(factors))
            for d in range(3):
                f = factors[d]
                if f is None or d >= self.dim:
                    arr[t].factor[d] = None
                    continue
                if id(f) not in keep:
                    x = self.field_points(d)
                    v = np.array([f(xi) for xi in x], dtype=np.float64) if callable(f) else \
                        np.ascontiguousarray(f, dtype=np.float64)
                    if v.shape != x.shape:
                        raise GdmError("set_advection_field: term %d factor %d has shape %s, field_points(%d) %s"
                                       % (t, d, v.shape, d, x.shape))
                    keep[id(f)] = (f, v)
                arr[t].factor[d] = keep[id(f)][1].ctypes.data
        check(self.lib.gdm_op_set_advection_field(self.h, len(terms), arr if terms else None),
              "gdm_op_set_advection_field")
        self.n_field_terms = len(terms)

    def set_field_scale(self, s):
        """the time factors s_t of the field's terms (gdm_op_set_field_scale):
        used by every apply enqueued afterwards"""
        s = [float(v) for v in s]
        if len(s) != getattr(self, "n_field_terms", 0):
            raise GdmError("set_field_scale: %d values for %d terms" % (len(s), getattr(self, "n_field_terms", 0)))
        check(self.lib.gdm_op_set_field_scale(self.h, (ctypes.c_double * max(len(s), 1))(*s)),
              "gdm_op_set_field_scale")

    def mass_apply(self, src_local, dst_owned):
        self._check_sizes(src_local, dst_owned)
        check(self.lib.gdm_mass_apply(self.h, _ptr(src_local), _ptr(dst_owned)), "gdm_mass_apply")
        return dst_owned

    def mass_solve_rk(self, rhs_owned, beta, acc_in, acc_out, alpha=0.0, y=None, Y=None):
        """k = M^-1 rhs; acc_out = acc_in + beta k; Y = y + alpha k (when Y is
        given), with the update fused into the last line-solve pass
        (gdm_mass_solve_rk): rhs_owned is overwritten; the same bits as
        mass_solve(rhs, rhs) + rk_update"""
        n = self.n_owned
        for v in (rhs_owned, acc_in, acc_out) + ((y, Y) if Y is not None else ()):
            if v.numel() != n:
                raise GdmError("mass_solve_rk: vectors need n_owned = %d entries" % n)
        check(self.lib.gdm_mass_solve_rk(self.h, _ptr(rhs_owned), float(beta), _ptr(acc_in), _ptr(acc_out),
                                         float(alpha), _ptr(y) if Y is not None else None, _ptr(Y)),
              "gdm_mass_solve_rk")
        return acc_out

    # -- dispatch control for tests and A/B runs -------------------------------
    def set_mass_seg_waves(self, waves):
        """passes of the mass inverse with fewer than `waves` waves of 64 lines
        run segmented (gdm_op_set_mass_seg_waves): 0 = never, -1 = the default"""
        check(self.lib.gdm_op_set_mass_seg_waves(self.h, int(waves)), "gdm_op_set_mass_seg_waves")

    def mass_path(self):
        """what the last mass inverse launched (gdm_op_mass_path): {"rk_mode":
        0 or the fused kernel's variant 1 / 2 / 3, "passes": [{"axis", "v3",
        "segments", "in_place"}, ...] in launch order}"""
        mp = _capi.MassPath()
        check(self.lib.gdm_op_mass_path(self.h, ctypes.byref(mp)), "gdm_op_mass_path")
        return {"rk_mode": mp.rk_mode,
                "passes": [{"axis": q.axis, "v3": bool(q.v3), "segments": q.segments, "in_place": bool(q.in_place)}
                           for q in mp.passes[:mp.n_passes]]}

    def mass_solve(self, rhs_owned, x_owned):
        self._check_sizes(None, rhs_owned)
        self._check_sizes(None, x_owned)
        check(self.lib.gdm_mass_solve(self.h, _ptr(rhs_owned), _ptr(x_owned)), "gdm_mass_solve")
        return x_owned

    def mass_solve_periodic(self, rhs_owned, x_owned):
        """x = distribute((P^T M P)^-1 rhs): the exact, direct mass inverse
        with periodicity constraints (gdm_mass_solve_periodic); rhs entries on
        constrained DoFs are ignored; x may be rhs.  Without periodic
        constraints: mass_solve."""
        self._check_sizes(None, rhs_owned)
        self._check_sizes(None, x_owned)
        check(self.lib.gdm_mass_solve_periodic(self.h, _ptr(rhs_owned), _ptr(x_owned)), "gdm_mass_solve_periodic")
        return x_owned

    def mass_solve_periodic_rk(self, rhs_owned, beta, acc_in, acc_out, alpha=0.0, y=None, Y=None):
        """mass_solve_rk with periodicity constraints
        (gdm_mass_solve_periodic_rk): rhs_owned is overwritten; the same bits
        as mass_solve_periodic(rhs, rhs) + rk_update"""
        n = self.n_owned
        for v in (rhs_owned, acc_in, acc_out) + ((y, Y) if Y is not None else ()):
            if v.numel() != n:
                raise GdmError("mass_solve_periodic_rk: vectors need n_owned = %d entries" % n)
        check(self.lib.gdm_mass_solve_periodic_rk(self.h, _ptr(rhs_owned), float(beta), _ptr(acc_in), _ptr(acc_out),
                                                  float(alpha), _ptr(y) if Y is not None else None, _ptr(Y)),
              "gdm_mass_solve_periodic_rk")
        return acc_out

    def mass_periodic_tables(self, axis):
        """(T, m, rows_lo, rows_hi) of the periodic mass inverse along `axis`
        (gdm_mass_periodic_tables, pure host)"""
        return _capi.mass_periodic_tables(self.mesh, axis)

    def mass_solve_cg(self, rhs_owned, x_owned, rel_tol=1e-8, abs_tol=1e-10, max_it=100, precond=1):
        """SolverCG on the matrix-free (condensed) mass: returns (iterations, residual)"""
        self._check_sizes(None, rhs_owned)
        self._check_sizes(None, x_owned)
        its, res = ctypes.c_int(0), ctypes.c_double(0.0)
        check(self.lib.gdm_mass_solve_cg(self.h, _ptr(rhs_owned), _ptr(x_owned), float(rel_tol), float(abs_tol),
                                         int(max_it), int(precond), ctypes.byref(its), ctypes.byref(res)),
              "gdm_mass_solve_cg")
        return its.value, res.value

    def distribute(self, v_owned):
        """constraints.distribute (periodicity constraints; no-op otherwise)"""
        check(self.lib.gdm_constraints_distribute(self.h, _ptr(v_owned)), "gdm_constraints_distribute")
        return v_owned

    def mass_solve_lines(self, axis, v, n_lines, stride, A, B, C):
        """In-place 1D mass solves along `axis` (gdm_mass_solve_lines)."""
        check(self.lib.gdm_mass_solve_lines(self.h, int(axis), _ptr(v), int(n_lines), int(stride), int(A), int(B),
                                            int(C)), "gdm_mass_solve_lines")
        return v

    def axpby(self, a, x, b, y):
        """y = a x + b y (gdm_vec_axpby): an operand with a zero factor is not
        read; x may be y"""
        if y.numel() != x.numel():
            raise GdmError("axpby: vector sizes differ")
        check(self.lib.gdm_vec_axpby(self.h, x.numel(), float(a), _ptr(x), float(b), _ptr(y)), "gdm_vec_axpby")
        return y

    def pointwise_mult(self, w, x, y):
        """y = w .* x (gdm_vec_pointwise_mult); y may be x or w"""
        if w.numel() != x.numel() or y.numel() != x.numel():
            raise GdmError("pointwise_mult: vector sizes differ")
        check(self.lib.gdm_vec_pointwise_mult(self.h, x.numel(), _ptr(w), _ptr(x), _ptr(y)),
              "gdm_vec_pointwise_mult")
        return y

    def mass_diagonal(self, diag_owned=None):
        """the diagonal of the (condensed) mass matrix on the owned DoFs,
        constrained rows 1 (gdm_mass_diagonal)"""
        if diag_owned is None:
            diag_owned = self.new_vector(local=False)
        self._check_sizes(None, diag_owned)
        check(self.lib.gdm_mass_diagonal(self.h, _ptr(diag_owned)), "gdm_mass_diagonal")
        return diag_owned

    def rk_update(self, beta, k, acc_in, acc_out, alpha=0.0, y=None, Y=None):
        """acc_out = acc_in + beta k; Y = y + alpha k (when Y is given), one pass"""
        n = k.numel()
        for v in (acc_in, acc_out) + ((y, Y) if Y is not None else ()):
            if v.numel() != n:
                raise GdmError("rk_update: vector sizes differ")
        check(self.lib.gdm_vec_rk_update(self.h, n, float(beta), _ptr(k), _ptr(acc_in), _ptr(acc_out), float(alpha),
                                         _ptr(y) if Y is not None else None, _ptr(Y)), "gdm_vec_rk_update")
        return acc_out

    FN_CONSTANT, FN_CONE, FN_SINE_PRODUCT = 0, 1, 2

    def eval_boundary(self, fn_kind, params, t, derivative, out):
        """out (device order, n_bc_points) = g(t) or dg/dt(t) of a built-in function"""
        if out.numel() != self.n_bc_points:
            raise GdmError("eval_boundary: out has %d entries, expected %d" % (out.numel(), self.n_bc_points))
        prm = (ctypes.c_double * max(len(params), 1))(*[float(v) for v in params])
        check(self.lib.gdm_eval_boundary(self.h, int(fn_kind), prm, len(params), float(t), int(derivative),
                                         _ptr(out)), "gdm_eval_boundary")
        return out

    def apply_bc_fn(self, src_local, dst_owned, fn_kind, params, t_g, alpha=0.0, t_k=0.0):
        """apply() with the stage boundary values g(t_g) + alpha dg/dt(t_k) of a
        built-in function computed by the engine right before the stencil (gdm_apply_bc_fn):
        the same bits as eval_boundary + rk_update + apply(bc_values)"""
        self._check_sizes(src_local, dst_owned)
        prm = (ctypes.c_double * max(len(params), 1))(*[float(v) for v in params])
        check(self.lib.gdm_apply_bc_fn(self.h, _ptr(src_local), _ptr(dst_owned), int(fn_kind), prm, len(params),
                                       float(t_g), float(alpha), float(t_k)), "gdm_apply_bc_fn")
        return dst_owned

    def add_boundary_fn(self, dst_owned, fn_kind, params, t_g, alpha=0.0, t_k=0.0):
        """add_boundary_data() with the stage boundary values of apply_bc_fn (gdm_add_boundary_fn)"""
        self._check_sizes(None, dst_owned)
        prm = (ctypes.c_double * max(len(params), 1))(*[float(v) for v in params])
        check(self.lib.gdm_add_boundary_fn(self.h, _ptr(dst_owned), int(fn_kind), prm, len(params), float(t_g),
                                           float(alpha), float(t_k)), "gdm_add_boundary_fn")
        return dst_owned

    # -- forcing and Dirichlet data (wave / heat right-hand side) ----------------
    def quadrature_points(self):
        """Per-axis Gauss abscissae of the tensor quadrature grid of add_load:
        entries 1 .. Q_d of field_points(d), Q_d = n_sub_d (p + 1)."""
        return [_capi.field_points(self.mesh, d)[1:-1] for d in range(self.dim)]

    def gauss_grid_points(self):
        """the tensor Gauss grid as (n, 3) points in add_load's order (qz, qy, qx)"""
        xq = self.quadrature_points() + [np.zeros(1)] * (3 - self.dim)
        x = np.zeros((xq[2].size, xq[1].size, xq[0].size, 3))
        x[..., 0] = xq[0][None, None, :]
        x[..., 1] = xq[1][None, :, None]
        x[..., 2] = xq[2][:, None, None]
        return x.reshape(-1, 3)

    def add_load_fn(self, fn_kind, params, t, dst_owned, derivative=0, scale=1.0):
        """dst += scale (v, f) over QGauss(p+1), f a built-in function at time
        t or (derivative=1) its d/dt (gdm_add_load_fn; wave/stiffness.h:196-200)"""
        self._check_sizes(None, dst_owned)
        prm = (ctypes.c_double * max(len(params), 1))(*[float(v) for v in params])
        check(self.lib.gdm_add_load_fn(self.h, int(fn_kind), prm, len(params), float(t), int(derivative),
                                       float(scale), _ptr(dst_owned)), "gdm_add_load_fn")
        return dst_owned

    def add_load(self, fq, dst_owned, scale=1.0):
        """dst += scale (v, f), f a device array on the tensor Gauss grid
        fq[(qz Q_y + qy) Q_x + qx] (quadrature_points(); gdm_add_load)"""
        self._check_sizes(None, dst_owned)
        nq = 1
        for d in range(self.dim):
            nq *= self.mesh.n_subdivisions[d] * (self.p + 1)
        if fq.numel() != nq:
            raise GdmError("add_load: fq has %d entries, the quadrature grid %d" % (fq.numel(), nq))
        check(self.lib.gdm_add_load(self.h, _ptr(fq), float(scale), _ptr(dst_owned)), "gdm_add_load")
        return dst_owned

    def add_dirichlet_data(self, g_bc, dst_owned):
        """dst += sum_faces <gamma / h_min v - dv/dn, g>, g in the device
        block(0) order (gdm_add_dirichlet_data; wave/stiffness.h:320-326)"""
        self._check_sizes(None, dst_owned)
        if g_bc.numel() != self.n_bc_points:
            raise GdmError("add_dirichlet_data: g has %d entries, expected %d" % (g_bc.numel(), self.n_bc_points))
        check(self.lib.gdm_add_dirichlet_data(self.h, _ptr(g_bc), _ptr(dst_owned)), "gdm_add_dirichlet_data")
        return dst_owned

    def load_vector_1d(self, axis, f=None):
        """1D load vector along `axis` (gdm_load_vector_1d, pure host)"""
        return _capi.load_vector_1d(self.mesh, axis, f)

    def load_tile(self):
        """(tile_x, tile_y, z_chunk) of the general load kernel, kernel axes"""
        return _capi.load_tile(self.p, self.dim)

    # -- grid evaluation: u, grad u, the flux load and the wall trace ---------------
    @property
    def n_grid_points(self):
        """Q = prod_d n_sub_d (p + 1), the points of the tensor Gauss grid"""
        nq = 1
        for d in range(self.dim):
            nq *= self.mesh.n_subdivisions[d] * (self.p + 1)
        return nq

    def _new(self, n):
        return self._torch.empty(n, dtype=self._torch.float64, device="cuda:%d" % self.device)

    def eval_grid(self, u, values=None, gradients=None):
        """u and its physical gradient at the Gauss points (gdm_eval_grid;
        FEValues::get_function_values / get_function_gradients): values[Q] in
        add_load's layout, gradients[dim Q] component-major (gradients[e Q + q],
        e the reference direction).  values=False / gradients=False leaves that
        output out (it then costs nothing); None allocates it.  u is one
        component's vector (elasticity: GdmOperator.component).  Returns
        (values, gradients), the values alone with gradients=False, the
        gradients alone with values=False."""
        if u.numel() != self.n_local:
            raise GdmError("eval_grid: u has %d entries, expected n_local %d" % (u.numel(), self.n_local))
        nq = self.n_grid_points
        if values is None:
            values = self._new(nq)
        if gradients is None:
            gradients = self._new(self.dim * nq)
        want_v, want_g = values is not False, gradients is not False
        if want_v and values.numel() != nq:
            raise GdmError("eval_grid: values has %d entries, the quadrature grid %d" % (values.numel(), nq))
        if want_g and gradients.numel() != self.dim * nq:
            raise GdmError("eval_grid: gradients has %d entries, expected %d" % (gradients.numel(), self.dim * nq))
        check(self.lib.gdm_eval_grid(self.h, _ptr(u), _ptr(values) if want_v else None,
                                     _ptr(gradients) if want_g else None), "gdm_eval_grid")
        if want_v and want_g:
            return values, gradients
        return values if want_v else gradients

    def add_load_grad(self, Fq, dst_owned, scale=1.0):
        """dst += scale sum_e (d_e v, F_e) over QGauss(p+1), Fq[dim Q]
        component-major on the tensor Gauss grid (gdm_add_load_grad): the
        transpose of eval_grid's gradients with the Gauss weights"""
        self._check_sizes(None, dst_owned)
        if Fq.numel() != self.dim * self.n_grid_points:
            raise GdmError("add_load_grad: Fq has %d entries, expected %d" % (Fq.numel(),
                                                                             self.dim * self.n_grid_points))
        check(self.lib.gdm_add_load_grad(self.h, _ptr(Fq), float(scale), _ptr(dst_owned)), "gdm_add_load_grad")
        return dst_owned

    def eval_trace(self, u, u_bc=None, dn_bc=None):
        """the wall trace and the outward normal derivative of u at the
        n_bc_points boundary points, device block(0) order (gdm_eval_trace).
        u_bc=False / dn_bc=False leaves that output out; None allocates it.
        Returns (u_bc, dn_bc), or the one that was asked for."""
        if u.numel() != self.n_local:
            raise GdmError("eval_trace: u has %d entries, expected n_local %d" % (u.numel(), self.n_local))
        n = self.n_bc_points
        if u_bc is None:
            u_bc = self._new(n)
        if dn_bc is None:
            dn_bc = self._new(n)
        want_u, want_d = u_bc is not False, dn_bc is not False
        for name, t, want in (("u_bc", u_bc, want_u), ("dn_bc", dn_bc, want_d)):
            if want and t.numel() != n:
                raise GdmError("eval_trace: %s has %d entries, expected %d" % (name, t.numel(), n))
        check(self.lib.gdm_eval_trace(self.h, _ptr(u), _ptr(u_bc) if want_u else None,
                                      _ptr(dn_bc) if want_d else None), "gdm_eval_trace")
        if want_u and want_d:
            return u_bc, dn_bc
        return u_bc if want_u else dn_bc

    def eval_grid_tile(self):
        """(cells_x, cells_y, cells_z) of one work item of the evaluation kernel, kernel axes"""
        return _capi.eval_grid_tile(self.p, self.dim)

    # -- direct heat-implicit / Poisson solve (fast diagonalisation) -------------
    @property
    def nitsche(self):
        """the Nitsche parameter of a wave operator (params[0]; 0 otherwise)"""
        return float(self._params[0]) if self.kind == KINDS["wave"] and len(self._params) else 0.0

    def fastdiag_tables(self, axis):
        """(S, lambda) of direction `axis` on the host (gdm_fastdiag_tables)"""
        return _capi.fastdiag_tables(self.mesh, self.nitsche, axis)

    def system_solve_setup(self):
        """Build and upload the fast-diagonalisation tables and the scratch
        vectors (gdm_system_solve_setup; idempotent)"""
        check(self.lib.gdm_system_solve_setup(self.h), "gdm_system_solve_setup")

    def system_solve(self, alpha, tau, rhs_owned, x_owned=None):
        """x = (alpha M - tau K)^-1 rhs, K = apply (gdm_system_solve):
        heat-impl alpha = 1, tau = dt; Poisson alpha = 0, tau = 1.  x may be
        rhs; None allocates it."""
        if x_owned is None:
            x_owned = self.new_vector(False)
        self._check_sizes(None, rhs_owned)
        self._check_sizes(None, x_owned)
        check(self.lib.gdm_system_solve(self.h, float(alpha), float(tau), _ptr(rhs_owned), _ptr(x_owned)),
              "gdm_system_solve")
        return x_owned

    # -- separable coefficient of the wave / heat / Poisson operator ---------------
    def _coef_terms(self, terms, what):
        """(ctypes array of gdm_coef_term, the sampled arrays it points into)"""
        terms = [list(t) for t in terms]
        if len(terms) > _capi.COEF_MAX_TERMS:
            raise GdmError("%s: at most %d terms" % (what, _capi.COEF_MAX_TERMS))
        arr = (_capi.CoefTerm * max(len(terms), 1))()
        keep = {}  # (id(factor object), axis) -> sampled array: object identity becomes pointer identity
        for t, factors in enumerate(terms):
            factors = factors + [None] * (3 - len(factors))
            for d in range(3):
                f = factors[d]
                if f is None or d >= self.dim:
                    arr[t].factor[d] = None
                    continue
                key = (id(f), d)
                if key not in keep:
                    x = self.field_points(d)
                    v = np.array([f(xi) for xi in x], dtype=np.float64) if callable(f) else \
                        np.ascontiguousarray(f, dtype=np.float64)
                    if v.shape != x.shape:
                        raise GdmError("%s: term %d factor %d has shape %s, field_points(%d) %s"
                                       % (what, t, d, v.shape, d, x.shape))
                    keep[key] = (f, v)
                arr[t].factor[d] = keep[key][1].ctypes.data
        return arr, keep

    def set_coefficient(self, terms):
        """kappa(x) = sum of the terms [k0, k1, k2] of products k0(x_0) k1(x_1)
        k2(x_2) (gdm_op_set_coefficient; wave operators).  A factor is an array
        sampled at field_points(axis), a callable evaluated there, or None
        (= 1).  Terms that pass the same array object share its tables.  An
        empty list restores the constant operator."""
        terms = list(terms)
        arr, _keep = self._coef_terms(terms, "set_coefficient")
        check(self.lib.gdm_op_set_coefficient(self.h, len(terms), arr if terms else None), "gdm_op_set_coefficient")
        self.n_coef_terms = len(terms)
        self._coef_grid = None  # a separable coefficient replaces a grid one

    def set_coefficient_grid(self, kq, kbc=None):
        """A general kappa > 0 sampled on the tensor Gauss grid
        (gdm_op_set_coefficient_grid; wave operators).  kq is a device tensor
        in add_load's layout kq[(qz Q_y + qy) Q_x + qx] (quadrature_points()),
        kbc a device tensor of kappa at bc_points() (needed with nitsche > 0);
        the engine borrows both, the operator keeps the references, and values
        overwritten in place are seen by the next apply.  kq may also be a
        callable kappa(x), x of shape (n, 3): it is evaluated on the host at
        the Gauss grid and at bc_points() and uploaded.  None removes the
        coefficient."""
        if kq is None:
            check(self.lib.gdm_op_set_coefficient_grid(self.h, None, None), "gdm_op_set_coefficient_grid")
            self._coef_grid = None
            self.n_coef_terms = 0
            return
        torch = self._torch
        dev = "cuda:%d" % self.device
        if callable(kq):
            kappa = kq
            kq = torch.from_numpy(np.ascontiguousarray(kappa(self.gauss_grid_points()), dtype=np.float64)).to(dev)
            if self.n_bc_points > 0:  # ignored by an operator without Nitsche terms
                kbc = torch.from_numpy(np.ascontiguousarray(kappa(self.bc_points()), dtype=np.float64)).to(dev)
        nq = 1
        for d in range(self.dim):
            nq *= self.mesh.n_subdivisions[d] * (self.p + 1)
        if kq.numel() != nq:
            raise GdmError("set_coefficient_grid: kq has %d entries, the quadrature grid %d" % (kq.numel(), nq))
        if kbc is not None and kbc.numel() != self.n_bc_points:
            raise GdmError("set_coefficient_grid: kbc has %d entries, expected %d" % (kbc.numel(), self.n_bc_points))
        check(self.lib.gdm_op_set_coefficient_grid(self.h, _ptr(kq), _ptr(kbc)), "gdm_op_set_coefficient_grid")
        self._coef_grid = (kq, kbc)  # keeps the borrowed memory alive
        self.n_coef_terms = 0

    @property
    def has_coefficient(self):
        return getattr(self, "n_coef_terms", 0) > 0 or getattr(self, "_coef_grid", None) is not None

    def coef_grid_tile(self):
        """(tile_x, tile_y, z_chunk) of the grid coefficient kernel, kernel axes"""
        return _capi.coef_grid_tile(self.p, self.dim)

    def coef_grid_tables_1d(self, axis):
        """(val[Q][p+1], der[Q][p+1], first[Q]) of the grid coefficient kernel
        along `axis` (gdm_coef_grid_tables_1d)"""
        return _capi.coef_grid_tables_1d(self.mesh, axis)

    def coef_tile(self):
        """(tile_x, tile_y, z_chunk) of the coefficient kernel, kernel axes"""
        return _capi.coef_tile(self.p, self.dim)

    def coef_solve(self, alpha, tau, rhs_owned, x_owned, rel_tol=1e-8, abs_tol=1e-30, max_it=1000):
        """x = (alpha M - tau K[kappa])^-1 rhs by CG from the initial guess x,
        preconditioned by the constant-coefficient direct solve
        (gdm_coef_solve; system_solve_setup first): returns (iterations,
        residual)."""
        self._check_sizes(None, rhs_owned)
        self._check_sizes(None, x_owned)
        its, res = ctypes.c_int(0), ctypes.c_double(0.0)
        check(self.lib.gdm_coef_solve(self.h, float(alpha), float(tau), _ptr(rhs_owned), _ptr(x_owned),
                                      float(rel_tol), float(abs_tol), int(max_it), ctypes.byref(its),
                                      ctypes.byref(res)), "gdm_coef_solve")
        return its.value, res.value

    # -- separable density: the weighted mass of the wave / heat operator ---------
    def set_density(self, terms):
        """rho(x) = sum of the terms [r0, r1, r2] of products r0(x_0) r1(x_1)
        r2(x_2) > 0 (gdm_op_set_density; wave operators); factors as in
        set_coefficient.  An empty list removes the density."""
        terms = list(terms)
        arr, _keep = self._coef_terms(terms, "set_density")
        check(self.lib.gdm_op_set_density(self.h, len(terms), arr if terms else None), "gdm_op_set_density")
        self.n_density_terms = len(terms)
        self._density_grid = None  # a separable density replaces a grid one

    def set_density_grid(self, rq):
        """A general rho > 0 sampled on the tensor Gauss grid
        (gdm_op_set_density_grid; wave operators).  rq is a device tensor in
        add_load's layout rq[(qz Q_y + qy) Q_x + qx] (quadrature_points()); the
        engine borrows it, the operator keeps the reference, and values
        overwritten in place are seen by the next density_apply and
        density_solve (call this again with the same tensor to refresh the
        mean that coef_solve's preconditioner uses).  rq may also be a callable
        rho(x), x of shape (n, 3): it is evaluated on the host at the Gauss
        grid and uploaded.  None removes the density."""
        if rq is None:
            check(self.lib.gdm_op_set_density_grid(self.h, None), "gdm_op_set_density_grid")
            self._density_grid = None
            self.n_density_terms = 0
            return
        if callable(rq):
            rho = np.ascontiguousarray(rq(self.gauss_grid_points()), dtype=np.float64)
            rq = self._torch.from_numpy(rho).to("cuda:%d" % self.device)
        nq = 1
        for d in range(self.dim):
            nq *= self.mesh.n_subdivisions[d] * (self.p + 1)
        if rq.numel() != nq:
            raise GdmError("set_density_grid: rq has %d entries, the quadrature grid %d" % (rq.numel(), nq))
        check(self.lib.gdm_op_set_density_grid(self.h, _ptr(rq)), "gdm_op_set_density_grid")
        self._density_grid = rq  # keeps the borrowed memory alive
        self.n_density_terms = 0

    @property
    def has_density(self):
        return getattr(self, "n_density_terms", 0) > 0 or getattr(self, "_density_grid", None) is not None

    def density_grid_tile(self):
        """(tile_x, tile_y, z_chunk) of the grid density kernel, kernel axes"""
        return _capi.density_grid_tile(self.p, self.dim)

    def set_density_grid_z_chunk(self, z_chunk=-1):
        """node planes per workgroup of the grid density kernel, in [1,
        density_grid_tile()[2]]; -1 restores the automatic choice.  Steers the
        launch only: the bits do not depend on it
        (gdm_op_set_density_grid_z_chunk)"""
        check(self.lib.gdm_op_set_density_grid_z_chunk(self.h, int(z_chunk)), "gdm_op_set_density_grid_z_chunk")

    def density_diag(self, dst_owned=None):
        """dst = diag(M[rho]) of the density that is set, grid or separable
        (gdm_density_diag)"""
        if dst_owned is None:
            dst_owned = self.new_vector(False)
        self._check_sizes(None, dst_owned)
        check(self.lib.gdm_density_diag(self.h, _ptr(dst_owned)), "gdm_density_diag")
        return dst_owned

    def density_tile(self):
        """(tile_x, tile_y, z_chunk) of the density kernel, kernel axes"""
        return _capi.density_tile(self.p, self.dim)

    def density_apply(self, src_owned, dst_owned=None, c=0.0, add=None):
        """dst = M[rho] src, or with `add` dst = M[rho] src + c * add in the same
        launch (gdm_density_apply / gdm_density_apply_add)"""
        if dst_owned is None:
            dst_owned = self.new_vector(False)
        self._check_sizes(None, src_owned)
        self._check_sizes(None, dst_owned)
        if add is None:
            check(self.lib.gdm_density_apply(self.h, _ptr(src_owned), _ptr(dst_owned)), "gdm_density_apply")
        else:
            self._check_sizes(None, add)
            check(self.lib.gdm_density_apply_add(self.h, _ptr(src_owned), float(c), _ptr(add), _ptr(dst_owned)),
                  "gdm_density_apply_add")
        return dst_owned

    def density_solve(self, rhs_owned, x_owned, rel_tol=1e-8, abs_tol=1e-30, max_it=1000):
        """x = M[rho]^-1 rhs (gdm_density_solve): one term exact and direct (0
        iterations, x may be rhs), a sum by preconditioned CG from the initial
        guess x; returns (iterations, residual)."""
        self._check_sizes(None, rhs_owned)
        self._check_sizes(None, x_owned)
        its, res = ctypes.c_int(0), ctypes.c_double(0.0)
        check(self.lib.gdm_density_solve(self.h, _ptr(rhs_owned), _ptr(x_owned), float(rel_tol), float(abs_tol),
                                         int(max_it), ctypes.byref(its), ctypes.byref(res)), "gdm_density_solve")
        return its.value, res.value

    def fastdiag_transform(self, axis, transpose, src_owned, dst_owned):
        """dst = T src along `axis`, T = S (transpose 0) or S^T (1)
        (gdm_fastdiag_transform)"""
        self._check_sizes(None, src_owned)
        self._check_sizes(None, dst_owned)
        check(self.lib.gdm_fastdiag_transform(self.h, int(axis), int(transpose), _ptr(src_owned), _ptr(dst_owned)),
              "gdm_fastdiag_transform")
        return dst_owned

    # -- linear elasticity (kind "elasticity": component-major vectors) -----------
    def new_vector_field(self):
        """a zero vector of n_components blocks [u_0 | u_1 | (u_2)]"""
        return self._torch.zeros(self.n_components * self.n_owned, dtype=self._torch.float64,
                                 device="cuda:%d" % self.device)

    def component(self, v, c):
        """the view of component c of a component-major vector"""
        return v[c * self.n_owned:(c + 1) * self.n_owned]

    def elasticity_tile(self):
        """(tile_x, tile_y, z_chunk) of the elasticity kernel, kernel axes"""
        return _capi.elasticity_tile(self.p, self.dim)

    def elasticity_tables_1d(self, axis):
        """(bands, S, lambda) of direction `axis` on the host (gdm_elasticity_tables_1d)"""
        return _capi.elasticity_tables_1d(self.mesh, axis)

    def elasticity_diagonal(self, diag=None):
        """the diagonal of P A P + I - P (gdm_elasticity_diagonal)"""
        if diag is None:
            diag = self.new_vector_field()
        self._check_sizes(None, diag, self.n_components)
        check(self.lib.gdm_elasticity_diagonal(self.h, _ptr(diag)), "gdm_elasticity_diagonal")
        return diag

    def elasticity_precond_setup(self):
        """Build and upload the tables of the block fast-diagonalisation
        preconditioner (gdm_elasticity_precond_setup; idempotent)"""
        check(self.lib.gdm_elasticity_precond_setup(self.h), "gdm_elasticity_precond_setup")

    def elasticity_precond(self, r, z=None):
        """z = B^-1 r, B the block diagonal of the operator (gdm_elasticity_precond)"""
        if z is None:
            z = self.new_vector_field()
        self._check_sizes(None, r, self.n_components)
        self._check_sizes(None, z, self.n_components)
        check(self.lib.gdm_elasticity_precond(self.h, _ptr(r), _ptr(z)), "gdm_elasticity_precond")
        return z

    def elasticity_solve(self, rhs, x, precond="fastdiag", rel_tol=1e-8, abs_tol=1e-10, max_it=1000):
        """Preconditioned CG on P A P + I - P from the initial guess x
        (gdm_elasticity_solve): returns (iterations, residual).  precond:
        "none", "jacobi" or "fastdiag" (set up on first use)."""
        self._check_sizes(None, rhs, self.n_components)
        self._check_sizes(None, x, self.n_components)
        pc = PRECONDS[precond] if isinstance(precond, str) else int(precond)
        if pc == 2 and isinstance(precond, str):
            self.elasticity_precond_setup()
        its, res = ctypes.c_int(0), ctypes.c_double(0.0)
        check(self.lib.gdm_elasticity_solve(self.h, _ptr(rhs), _ptr(x), pc, float(rel_tol), float(abs_tol),
                                            int(max_it), ctypes.byref(its), ctypes.byref(res)),
              "gdm_elasticity_solve")
        return its.value, res.value

    def interleave(self, src, dst=None, n_components=None, to_reference=True):
        """component-major -> the reference's vertex * n_components + component
        numbering (to_reference) or back (gdm_vec_interleave)"""
        nc = self.n_components if n_components is None else int(n_components)
        if dst is None:
            dst = self._torch.empty_like(src)
        self._check_sizes(None, src, nc)
        self._check_sizes(None, dst, nc)
        check(self.lib.gdm_vec_interleave(self.h, nc, int(bool(to_reference)), _ptr(src), _ptr(dst)),
              "gdm_vec_interleave")
        return dst

    def error_norms_grid(self, u_local, exact_q, cell_errors=None):
        """error_norms against an exact solution sampled on the tensor Gauss
        grid (device array in add_load's fq layout; gdm_error_norms_grid)"""
        if u_local.numel() != self.n_local:
            raise GdmError("error_norms_grid: u has %d entries, expected n_local %d" % (u_local.numel(),
                                                                                        self.n_local))
        nq = 1
        for d in range(self.dim):
            nq *= self.mesh.n_subdivisions[d] * (self.p + 1)
        if exact_q.numel() != nq:
            raise GdmError("error_norms_grid: exact_q has %d entries, the quadrature grid %d" % (exact_q.numel(), nq))
        if cell_errors is not None and cell_errors.numel() != self.n_owned_cells:
            raise GdmError("error_norms_grid: cell_errors has %d entries, expected %d" % (cell_errors.numel(),
                                                                                          self.n_owned_cells))
        out = (ctypes.c_double * 3)()
        check(self.lib.gdm_error_norms_grid(self.h, _ptr(u_local), _ptr(exact_q), _ptr(cell_errors), out),
              "gdm_error_norms_grid")
        return tuple(out)

    def mass_solve_slab(self, rhs_owned, x_owned):
        """Distributed exact mass inverse, step 1: the slab-local solve
        (gdm_mass_solve_slab).  Then exchange the ghost planes of the local
        vector holding x_owned and call mass_solve_interface."""
        check(self.lib.gdm_mass_solve_slab(self.h, _ptr(rhs_owned), _ptr(x_owned)), "gdm_mass_solve_slab")
        return x_owned

    def mass_solve_interface_round(self, x_local, round_):
        """Distributed exact mass inverse, refinement round `round_` of
        gdm_mass_spike_rounds (thin slabs): the slab's edge planes become the
        next interface systems' right-hand sides; exchange the ghost planes of
        x_local again afterwards."""
        if x_local.numel() != self.n_local:
            raise GdmError("mass_solve_interface_round: x has %d entries, expected n_local %d"
                           % (x_local.numel(), self.n_local))
        check(self.lib.gdm_mass_solve_interface_round(self.h, _ptr(x_local), int(round_)),
              "gdm_mass_solve_interface_round")
        return x_local

    def mass_solve_interface(self, x_local):
        """Distributed exact mass inverse, step 2 (gdm_mass_solve_interface):
        the owned part of x_local (ghost planes = the neighbours' slab solves)
        becomes M^-1 rhs."""
        if x_local.numel() != self.n_local:
            raise GdmError("mass_solve_interface: x has %d entries, expected n_local %d" % (x_local.numel(),
                                                                                          self.n_local))
        check(self.lib.gdm_mass_solve_interface(self.h, _ptr(x_local)), "gdm_mass_solve_interface")
        return x_local

    def mass_solve_interface_ghosts(self, x_local):
        """mass_solve_interface, and the ghost planes of x_local become the
        interface solution (the neighbours' edge planes of M^-1 rhs,
        gdm_mass_solve_interface_ghosts): x_local is a valid local vector
        without another exchange"""
        if x_local.numel() != self.n_local:
            raise GdmError("mass_solve_interface_ghosts: x has %d entries, expected n_local %d"
                           % (x_local.numel(), self.n_local))
        check(self.lib.gdm_mass_solve_interface_ghosts(self.h, _ptr(x_local)), "gdm_mass_solve_interface_ghosts")
        return x_local

    def mass_solve_interface_rk(self, x_local, beta, acc_in, acc_out, alpha=0.0, y=None, Y=None):
        """mass_solve_interface_ghosts fused with rk_update over the local
        vectors (gdm_mass_solve_interface_rk): acc_out = acc_in + beta k, Y =
        y + alpha k (when Y is given) with k the interface-corrected solve of
        every local plane; x_local is only read.  The bits of
        mass_solve_interface_ghosts(x) + rk_update(beta, x, ...)."""
        n = self.n_local
        for v in (x_local, acc_in, acc_out) + ((y, Y) if Y is not None else ()):
            if v.numel() != n:
                raise GdmError("mass_solve_interface_rk: vectors need n_local = %d entries" % n)
        check(self.lib.gdm_mass_solve_interface_rk(self.h, _ptr(x_local), float(beta), _ptr(acc_in), _ptr(acc_out),
                                                   float(alpha), _ptr(y) if Y is not None else None, _ptr(Y)),
              "gdm_mass_solve_interface_rk")
        return acc_out

    def error_norms(self, u_local, fn_kind, params, t, cell_errors=None):
        """(Linf, L1, L2) of u - f(t) over QGauss(p+1) on the owned cells
        (advection/problem.h:269-425 postprocess, volume part); cell_errors
        (device, n_owned_cells) receives integrate_difference's per-cell L2
        errors (vector_tools.h:25-86).  Multi-rank callers reduce: max, sum,
        sqrt(sum of squares)."""
        if u_local.numel() != self.n_local:
            raise GdmError("error_norms: u has %d entries, expected n_local %d" % (u_local.numel(), self.n_local))
        if cell_errors is not None and cell_errors.numel() != self.n_owned_cells:
            raise GdmError("error_norms: cell_errors has %d entries, expected %d" % (cell_errors.numel(),
                                                                                     self.n_owned_cells))
        prm = (ctypes.c_double * max(len(params), 1))(*[float(v) for v in params])
        out = (ctypes.c_double * 3)()
        check(self.lib.gdm_error_norms(self.h, _ptr(u_local), int(fn_kind), prm, len(params), float(t),
                                       _ptr(cell_errors), out), "gdm_error_norms")
        return tuple(out)

    @property
    def n_owned_cells(self):
        n = max(0, self.layout["cell_plane_end"] - self.layout["cell_plane_begin"])
        for d in range(self.dim - 1):
            n *= self.mesh.n_subdivisions[d]
        return n

    def dot(self, x, y):
        r = ctypes.c_double(0.0)
        check(self.lib.gdm_vec_dot(self.h, x.numel(), _ptr(x), _ptr(y), ctypes.byref(r)), "gdm_vec_dot")
        return r.value

    def synchronize(self):
        check(self.lib.gdm_synchronize(self.h), "gdm_synchronize")

    def time_op(self, which, src, dst, bc=None, n_iter=10):
        ms = ctypes.c_double(0.0)
        check(self.lib.gdm_time_op(self.h, int(which), _ptr(src), _ptr(dst), _ptr(bc), int(n_iter), ctypes.byref(ms)),
              "gdm_time_op")
        return ms.value

    # -- boundary points -------------------------------------------------------
    def bc_points(self):
        n = self.n_bc_points
        xyz = np.zeros((max(n, 1), 3))
        check(self.lib.gdm_bc_points(self.h, xyz.ctypes.data_as(ctypes.c_void_p)), "gdm_bc_points")
        return xyz[:n]

    @property
    def n_bc_points_ref(self):
        return self.layout["n_bc_points_ref"]

    def bc_reference_order(self):
        n = self.n_bc_points_ref
        perm = np.zeros(max(n, 1), dtype=np.int64)
        check(self.lib.gdm_bc_reference_order(self.h, perm.ctypes.data_as(ctypes.c_void_p)),
              "gdm_bc_reference_order")
        return perm[:n]
