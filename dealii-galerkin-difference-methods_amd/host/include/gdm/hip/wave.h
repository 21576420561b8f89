// gdm/hip/wave.h -- C++ host mirror of the reference's wave application
// operator surface over the C ABI (include/gdm_hip.h), uncut configuration.
//
// Same class and method names, argument meaning and error behaviour as the
// reference (paths relative to peterrum/dealii-galerkin-difference-methods):
//   Parameters<dim>              applications/wave/include/gdm/wave/parameters.h:7-52
//   StiffnessMatrixOperator<dim> .../wave/stiffness.h:18-420
//     compute_rhs(dst, src, compute_impl_part, time)   :409-420
//   MassMatrixOperator<dim>      .../wave/mass.h:18-250 (get_sparse_matrix / solve)
//   WaveProblem<dim>             .../wave/problem.h:22-346, "wave-rk" branch :280-346
// The level set contains the box (no cut cells): the volume term
// -(grad v, grad u), and with function_domain_dbc the box Nitsche terms
// (gamma_D / h, :261-330).  Parameters::function_rhs and function_domain_dbc
// bind the source term (v, f(., t)) (:196-200) and the Nitsche Dirichlet data
// <gamma_D / h v - dv/dn, g_D(., t)> (:320-326): compute_rhs evaluates them on
// the host at the quadrature / boundary points of the stage time, uploads the
// values and adds both terms on the device (gdm_add_load,
// gdm_add_dirichlet_data).  Left empty they are zero and the launches are
// those of the homogeneous problem (the uncut C4 configuration of
// BASELINE.json).
#pragma once

#include <gdm/hip/operators.h>

namespace GDM {
namespace HIP {
namespace Wave {

template <int dim>
struct Parameters {
  unsigned int fe_degree = 3;
  unsigned int n_subdivisions_1D = 40;
  double geometry_left = -1.21;
  double geometry_right = 1.21;
  double nitsche_parameter = 0.0;  // > 0: box Nitsche (function_domain_dbc; g = 0 when it is empty)
  Function exact_solution;         // initial condition u(x, 0)
  Function function_rhs;           // f(x, t) of the source term (v, f) (empty: 0)
  Function function_domain_dbc;    // g_D(x, t) on the box (needs nitsche_parameter > 0; empty: 0)
  double start_t = 0.0;
  double end_t = 2.0;
  double cfl = 0.3;
  double cfl_pow = 1.0;
  int device = 0;
  int n_ranks = 1, rank = 0;
  // "wave-rk" (problem.h:280-346), "heat-rk" (:72-128), "heat-impl" (:210-279) or "poisson" (:46-71)
  std::string simulation_type = "wave-rk";
};

template <int dim>
class Discretization {
 public:
  void reinit(const Parameters<dim> &params) {
    desc = gdm_mesh_desc{};
    desc.dim = dim;
    desc.fe_degree = (int)params.fe_degree;
    for (int d = 0; d < 3; ++d) {
      desc.n_subdivisions[d] = d < dim ? (int)params.n_subdivisions_1D : 1;
      desc.lo[d] = d < dim ? params.geometry_left : 0.0;
      desc.hi[d] = d < dim ? params.geometry_right : 1.0;
    }
    desc.n_ranks = params.n_ranks;
    desc.rank = params.rank;
    device = params.device;
  }
  double get_dx() const { return (desc.hi[0] - desc.lo[0]) / desc.n_subdivisions[0]; }  // discretization.h:53
  const gdm_mesh_desc &get_mesh() const { return desc; }
  int get_device() const { return device; }

 private:
  gdm_mesh_desc desc{};
  int device = 0;
};

using VectorType = DeviceVector;  // LinearAlgebra::distributed::Vector<double>, local layout

template <int dim>
class StiffnessMatrixOperator {
 public:
  explicit StiffnessMatrixOperator(const Discretization<dim> &discretization) : discretization(discretization) {}
  StiffnessMatrixOperator(const StiffnessMatrixOperator &) = delete;
  ~StiffnessMatrixOperator() { release(); }

  void reinit(const Parameters<dim> &params) {
    release();
    const double nitsche = params.nitsche_parameter;
    check(gdm_op_create(&discretization.get_mesh(), GDM_OP_WAVE, nitsche > 0 ? &nitsche : nullptr,
                        nitsche > 0 ? 1 : 0, discretization.get_device(), &op),
          "gdm_op_create");
    check(gdm_op_layout(op, &layout), "gdm_op_layout");
    check(gdm_op_set_stream(op, nullptr), "gdm_op_set_stream");
    function_rhs = params.function_rhs;
    function_domain_dbc = params.function_domain_dbc;
    const gdm_mesh_desc &m = discretization.get_mesh();
    if (function_rhs) {  // the tensor Gauss grid of gdm_add_load
      std::size_t nq = 1;
      for (int d = 0; d < dim; ++d) {
        std::vector<double> x((std::size_t)m.n_subdivisions[d] * (m.fe_degree + 1) + 2);
        check(gdm_field_points(&m, d, x.data()), "gdm_field_points");
        xq[d].assign(x.begin() + 1, x.end() - 1);
        nq *= xq[d].size();
      }
      fq_host.assign(nq, 0.0);
      fq_dev = device_buffer(nq);
    }
    if (function_domain_dbc) {
      if (!(nitsche > 0)) throw Error("function_domain_dbc needs nitsche_parameter > 0");
      bc_xyz.assign((std::size_t)std::max<int64_t>(layout.n_bc_points, 1) * 3, 0.0);
      check(gdm_bc_points(op, bc_xyz.data()), "gdm_bc_points");
      g_host.assign((std::size_t)layout.n_bc_points, 0.0);
      g_dev = device_buffer(g_host.size());
    }
  }

  void initialize_dof_vector(VectorType &vec) const { vec.reinit(op, layout.n_local); }

  // vec_rhs (owned entries) = -(grad v, grad u) [+ box Nitsche] if
  // compute_impl_part, + (v, f(., time)) + the Nitsche data of g_D(., time)
  // (stiffness.h:409-420; both data terms are part of the explicit part)
  void compute_rhs(VectorType &vec_rhs, const VectorType &solution, const bool compute_impl_part,
                   const double time) const {
    if (compute_impl_part)
      check(gdm_apply(op, solution.get_values(), owned(vec_rhs), nullptr), "gdm_apply");
    else
      check(gdm_vec_axpby(op, layout.n_owned, 0.0, owned(vec_rhs), 0.0, owned(vec_rhs)), "gdm_vec_axpby");
    if (function_rhs) {
      const std::size_t Q0 = xq[0].size(), Q1 = dim > 1 ? xq[1].size() : 1, Q2 = dim > 2 ? xq[2].size() : 1;
      for (std::size_t k = 0; k < Q2; ++k)
        for (std::size_t j = 0; j < Q1; ++j)
          for (std::size_t i = 0; i < Q0; ++i) {
            const Point x{xq[0][i], dim > 1 ? xq[1][j] : 0.0, dim > 2 ? xq[2][k] : 0.0};
            fq_host[(k * Q1 + j) * Q0 + i] = function_rhs(x, time);
          }
      check(gdm_memcpy_h2d(op, fq_dev, fq_host.data(), sizeof(double) * fq_host.size()), "gdm_memcpy_h2d");
      check(gdm_add_load(op, fq_dev, 1.0, owned(vec_rhs)), "gdm_add_load");
    }
    if (function_domain_dbc && !g_host.empty()) {
      for (std::size_t i = 0; i < g_host.size(); ++i)
        g_host[i] = function_domain_dbc(Point{bc_xyz[3 * i], bc_xyz[3 * i + 1], bc_xyz[3 * i + 2]}, time);
      check(gdm_memcpy_h2d(op, g_dev, g_host.data(), sizeof(double) * g_host.size()), "gdm_memcpy_h2d");
      check(gdm_add_dirichlet_data(op, g_dev, owned(vec_rhs)), "gdm_add_dirichlet_data");
    }
  }

  // The linear solves of "heat-impl" and "poisson" (problem.h:217-226, 263-269
  // and :46-67): x = (alpha M + tau S)^-1 rhs with S = get_sparse_matrix() =
  // -compute_rhs's operator part; the reference's CG + AMG on the assembled
  // matrix is replaced by the engine's fast diagonalisation.  A changed tau
  // (the last time step) needs no new setup.
  void setup_system_solve() const { check(gdm_system_solve_setup(op), "gdm_system_solve_setup"); }
  void system_solve(double alpha, double tau, double *x_owned, const double *rhs_owned) const {
    check(gdm_system_solve(op, alpha, tau, rhs_owned, x_owned), "gdm_system_solve");
  }

  // A separable coefficient kappa(x) = sum_t k_t0(x_0) ... k_t(dim-1)(x_(dim-1)) > 0
  // (gdm_op_set_coefficient, after reinit; single rank): every JxW of the
  // operator part and of the box-face part of compute_rhs is multiplied by
  // kappa at the quadrature point (stiffness.h:171-181, 296-327).  factors[d]
  // holds k_td sampled at field_points(d) (nullptr or empty = 1); terms that
  // pass the same vector object share its tables.  No terms: the constant
  // operator again.
  struct CoefTerm {
    std::array<const std::vector<double> *, dim> factors{};
  };

  // abscissae at which a factor along direction d is sampled: lo, the Gauss
  // points cell by cell, hi
  std::vector<double> field_points(int d) const {
    const gdm_mesh_desc &m = discretization.get_mesh();
    std::vector<double> x((std::size_t)m.n_subdivisions[d] * (m.fe_degree + 1) + 2);
    check(gdm_field_points(&m, d, x.data()), "gdm_field_points");
    return x;
  }

  void set_coefficient(const std::vector<CoefTerm> &terms) {
    std::vector<gdm_coef_term> t(terms.size());
    for (std::size_t i = 0; i < terms.size(); ++i)
      for (int d = 0; d < 3; ++d)
        t[i].factor[d] = d < dim && terms[i].factors[d] && !terms[i].factors[d]->empty() ? terms[i].factors[d]->data()
                                                                                            : nullptr;
    check(gdm_op_set_coefficient(op, (int)t.size(), t.data()), "gdm_op_set_coefficient");
    has_coefficient = !terms.empty();
  }

  // A general coefficient kappa > 0 on the tensor Gauss grid
  // (gdm_op_set_coefficient_grid, after reinit; single rank): kq_dev holds
  // kappa at the Gauss points in the layout of the source term's grid,
  // kq[(qz Q_y + qy) Q_x + qx], kbc_dev kappa at the boundary points in the
  // engine's block(0) order (needed with nitsche > 0).  Both are DEVICE arrays
  // the engine borrows: they must outlive the coefficient and may be
  // overwritten in place between applies.  nullptr: the constant operator again.
  void set_coefficient_grid(const double *kq_dev, const double *kbc_dev) {
    check(gdm_op_set_coefficient_grid(op, kq_dev, kbc_dev), "gdm_op_set_coefficient_grid");
    has_coefficient = kq_dev != nullptr;
  }

  // The solve with a coefficient: CG on alpha M + tau S[kappa] from the initial
  // guess x, preconditioned by the constant-coefficient direct solve
  // (setup_system_solve first); SolverCG with ReductionControl(max_it,
  // abs_tol, rel_tol).  Returns last_step.  Without a coefficient: system_solve.
  // With a density the system is alpha M[rho] + tau S[kappa] (with or without
  // a coefficient).
  int solve(double alpha, double tau, double *x_owned, const double *rhs_owned, double rel_tol = 1e-8,
            double abs_tol = 1e-30, int max_it = 1000) const {
    if (!has_coefficient && !has_density) {
      system_solve(alpha, tau, x_owned, rhs_owned);
      return 0;
    }
    int its = 0;
    check(gdm_coef_solve(op, alpha, tau, rhs_owned, x_owned, rel_tol, abs_tol, max_it, &its, nullptr), "gdm_coef_solve");
    return its;
  }

  // A separable density rho(x) = sum_t r_t0(x_0) ... r_t(dim-1)(x_(dim-1)) > 0
  // (gdm_op_set_density, after reinit; single rank): the mass matrix with
  // every JxW multiplied by rho at the quadrature point (mass.h:47-249), terms
  // as in set_coefficient.  No terms: the unit density again.
  void set_density(const std::vector<CoefTerm> &terms) {
    std::vector<gdm_coef_term> t(terms.size());
    for (std::size_t i = 0; i < terms.size(); ++i)
      for (int d = 0; d < 3; ++d)
        t[i].factor[d] = d < dim && terms[i].factors[d] && !terms[i].factors[d]->empty() ? terms[i].factors[d]->data()
                                                                                            : nullptr;
    check(gdm_op_set_density(op, (int)t.size(), t.data()), "gdm_op_set_density");
    has_density = !terms.empty();
  }

  // A general density rho > 0 given by its samples on the tensor Gauss grid
  // (gdm_op_set_density_grid, after reinit; single rank): rq_dev is a DEVICE
  // array in the layout of set_coefficient_grid's kq, borrowed by the engine:
  // it must outlive the density, and values overwritten in place are seen by
  // the next density_apply and density_solve (call this again to refresh the
  // mean that solve()'s preconditioner uses).
  // nullptr: the unit density again.
  void set_density_grid(const double *rq_dev) {
    check(gdm_op_set_density_grid(op, rq_dev), "gdm_op_set_density_grid");
    has_density = rq_dev != nullptr;
  }

  // dst = diag(M[rho]) of the density that is set, grid or separable
  void density_diag(double *dst_owned) const { check(gdm_density_diag(op, dst_owned), "gdm_density_diag"); }

  // dst = M[rho] src (distinct device vectors)
  void density_apply(double *dst_owned, const double *src_owned) const {
    check(gdm_density_apply(op, src_owned, dst_owned), "gdm_density_apply");
  }

  // x = M[rho]^-1 rhs: one term exact and direct (returns 0; x may be rhs), a
  // sum by CG from the initial guess x with ReductionControl(max_it, abs_tol,
  // rel_tol), preconditioned by the diagonally scaled exact mass inverse.
  // Returns last_step.
  int density_solve(double *x_owned, const double *rhs_owned, double rel_tol = 1e-8, double abs_tol = 1e-30,
                    int max_it = 1000) const {
    int its = 0;
    check(gdm_density_solve(op, rhs_owned, x_owned, rel_tol, abs_tol, max_it, &its, nullptr), "gdm_density_solve");
    return its;
  }

  gdm_op *handle() const { return op; }
  const gdm_layout &get_layout() const { return layout; }
  double *owned(VectorType &v) const { return v.get_values() + layout.ghost_planes_below * layout.plane_size; }
  const double *owned(const VectorType &v) const {
    return v.get_values() + layout.ghost_planes_below * layout.plane_size;
  }

 private:
  double *device_buffer(std::size_t n) const {
    void *p = nullptr;
    check(gdm_malloc(op, sizeof(double) * std::max<std::size_t>(n, 1), &p), "gdm_malloc");
    return static_cast<double *>(p);
  }
  void release() {
    if (op && fq_dev) gdm_free(op, fq_dev);
    if (op && g_dev) gdm_free(op, g_dev);
    fq_dev = g_dev = nullptr;
    gdm_op_destroy(op);
    op = nullptr;
    has_coefficient = false;
    has_density = false;
  }

  const Discretization<dim> &discretization;
  gdm_op *op = nullptr;
  gdm_layout layout{};
  bool has_coefficient = false, has_density = false;
  // data terms: the functions, their evaluation points and the staging buffers
  Function function_rhs, function_domain_dbc;
  std::vector<double> xq[3], bc_xyz;
  mutable std::vector<double> fq_host, g_host;
  double *fq_dev = nullptr, *g_dev = nullptr;
};

template <int dim>
class MassMatrixOperator {
 public:
  explicit MassMatrixOperator(const Discretization<dim> &discretization) : discretization(discretization) {}
  MassMatrixOperator(const MassMatrixOperator &) = delete;
  ~MassMatrixOperator() { gdm_op_destroy(op); }
  void reinit(const Parameters<dim> &) {
    gdm_op_destroy(op);
    op = nullptr;
    check(gdm_op_create(&discretization.get_mesh(), GDM_OP_MASS, nullptr, 0, discretization.get_device(), &op),
          "gdm_op_create");
    check(gdm_op_layout(op, &layout), "gdm_op_layout");
    check(gdm_op_set_stream(op, nullptr), "gdm_op_set_stream");
  }
  // WaveProblem::solve (problem.h:471-502): the AMG / ILU CG replaced by the
  // exact Kronecker inverse
  void solve(double *x_owned, const double *rhs_owned) const {
    check(gdm_mass_solve(op, rhs_owned, x_owned), "gdm_mass_solve");
  }
  void vmult(double *dst_owned, const double *src_local) const {
    check(gdm_mass_apply(op, src_local, dst_owned), "gdm_mass_apply");
  }
  std::size_t m() const { return (std::size_t)layout.n_dofs_global; }

 private:
  const Discretization<dim> &discretization;
  gdm_op *op = nullptr;
  gdm_layout layout{};
};

// WaveProblem<dim>::run, dispatched on Parameters::simulation_type as the
// reference's (problem.h:40-346):
//   "wave-rk"   y = (u, v), du/dt = v, dv/dt = M^-1 compute_rhs(u, true, t),
//               RK_CLASSIC_FOURTH_ORDER, DiscreteTime(start, end, cfl
//               dx^cfl_pow), device-resident in low-storage form
//               (gdm_vec_rk_update)
//   "heat-rk"   du/dt = M^-1 compute_rhs(u, true, t), the same RK4
//   "heat-impl" u := (M + h S)^-1 (M u + h compute_rhs(u, false, t + h)), h the
//               DiscreteTime step of every step
//   "poisson"   S u = compute_rhs(., false, 0); no time steps
template <int dim>
class WaveProblem {
 public:
  explicit WaveProblem(const Parameters<dim> &params)
      : params(params), mass_matrix_operator(discretization), stiffness_matrix_operator(discretization) {}

  unsigned int run(unsigned int max_steps = ~0u) {
    if (params.n_ranks != 1) throw Error("WaveProblem: the host RK driver is single-rank");
    discretization.reinit(params);
    mass_matrix_operator.reinit(params);
    stiffness_matrix_operator.reinit(params);
    const double delta_t = params.cfl * std::pow(discretization.get_dx(), params.cfl_pow);  // problem.h:284
    for (auto *v : {&u, &v_, &acc_u, &acc_v, &Yu, &Yv, &kv}) stiffness_matrix_operator.initialize_dof_vector(*v);
    const std::string &type = params.simulation_type;
    const StiffnessMatrixOperator<dim> &S = stiffness_matrix_operator;
    if (type == "poisson") {
      S.compute_rhs(kv, u, false, 0.0);
      S.setup_system_solve();
      S.system_solve(0.0, 1.0, S.owned(u), S.owned(kv));
      return 0;
    }
    if (type != "wave-rk" && type != "heat-rk" && type != "heat-impl")
      throw Error("WaveProblem: simulation_type is wave-rk, heat-rk, heat-impl or poisson");
    set_initial_condition(u);
    DiscreteTime time(params.start_t, params.end_t, delta_t);
    unsigned int n = 0;
    if (type == "heat-impl") {
      S.setup_system_solve();
      const int64_t n_owned = S.get_layout().n_owned;
      while (!time.is_at_end() && n < max_steps) {
        const double t0 = time.get_current_time(), h = time.get_next_step_size();
        // rhs = h compute_rhs(u, false, t0 + h) + M u
        S.compute_rhs(acc_u, u, false, t0 + h);
        mass_matrix_operator.vmult(S.owned(kv), u.get_values());
        check(gdm_vec_axpby(S.handle(), n_owned, h, S.owned(acc_u), 1.0, S.owned(kv)), "gdm_vec_axpby");
        S.system_solve(1.0, h, S.owned(u), S.owned(kv));
        time.advance_time();
        ++n;
      }
      return n;
    }
    if (type == "heat-rk") {
      while (!time.is_at_end() && n < max_steps) {
        const double t0 = time.get_current_time(), h = time.get_next_step_size();
        const DeviceVector *su = &u;
        for (int s = 0; s < 4; ++s) {
          S.compute_rhs(kv, *su, true, t0 + ClassicRK4::c[s] * h);
          double *r = S.owned(kv);
          mass_matrix_operator.solve(r, r);
          rk4_stage_update(s, h, kv, u, acc_u, Yu);
          su = &Yu;
        }
        time.advance_time();
        ++n;
      }
      return n;
    }
    while (!time.is_at_end() && n < max_steps) {
      const double t0 = time.get_current_time(), h = time.get_next_step_size();
      const DeviceVector *su = &u, *sv = &v_;
      for (int s = 0; s < 4; ++s) {
        // k = (stage v, M^-1 compute_rhs(stage u))   (problem.h:303-318)
        stiffness_matrix_operator.compute_rhs(kv, *su, true, t0 + ClassicRK4::c[s] * h);
        double *r = stiffness_matrix_operator.owned(kv);
        mass_matrix_operator.solve(r, r);
        // u block first: its k is the stage v, which the v update overwrites
        rk4_stage_update(s, h, *sv, u, acc_u, Yu);
        rk4_stage_update(s, h, kv, v_, acc_v, Yv);
        su = &Yu;
        sv = &Yv;
      }
      time.advance_time();
      ++n;
    }
    return n;
  }

  std::vector<double> get_solution() const { return u.download(); }
  std::vector<double> get_velocity() const { return v_.download(); }

 private:
  void set_initial_condition(DeviceVector &vec) const {  // VectorTools::interpolate: vertex values
    const gdm_mesh_desc &m = discretization.get_mesh();
    const gdm_layout &L = stiffness_matrix_operator.get_layout();
    std::vector<double> h(L.n_local);
    const int64_t N0 = m.n_subdivisions[0] + 1, N1 = dim > 1 ? m.n_subdivisions[1] + 1 : 1;
    const int64_t first_plane = L.owned_plane_begin - L.ghost_planes_below;
    for (int64_t i = 0; i < L.n_local; ++i) {
      const int64_t g = first_plane * L.plane_size + i;
      const int64_t id[3] = {g % N0, (g / N0) % N1, g / (N0 * N1)};
      Point x{0.0, 0.0, 0.0};
      for (int d = 0; d < dim; ++d) {
        const int64_t k = dim == 1 ? g : (dim == 2 ? (d == 0 ? g % N0 : g / N0) : id[d]);
        x[d] = m.lo[d] + k * (m.hi[d] - m.lo[d]) / m.n_subdivisions[d];
      }
      h[i] = params.exact_solution ? params.exact_solution(x, params.start_t) : 0.0;
    }
    vec.upload(h);
  }

  Parameters<dim> params;
  Discretization<dim> discretization;
  MassMatrixOperator<dim> mass_matrix_operator;
  StiffnessMatrixOperator<dim> stiffness_matrix_operator;
  DeviceVector u, v_, acc_u, acc_v, Yu, Yv, kv;
};

}  // namespace Wave
}  // namespace HIP
}  // namespace GDM
