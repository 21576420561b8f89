// gdm/hip/elasticity.h -- C++ host mirror of the linear-elasticity test of the
// reference (tests/elasticity_01_gdm.cc) over the C ABI of libgdm_hip.so:
//   ElasticityOperator<dim>   the assembled matrix of :143-160 with the zero
//                             boundary constraints of :93-96 (system.h:466-498),
//                             matrix-free on the device; vmult = SparseMatrix::vmult
//   assemble_rhs              the element vectors of :162-170 (gdm_add_load per
//                             component, the function sampled on the Gauss grid)
//   solve                     SolverCG + ReductionControl of :181-184 with
//                             PreconditionJacobi (:178-179) or the block
//                             fast-diagonalisation preconditioner
//   l2_error                  integrate_difference + compute_global_error, :186-198
// Vectors are component-major device buffers [u_0 | u_1 | (u_2)]; to_reference /
// from_reference convert to the reference's vertex * n_components + component
// numbering (system.h:242-244).
#pragma once

#include <gdm/hip/operators.h>

namespace GDM {
namespace HIP {
namespace Elasticity {

enum class Preconditioner { none = 0, jacobi = 1, fastdiag = 2 };

// (x, component) -> value
using VectorFunction = std::function<double(const Point &, unsigned int)>;

template <int dim>
class ElasticityOperator {
  static_assert(dim == 2 || dim == 3, "elasticity: dim 2 or 3");

public:
  ElasticityOperator(unsigned int fe_degree, unsigned int n_subdivisions_1D, double mu = 1.0, double lambda = 0.0,
                     double left = 0.0, double right = 1.0, int device = 0) {
    mesh.dim = dim;
    mesh.fe_degree = (int)fe_degree;
    for (int d = 0; d < 3; ++d) {
      mesh.n_subdivisions[d] = d < dim ? (int)n_subdivisions_1D : 1;
      mesh.lo[d] = d < dim ? left : 0.0;
      mesh.hi[d] = d < dim ? right : 1.0;
    }
    mesh.n_ranks = 1;
    mesh.rank = 0;
    mesh.periodic = 0;
    const double params[2] = {mu, lambda};
    check(gdm_op_create(&mesh, GDM_OP_ELASTICITY, params, 2, device, &op), "gdm_op_create");
    check(gdm_op_layout(op, &layout), "gdm_op_layout");
    check(gdm_op_set_stream(op, nullptr), "gdm_op_set_stream");  // ordered with the DeviceVector copies
  }
  ~ElasticityOperator() { gdm_op_destroy(op); }
  ElasticityOperator(const ElasticityOperator &) = delete;
  ElasticityOperator &operator=(const ElasticityOperator &) = delete;

  static constexpr unsigned int n_components = dim;
  std::size_t n_vertices() const { return (std::size_t)layout.n_owned; }
  std::size_t n_dofs() const { return n_components * n_vertices(); }
  gdm_op *handle() const { return op; }

  void initialize_dof_vector(DeviceVector &v) const { v.reinit(op, n_dofs()); }

  void vmult(DeviceVector &dst, const DeviceVector &src) const {
    check(gdm_apply(op, src.get_values(), dst.get_values(), nullptr), "gdm_apply");
  }

  // the tensor Gauss grid of gdm_add_load: f(x_q, c) for every point, x fastest
  std::vector<double> sample(const VectorFunction &f, unsigned int c) const {
    std::vector<double> ax[3];
    std::size_t Q[3] = {1, 1, 1};
    for (int d = 0; d < dim; ++d) {
      Q[d] = (std::size_t)mesh.n_subdivisions[d] * (mesh.fe_degree + 1);
      std::vector<double> x(Q[d] + 2);
      check(gdm_field_points(&mesh, d, x.data()), "gdm_field_points");
      ax[d].assign(x.begin() + 1, x.end() - 1);
    }
    std::vector<double> out(Q[0] * Q[1] * Q[2]);
    for (std::size_t k = 0; k < Q[2]; ++k)
      for (std::size_t j = 0; j < Q[1]; ++j)
        for (std::size_t i = 0; i < Q[0]; ++i) {
          const Point x = {ax[0][i], dim > 1 ? ax[1][j] : 0.0, dim > 2 ? ax[2][k] : 0.0};
          out[(k * Q[1] + j) * Q[0] + i] = f(x, c);
        }
    return out;
  }

  // rhs_c = (v_c, f_c) over QGauss(p + 1); rhs is overwritten
  void assemble_rhs(DeviceVector &rhs, const VectorFunction &f) const {
    rhs = 0.0;
    for (unsigned int c = 0; c < n_components; ++c) {
      DeviceVector fq;
      const std::vector<double> h = sample(f, c);
      fq.reinit(op, h.size());
      fq.upload(h);
      check(gdm_add_load(op, fq.get_values(), 1.0, rhs.get_values() + c * n_vertices()), "gdm_add_load");
    }
  }

  // returns the iteration count; x is the initial guess
  unsigned int solve(DeviceVector &x, const DeviceVector &rhs, Preconditioner precond, unsigned int max_it = 100,
                     double abs_tol = 1e-10, double rel_tol = 1e-8) const {
    if (precond == Preconditioner::fastdiag) check(gdm_elasticity_precond_setup(op), "gdm_elasticity_precond_setup");
    int its = 0;
    double res = 0.0;
    check(gdm_elasticity_solve(op, rhs.get_values(), x.get_values(), (int)precond, rel_tol, abs_tol, (int)max_it, &its,
                               &res),
          "gdm_elasticity_solve");
    return (unsigned int)its;
  }

  double l2_error(const DeviceVector &x, const VectorFunction &exact) const {
    double e2 = 0.0;
    for (unsigned int c = 0; c < n_components; ++c) {
      DeviceVector eq;
      const std::vector<double> h = sample(exact, c);
      eq.reinit(op, h.size());
      eq.upload(h);
      double norms[3];
      check(gdm_error_norms_grid(op, x.get_values() + c * n_vertices(), eq.get_values(), nullptr, norms),
            "gdm_error_norms_grid");
      e2 += norms[2] * norms[2];
    }
    return std::sqrt(e2);
  }

  void to_reference(DeviceVector &dst, const DeviceVector &src) const {
    check(gdm_vec_interleave(op, (int)n_components, 1, src.get_values(), dst.get_values()), "gdm_vec_interleave");
  }
  void from_reference(DeviceVector &dst, const DeviceVector &src) const {
    check(gdm_vec_interleave(op, (int)n_components, 0, src.get_values(), dst.get_values()), "gdm_vec_interleave");
  }

private:
  gdm_mesh_desc mesh{};
  gdm_op *op = nullptr;
  gdm_layout layout{};
};

}  // namespace Elasticity
}  // namespace HIP
}  // namespace GDM
