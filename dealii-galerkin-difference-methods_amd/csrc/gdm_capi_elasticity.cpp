// gdm_capi_elasticity.cpp -- C ABI of the linear elasticity operator
// (GDM_OP_ELASTICITY): its tables, the block fast-diagonalisation preconditioner
// and the CG solve (declared in include/gdm_hip.h).
#include "gdm_capi_internal.h"
#include "gdm_fastdiag.h"

using namespace gdm_detail;

namespace {

// w[c][d]: weight of L_d in the diagonal block c of 2 mu (eps, eps) + lambda (div, div)
void elasticity_weights(double mu, double lambda, double w[3][3]) {
  for (int c = 0; c < 3; ++c)
    for (int d = 0; d < 3; ++d) w[c][d] = c == d ? 2.0 * mu + lambda : mu;
}

gdm::ElasticityBands1D elasticity_bands(const gdm_mesh_desc *mesh, int d) {
  const unsigned nc = (unsigned)mesh->n_subdivisions[d];
  return gdm::elasticity_bands_1d(mesh->fe_degree, nc, (mesh->hi[d] - mesh->lo[d]) / nc);
}

// the kernel's table of one direction: [4][N][2p+1] in the order M, C, C^T, L
std::vector<double> elasticity_table(const gdm::ElasticityBands1D &b) {
  std::vector<double> t;
  t.reserve(4 * b.M.a.size());
  for (const gdm::Band *f : {&b.M, &b.C, &b.Ct, &b.L}) t.insert(t.end(), f->a.begin(), f->a.end());
  return t;
}

// diag(P A P + I - P), component-major: C has a zero diagonal, so only the
// diagonal blocks contribute, each a sum of products of 1D diagonals
std::vector<double> elasticity_diagonal_host(const gdm_mesh_desc *mesh, double mu, double lambda) {
  const int dim = mesh->dim;
  double w[3][3];
  elasticity_weights(mu, lambda, w);
  std::vector<double> dm[3], dl[3];
  int N[3] = {1, 1, 1};
  for (int d = 0; d < 3; ++d) {
    if (d >= dim) {
      dm[d].assign(1, 1.0);
      dl[d].assign(1, 0.0);
      continue;
    }
    const gdm::ElasticityBands1D b = elasticity_bands(mesh, d);
    N[d] = b.M.n;
    dm[d].resize(N[d]);
    dl[d].resize(N[d]);
    for (int i = 0; i < N[d]; ++i) {
      dm[d][i] = b.M(i, i);
      dl[d][i] = b.L(i, i);
    }
  }
  const int64_t n = (int64_t)N[0] * N[1] * N[2];
  std::vector<double> out((size_t)(n * dim));
  for (int c = 0; c < dim; ++c)
    for (int i2 = 0; i2 < N[2]; ++i2)
      for (int i1 = 0; i1 < N[1]; ++i1)
        for (int i0 = 0; i0 < N[0]; ++i0) {
          const int id[3] = {i0, i1, i2};
          bool constrained = false;
          for (int d = 0; d < dim; ++d) constrained = constrained || id[d] == 0 || id[d] == N[d] - 1;
          double s = 0.0;
          for (int d = 0; d < dim; ++d) {
            double t = w[c][d];
            for (int e = 0; e < dim; ++e) t *= e == d ? dl[e][id[e]] : dm[e][id[e]];
            s += t;
          }
          out[(size_t)(c * n + ((int64_t)i2 * N[1] + i1) * N[0] + i0)] = constrained ? 1.0 : s;
        }
  return out;
}

// 1 on the free DoFs, 0 on the constrained ones, component-major
std::vector<double> elasticity_mask_host(const gdm_op *op) {
  const int64_t n = op->layout.n_owned;
  std::vector<double> m((size_t)(n * op->dim));
  for (int64_t i = 0; i < n; ++i) {
    const int64_t id[3] = {i % op->N[0], (i / op->N[0]) % op->N[1], i / ((int64_t)op->N[0] * op->N[1])};
    bool constrained = false;
    for (int d = 0; d < op->dim; ++d) constrained = constrained || id[d] == 0 || id[d] == op->N[d] - 1;
    for (int c = 0; c < op->dim; ++c) m[(size_t)(c * n + i)] = constrained ? 0.0 : 1.0;
  }
  return m;
}

}  // namespace

void gdm_detail::build_elasticity(gdm_op *op) {
  gdmk::ElasArgs &A = op->el.args;
  const double *tab[3] = {nullptr, nullptr, nullptr};
  for (int d = 0; d < op->dim; ++d) tab[d] = keep(op, dev_upload(elasticity_table(elasticity_bands(&op->mesh, d))));
  A.xtab = tab[0];
  A.ytab = tab[1];
  A.ztab = tab[2];
  A.Nx = op->K[0];
  A.Ny = op->K[1];
  A.Nz = op->K[2];
  A.comp_stride = op->layout.n_owned;
  A.mu = op->el.mu;
  A.lambda = op->el.lambda;
  elasticity_weights(op->el.mu, op->el.lambda, A.w);
}

void gdm_detail::elasticity_apply(gdm_op *op, const double *src, double *dst) {
  gdmk::ElasArgs A = op->el.args;
  A.src = src;
  A.dst = dst;
  hip_check(gdmk::launch_elasticity(op->p, op->dim, A, op->stream), "elasticity launch");
}

namespace {

// shared refusals of the elasticity entry points; 0 = ok
int check_elasticity_op(gdm_op *op, const char *what, bool need_setup) {
  if (!op) return fail(GDM_ERR_ARG, "op is NULL");
  if (op->kind != GDM_OP_ELASTICITY) return fail(GDM_ERR_UNSUPPORTED, std::string(what) + ": elasticity operators only");
  if (need_setup && !op->el.built)
    return fail(GDM_ERR_STATE, std::string(what) + ": call gdm_elasticity_precond_setup first");
  return GDM_OK;
}

// z = B^-1 r, component by component: S^T along x, y, z (the last one scales by
// 1 / sum_d w_cd lambda_d), S along z, y, x, through the two scratch vectors
void elasticity_precond_launch(gdm_op *op, const double *r, double *z) {
  const int64_t n = op->layout.n_owned;
  const int n_axes = op->dim, n_pass = 2 * n_axes;
  for (int c = 0; c < op->dim; ++c) {
    const double *src = r + c * n;
    for (int i = 0; i < n_pass; ++i) {
      const bool fwd = i < n_axes;
      const int ax = fwd ? i : n_pass - 1 - i;
      gdmk::FastdiagPass P = fastdiag_pass(op, ax, fwd ? op->el.S[ax] : op->el.St[ax]);
      if (i == n_axes - 1) {
        P.scale = 1;
        P.alpha = 0.0;
        P.tau = 1.0;
        P.lam0 = op->el.lam[c][0];
        P.lam1 = op->el.lam[c][1];
        P.lam2 = op->el.lam[c][2];
      }
      double *dst = i == n_pass - 1 ? z + c * n : op->el.tmp[i & 1];
      hip_check(gdmk_launch_fastdiag_pass(P, src, dst, op->stream), "fastdiag pass");
      src = dst;
    }
  }
}

void elasticity_need_invdiag(gdm_op *op) {
  if (op->el.invdiag) return;
  std::vector<double> inv = elasticity_diagonal_host(&op->mesh, op->el.mu, op->el.lambda);
  for (double &v : inv) v = 1.0 / v;
  op->el.invdiag = keep(op, dev_upload(inv));
}

}  // namespace

extern "C" {

int gdm_elasticity_tile(int fe_degree, int dim, int *tile_x, int *tile_y, int *z_chunk) {
  if (int rc = check_tile_query(fe_degree, dim, 2)) return rc;
  return tile_answer(gdmk::ELAS_TX, gdmk::ELAS_TY, dim == 3 ? gdmk::ELAS_ZC : 1, tile_x, tile_y, z_chunk);
}

int gdm_elasticity_tables_1d(const gdm_mesh_desc *mesh, int axis, double *bands_host, double *S_host,
                             double *lambda_host) {
  if (int rc = check_field_mesh(mesh, axis)) return rc;
  for (int d = 0; d < mesh->dim; ++d)
    if (mesh->n_subdivisions[d] < 1 || !(mesh->hi[d] > mesh->lo[d])) return fail(GDM_ERR_ARG, "empty box");
  if ((S_host == nullptr) != (lambda_host == nullptr)) return fail(GDM_ERR_ARG, "S_host and lambda_host go together");
  GDM_GUARD_BEGIN
  if (bands_host) {
    const std::vector<double> t = elasticity_table(elasticity_bands(mesh, axis));
    std::copy(t.begin(), t.end(), bands_host);
  }
  if (S_host) {
    const unsigned nc = (unsigned)mesh->n_subdivisions[axis];
    std::vector<double> S, lambda;
    gdm::elasticity_fastdiag_1d(mesh->fe_degree, nc, (mesh->hi[axis] - mesh->lo[axis]) / nc, S, lambda);
    std::copy(S.begin(), S.end(), S_host);
    std::copy(lambda.begin(), lambda.end(), lambda_host);
  }
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_elasticity_diagonal(gdm_op *op, double *diag) {
  if (int rc = check_elasticity_op(op, "gdm_elasticity_diagonal", false)) return rc;
  if (!diag) return fail(GDM_ERR_ARG, "NULL vector");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  const std::vector<double> d = elasticity_diagonal_host(&op->mesh, op->el.mu, op->el.lambda);
  hip_check(hipMemcpyAsync(diag, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice, op->stream), "h2d");
  hip_check(hipStreamSynchronize(op->stream), "sync");
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_elasticity_precond_setup(gdm_op *op) {
  if (int rc = check_elasticity_op(op, "gdm_elasticity_precond_setup", false)) return rc;
  if (op->el.built) return GDM_OK;
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  // everything is uploaded before the handle changes: a failure leaves it as it was
  gdm_op::Elasticity ne = op->el;
  std::vector<void *> made;
  try {
    double w[3][3];
    elasticity_weights(op->el.mu, op->el.lambda, w);
    for (int d = 0; d < op->dim; ++d) {  // kernel axis d = reference direction d in 2D and 3D
      const unsigned nc = (unsigned)op->mesh.n_subdivisions[d];
      std::vector<double> S, lambda;
      gdm::elasticity_fastdiag_1d(op->p, nc, (op->mesh.hi[d] - op->mesh.lo[d]) / nc, S, lambda);
      const int n = (int)lambda.size();
      std::vector<double> St((size_t)n * n);
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) St[(size_t)j * n + i] = S[(size_t)i * n + j];
      ne.S[d] = up(made, S);
      ne.St[d] = up(made, St);
      for (int c = 0; c < op->dim; ++c) {
        std::vector<double> wl(lambda);
        for (double &v : wl) v *= w[c][d];
        ne.lam[c][d] = up(made, wl);
      }
    }
    for (int i = 0; i < 2; ++i) {
      double *t = nullptr;
      hip_check(hipMalloc(&t, std::max<size_t>((size_t)op->layout.n_owned, 1) * sizeof(double)), "hipMalloc");
      made.push_back(t);
      ne.tmp[i] = t;
    }
  } catch (...) {
    for (void *ptr : made) (void)hipFree(ptr);
    throw;
  }
  for (void *ptr : made) op->allocations.push_back(ptr);
  ne.built = true;
  op->el = ne;
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_elasticity_precond(gdm_op *op, const double *r, double *z) {
  if (int rc = check_elasticity_op(op, "gdm_elasticity_precond", true)) return rc;
  if (!r || !z || r == z) return fail(GDM_ERR_ARG, "gdm_elasticity_precond: r and z are distinct device vectors");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  elasticity_precond_launch(op, r, z);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_elasticity_solve(gdm_op *op, const double *rhs, double *x, int precond, double rel_tol, double abs_tol,
                         int max_it, int *its_host, double *res_host) {
  if (int rc = check_elasticity_op(op, "gdm_elasticity_solve", precond == 2)) return rc;
  if (!rhs || !x || rhs == x) return fail(GDM_ERR_ARG, "rhs and x: distinct device vectors");
  if (precond < 0 || precond > 2) return fail(GDM_ERR_ARG, "precond: 0 none, 1 Jacobi, 2 block fast diagonalisation");
  if (max_it < 0) return fail(GDM_ERR_ARG, "max_it < 0");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  const int64_t n = op->layout.n_owned * op->dim;
  for (double *&v : op->el.cg)
    if (!v) v = keep(op, dev_upload(std::vector<double>((size_t)std::max<int64_t>(n, 1), 0.0)));
  if (!op->el.free_mask) op->el.free_mask = keep(op, dev_upload(elasticity_mask_host(op)));
  if (precond == 1) elasticity_need_invdiag(op);
  double *r = op->el.cg[0], *p = op->el.cg[1], *Ap = op->el.cg[2], *z = op->el.cg[3], *b = op->el.cg[4];
  auto apply = [&](const double *src, double *dst) { elasticity_apply(op, src, dst); };
  auto precondition = [&](const double *rr, double *zz) {
    if (precond == 2)
      elasticity_precond_launch(op, rr, zz);
    else if (precond == 1)
      hip_check(gdmk_launch_vmul(n, op->el.invdiag, rr, zz, op->stream), "jacobi");
    else
      hip_check(hipMemcpyAsync(zz, rr, sizeof(double) * n, hipMemcpyDeviceToDevice, op->stream), "copy");
  };
  // the constrained entries of rhs count as 0 and those of x are 0 (the zero
  // boundary constraints); then SolverCG with ReductionControl(max_it, abs_tol,
  // rel_tol) on P A P + I - P: r = b - A x
  hip_check(gdmk_launch_vmul(n, op->el.free_mask, rhs, b, op->stream), "mask");
  hip_check(gdmk_launch_vmul(n, op->el.free_mask, x, p, op->stream), "mask");
  hip_check(hipMemcpyAsync(x, p, sizeof(double) * n, hipMemcpyDeviceToDevice, op->stream), "copy");
  const gdm::PcgResult res = device_pcg(op, n, apply, precondition, r, p, Ap, z, b, x, rel_tol, abs_tol, max_it);
  return finish_pcg(res, "gdm_elasticity_solve", its_host, res_host);
  GDM_GUARD_END
}

}  // extern "C"
