// gdm_capi_cut.cpp -- C ABI of the cut-cell handles (declared in
// include/gdm_hip.h): cut Poisson, cut advection and cut wave / heat.  The host
// assembly is gdm_cut*.cpp, the box operator inside a handle a plain gdm_op.
#include <cstring>

#include "gdm_capi_internal.h"

using namespace gdm_detail;

extern "C" {

// ---- cut-cell systems (host assembly in gdm_cut.cpp) ----------------------
struct gdm_cut_system;
int gdmh_cut_poisson_create(int p, int n_sub, double lo, double hi, const double *center, double radius,
                            int ghost_penalty, double rhs_value, double bc_value, gdm_cut_system **out, char *err,
                            size_t err_len);
void gdmh_cut_info(const gdm_cut_system *S, int64_t *n_rows, int64_t *nnz, int64_t *n_inside, int64_t *n_intersected);
void gdmh_cut_arrays(const gdm_cut_system *S, const int64_t **row_ptr, const uint32_t **cols, const double **vals,
                     const double **rhs);
double gdmh_cut_l2_error(const gdm_cut_system *S, const double *u);
void gdmh_cut_destroy(gdm_cut_system *S);

int gdm_cut_poisson_create(int p, int n_sub, double lo, double hi, const double *center, double radius,
                           int ghost_penalty, double rhs_value, double bc_value, gdm_cut_system **out) {
  if (!out) return fail(GDM_ERR_ARG, "NULL argument");
  GDM_GUARD_BEGIN
  char err[256] = {0};
  if (gdmh_cut_poisson_create(p, n_sub, lo, hi, center, radius, ghost_penalty, rhs_value, bc_value, out, err,
                              sizeof(err)) != 0)
    return fail(std::strstr(err, "not implemented") ? GDM_ERR_UNSUPPORTED : GDM_ERR_ARG, err);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_poisson_info(const gdm_cut_system *S, int64_t *n_rows, int64_t *nnz, int64_t *n_inside_cells,
                         int64_t *n_intersected_cells) {
  if (!S || !n_rows || !nnz || !n_inside_cells || !n_intersected_cells) return fail(GDM_ERR_ARG, "NULL argument");
  gdmh_cut_info(S, n_rows, nnz, n_inside_cells, n_intersected_cells);
  return GDM_OK;
}

int gdm_cut_poisson_matrix(const gdm_cut_system *S, int device, gdm_csr **A) {
  if (!S || !A) return fail(GDM_ERR_ARG, "NULL argument");
  int64_t n, nnz, a, b;
  gdmh_cut_info(S, &n, &nnz, &a, &b);
  const int64_t *rp;
  const uint32_t *ci;
  const double *v, *r;
  gdmh_cut_arrays(S, &rp, &ci, &v, &r);
  return gdm_csr_create(device, n, n, nnz, rp, ci, v, 0, A);
}

int gdm_cut_poisson_csr(const gdm_cut_system *S, int64_t *row_ptr_host, uint32_t *cols_host, double *vals_host) {
  if (!S || !row_ptr_host || !cols_host || !vals_host) return fail(GDM_ERR_ARG, "NULL argument");
  int64_t n, nnz, a, b;
  gdmh_cut_info(S, &n, &nnz, &a, &b);
  const int64_t *rp;
  const uint32_t *ci;
  const double *v, *r;
  gdmh_cut_arrays(S, &rp, &ci, &v, &r);
  std::memcpy(row_ptr_host, rp, sizeof(int64_t) * (n + 1));
  std::memcpy(cols_host, ci, sizeof(uint32_t) * nnz);
  std::memcpy(vals_host, v, sizeof(double) * nnz);
  return GDM_OK;
}

int gdm_cut_poisson_rhs(const gdm_cut_system *S, double *rhs_host) {
  if (!S || !rhs_host) return fail(GDM_ERR_ARG, "NULL argument");
  int64_t n, nnz, a, b;
  gdmh_cut_info(S, &n, &nnz, &a, &b);
  const int64_t *rp;
  const uint32_t *ci;
  const double *v, *r;
  gdmh_cut_arrays(S, &rp, &ci, &v, &r);
  std::memcpy(rhs_host, r, sizeof(double) * n);
  return GDM_OK;
}

int gdm_cut_poisson_solve(const gdm_cut_system *S, gdm_csr *A, double rel_tol, double abs_tol, int max_it,
                          double *u_host, int *its_host, double *res_host) {
  if (!S || !A || !u_host) return fail(GDM_ERR_ARG, "NULL argument");
  int64_t n, nnz, a, b, m, mc, mz;
  gdmh_cut_info(S, &n, &nnz, &a, &b);
  if (gdm_csr_info(A, &m, &mc, &mz) != GDM_OK || m != n || mc != n) return fail(GDM_ERR_ARG, "matrix does not match the system");
  GDM_GUARD_BEGIN
  const int64_t *rp;
  const uint32_t *ci;
  const double *v, *r;
  gdmh_cut_arrays(S, &rp, &ci, &v, &r);
  double *bd = nullptr, *xd = nullptr;
  hip_check(hipMalloc(&bd, sizeof(double) * std::max<int64_t>(n, 1)), "hipMalloc rhs");
  if (hipMalloc(&xd, sizeof(double) * std::max<int64_t>(n, 1)) != hipSuccess) {
    (void)hipFree(bd);
    throw HipError("hipMalloc solution");
  }
  int rc = GDM_OK;
  try {
    hip_check(hipMemcpy(bd, r, sizeof(double) * n, hipMemcpyHostToDevice), "h2d rhs");
    hip_check(hipMemset(xd, 0, sizeof(double) * n), "memset");
    hip_check(hipDeviceSynchronize(), "sync");
    rc = gdm_csr_cg(A, bd, xd, 0, max_it, abs_tol, rel_tol, its_host, res_host);
    hip_check(hipDeviceSynchronize(), "sync");
    hip_check(hipMemcpy(u_host, xd, sizeof(double) * n, hipMemcpyDeviceToHost), "d2h solution");
  } catch (...) {
    (void)hipFree(bd);
    (void)hipFree(xd);
    throw;
  }
  (void)hipFree(bd);
  (void)hipFree(xd);
  return rc;
  GDM_GUARD_END
}

int gdm_cut_poisson_l2_error(const gdm_cut_system *S, const double *u_host, double *err) {
  if (!S || !u_host || !err) return fail(GDM_ERR_ARG, "NULL argument");
  GDM_GUARD_BEGIN
  *err = gdmh_cut_l2_error(S, u_host);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_poisson_destroy(gdm_cut_system *S) {
  gdmh_cut_destroy(S);
  return GDM_OK;
}

// ---------------------------------------------------------------------------
// Cut-cell advection (include/gdm_hip.h): host assembly of the corrections
// (gdm_cut_advection.cpp), the uncut stencil of the box, device CSR products
// and the banded mass solve (gdm_band.hip).
// ---------------------------------------------------------------------------
struct gdm_cut_adv_system;
int gdmh_cut_adv_create(int p, int n_sub, double lo, double hi, const double *level_set, const double *advection,
                        double gamma_A, double gamma_M, int composite, gdm_cut_adv_system **out, char *err,
                        size_t err_len);
void gdmh_cut_adv_coupling(const gdm_cut_adv_system *S, const int64_t **rp, const uint32_t **ci, const double **v,
                           int64_t *nnz);
void gdmh_cut_adv_info(const gdm_cut_adv_system *S, int64_t *n_dofs, int64_t *n_bc, int64_t *cells,
                       int64_t *bandwidth);
void gdmh_cut_adv_arrays(const gdm_cut_adv_system *S, const int64_t **c_rp, const uint32_t **c_ci,
                         const double **c_v, const int64_t **f_rp, const uint32_t **f_ci, const double **f_v,
                         const double **bc_xy, const double **lband);
void gdmh_cut_adv_zero_rows(const gdm_cut_adv_system *S, const int64_t **rows, int64_t *n);
void gdmh_cut_adv_destroy(gdm_cut_adv_system *S);
hipError_t gdmk_launch_zero_rows(int64_t n, const int64_t *rows, double *y, hipStream_t st);
hipError_t gdmk_launch_csr_accum(int64_t n_rows, const int64_t *rp, const uint32_t *ci, const double *v,
                                 const double *x, double *y, hipStream_t st);
hipError_t gdmk_launch_band_solve(int64_t n, int64_t bw, const double *L, double *x, hipStream_t st);

}  // extern "C"

struct gdm_cut_advection {
  gdm_cut_adv_system *host = nullptr;
  gdm_op *op = nullptr;
  int64_t n_dofs = 0, n_bc = 0, bw = 0, cells[3] = {0, 0, 0};
  int64_t *c_rp = nullptr, *f_rp = nullptr, *zrows = nullptr, n_zrows = 0;
  uint32_t *c_ci = nullptr, *f_ci = nullptr;
  double *c_v = nullptr, *f_v = nullptr, *lband = nullptr;
  int composite = 0;  // GDM_CUT_ADV_COMPOSITE: (II)'s inflow couples to the partner field (p_*)
  int64_t *p_rp = nullptr;
  uint32_t *p_ci = nullptr;
  double *p_v = nullptr;
  std::vector<double> bc_xy;
  void release() {
    for (void *q : {(void *)c_rp, (void *)f_rp, (void *)c_ci, (void *)f_ci, (void *)c_v, (void *)f_v, (void *)lband,
                    (void *)zrows, (void *)p_rp, (void *)p_ci, (void *)p_v})
      if (q) (void)hipFree(q);
    p_rp = nullptr;
    p_ci = nullptr;
    p_v = nullptr;
    zrows = nullptr;
    c_rp = f_rp = nullptr;
    c_ci = f_ci = nullptr;
    c_v = f_v = lband = nullptr;
    if (op) gdm_op_destroy(op);
    op = nullptr;
    if (host) gdmh_cut_adv_destroy(host);
    host = nullptr;
  }
};

extern "C" {

int gdm_cut_advection_create(int fe_degree, int n_subdivisions, double left, double right, const double *level_set,
                             const double *advection, double ghost_parameter_A, double ghost_parameter_M,
                             int device, gdm_cut_advection **out) {
  return gdm_cut_advection_create2(fe_degree, n_subdivisions, left, right, level_set, advection, ghost_parameter_A,
                                   ghost_parameter_M, GDM_CUT_INSIDE, 0, device, out);
}

int gdm_cut_advection_create2(int fe_degree, int n_subdivisions, double left, double right, const double *level_set,
                              const double *advection, double ghost_parameter_A, double ghost_parameter_M,
                              int location, int flags, int device, gdm_cut_advection **out) {
  if (!out || !level_set || !advection) return fail(GDM_ERR_ARG, "NULL argument");
  *out = nullptr;
  if (location != GDM_CUT_INSIDE && location != GDM_CUT_OUTSIDE)
    return fail(GDM_ERR_ARG, "location: GDM_CUT_INSIDE or GDM_CUT_OUTSIDE");
  if (flags & ~GDM_CUT_ADV_COMPOSITE) return fail(GDM_ERR_ARG, "flags: GDM_CUT_ADV_COMPOSITE only");
  GDM_GUARD_BEGIN
  auto *c = new gdm_cut_advection();
  try {
    char err[256] = {0};
    // the outside field = the same assembly on the negated level set (its inside is the outside region;
    // MeshClassifier, face parts, surface normal and ghost-penalty faces follow the sign)
    const size_t nv = n_subdivisions >= 0 ? (size_t)(n_subdivisions + 1) * (size_t)(n_subdivisions + 1) : 0;
    std::vector<double> ls(level_set, level_set + nv);
    if (location == GDM_CUT_OUTSIDE)
      for (double &v : ls) v = -v;
    c->composite = (flags & GDM_CUT_ADV_COMPOSITE) != 0;
    if (gdmh_cut_adv_create(fe_degree, n_subdivisions, left, right, ls.data(), advection, ghost_parameter_A,
                            ghost_parameter_M, c->composite, &c->host, err, sizeof(err)) != 0) {
      delete c;
      return fail(GDM_ERR_ARG, err);
    }
    // the uncut box operator S: 2D advection with the same a (stencil + outflow traces)
    gdm_mesh_desc m{};
    m.dim = 2;
    m.fe_degree = fe_degree;
    m.n_subdivisions[0] = m.n_subdivisions[1] = n_subdivisions;
    m.n_subdivisions[2] = 1;
    m.lo[0] = m.lo[1] = left;
    m.hi[0] = m.hi[1] = right;
    m.hi[2] = 1.0;
    m.n_ranks = 1;
    m.rank = 0;
    const int rc = gdm_op_create(&m, GDM_OP_ADVECTION, advection, 2, device, &c->op);
    if (rc != GDM_OK) {
      c->release();
      delete c;
      return rc;
    }
    c->op->cut_inner = true;  // the cut rows C, F are assembled for the constant field
    gdmh_cut_adv_info(c->host, &c->n_dofs, &c->n_bc, c->cells, &c->bw);
    const int64_t *crp, *frp;
    const uint32_t *cci, *fci;
    const double *cv, *fv, *xy, *lb;
    gdmh_cut_adv_arrays(c->host, &crp, &cci, &cv, &frp, &fci, &fv, &xy, &lb);
    const int64_t N = c->n_dofs;
    hip_check(hipSetDevice(device), "hipSetDevice");
    c->c_rp = dev_upload(std::vector<int64_t>(crp, crp + N + 1));
    c->c_ci = dev_upload(std::vector<uint32_t>(cci, cci + crp[N]));
    c->c_v = dev_upload(std::vector<double>(cv, cv + crp[N]));
    c->f_rp = dev_upload(std::vector<int64_t>(frp, frp + N + 1));
    c->f_ci = dev_upload(std::vector<uint32_t>(fci, fci + frp[N]));
    c->f_v = dev_upload(std::vector<double>(fv, fv + frp[N]));
    c->lband = dev_upload(std::vector<double>(lb, lb + N * (c->bw + 1)));
    const int64_t *zr;
    gdmh_cut_adv_zero_rows(c->host, &zr, &c->n_zrows);
    if (c->n_zrows > 0) c->zrows = dev_upload(std::vector<int64_t>(zr, zr + c->n_zrows));
    c->bc_xy.assign(xy, xy + 2 * c->n_bc);
    if (c->composite) {
      const int64_t *prp;
      const uint32_t *pci;
      const double *pv;
      int64_t pnnz = 0;
      gdmh_cut_adv_coupling(c->host, &prp, &pci, &pv, &pnnz);
      // (a field the flow only leaves through the surface has no coupling entries: pci / pv may be NULL)
      std::vector<uint32_t> ci(std::max<int64_t>(pnnz, 1), 0u);
      std::vector<double> cv(std::max<int64_t>(pnnz, 1), 0.0);
      if (pnnz > 0) {
        std::copy(pci, pci + pnnz, ci.begin());
        std::copy(pv, pv + pnnz, cv.begin());
      }
      c->p_rp = dev_upload(std::vector<int64_t>(prp, prp + N + 1));
      c->p_ci = dev_upload(ci);
      c->p_v = dev_upload(cv);
    }
  } catch (...) {
    c->release();
    delete c;
    throw;
  }
  *out = c;
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_advection_info(const gdm_cut_advection *c, int64_t *n_dofs, int64_t *n_bc_points, int64_t *cells,
                           int64_t *mass_bandwidth) {
  if (!c || !n_dofs || !n_bc_points || !cells || !mass_bandwidth) return fail(GDM_ERR_ARG, "NULL argument");
  *n_dofs = c->n_dofs;
  *n_bc_points = c->n_bc;
  for (int k = 0; k < 3; ++k) cells[k] = c->cells[k];
  *mass_bandwidth = c->bw;
  return GDM_OK;
}

int gdm_cut_advection_bc_points(const gdm_cut_advection *c, double *xy_host) {
  if (!c || (c->n_bc > 0 && !xy_host)) return fail(GDM_ERR_ARG, "NULL argument");
  std::copy(c->bc_xy.begin(), c->bc_xy.end(), xy_host);
  return GDM_OK;
}

int gdm_cut_advection_op(gdm_cut_advection *c, gdm_op **op) {
  if (!c || !op) return fail(GDM_ERR_ARG, "NULL argument");
  *op = c->op;
  return GDM_OK;
}

int gdm_cut_advection_compute_rhs(gdm_cut_advection *c, const double *u, const double *bc, double *rhs) {
  if (!c || !u || !rhs || (c->n_bc > 0 && !bc)) return fail(GDM_ERR_ARG, "NULL argument");
  if (u == rhs) return fail(GDM_ERR_ARG, "u and rhs must be distinct");
  const int rc = gdm_apply(c->op, u, rhs, nullptr);  // S u (no inflow data)
  if (rc != GDM_OK) return rc;
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(c->op->device), "hipSetDevice");
  hip_check(gdmk_launch_zero_rows(c->n_zrows, c->zrows, rhs, c->op->stream), "cut rows");
  hip_check(gdmk_launch_csr_accum(c->n_dofs, c->c_rp, c->c_ci, c->c_v, u, rhs, c->op->stream), "cut correction");
  if (c->n_bc > 0)
    hip_check(gdmk_launch_csr_accum(c->n_dofs, c->f_rp, c->f_ci, c->f_v, bc, rhs, c->op->stream), "inflow data");
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_advection_couple(gdm_cut_advection *c, const double *u_partner, double *rhs) {
  if (!c || !u_partner || !rhs) return fail(GDM_ERR_ARG, "NULL argument");
  if (!c->composite) return fail(GDM_ERR_STATE, "gdm_cut_advection_couple: created without GDM_CUT_ADV_COMPOSITE");
  if (u_partner == rhs) return fail(GDM_ERR_ARG, "u_partner and rhs must be distinct");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(c->op->device), "hipSetDevice");
  hip_check(gdmk_launch_csr_accum(c->n_dofs, c->p_rp, c->p_ci, c->p_v, u_partner, rhs, c->op->stream), "coupling");
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_advection_mass_solve(gdm_cut_advection *c, const double *rhs, double *x) {
  if (!c || !rhs || !x) return fail(GDM_ERR_ARG, "NULL argument");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(c->op->device), "hipSetDevice");
  if (x != rhs)
    hip_check(hipMemcpyAsync(x, rhs, sizeof(double) * c->n_dofs, hipMemcpyDeviceToDevice, c->op->stream), "copy");
  hip_check(gdmk_launch_band_solve(c->n_dofs, c->bw, c->lband, x, c->op->stream), "band solve");
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_advection_destroy(gdm_cut_advection *c) {
  if (!c) return GDM_OK;
  c->release();
  delete c;
  return GDM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Cut-cell wave / heat (1D and 2D; host assembly csrc/gdm_cut_wave.cpp)
// ---------------------------------------------------------------------------
struct gdm_cut_wave_system;
extern "C" {
int gdmh_cut_wave_create(int dim, int p, int n_sub, double lo, double hi, int ls_degree, const double *ls_values,
                         int location, int flags, double gamma_M, double gamma_A, double nitsche,
                         gdm_cut_wave_system **out, char *err, size_t err_len);
void gdmh_cut_wave_info(const gdm_cut_wave_system *S, int64_t *n_dofs, int64_t *n_quad, int64_t *n_surface,
                        int64_t *cells);
void gdmh_cut_wave_csr(const gdm_cut_wave_system *S, int which, const int64_t **rp, const uint32_t **ci,
                       const double **v);
void gdmh_cut_wave_points(const gdm_cut_wave_system *S, const double **qx, const double **qw, const double **sx,
                          const double **sn, const int64_t **zero_rows, int64_t *n_zero);
void gdmh_cut_wave_destroy(gdm_cut_wave_system *S);
int gdmh_cut_wave_splits(const gdm_cut_wave_system *S);
int64_t gdmh_band_cholesky(int64_t n, const int64_t *rp, const uint32_t *ci, const double *v, double alpha,
                           const int64_t *rp2, const uint32_t *ci2, const double *v2, std::vector<double> &lband);
}

// message for a failed gdmh_band_cholesky (-1: not positive definite, -2: too large)
static std::string band_error(int64_t code, const char *what) {
  return std::string("cut wave: ") + what +
         (code == -2 ? ": banded factor larger than 2^28 entries (mesh too large for the dense-band solve)"
                     : " not positive definite");
}


namespace {
struct DevCsr {
  int64_t rows = 0;
  int64_t *rp = nullptr;
  uint32_t *ci = nullptr;
  double *v = nullptr;
  void upload(const gdm_cut_wave_system *S, int which, int64_t n_rows) {
    const int64_t *hrp;
    const uint32_t *hci;
    const double *hv;
    gdmh_cut_wave_csr(S, which, &hrp, &hci, &hv);
    rows = n_rows;
    rp = dev_upload(std::vector<int64_t>(hrp, hrp + n_rows + 1));
    const int64_t nnz = hrp[n_rows];
    std::vector<uint32_t> c1(std::max<int64_t>(nnz, 1), 0);  // one padding entry for an empty matrix
    std::vector<double> v1(c1.size(), 0.0);
    if (nnz > 0) {
      std::copy(hci, hci + nnz, c1.begin());
      std::copy(hv, hv + nnz, v1.begin());
    }
    ci = dev_upload(c1);
    v = dev_upload(v1);
  }
  void release() {
    for (void *q : {(void *)rp, (void *)ci, (void *)v})
      if (q) (void)hipFree(q);
    rp = nullptr;
    ci = nullptr;
    v = nullptr;
  }
  void accum(const double *x, double *y, hipStream_t st) const {
    hip_check(gdmk_launch_csr_accum(rows, rp, ci, v, x, y, st), "csr accumulate");
  }
};
}  // namespace

struct gdm_cut_wave {
  gdm_cut_wave_system *host = nullptr;
  gdm_op *op = nullptr;
  int dim = 1;
  int64_t n_dofs = 0, n_quad = 0, n_surf = 0, cells[3] = {0, 0, 0};
  DevCsr C, Ff, Fg, E, M, X;
  bool coupled = false;
  int64_t *zrows = nullptr, n_zrows = 0;
  int64_t bw_m = -1, bw_a = -1, bw_k = -1;  // -1: no factor (no mass matrix when gamma_M < 0)
  double *lband_m = nullptr, *lband_a = nullptr, *lband_k = nullptr, dt_a = 0.0;
  void release() {
    for (DevCsr *q : {&C, &Ff, &Fg, &E, &M, &X}) q->release();
    for (void *q : {(void *)zrows, (void *)lband_m, (void *)lband_a, (void *)lband_k})
      if (q) (void)hipFree(q);
    zrows = nullptr;
    lband_m = lband_a = lband_k = nullptr;
    if (op) gdm_op_destroy(op);
    op = nullptr;
    if (host) gdmh_cut_wave_destroy(host);
    host = nullptr;
  }
};

extern "C" {

int gdm_cut_wave_create(int dim, int fe_degree, int n_subdivisions, double left, double right, int ls_degree,
                        const double *ls_values, int location, int flags, double gamma_M, double gamma_A,
                        double nitsche, int device, gdm_cut_wave **out) {
  if (!out || !ls_values) return fail(GDM_ERR_ARG, "NULL argument");
  *out = nullptr;
  GDM_GUARD_BEGIN
  auto *c = new gdm_cut_wave();
  try {
    char err[256] = {0};
    if (gdmh_cut_wave_create(dim, fe_degree, n_subdivisions, left, right, ls_degree, ls_values, location, flags,
                             gamma_M, gamma_A, nitsche, &c->host, err, sizeof(err)) != 0) {
      delete c;
      return fail(GDM_ERR_ARG, err);
    }
    // the uncut box operator S: wave -(grad v, grad u) of the box (no box Nitsche)
    c->dim = dim;
    gdm_mesh_desc m{};
    m.dim = dim;
    m.fe_degree = fe_degree;
    for (int d = 0; d < 3; ++d) {
      m.n_subdivisions[d] = d < dim ? n_subdivisions : 1;
      m.lo[d] = d < dim ? left : 0.0;
      m.hi[d] = d < dim ? right : 1.0;
    }
    m.n_ranks = 1;
    m.rank = 0;
    const int rc = gdm_op_create(&m, GDM_OP_WAVE, nullptr, 0, device, &c->op);
    if (rc != GDM_OK) {
      c->release();
      delete c;
      return rc;
    }
    c->op->cut_inner = true;  // the data terms of the cut system are Ff, Fg, not the box's
    gdmh_cut_wave_info(c->host, &c->n_dofs, &c->n_quad, &c->n_surf, c->cells);
    gdm_layout L{};
    if (gdm_op_layout(c->op, &L) != GDM_OK || L.n_local != c->n_dofs || L.n_owned != c->n_dofs)
      throw std::runtime_error("cut wave: the box operator's layout is not the cut system's DoF range");
    hip_check(hipSetDevice(device), "hipSetDevice");
    c->C.upload(c->host, 0, c->n_dofs);
    c->Ff.upload(c->host, 1, c->n_dofs);
    c->Fg.upload(c->host, 2, c->n_dofs);
    c->E.upload(c->host, 3, c->n_quad);
    c->M.upload(c->host, 4, c->n_dofs);
    c->coupled = (flags & GDM_CUT_WAVE_COUPLED) != 0;
    if (c->coupled) c->X.upload(c->host, 6, c->n_dofs);
    const double *qx, *qw, *sx, *sn;
    const int64_t *zr;
    gdmh_cut_wave_points(c->host, &qx, &qw, &sx, &sn, &zr, &c->n_zrows);
    if (c->n_zrows > 0) c->zrows = dev_upload(std::vector<int64_t>(zr, zr + c->n_zrows));
    const int64_t *rp;
    const uint32_t *ci;
    const double *v;
    if (gamma_M >= 0.0) {
      gdmh_cut_wave_csr(c->host, 4, &rp, &ci, &v);
      std::vector<double> lb;
      c->bw_m = gdmh_band_cholesky(c->n_dofs, rp, ci, v, 0.0, nullptr, nullptr, nullptr, lb);
      if (c->bw_m < 0) throw std::runtime_error(band_error(c->bw_m, "mass matrix"));
      c->lband_m = dev_upload(lb);
    }
  } catch (...) {
    c->release();
    delete c;
    throw;
  }
  *out = c;
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_wave_info(const gdm_cut_wave *c, int64_t *n_dofs, int64_t *n_quad, int64_t *n_surface, int64_t *cells) {
  if (!c || !n_dofs || !n_quad || !n_surface || !cells) return fail(GDM_ERR_ARG, "NULL argument");
  *n_dofs = c->n_dofs;
  *n_quad = c->n_quad;
  *n_surface = c->n_surf;
  for (int k = 0; k < 3; ++k) cells[k] = c->cells[k];
  return GDM_OK;
}

int gdm_cut_wave_points(const gdm_cut_wave *c, double *qx, double *qw, double *sx, double *sn) {
  if (!c) return fail(GDM_ERR_ARG, "NULL argument");
  const double *hqx, *hqw, *hsx, *hsn;
  const int64_t *zr;
  int64_t nz;
  gdmh_cut_wave_points(c->host, &hqx, &hqw, &hsx, &hsn, &zr, &nz);
  if (qx) std::copy(hqx, hqx + c->n_quad * c->dim, qx);
  if (qw) std::copy(hqw, hqw + c->n_quad, qw);
  if (sx) std::copy(hsx, hsx + c->n_surf * c->dim, sx);
  if (sn) std::copy(hsn, hsn + c->n_surf * c->dim, sn);
  return GDM_OK;
}

int gdm_cut_wave_op(gdm_cut_wave *c, gdm_op **op) {
  if (!c || !op) return fail(GDM_ERR_ARG, "NULL argument");
  *op = c->op;
  return GDM_OK;
}

int gdm_cut_wave_compute_rhs(gdm_cut_wave *c, const double *u, const double *fq, const double *gs, double *rhs) {
  if (!c || !rhs) return fail(GDM_ERR_ARG, "NULL argument");
  if (u == rhs) return fail(GDM_ERR_ARG, "u and rhs must be distinct");
  if (u) {
    const int rc = gdm_apply(c->op, u, rhs, nullptr);  // S u
    if (rc != GDM_OK) return rc;
  }
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(c->op->device), "hipSetDevice");
  hipStream_t st = c->op->stream;
  if (u) {
    hip_check(gdmk_launch_zero_rows(c->n_zrows, c->zrows, rhs, st), "cut rows");
    c->C.accum(u, rhs, st);
  } else {
    hip_check(gdmk_launch_zero(c->n_dofs, rhs, st), "zero");
  }
  if (fq && c->n_quad > 0) c->Ff.accum(fq, rhs, st);
  if (gs && c->n_surf > 0) c->Fg.accum(gs, rhs, st);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_wave_couple(gdm_cut_wave *c, const double *u_other, double *rhs) {
  if (!c || !u_other || !rhs) return fail(GDM_ERR_ARG, "NULL argument");
  if (!c->coupled) return fail(GDM_ERR_ARG, "gdm_cut_wave_couple: created without GDM_CUT_WAVE_COUPLED");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(c->op->device), "hipSetDevice");
  c->X.accum(u_other, rhs, c->op->stream);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_wave_mass_apply(gdm_cut_wave *c, const double *u, double *out) {
  if (!c || !u || !out || u == out) return fail(GDM_ERR_ARG, "NULL or aliased argument");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(c->op->device), "hipSetDevice");
  hip_check(gdmk_launch_zero(c->n_dofs, out, c->op->stream), "zero");
  c->M.accum(u, out, c->op->stream);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_wave_mass_solve(gdm_cut_wave *c, const double *rhs, double *x) {
  if (!c || !rhs || !x) return fail(GDM_ERR_ARG, "NULL argument");
  if (c->bw_m < 0) return fail(GDM_ERR_ARG, "gdm_cut_wave_mass_solve: no mass matrix (gamma_M < 0)");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(c->op->device), "hipSetDevice");
  if (x != rhs)
    hip_check(hipMemcpyAsync(x, rhs, sizeof(double) * c->n_dofs, hipMemcpyDeviceToDevice, c->op->stream), "copy");
  hip_check(gdmk_launch_band_solve(c->n_dofs, c->bw_m, c->lband_m, x, c->op->stream), "band solve");
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_wave_system_solve(gdm_cut_wave *c, double dt, const double *rhs, double *x) {
  if (!c || !rhs || !x) return fail(GDM_ERR_ARG, "NULL argument");
  if (!(dt > 0.0)) return fail(GDM_ERR_ARG, "gdm_cut_wave_system_solve: dt must be positive");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(c->op->device), "hipSetDevice");
  if (c->bw_a < 0 || dt != c->dt_a) {
    const int64_t *rp, *rp2;
    const uint32_t *ci, *ci2;
    const double *v, *v2;
    gdmh_cut_wave_csr(c->host, 4, &rp, &ci, &v);
    gdmh_cut_wave_csr(c->host, 5, &rp2, &ci2, &v2);
    std::vector<double> lb;
    const int64_t bw = gdmh_band_cholesky(c->n_dofs, rp, ci, v, dt, rp2, ci2, v2, lb);
    if (bw < 0) throw std::runtime_error(band_error(bw, "M + dt K"));
    // the previous factor may still be read by queued solves
    hip_check(hipStreamSynchronize(c->op->stream), "hipStreamSynchronize");
    if (c->lband_a) (void)hipFree(c->lband_a);
    c->lband_a = dev_upload(lb);
    c->bw_a = bw;
    c->dt_a = dt;
  }
  if (x != rhs)
    hip_check(hipMemcpyAsync(x, rhs, sizeof(double) * c->n_dofs, hipMemcpyDeviceToDevice, c->op->stream), "copy");
  hip_check(gdmk_launch_band_solve(c->n_dofs, c->bw_a, c->lband_a, x, c->op->stream), "band solve");
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_wave_stiffness_solve(gdm_cut_wave *c, const double *rhs, double *x) {
  if (!c || !rhs || !x) return fail(GDM_ERR_ARG, "NULL argument");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(c->op->device), "hipSetDevice");
  if (c->bw_k < 0) {
    const int64_t *rp;
    const uint32_t *ci;
    const double *v;
    gdmh_cut_wave_csr(c->host, 5, &rp, &ci, &v);
    std::vector<double> lb;
    const int64_t bw = gdmh_band_cholesky(c->n_dofs, rp, ci, v, 0.0, nullptr, nullptr, nullptr, lb);
    if (bw < 0) throw std::runtime_error(band_error(bw, "stiffness matrix"));
    c->lband_k = dev_upload(lb);
    c->bw_k = bw;
  }
  if (x != rhs)
    hip_check(hipMemcpyAsync(x, rhs, sizeof(double) * c->n_dofs, hipMemcpyDeviceToDevice, c->op->stream), "copy");
  hip_check(gdmk_launch_band_solve(c->n_dofs, c->bw_k, c->lband_k, x, c->op->stream), "band solve");
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_wave_eval(gdm_cut_wave *c, const double *u, double *vals) {
  if (!c || !u || !vals) return fail(GDM_ERR_ARG, "NULL argument");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(c->op->device), "hipSetDevice");
  hip_check(gdmk_launch_zero(c->n_quad, vals, c->op->stream), "zero");
  c->E.accum(u, vals, c->op->stream);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_cut_wave_destroy(gdm_cut_wave *c) {
  if (!c) return GDM_OK;
  c->release();
  delete c;
  return GDM_OK;
}

}  // extern "C"