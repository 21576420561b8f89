// gdm_capi_internal.h -- what the translation units of the C ABI share (gdm_capi.cpp,
// gdm_capi_coef.cpp, gdm_capi_elasticity.cpp, gdm_capi_cut.cpp): the operator handle, the
// error plumbing and the helpers that cross file boundaries (namespace gdm_detail).
#ifndef GDM_CAPI_INTERNAL_H
#define GDM_CAPI_INTERNAL_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/gdm_hip.h"
#include "gdm_coefgrid.h"
#include "gdm_elasticity.h"
#include "gdm_evalgrid.h"
#include "gdm_kernels.h"
#include "gdm_massgrid.h"
#include "gdm_pcg.h"
#include "gdm_periodic.h"
#include "gdm_rk.h"
#include "gdm_setup.h"
#include "gdm_vardiff.h"
#include "gdm_varmass.h"
#include "gdm_varstencil.h"

namespace gdmk {
struct FastdiagPass;
}

namespace gdm_detail {

// records msg as the calling thread's last error (gdm_last_error) and returns code
int fail(int code, const std::string &msg);

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

inline void hip_check(hipError_t e, const char *what) {
  if (e != hipSuccess) throw HipError(std::string(what) + ": " + hipGetErrorString(e));
}

template <typename T>
T *dev_upload(const std::vector<T> &h) {
  T *d = nullptr;
  const size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
  hip_check(hipMalloc(&d, bytes), "hipMalloc");
  if (!h.empty()) hip_check(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
  return d;
}

// one tangential direction of a boundary face
struct FaceDir {
  int dim_index = -1;     // reference direction, -1 = trivial
  int n_nodes = 1;        // nodes along this direction
  int Q = 1;              // quadrature points along this direction (local cells x (p+1))
  int cell_begin = 0;     // first local cell
  int node_begin = 0, node_end = 1;  // output node range (owned)
  int64_t stride = 0;     // global index stride
  int wmax = 1;
  int qmax = 1;           // largest q-range of FACE_CHUNK consecutive owned nodes
  int *qs = nullptr, *qc = nullptr;
  double *w = nullptr;    // [n_nodes][wmax]
  double *wT = nullptr;   // [wmax][n_nodes]
  double *phi = nullptr;  // [p][p+1][p+1] cell tables (cell form of the face step 1)
  int *crange = nullptr;  // [n_nodes][2] first / last local cell of each node
  int ncell_total = 0;
};

struct Face {
  int d = 0, side = 0;
  double scale = 0.0;     // |a.n| for inflow faces, 0 otherwise
  int64_t offset = 0;     // offset into the device bc array
  int64_t n_points = 0;
  FaceDir t0, t1;
  int64_t base = 0;       // owned index of node (i0 = 0, i1 = t1.node_begin)
  double *T = nullptr;    // step-1 result of this face (faces run concurrently)
};

}  // namespace gdm_detail

// line-solve tables of one banded SPD matrix (build_line_tables)
struct LineTables {
  double *lrow = nullptr, *invd = nullptr;               // v2 row form
  double *l3 = nullptr, *u3 = nullptr, *d3 = nullptr;    // v3 split rows
  std::vector<double> cst;                               // v3 interior fixed-point row
  int row_lo = 0, row_hi = 0;
};

// Distributed exact mass inverse along the partitioned direction (truncated
// SPIKE, gdm_mass_solve_slab / gdm_mass_solve_interface): the slab's own
// diagonal block A_r of M_q, its spikes V = A_r^-1 B_r (coupling to the next
// slab's first p planes) and W = A_r^-1 C_r (previous slab's last p planes),
// and the two p x 2p rows of the interface-system inverses.
struct SpikeTables {
  bool built = false;
  double eps = 0.0;        // largest dropped far-spike entry over all slabs
  int rounds = 0;          // refinement exchanges (-1: partition refused)
  int next_round = -1;     // progress of the current solve: -1 no slab solve
                           // pending, k: rounds [0, k) done
  double *G0 = nullptr;    // device [2p][plane]: saved slab-solve edge planes (rounds > 0)
  int n_planes = 0;        // owned planes of this rank
  int has_lo = 0, has_hi = 0;
  LineTables slab;         // A_r
  double *VW = nullptr;    // device [n_planes][2p]: V row k | W row k
  double *S = nullptr;     // device [2][p][2p]: lower-interface rows (x_{r-1}^bot), upper (x_{r+1}^top)
  int k_begin = 0, k_end = 0;  // planes the correction touches
};

// Exact mass inverse with periodicity constraints (gdm_mass_solve_periodic):
// per periodic direction the line tables of A~ = blockdiag(A, 1) (kernel axis
// of the direction) and the rank-2 Woodbury correction (gdm_periodic.hip); w =
// the gather scratch [2][most lines of a periodic direction].  All of it is
// built by gdm_op_create, so the first solve may run inside a stream capture.
struct PeriodicMass {
  LineTables tab[3];           // by kernel axis
  const LineTables *axis_tab[3] = {nullptr, nullptr, nullptr};
  gdmk::PeriodicDir dir[3]{};  // by reference direction
  double *w = nullptr;
};

struct gdm_op {
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  bool concurrent = true;  // compute_rhs: face step 1 in the stencil's tail (apply_with_faces)
  gdm_mesh_desc mesh{};
  int kind = 0, p = 1, dim = 1;
  int N[3] = {1, 1, 1};        // vertices per reference direction
  int K[3] = {1, 1, 1};        // kernel-space extents (X, Y, Z)
  int kdir[3] = {-1, -1, -1};  // kernel axis -> reference direction (-1 trivial)
  int part_axis = 2;           // kernel axis of the slab partition (1 = Y, 2 = Z)
  gdm_layout layout{};
  double a[3] = {0, 0, 0};
  double nitsche = 0.0;
  // device tables
  // stencil tables (kernel axes) and the scalars of the compile-time bands
  double *corrX = nullptr, *yT1 = nullptr, *yT3 = nullptr, *zt = nullptr;
  int x_corr_left = 0, x_corr_right = 0, x_toep = 0, y_toep = 0, z_toep = 0;
  double sx = 0, cy[19] = {0};
  // v8 variants: E pre-scaled by h_z (sx, cy, corrX's B part, yT3), z table e = M_z / h_z
  double *corrX8 = nullptr, *yT3_8 = nullptr, *zt8 = nullptr;
  double *yT1d = nullptr, *yT3d = nullptr, *m_yT3d = nullptr;  // v8 y corrections
  double sx8 = 0, cy8[19] = {0}, cxs8[19] = {0};
  double dint = 0, m_dint = 0;  // interior z scales of D (operator, mass)
  double zd8[19] = {0}, m_zd8[19] = {0};  // dint * dhat[2p - k] (operator, mass)
  int xcd_map = 1;
  // the same for the mass operator of an advection/wave op (gdm_mass_apply)
  double *m_corrX = nullptr, *m_zt = nullptr;
  double *lrow[3] = {nullptr, nullptr, nullptr}, *invd[3] = {nullptr, nullptr, nullptr};
  // mass inverse v3 tables (gdm_mass.hip): [rows][p] lower / upper factor rows,
  // inverse diagonal, the interior fixed-point row and its row range
  double *l3[3] = {nullptr, nullptr, nullptr}, *u3[3] = {nullptr, nullptr, nullptr}, *d3[3] = {nullptr, nullptr, nullptr};
  double *cst3[3] = {nullptr, nullptr, nullptr};
  int row_lo3[3] = {0, 0, 0}, row_hi3[3] = {0, 0, 0};
  std::vector<double> cst3_host[3];
  double *bc_tab = nullptr;  // gdm_eval_boundary: per-face 1D factor tables
  SpikeTables spike;         // distributed mass inverse (n_ranks > 1)
  PeriodicMass pmass;        // exact mass inverse with periodicity constraints
  // gdm_error_norms: shape values per category, per-workgroup partials, result
  double *err_S = nullptr, *err_partial = nullptr;
  static constexpr int n_err_partial = 1024;
  int bc_tab_ld = 0;
  double *bc_stage_tab = nullptr;  // gdm_apply_bc_fn: BcStage factor tables (2 x 6 faces)
  double *bc_stage_vals = nullptr;  // gdm_apply_bc_fn: the stage boundary values (n_bc_points)
  int bc_stage_ld = 0;
  // periodicity constraints (system.h:427-463): scratch copy of the input for
  // distribute; CG work vectors and the Jacobi inverse diagonal
  double *pscratch = nullptr;
  double *cg_r = nullptr, *cg_p = nullptr, *cg_Ap = nullptr, *cg_z = nullptr, *cg_invdiag = nullptr;
  std::vector<gdm_detail::Face> faces;
  double *face_tmp = nullptr;
  // the stencil's tail work (face step 1, gdmk_launch_stencil8): device claim
  // counter, 0 between launches (each launch resets it with its last claim)
  unsigned long long *tail_counter = nullptr;
  double *mass_tmp = nullptr;  // ping-pong vector of the segmented mass passes (small meshes)
  int64_t mass_tmp_size = 0;
  int mass_seg_waves = -1;      // gdm_op_set_mass_seg_waves (-1: gdmk_mass3_seg_waves())
  gdm_mass_path mass_path = {};  // what the last mass_solve_passes launched (gdm_op_mass_path)
  int64_t face_tmp_size = 0;
  double *dot_partial = nullptr, *dot_out = nullptr;
  int n_dot_partial = 1024;
  int zchunk = 64;
  // host copies for bc ordering
  std::vector<double> xq;
  gdm::Slab slab{};
  std::vector<void *> allocations;
  // separable advection field (gdm_op_set_advection_field): the launch plan of
  // the volume kernel and the per-face arguments, all device memory allocated
  // when the field is set
  struct Field {
    bool active = false;
    int n_terms = 0;
    double scale[gdmk::VAR_MAX_TERMS];       // s_t (gdm_op_set_field_scale)
    gdmk::VarArgs vol{};                     // src / dst / scale filled per apply
    size_t lds = 0;
    std::vector<gdmk::VarFaceArgs> faces;    // u / bc / dst / coef filled per apply
    std::vector<int64_t> face_bc_offset;
    // per face and face term: the term and sign * f_normal(end) (coef = that * s_t)
    std::vector<std::vector<int>> face_term;
    std::vector<std::vector<double>> face_end;
    std::vector<void *> allocations;
  } field;
  // separable coefficient of the wave operator (gdm_op_set_coefficient): the
  // launch plan of gdm_vardiff.hip, kappa at the boundary points with the
  // scratch of kappa g, the domain mean of kappa and the CG vectors of
  // gdm_coef_solve, all device memory allocated when the coefficient is set
  struct Coef {
    bool active = false;
    int n_terms = 0;
    gdmk::DiffArgs args{};  // src / dst filled per apply
    size_t lds = 0;
    double *kappa_bc = nullptr, *g_scaled = nullptr;  // [n_bc_points]
    double mean = 1.0;
    double *cg[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // r, p, Ap, z, M p
    // general coefficient on the Gauss grid (gdm_op_set_coefficient_grid): the
    // launch plan of gdm_coefgrid.hip; kq and kappa_bc are the caller's arrays
    bool grid = false;
    gdmk::CgArgs grid_args{};  // src / dst filled per apply
    std::vector<gdmk::CgFace> grid_faces;
    double *face_scratch = nullptr;  // [2][largest face's Gauss points]
    std::vector<void *> allocations;
  } coef;
  // separable density of the wave operator (gdm_op_set_density): the launch
  // plan of gdm_varmass.hip, the domain mean of rho, for one term the two-sweep
  // line tables of every M_d[r_d] (by kernel axis), for sums W^-1/2 of the
  // preconditioner, and the CG vectors of gdm_density_solve / gdm_coef_solve,
  // all device memory allocated when the density is set
  struct Density {
    bool active = false;
    int n_terms = 0;
    gdmk::VarMassArgs args{};  // src / dst / add / c filled per apply
    size_t lds = 0;
    double mean = 1.0;
    LineTables tab[3];
    const LineTables *axis_tab[3] = {nullptr, nullptr, nullptr};
    double *w_isqrt = nullptr;  // [n_owned]: (diag M[rho] / diag M)^-1/2 (n_terms > 1)
    double *cg[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // r, p, Ap, z, K p
    // per term and kernel axis diag(M_d[r_td]) (gdm_density_diag)
    std::vector<std::vector<double>> band_diag;
    // general density on the Gauss grid (gdm_op_set_density_grid): the launch
    // plan of gdm_massgrid.hip; rq is the caller's array.  n_terms is 0, the
    // solve is the CG with w_isqrt
    bool grid = false;
    gdmk::MgArgs grid_args{};  // src / dst / add / c filled per apply
    double *mdiag = nullptr;   // [n_owned] diag(M): W of a grid density is formed from the current samples
    const gdmk::CgAxis *grid_axes_dev = nullptr;  // the reduction's copy of grid_args.ax
    double *grid_partial = nullptr;               // [2][1024] partial sums and bad counts of the reduction
    double volume = 1.0;
    int zc_auto = 0;  // mg_pick_zc of the mesh (gdm_op_set_density_grid_z_chunk restores it)
    std::vector<void *> allocations;
  } dens;
  bool cut_inner = false;  // the inner operator of a cut handle
  // load vector / Dirichlet data (gdm_add_load*, gdm_add_dirichlet_data; single
  // rank, non-periodic): shape values times quadrature weights per category,
  // the per-axis (sin, cos) load vectors of the rank-1 path [3][2][load_ld]
  double *load_Sw = nullptr, *load_bvec = nullptr;
  int load_ld = 0;
  // the tensor Gauss grid (single rank, non-periodic; build_grid_axes): the
  // kernel axes that the grid coefficient, the grid density and the grid
  // evaluation share, with host copies of the box offsets and point ranges and
  // the box volume; for gdm_eval_grid, gdm_add_load_grad and gdm_eval_trace the
  // derivative tables times quadrature weights per category next to load_Sw
  // and the box faces
  struct Eval {
    bool built = false;
    gdmk::CgAxis ax[3]{};
    std::vector<int32_t> first[3], qlo[3], qhi[3];
    double volume = 1.0;
    double *Dw = nullptr;
    std::vector<gdmk::EvFace> faces;
  } ev;
  // fast diagonalisation (gdm_system_solve_setup): per kernel axis the tables
  // S and S^T (row-major N x N) and lambda, the eigenvalue extremes for the
  // host check of a solve, two scratch vectors
  struct FastDiag {
    bool built = false;
    double *S[3] = {nullptr, nullptr, nullptr}, *St[3] = {nullptr, nullptr, nullptr};
    double *lam[3] = {nullptr, nullptr, nullptr};
    double lam_min[3] = {0, 0, 0}, lam_max[3] = {0, 0, 0};
    double *tmp[2] = {nullptr, nullptr};
  } fd;
  // linear elasticity (GDM_OP_ELASTICITY): the Dirichlet-reduced 1D tables of
  // the kernel (built by gdm_op_create), the diagonal, and the block
  // fast-diagonalisation preconditioner (gdm_elasticity_precond_setup): per
  // kernel axis S, S^T and per component the eigenvalues pre-scaled by w_cd
  struct Elasticity {
    double mu = 0.0, lambda = 0.0;
    gdmk::ElasArgs args{};       // src / dst filled per apply
    double *invdiag = nullptr;   // Jacobi: 1 / diag, built on first use
    double *free_mask = nullptr; // 1 on free DoFs, 0 on constrained ones (first solve)
    bool built = false;
    double *S[3] = {nullptr, nullptr, nullptr}, *St[3] = {nullptr, nullptr, nullptr};
    double *lam[3][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    double *tmp[2] = {nullptr, nullptr};
    double *cg[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // r, p, Ap, z, b (masked rhs)
  } el;
};

namespace gdm_detail {

template <typename T>
T *keep(gdm_op *op, T *ptr) {
  op->allocations.push_back((void *)ptr);
  return ptr;
}

// upload h, the allocation recorded in `made` as it is made
template <typename T>
T *up(std::vector<void *> &made, const std::vector<T> &h) {
  T *d = dev_upload(h);
  made.push_back((void *)d);
  return d;
}

// the kernel's table of a band matrix along kernel axis ax: x the plain rows;
// y zero rows up to a whole tile (y_rows); z p zero rows in front and behind
inline std::vector<double> padded_table(const gdm::Band &B, int ax, size_t y_rows) {
  const int p = B.hb, W = 2 * p + 1;
  const size_t rows = ax == 0 ? B.n : (ax == 1 ? y_rows : B.n + 2 * p);
  std::vector<double> t(rows * W, 0.0);
  std::copy(B.a.begin(), B.a.end(), t.begin() + (ax == 2 ? (size_t)p * W : 0));
  return t;
}

// the refusals of the gdm_*_tile queries (dim in [dim_min, 3]); 0 = ok
inline int check_tile_query(int fe_degree, int dim = 1, int dim_min = 1) {
  if (fe_degree < 1 || fe_degree > 9 || fe_degree % 2 == 0) return fail(GDM_ERR_UNSUPPORTED, "fe_degree must be odd in [1, 9]");
  if (dim < dim_min || dim > 3) return fail(GDM_ERR_ARG, dim_min == 2 ? "dim must be 2 or 3" : "dim must be 1, 2 or 3");
  return GDM_OK;
}

// ... and their answer: the three constants into whichever pointers are given
inline int tile_answer(int tx, int ty, int zc, int *tile_x, int *tile_y, int *z_chunk) {
  if (tile_x) *tile_x = tx;
  if (tile_y) *tile_y = ty;
  if (z_chunk) *z_chunk = zc;
  return GDM_OK;
}

// The body of a gdm_op_set_* call: build(fresh) fills a fresh object (not
// called when nothing is to be set: the fresh object then clears the operator's)
// and returns false to reject the input, which is then `rejected`; the fresh
// object's allocations are freed when build throws or rejects and the operator
// stays as it was, otherwise install(op, fresh) makes it the operator's.
template <typename T, typename Build>
int build_and_install(gdm_op *op, bool set, Build &&build, void (*install)(gdm_op *, T &), const char *rejected) {
  T fresh;
  if (set) {
    bool ok = true;
    try {
      ok = build(fresh);
    } catch (...) {
      for (void *ptr : fresh.allocations) (void)hipFree(ptr);
      throw;
    }
    if (!ok) {
      for (void *ptr : fresh.allocations) (void)hipFree(ptr);
      return fail(GDM_ERR_ARG, rejected);
    }
  }
  install(op, fresh);
  return GDM_OK;
}

// gdm::pcg (gdm_pcg.h) on device vectors of length n: the vector operations are
// the library's kernels on the operator's stream, dot is gdm_vec_dot (one host
// synchronisation each)
template <typename Apply, typename Precondition>
gdm::PcgResult device_pcg(gdm_op *op, int64_t n, Apply &&apply, Precondition &&precondition, double *r, double *p,
                          double *Ap, double *z, const double *rhs, double *x, double rel_tol, double abs_tol,
                          int max_it) {
  auto dot = [&](const double *u, const double *v) {
    double s = 0.0;
    if (gdm_vec_dot(op, n, u, v, &s) != GDM_OK) throw std::runtime_error("dot");
    return s;
  };
  auto axpby = [&](double a, const double *u, double b, double *v) {
    hip_check(gdmk_launch_axpby(n, a, u, b, v, op->stream), "axpby");
  };
  auto copy = [&](double *dst, const double *src) {
    hip_check(hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyDeviceToDevice, op->stream), "copy");
  };
  return gdm::pcg(apply, precondition, dot, axpby, copy, r, p, Ap, z, rhs, x, rel_tol, abs_tol, max_it);
}

// the end of a CG entry point `what`: the count and the residual to the caller,
// the status to the return code (breakdown: the entry point's own wording)
inline int finish_pcg(const gdm::PcgResult &r, const char *what, int *its_host, double *res_host,
                      const char *breakdown = "(p^T A p <= 0): the operator is not positive definite on this input "
                                              "(a rhs or x that is not finite)") {
  if (its_host) *its_host = r.its;
  if (res_host) *res_host = r.res;
  const std::string w(what);
  switch (r.status) {
    case gdm::PcgStatus::converged: return GDM_OK;
    case gdm::PcgStatus::max_it: return fail(GDM_ERR_STATE, w + ": max_it reached (SolverControl::NoConvergence)");
    case gdm::PcgStatus::non_finite: return fail(GDM_ERR_STATE, w + ": the residual is not finite");
    default: return fail(GDM_ERR_STATE, w + ": breakdown " + breakdown);
  }
}

// ---- gdm_capi.cpp ----
std::vector<double> mass_diagonal_owned(const gdm_op *op);
gdm::Band identity_band(int p);
double nitsche_over_hmin(const gdm_mesh_desc *mesh, double nitsche);
gdm::Band mesh_mass_1d(const gdm_mesh_desc *mesh, int axis);
const char *host_mesh_error(const gdm_mesh_desc *mesh, int axis);
int check_field_mesh(const gdm_mesh_desc *mesh, int axis);
hipError_t launch_stencil(gdm_op *op, bool mass, const double *src, double *dst, int zb = -1, int ze = -1,
                          const gdmk::FaceArgs *tail = nullptr, int n_tail = 0, bool *tail_done = nullptr,
                          int zb2 = 0, int ze2 = 0);
void any_stencil(gdm_op *op, bool mass, const double *src, double *dst);
int check_load_op(gdm_op *op, const char *what);
gdmk::LoadGeom load_geom(const gdm_op *op);
bool mass_solve_passes(gdm_op *op, const double *rhs_owned, double *x_owned, const LineTables *part,
                       const gdmk::RkOut *rk = nullptr, const LineTables *const *axis_tab = nullptr);

// ---- gdm_capi_coef.cpp ----
void coef_apply(gdm_op *op, const double *src, double *dst);
void build_grid_axes(gdm_op *op);
double grid_axes(const gdm_op *op, const int tile[2], const int nq_max[2], const int span_max[2], const char *what,
                 gdmk::CgAxis ax[3]);
gdmk::FastdiagPass fastdiag_pass(const gdm_op *op, int ax, const double *Tt);  // gdm_fastdiag.h

// ---- gdm_capi_evalgrid.cpp ----
void build_evalgrid(gdm_op *op);

// ---- gdm_capi_elasticity.cpp ----
void build_elasticity(gdm_op *op);
void elasticity_apply(gdm_op *op, const double *src, double *dst);

}  // namespace gdm_detail

#define GDM_GUARD_BEGIN try {
#define GDM_GUARD_END                                             \
  }                                                               \
  catch (const HipError &e) { return fail(GDM_ERR_HIP, e.what()); } \
  catch (const std::bad_alloc &) { return fail(GDM_ERR_NOMEM, "out of host memory"); } \
  catch (const std::invalid_argument &e) { return fail(GDM_ERR_ARG, e.what()); } \
  catch (const std::exception &e) { return fail(GDM_ERR_STATE, e.what()); }

#endif
