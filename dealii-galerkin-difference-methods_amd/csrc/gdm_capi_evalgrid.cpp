// gdm_capi_evalgrid.cpp -- C ABI of the grid evaluation (declared in
// include/gdm_hip.h): u and grad u on the tensor Gauss grid, the flux load and
// the wall trace (gdm_evalgrid.hip).
#include <cstdint>

#include "gdm_capi_internal.h"

using namespace gdm_detail;

// Tables of the grid evaluation, built by gdm_op_create next to build_load:
// no entry point allocates or synchronises.
void gdm_detail::build_evalgrid(gdm_op *op) {
  const int p = op->p, n1 = p + 1, ncat = std::max(1, p);
  gdm_op::Eval &ev = op->ev;
  build_grid_axes(op);
  std::vector<double> xq, wq;
  gdm::gauss_unit(n1, xq, wq);
  std::vector<double> Dw((size_t)ncat * n1 * n1);
  for (int c = 0; c < ncat; ++c)
    for (int i = 0; i < n1; ++i)
      for (int q = 0; q < n1; ++q) Dw[((size_t)c * n1 + i) * n1 + q] = gdm::shape_1d(p, c, i, xq[q], 1) * wq[q];
  ev.Dw = keep(op, dev_upload(Dw));
  hip_check(gdmk::ev_prepare(p), "grid evaluation: LDS limit");

  // the box faces of the trace, in the order of the boundary points
  const int64_t stride[3] = {1, op->N[0], (int64_t)op->N[0] * op->N[1]};
  auto axis_of = [&](int e) {  // kernel axis of reference direction e (-1: any trivial axis)
    for (int k = 0; k < 3; ++k)
      if (op->kdir[k] == e) return k;
    throw std::runtime_error("grid evaluation: direction without a kernel axis");
  };
  for (const Face &F : op->faces) {
    gdmk::EvFace f{};
    const gdmk::CgAxis &A0 = ev.ax[axis_of(F.t0.dim_index)], &A1 = ev.ax[axis_of(F.t1.dim_index)];
    f.n0 = F.t0.n_nodes;
    f.n1 = F.t1.n_nodes;
    f.Q0 = F.t0.Q;
    f.Q1 = F.t1.Q;
    f.nk = n1;
    f.first0 = A0.first;
    f.val0 = A0.val;
    f.first1 = A1.first;
    f.val1 = A1.val;
    f.stride0 = F.t0.stride;
    f.stride1 = F.t1.stride;
    f.stride_d = stride[F.d];
    f.base = (F.side ? (int64_t)(op->N[F.d] - 1 - p) : 0) * stride[F.d];
    f.goff = F.offset;
    const unsigned ncd = (unsigned)op->mesh.n_subdivisions[F.d];
    const double hd = (op->mesh.hi[F.d] - op->mesh.lo[F.d]) / ncd;
    const int cat = F.side ? (int)gdm::category(ncd - 1, (unsigned)p, ncd) : 0;
    const double xs = F.side ? 1.0 : 0.0, nrm = F.side ? 1.0 : -1.0;
    for (int k = 0; k < n1; ++k) {
      f.tr[k] = gdm::shape_1d(p, cat, k, xs, 0);
      f.dk[k] = nrm * gdm::shape_1d(p, cat, k, xs, 1) / hd;
    }
    if (f.Q0 != A0.Q || f.Q1 != A1.Q || f.n0 != A0.N || f.n1 != A1.N)
      throw std::runtime_error("grid evaluation: face and volume tables disagree");
    ev.faces.push_back(f);
  }
  ev.built = true;
}

namespace {

int check_eval_op(gdm_op *op, const char *what) {
  if (int rc = check_load_op(op, what)) return rc;
  if (!op->ev.built) return fail(GDM_ERR_STATE, std::string(what) + ": evaluation tables missing");
  return GDM_OK;
}

int64_t grid_points(const gdm_op *op) {
  return (int64_t)op->ev.ax[0].Q * op->ev.ax[1].Q * op->ev.ax[2].Q;
}

bool overlaps(const double *a, int64_t na, const double *b, int64_t nb) {
  return a && b && a < b + nb && b < a + na;
}

}  // namespace

extern "C" {

int gdm_eval_grid(gdm_op *op, const double *u_local, double *uq, double *gq) {
  if (int rc = check_eval_op(op, "gdm_eval_grid")) return rc;
  if (!u_local) return fail(GDM_ERR_ARG, "gdm_eval_grid: u_local is NULL");
  if (!uq && !gq) return fail(GDM_ERR_ARG, "gdm_eval_grid: uq and gq are both NULL");
  const int64_t Q = grid_points(op);
  if (overlaps(u_local, op->layout.n_local, uq, Q) || overlaps(u_local, op->layout.n_local, gq, op->dim * Q))
    return fail(GDM_ERR_ARG, "gdm_eval_grid: an output overlaps u_local");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  gdmk::EvArgs a{};
  a.u = u_local;
  a.uq = uq;
  uintptr_t bits = reinterpret_cast<uintptr_t>(uq);
  for (int k = 0; k < 3; ++k) {
    a.ax[k] = op->ev.ax[k];
    a.g[k] = gq && op->kdir[k] >= 0 ? gq + (int64_t)op->kdir[k] * Q : nullptr;
    bits |= reinterpret_cast<uintptr_t>(a.g[k]);
  }
  a.vec = (bits & 15) == 0 && a.ax[0].Q % 2 == 0;
  hip_check(gdmk::launch_ev(op->p, a, op->stream), "grid evaluation launch");
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_add_load_grad(gdm_op *op, const double *Fq, double scale, double *dst_owned) {
  if (int rc = check_eval_op(op, "gdm_add_load_grad")) return rc;
  if (!Fq || (op->layout.n_owned > 0 && !dst_owned)) return fail(GDM_ERR_ARG, "gdm_add_load_grad: NULL vector");
  if (scale == 0.0) return GDM_OK;
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  const gdmk::LoadGeom g = load_geom(op);
  hip_check(gdmk::launch_ev_flux(op->p, g, op->load_Sw, op->ev.Dw, Fq, grid_points(op), scale, dst_owned, op->stream),
            "flux load launch");
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_eval_trace(gdm_op *op, const double *u_local, double *u_bc, double *dn_bc) {
  if (int rc = check_eval_op(op, "gdm_eval_trace")) return rc;
  if (op->layout.n_bc_points == 0) return GDM_OK;
  if (!u_local) return fail(GDM_ERR_ARG, "gdm_eval_trace: u_local is NULL");
  if (!u_bc && !dn_bc) return fail(GDM_ERR_ARG, "gdm_eval_trace: u_bc and dn_bc are both NULL");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  for (const gdmk::EvFace &F : op->ev.faces)
    hip_check(gdmk_ev_trace(F, u_local, u_bc, dn_bc, op->stream), "trace launch");
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_eval_grid_tile(int fe_degree, int dim, int *cx, int *cy, int *cz) {
  if (int rc = check_tile_query(fe_degree, dim)) return rc;
  // kernel axes: 3D (x, y, z), 2D (x, y, -), 1D (-, -, x): a work item is a run of cells along kernel axis x
  return tile_answer(dim == 1 ? 1 : gdmk::ev_cx(fe_degree), 1, 1, cx, cy, cz);
}

}  // extern "C"
