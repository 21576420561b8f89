// gdm_evalgrid.h -- argument blocks and launchers of gdm_evalgrid.hip: a GDM
// field on the tensor Gauss grid and back,
//   u_q = (B_z (x) B_y (x) B_x) u,  (grad u)_e = G_e u     (gdm_eval_grid)
//   b  += scale sum_e G_e^T diag(w) F_e                     (gdm_add_load_grad)
// and the wall trace / outward normal derivative at the boundary points
// (gdm_eval_trace).  G_e = (x)_d (D_d if d == e else B_d), B_d / D_d the
// (Q_d x N_d) matrices of basis values / physical derivatives at the Gauss
// points of direction d (gdm_coefgrid.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gdm_coefgrid.h"  // CgAxis: the tables of one kernel axis
#include "gdm_load.h"      // LoadGeom and the node tile of the load kernel
#include "gdm_parts.h"

namespace gdmk {

// Evaluation: a work item is a run of ev_cx(p) cells along kernel axis x at one
// (cell_y, cell_z); a workgroup keeps its x run and strides over the (y, z) cells.
constexpr int EV_THREADS = 256;
constexpr int ev_cx(int p) { return p == 1 ? 128 : (p <= 5 ? 32 : 16); }
// dynamic LDS: the node rows of the run's DoF boxes [p+1][p+1][W], W = cx + p; the z contraction (value,
// derivative) [2][p+1][W]; the y contraction [3][p+1][W]; the x tables of the run [2][cx (p+1)][p+1] and its
// box offsets
constexpr size_t ev_lds(int p) {
  return sizeof(double) * ((size_t)((p + 1) * (p + 1) + 5 * (p + 1)) * (ev_cx(p) + p) +
                           (size_t)2 * ev_cx(p) * (p + 1) * (p + 1)) +
         sizeof(int) * (size_t)ev_cx(p) * (p + 1);
}
static_assert(ev_lds(1) <= 64 * 1024 && ev_lds(3) <= 64 * 1024 && ev_lds(5) <= 64 * 1024 && ev_lds(7) <= 64 * 1024 &&
                  ev_lds(9) <= 64 * 1024,
              "the evaluation runs within the default dynamic LDS limit");

struct EvArgs {
  const double *u;
  double *uq;    // [Qz][Qy][Qx] or NULL
  double *g[3];  // the derivative along kernel axis k, or NULL (a trivial axis; values only)
  int vec;       // every output is 16-byte aligned and Q_x is even: two points per store
  CgAxis ax[3];
};

// Flux load: load_kernel's geometry (gdm_load.h) with the derivative tables next to the value tables.
// dynamic LDS: Sw | Dw [max(1, p)][p+1][p+1] each, F[R][QF], T[QF][LOAD_TX]
constexpr int ev_flux_qf(int p) { return (LOAD_TX + p + p / 2) * (p + 1); }
constexpr size_t ev_flux_lds(int p) {
  return sizeof(double) * ((size_t)2 * (p > 1 ? p : 1) * (p + 1) * (p + 1) + (size_t)load_rows(p) * ev_flux_qf(p) +
                           (size_t)ev_flux_qf(p) * LOAD_TX);
}
static_assert(ev_flux_lds(9) <= 160 * 1024, "the flux load exceeds the LDS of a CU");

// One box face of the trace: gdm_coefgrid.h's CgFace without kappa and the back projection
struct EvFace {
  int n0, n1, Q0, Q1, nk;
  const int32_t *first0, *first1;
  const double *val0, *val1;
  int64_t stride0, stride1, stride_d, base, goff;
  double tr[10], dk[10];  // wall trace and outward normal derivative of the p + 1 basis functions
};

}  // namespace gdmk

extern "C" {
// degree-independent part (gdm_evalgrid.o, the unit of -DGDM_PART=0)
hipError_t gdmk_ev_trace(const gdmk::EvFace &F, const double *u, double *u_bc, double *dn_bc, hipStream_t st);
// per degree (gdm_parts.h): prepare raises the flux kernel's dynamic LDS limit on the current device
GDM_PARTS_DECLARE(gdmk_ev_prepare_p, void)
GDM_PARTS_DECLARE(gdmk_ev_eval_p, const gdmk::EvArgs &a, hipStream_t st)
// Sw / Dw: phi_i(xq_q) wq_q / phi_i'(xq_q) wq_q per category; Fq component e at Fq + e * comp_stride
GDM_PARTS_DECLARE(gdmk_ev_flux_p, const gdmk::LoadGeom &g, const double *Sw, const double *Dw, const double *Fq,
                  int64_t comp_stride, double scale, double *dst, hipStream_t st)
}

namespace gdmk {

inline hipError_t ev_prepare(int p) { GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_ev_prepare_p) }
inline hipError_t launch_ev(int p, const EvArgs &a, hipStream_t st) {
  GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_ev_eval_p, a, st)
}
inline hipError_t launch_ev_flux(int p, const LoadGeom &g, const double *Sw, const double *Dw, const double *Fq,
                                 int64_t comp_stride, double scale, double *dst, hipStream_t st) {
  GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_ev_flux_p, g, Sw, Dw, Fq, comp_stride, scale, dst, st)
}

}  // namespace gdmk
