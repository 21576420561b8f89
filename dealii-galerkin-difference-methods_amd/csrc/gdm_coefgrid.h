// gdm_coefgrid.h -- argument blocks and launchers of gdm_coefgrid.hip: the wave /
// heat / Poisson operator with a general coefficient kappa sampled on the tensor
// Gauss grid (gdm_op_set_coefficient_grid),
//   K[kappa] u = - sum_e G_e^T diag(w kappa) G_e u  -  box-face terms,
//   G_e = (x)_d (D_d if d == e else B_d),
// B_d / D_d the (Q_d x N_d) matrices of basis values / physical derivatives at
// the Gauss points of direction d (p + 1 non-zeros per row).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_parts.h"

namespace gdmk {

// Kernel geometry per degree: a workgroup owns a TX x TY tile of nodes and ZC
// node planes.  The tile shrinks with the degree: the x sweep of the tile's
// node rows (halo included) on its quadrature footprint lives in LDS.
constexpr int cg_tx(int p) { return p <= 5 ? 16 : (p == 7 ? 8 : 4); }
constexpr int cg_ty(int p) { return p <= 5 ? 16 : (p == 7 ? 8 : 4); }
constexpr int cg_zc(int p) { return p <= 5 ? 32 : 16; }
// the footprint of T consecutive nodes: at most T + p + p/2 cells (gdm_load.hip),
// whose DoF boxes span at most p nodes more
constexpr int cg_cells(int p, int t) { return t + p + p / 2; }
constexpr int cg_sx(int p) { return cg_cells(p, cg_tx(p)) + p; }
constexpr int cg_sy(int p) { return cg_cells(p, cg_ty(p)) + p; }
constexpr int cg_nqx(int p) { return cg_cells(p, cg_tx(p)) * (p + 1); }
constexpr int cg_nqy(int p) { return cg_cells(p, cg_ty(p)) * (p + 1); }
// columns of one component in the y sweep, whole waves
constexpr int cg_cw(int p) { return (cg_nqx(p) + 63) / 64 * 64; }
constexpr int cg_threads(int p) { return 3 * cg_cw(p) > 256 ? 3 * cg_cw(p) : 256; }
// the x tables of the footprint are staged in LDS too where it has the room (p = 9 reads them from global memory)
constexpr bool cg_xt(int p) { return p <= 7; }
// dynamic LDS: two node planes [SY][SX], three sweep planes [SY][NQX], the y tables of the footprint
// (values, derivatives, weights), the x tables (values, derivatives) and the box offsets of both footprints
constexpr size_t cg_lds(int p) {
  return sizeof(double) * ((size_t)2 * cg_sy(p) * cg_sx(p) + (size_t)3 * cg_sy(p) * cg_nqx(p) +
                           (size_t)(2 * (p + 1) + 1) * cg_nqy(p) + (cg_xt(p) ? (size_t)2 * (p + 1) * cg_nqx(p) : 0)) +
         sizeof(int) * (size_t)(cg_nqx(p) + cg_nqy(p));
}
static_assert(cg_lds(1) <= 160 * 1024 && cg_lds(3) <= 160 * 1024 && cg_lds(5) <= 160 * 1024 &&
                  cg_lds(7) <= 160 * 1024 && cg_lds(9) <= 160 * 1024,
              "the launch plan exceeds the LDS of a CU");

// One kernel axis.  A trivial axis has N = Q = 1, first = {0}, val = {1, 0, ...},
// der = {0, ...}, w = {1}: the node guards make the same code serve it.
struct CgAxis {
  int N, Q;                      // nodes, Gauss points
  const int32_t *first;          // [Q] first node of the cell's DoF box
  const double *val, *der;       // [Q][p+1] basis values, physical derivatives
  const double *w;               // [Q] Gauss weight times h
  const int32_t *qlo, *qhi;      // [N] the Gauss points whose box holds the node: [qlo, qhi)
};

struct CgArgs {
  const double *src;
  double *dst;
  const double *kq;  // [Qz][Qy][Qx]
  CgAxis ax[3];
};

// One box face of the Nitsche part.  Tangential directions t0 (fast) and t1;
// the p + 1 node planes behind the wall start at `base`, stride_d apart.
struct CgFace {
  int n0, n1, Q0, Q1, nk;
  const int32_t *first0, *first1;  // evaluation tables of the tangential directions
  const double *val0, *val1;
  const int32_t *qs0, *qc0, *qs1, *qc1;  // back projection (gdm::FaceTable): weights phi w_q h
  const double *w0, *w1;
  int wmax0, wmax1;
  int64_t stride0, stride1, stride_d, base, goff;
  double gamma;          // nitsche / h_min
  double tr[10], dk[10];  // wall trace and outward normal derivative of the p + 1 basis functions
};

}  // namespace gdmk

extern "C" {
// degree-independent part (gdm_coefgrid.o, the unit of -DGDM_PART=0)
//   reduce: partial[b] = sum over block b's samples of w kappa, bad[b] = number
//           of samples that are not finite or not positive (ax NULL: w = 1)
hipError_t gdmk_cg_reduce(const double *k, int64_t n, const gdmk::CgAxis *ax, double *partial, double *bad, int blocks,
                          hipStream_t st);
hipError_t gdmk_cg_face(const gdmk::CgFace &F, const double *u, const double *kbc, double *scratch, double *dst,
                        hipStream_t st);
// per degree (gdm_parts.h): prepare raises the kernel's dynamic LDS limit on the current device
GDM_PARTS_DECLARE(gdmk_cg_prepare_p, void)
GDM_PARTS_DECLARE(gdmk_cg_apply_p, const gdmk::CgArgs &a, hipStream_t st)
}

namespace gdmk {

inline hipError_t cg_prepare(int p) { GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_cg_prepare_p) }
inline hipError_t launch_cg(int p, const CgArgs &a, hipStream_t st) {
  GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_cg_apply_p, a, st)
}

}  // namespace gdmk
