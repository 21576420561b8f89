// gdm_massgrid.h -- argument block and launchers of gdm_massgrid.hip: the mass
// matrix weighted by a general density rho sampled on the tensor Gauss grid
// (gdm_op_set_density_grid),
//   M[rho] u = (B_z (x) B_y (x) B_x)^T diag(w rho) (B_z (x) B_y (x) B_x) u  [+ c * add],
// B_d the (Q_d x N_d) matrices of basis values at the Gauss points of direction
// d (p + 1 non-zeros per row), and its diagonal
//   diag_i = sum_q w_q rho_q prod_d B_d[q_d, i_d]^2.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_coefgrid.h"  // CgAxis: the tables of one kernel axis (the derivatives are not read)

namespace gdmk {

// Kernel geometry per degree: a workgroup of MG_THREADS threads owns a TX x TY
// tile of nodes and MgArgs::zc <= ZC node planes (the bits do not depend on
// zc).  One node plane and one sweep plane live in LDS, so the tile can stay at
// 16 x 16 up to p = 5 and at 8 x 8 above with at least two workgroups on a CU
// (mg_lds).
constexpr int MG_THREADS = 256;
// cells of rho that a column's y march keeps in flight
constexpr int MG_AHEAD = 3;
constexpr int mg_tx(int p) { return p <= 5 ? 16 : 8; }
constexpr int mg_ty(int p) { return p <= 5 ? 16 : 8; }
constexpr int mg_zc(int p) { return p <= 5 ? 32 : 16; }
// the footprint of T consecutive nodes: at most T + p + p/2 cells (gdm_load.hip),
// whose DoF boxes span at most p nodes more
constexpr int mg_cells(int p, int t) { return t + p + p / 2; }
constexpr int mg_sx(int p) { return mg_cells(p, mg_tx(p)) + p; }
constexpr int mg_sy(int p) { return mg_cells(p, mg_ty(p)) + p; }
constexpr int mg_nqx(int p) { return mg_cells(p, mg_tx(p)) * (p + 1); }
constexpr int mg_nqy(int p) { return mg_cells(p, mg_ty(p)) * (p + 1); }
// the x table of the footprint is staged in LDS where two workgroups still fit (p = 9 reads it from global memory)
constexpr bool mg_xt(int p) { return p <= 7; }
// dynamic LDS: the node plane [SY][SX], the sweep plane [SY][NQX], the y table of the footprint with its
// weights, the x table, the box offsets of both footprints
constexpr size_t mg_lds(int p) {
  return sizeof(double) * ((size_t)mg_sy(p) * mg_sx(p) + (size_t)mg_sy(p) * mg_nqx(p) + (size_t)(p + 2) * mg_nqy(p) +
                           (mg_xt(p) ? (size_t)(p + 1) * mg_nqx(p) : 0)) +
         sizeof(int) * (size_t)(mg_nqx(p) + mg_nqy(p));
}
static_assert(mg_nqx(1) <= MG_THREADS && mg_nqx(3) <= MG_THREADS && mg_nqx(5) <= MG_THREADS &&
                  mg_nqx(7) <= MG_THREADS && mg_nqx(9) <= MG_THREADS,
              "one thread per quadrature column of the tile");
static_assert(mg_lds(1) <= 80 * 1024 && mg_lds(3) <= 80 * 1024 && mg_lds(5) <= 80 * 1024 && mg_lds(7) <= 80 * 1024 &&
                  mg_lds(9) <= 80 * 1024,
              "two workgroups share the LDS of a CU");

struct MgArgs {
  const double *src;
  double *dst;
  const double *add;  // NULL: dst = M[rho] src; else dst = M[rho] src + c * add
  double c;
  const double *rq;  // [Qz][Qy][Qx]
  int zc;            // node planes per workgroup, in [1, mg_zc(p)]
  CgAxis ax[3];
};

// The z chunk of a mesh: mg_zc(p), halved (twice at most) while the launch has
// fewer than two workgroups per CU; a chunk's z halo of p + p/2 cell layers is
// recomputed, so a large mesh keeps the whole chunk.
inline int mg_pick_zc(int p, int Nx, int Ny, int Nz, int n_cu) {
  const int64_t tiles = (int64_t)((Nx + mg_tx(p) - 1) / mg_tx(p)) * ((Ny + mg_ty(p) - 1) / mg_ty(p));
  int zc = mg_zc(p);
  while (zc > mg_zc(p) / 4 && tiles * ((Nz + zc - 1) / zc) < 2 * (int64_t)n_cu) zc /= 2;
  return zc;
}

}  // namespace gdmk

extern "C" {
// degree-independent part (gdm_massgrid.o, the unit of -DGDM_PART=0):
//   out[i] = (diag[i] / mdiag[i])^-1/2, 1 where the ratio is not positive
hipError_t gdmk_mg_wisqrt(int64_t n, const double *diag, const double *mdiag, double *out, hipStream_t st);
// per degree (gdm_parts.h): prepare raises the kernel's dynamic LDS limit on the current device; apply is the one volume
// launch; diag writes diag(M[rho]) to a.dst (src, add and c are not read)
GDM_PARTS_DECLARE(gdmk_mg_prepare_p, void)
GDM_PARTS_DECLARE(gdmk_mg_apply_p, const gdmk::MgArgs &a, hipStream_t st)
GDM_PARTS_DECLARE(gdmk_mg_diag_p, const gdmk::MgArgs &a, hipStream_t st)
}

namespace gdmk {

inline hipError_t mg_prepare(int p) { GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_mg_prepare_p) }
inline hipError_t launch_mg(int p, const MgArgs &a, hipStream_t st) {
  GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_mg_apply_p, a, st)
}
inline hipError_t launch_mg_diag(int p, const MgArgs &a, hipStream_t st) {
  GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_mg_diag_p, a, st)
}

}  // namespace gdmk
