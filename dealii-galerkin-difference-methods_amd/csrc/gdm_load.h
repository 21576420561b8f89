// gdm_load.h -- argument blocks and launchers of gdm_load.hip: the data terms
// of the uncut wave / heat right-hand side, the load vector (v, f) over
// QGauss(p+1) and the Nitsche Dirichlet data on the box faces.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gdm_rk.h"  // BcFn: the built-in analytic functions

namespace gdmk {

// geometry of the general load kernel: a workgroup owns LOAD_TX x LOAD_TY
// nodes of the (x, y) kernel plane and LOAD_ZC node planes along z
constexpr int LOAD_TX = 16, LOAD_TY = 16, LOAD_ZC = 32;
// quadrature rows staged per pass of the x contraction
__host__ __device__ constexpr int load_rows(int p) { return p >= 9 ? 8 : 16; }

// The mesh in kernel axes (3D: x, y, z; 2D: x, y, -; 1D: -, -, x).  A trivial
// axis has on = 0, K = nc = Q = 1, rdir = -1.
struct LoadGeom {
  int p;
  int on[3];
  int K[3];     // nodes
  int nc[3];    // cells
  int Q[3];     // quadrature points, nc * (p + 1)
  int rdir[3];  // reference direction of the axis
  double lo[3], h[3];
  double jxw;   // prod of the h of the non-trivial axes
  double xq[10];
};

// the index helpers of the gather kernels (load_kernel; ev_flux_kernel of gdm_evalgrid.hip)
#ifdef __HIPCC__
// cell category / DoF box offset / cells whose box holds node i (odd p, n >= p)
__device__ __forceinline__ int ld_cat(int c, int p, int n) {
  const int half = p / 2;
  if (c < half) return c;
  if (c < n - half) return half;
  return p + c - n;
}
__device__ __forceinline__ int ld_off(int c, int p, int n) {
  const int half = p / 2;
  if (c < half) return 0;
  return min(n, c + half + 1) - p;
}
__device__ __forceinline__ int ld_first(int i, int p, int n) { return i <= p ? 0 : i - p + p / 2; }
__device__ __forceinline__ int ld_last(int i, int p, int n) { return i >= n - p ? n - 1 : i + p / 2; }
#endif

// One box face of the Dirichlet data term: the tangential projection tables
// (FaceTable of gdm_setup.h: w includes the face JxW factor of its direction)
// and the p + 1 node planes behind the face with their weights
// c_k = gamma / h_min phi_k(face) - n phi_k'(face) / h_d.
struct DirFace {
  int n0, n1;                // nodes along t0, t1
  int Q0, Q1;                // points along t0 (row length of g), t1
  int wmax0, wmax1;
  const int *qs0, *qc0, *qs1, *qc1;
  const double *w0, *w1;
  int64_t stride0, stride1;  // owned-index strides of t0, t1
  int64_t goff;              // first point of the face in the bc array
  int64_t base;              // owned index of node (0, 0) of the first plane
  int64_t stride_d;          // owned-index stride of the normal direction
  int nk;                    // p + 1
  double ck[10];
};

}  // namespace gdmk

extern "C" {
// dst += scale * (v, f): Sw [max(1, p)][p+1][p+1] = phi^cat_i(xq_q) wq_q;
// mode 0: f = fq on the tensor Gauss grid (x fastest), mode 1: GDM_FN_CONE
hipError_t gdmk_launch_load(const gdmk::LoadGeom &g, const gdmk::BcFn &f, int mode, const double *Sw,
                            const double *fq, double scale, double *dst, hipStream_t st);
// rank-1 load of GDM_FN_CONSTANT / GDM_FN_SINE_PRODUCT at time t (derivative
// 1: d/dt): bvec = scratch [3][2][ld] of the per-axis (sin, cos) load vectors
hipError_t gdmk_launch_load_rank1(const gdmk::LoadGeom &g, const gdmk::BcFn &f, double t, int derivative,
                                  double scale, const double *Sw, double *bvec, int ld, double *dst,
                                  hipStream_t st);
// tmp: scratch of Q1 * n0 doubles (g projected along t0)
hipError_t gdmk_launch_dirichlet_face(const gdmk::DirFace &F, const double *g, double *tmp, double *dst,
                                      hipStream_t st);
}
