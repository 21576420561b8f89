// gdm_elasticity.h -- argument block and launchers of gdm_elasticity.hip: the
// vector-valued operator of linear elasticity with zero boundary constraints,
//   y = (P A P + I - P) u,  a(u, v) = 2 mu (eps(u), eps(v)) + lambda (div u, div v),
// on component-major vectors u = [u_0 | u_1 | (u_2)].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_parts.h"

namespace gdmk {

// Kernel geometry: one workgroup of ELAS_TX * ELAS_TY threads owns an (x, y)
// tile and ELAS_ZC output planes of every component (the same for every degree).
constexpr int ELAS_TX = 32, ELAS_TY = 8, ELAS_ZC = 16;

// 1D factors of the Kronecker terms, the order of the tables below
enum ElasFactor { ELAS_M = 0, ELAS_C = 1, ELAS_CT = 2, ELAS_L = 3 };

// Tables are row-major [4][rows][2p+1] in the order M, C, C^T, L, entry
// [f][i][k] = A_f(i, i - p + k), zero outside the matrix, with row and column 0
// and rows - 1 zeroed (the constraints).  2D: ztab is not read.
struct ElasArgs {
  const double *__restrict__ src;
  double *__restrict__ dst;
  int64_t comp_stride;  // entries of one component block
  int Nx, Ny, Nz;       // kernel-space extents (2D: Nz = 1)
  const double *xtab, *ytab, *ztab;
  double mu, lambda;
  double w[3][3];       // w[c][d]: weight of L_d in the diagonal block c
};

}  // namespace gdmk

// gdm_elasticity.hip compiles as one unit per degree next to the unit with the
// degree-independent kernels (gdm_parts.h).
extern "C" {
GDM_PARTS_DECLARE(gdmk_elas_apply_p, const gdmk::ElasArgs &a, int dim, hipStream_t st)
// to_reference 1: dst[v * nc + c] = src[c * n + v]; 0: the inverse.  src != dst.
hipError_t gdmk_launch_interleave(int64_t n, int nc, int to_reference, const double *src, double *dst, hipStream_t st);
}

namespace gdmk {

inline hipError_t launch_elasticity(int p, int dim, const ElasArgs &a, hipStream_t st) {
  GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_elas_apply_p, a, dim, st)
}

}  // namespace gdmk
