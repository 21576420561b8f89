// gdm_vardiff.h -- argument block and launchers of gdm_vardiff.hip: the wave /
// heat / Poisson operator with a separable coefficient (gdm_op_set_coefficient),
//   dst = sum_t (B^t_x (x) M^t_y (x) M^t_z + M^t_x (x) B^t_y (x) M^t_z + M^t_x (x) M^t_y (x) B^t_z) src,
// M^t_d = M[k_td], B^t_d = B[k_td] (gdm::wave_band_1d_weighted): symmetric bands
// whose rows all differ.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_parts.h"

namespace gdmk {

// Kernel geometry (the same for every degree): a workgroup of DIFF_TY / DIFF_RY
// waves owns a DIFF_TX x DIFF_TY (x, y) tile and DIFF_ZC output planes; a wave
// owns DIFF_RY consecutive y rows of the tile, a lane one x column.
constexpr int DIFF_TX = 64, DIFF_TY = 16, DIFF_RY = 4, DIFF_ZC = 16;
constexpr int DIFF_THREADS = DIFF_TX * (DIFF_TY / DIFF_RY);
constexpr int DIFF_MAX_TERMS = 4;

// Tables are row-major [rows][2p+1], entry [i][k] = A(i, i - p + k), zero
// outside the matrix.  A trivial axis has M = (1), B = (0).
struct DiffArgs {
  const double *__restrict__ src;
  double *__restrict__ dst;
  int Nx, Ny, Nz;  // kernel-space extents (trivial axes 1)
  int n_terms;
  const double *xm[DIFF_MAX_TERMS], *xb[DIFF_MAX_TERMS];  // [Nx][2p+1]
  const double *ym[DIFF_MAX_TERMS], *yb[DIFF_MAX_TERMS];  // [Ny rounded up to DIFF_TY][2p+1]: zero rows behind
  const double *zm[DIFF_MAX_TERMS], *zb[DIFF_MAX_TERMS];  // [Nz + 2p][2p+1]: p zero rows in front and behind
};

// rows of a y table
inline int diff_y_rows(int Ny) { return (Ny + DIFF_TY - 1) / DIFF_TY * DIFF_TY; }

// dynamic LDS bytes: the source tile with its halo, the two x sweep results of
// one term, the tile's rows of both x tables of every term
inline size_t diff_lds(int p, int n_terms) {
  const size_t W = 2 * p + 1, SX = DIFF_TX + 2 * p, SY = DIFF_TY + 2 * p;
  return sizeof(double) * (SY * SX + 2 * SY * DIFF_TX + (size_t)n_terms * 2 * W * DIFF_TX);
}

}  // namespace gdmk

// gdm_vardiff.hip compiles as one unit per degree (gdm_parts.h); each
// defines its own two entry points, dispatched by degree below.
//   prepare  raise the kernel's dynamic LDS limit to `lds` bytes on the current
//            device (when the coefficient is set)
//   apply    the kernel with `lds` bytes of dynamic LDS
extern "C" {
GDM_PARTS_DECLARE(gdmk_diff_prepare_p, size_t lds)
GDM_PARTS_DECLARE(gdmk_diff_apply_p, const gdmk::DiffArgs &a, size_t lds, hipStream_t st)
}

namespace gdmk {

inline hipError_t diff_prepare(int p, size_t lds) { GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_diff_prepare_p, lds) }
inline hipError_t launch_diff(int p, const DiffArgs &a, size_t lds, hipStream_t st) {
  GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_diff_apply_p, a, lds, st)
}

}  // namespace gdmk
