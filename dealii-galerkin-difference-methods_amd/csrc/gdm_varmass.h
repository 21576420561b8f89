// gdm_varmass.h -- argument block and launchers of gdm_varmass.hip: the mass
// matrix weighted by a separable density (gdm_op_set_density),
//   dst = sum_t (M^t_x (x) M^t_y (x) M^t_z) src  [+ c * add],
// M^t_d = M[r_td] (gdm::assemble_1d_weighted): symmetric bands whose rows all
// differ.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_parts.h"

namespace gdmk {

// Kernel geometry (the same for every degree, and the same as gdm_vardiff.h):
// a workgroup of VMASS_TY / VMASS_RY waves owns a VMASS_TX x VMASS_TY (x, y)
// tile and VMASS_ZC output planes; a wave owns VMASS_RY consecutive y rows of
// the tile, a lane one x column.
constexpr int VMASS_TX = 64, VMASS_TY = 16, VMASS_RY = 4, VMASS_ZC = 16;
constexpr int VMASS_THREADS = VMASS_TX * (VMASS_TY / VMASS_RY);
constexpr int VMASS_MAX_TERMS = 4;

// Tables are row-major [rows][2p+1], entry [i][k] = A(i, i - p + k), zero
// outside the matrix.  A trivial axis has M = (1).
struct VarMassArgs {
  const double *__restrict__ src;
  double *__restrict__ dst;
  const double *__restrict__ add;  // NULL: dst = M[rho] src; else dst = M[rho] src + c * add
  double c;
  int Nx, Ny, Nz;  // kernel-space extents (trivial axes 1)
  int n_terms;
  const double *xm[VMASS_MAX_TERMS];  // [Nx][2p+1]
  const double *ym[VMASS_MAX_TERMS];  // [Ny rounded up to VMASS_TY][2p+1]: zero rows behind
  const double *zm[VMASS_MAX_TERMS];  // [Nz + 2p][2p+1]: p zero rows in front and behind
};

// rows of a y table
inline int varmass_y_rows(int Ny) { return (Ny + VMASS_TY - 1) / VMASS_TY * VMASS_TY; }

// dynamic LDS bytes: the source tile with its halo, the x sweep result of one
// term, the tile's rows of the x table of every term
inline size_t varmass_lds(int p, int n_terms) {
  const size_t W = 2 * p + 1, SX = VMASS_TX + 2 * p, SY = VMASS_TY + 2 * p;
  return sizeof(double) * (SY * SX + SY * VMASS_TX + (size_t)n_terms * W * VMASS_TX);
}

}  // namespace gdmk

// gdm_varmass.hip compiles as one unit per degree (gdm_parts.h); each
// defines its own two entry points, dispatched by degree below.
//   prepare  raise the kernel's dynamic LDS limit to `lds` bytes on the current
//            device (when the density is set)
//   apply    the kernel with `lds` bytes of dynamic LDS
extern "C" {
GDM_PARTS_DECLARE(gdmk_vmass_prepare_p, size_t lds)
GDM_PARTS_DECLARE(gdmk_vmass_apply_p, const gdmk::VarMassArgs &a, size_t lds, hipStream_t st)
}

namespace gdmk {

inline hipError_t varmass_prepare(int p, size_t lds) { GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_vmass_prepare_p, lds) }
inline hipError_t launch_varmass(int p, const VarMassArgs &a, size_t lds, hipStream_t st) {
  GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_vmass_apply_p, a, lds, st)
}

}  // namespace gdmk
