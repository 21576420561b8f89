// gdm_varstencil.h -- argument blocks and launchers of gdm_varstencil.hip: the
// advection operator of a separable velocity field (gdm_op_set_advection_field),
//   dst = sum_t s_t (A^t_x (x) A^t_y (x) A^t_z) src  +  box-face term,
// with banded 1D matrices whose rows all differ (no Toeplitz interior).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_parts.h"

namespace gdmk {

// Volume kernel geometry: one workgroup of VAR_TX * VAR_TY threads owns an
// (x, y) tile and VAR_ZC output planes (the same for every degree).
constexpr int VAR_TX = 32, VAR_TY = 8, VAR_ZC = 16;
constexpr int VAR_MAX_TERMS = 8;

// Tables are row-major [rows][2p+1], entry [i][k] = A(i, i - p + k), zero
// outside the matrix.  Terms that share an x table share its x sweep, terms
// that share an (x, y) table pair share the y sweep too: the host passes the
// distinct tables and pairs only.
struct VarArgs {
  const double *__restrict__ src;
  double *__restrict__ dst;
  int Nx, Ny, Nz;          // kernel-space extents (trivial axes 1)
  int n_x, n_xy, n_terms;  // distinct x tables, distinct (x, y) pairs, terms
  const double *xtab[VAR_MAX_TERMS];  // [Nx][2p+1]
  const double *ytab[VAR_MAX_TERMS];  // [Ny][2p+1] of pair v
  int xy_x[VAR_MAX_TERMS];            // x table of pair v
  const double *ztab[VAR_MAX_TERMS];  // [Nz + 2p][2p+1] of term t: p zero rows in front and behind
  int term_xy[VAR_MAX_TERMS];         // pair of term t
  double scale[VAR_MAX_TERMS];        // s_t
};

// Box-face term of one face: <(a.n)(-[a.n >= 0 ? u : u+]), v> on the face
// quadrature points (advection/stiffness.h:473-532, alpha = 0).  t0 / t1 are
// the tangential directions (a trivial one has one node, one point, weight 1).
struct VarFaceArgs {
  const double *u;    // source vector (NULL: the inflow data alone)
  const double *bc;   // [Q1][Q0] stage boundary values of the face (NULL: u+ = 0)
  double *G;          // scratch [Q1][Q0]: -(a.n) u_upwind per point
  double *T;          // scratch [Q1][n0]: G projected along t0
  double *dst;
  int Q0, Q1;         // quadrature points along t0 / t1 (cells * (p+1))
  int nc0, nc1;       // cells along t0 / t1 (0: trivial direction)
  int n0, n1;         // nodes along t0 / t1
  int64_t base, stride0, stride1;  // index of face node (0, 0), strides along t0 / t1
  const double *shape;             // [p][p+1][p+1] phi_l^{cat}(x_q)
  // projection tables of gdm::face_table_1d, node-major
  const int *qs0, *qc0, *qs1, *qc1;
  const double *w0, *w1;
  int wmax0, wmax1;
  // a.n = sum over the terms of the face's normal component:
  // coef (= +-s_t f_normal(end)) * f0[q0] * f1[q1]; NULL factor = 1
  int n_terms;
  double coef[VAR_MAX_TERMS];
  const double *f0[VAR_MAX_TERMS], *f1[VAR_MAX_TERMS];
};

}  // namespace gdmk

// gdm_varstencil.hip compiles as one unit per degree (gdm_parts.h); each
// defines its own three entry points, dispatched by degree below.
//   prepare  raise the volume kernel's dynamic LDS limit to `lds` bytes on the
//            current device (once, when the launch plan is built)
//   volume   the volume kernel with `lds` bytes of dynamic LDS
//   face     the three launches of one box face (points, t0 projection, t1
//            projection + add into dst), stream-ordered
extern "C" {
GDM_PARTS_DECLARE(gdmk_var_prepare_p, size_t lds)
GDM_PARTS_DECLARE(gdmk_var_volume_p, const gdmk::VarArgs &a, size_t lds, hipStream_t st)
GDM_PARTS_DECLARE(gdmk_var_face_p, const gdmk::VarFaceArgs &f, hipStream_t st)
}

namespace gdmk {

// dynamic LDS bytes of the volume kernel: the source tile with its halo, one x
// sweep result per distinct x table, the tile's rows of every x and y table
inline size_t var_volume_lds(int p, int n_x, int n_xy) {
  const size_t W = 2 * p + 1, SX = VAR_TX + 2 * p, SY = VAR_TY + 2 * p;
  return sizeof(double) * (SY * SX + (size_t)n_x * SY * VAR_TX + (size_t)n_x * VAR_TX * W + (size_t)n_xy * VAR_TY * W);
}

inline hipError_t var_prepare(int p, size_t lds) { GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_var_prepare_p, lds) }
inline hipError_t launch_var_volume(int p, const VarArgs &a, size_t lds, hipStream_t st) {
  GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_var_volume_p, a, lds, st)
}
inline hipError_t launch_var_face(int p, const VarFaceArgs &f, hipStream_t st) {
  GDM_PARTS_SWITCH(p, hipErrorInvalidValue, gdmk_var_face_p, f, st)
}

}  // namespace gdmk
