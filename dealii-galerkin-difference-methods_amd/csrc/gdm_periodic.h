// gdm_periodic.h -- launchers of gdm_periodic.hip: the rank-2 correction that
// turns the line solves with A~ = blockdiag(A, 1) into the exact inverse of the
// periodically condensed 1D mass matrix (gdm_mass_solve_periodic).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_kernels.h"

namespace gdmk {

// One periodic reference direction in the memory geometry of an owned vector
// (lexicographic, x fastest): entry k of line l = (outer, inner) lives at
// (outer * N + k) * s + inner with inner in [0, s), l = outer * s + inner.
// s = 1: the contiguous x lines; s > 1: strided lines, contiguous across lines.
struct PeriodicDir {
  int64_t s, n_outer;
  int N, p;
  int rows_lo, rows_hi;  // the correction touches rows [0, rows_lo) and [N-1-rows_hi, N-1)
  const double *T;       // device [N-1][2]
  const double *m;       // device [p]: M[N-1-p+j, N-1]
};

}  // namespace gdmk

extern "C" {
// w[0][l] = g_0, w[1][l] = sum_j m_j g_{N-1-p+j} of every line l (w: [2][n_lines])
hipError_t gdmk_launch_periodic_gather(const gdmk::PeriodicDir &d, const double *x, double *w, hipStream_t st);
// x_k -= T[k][0] w_0 + T[k][1] w_1 on the touched rows and x_{N-1} = x_0 (rk ==
// NULL, in place), or the same k_k of every row, not stored, into acc_out =
// acc_in + beta k and Y = y + alpha k (rk != NULL; x is only read)
hipError_t gdmk_launch_periodic_apply(const gdmk::PeriodicDir &d, double *x, const double *w, const gdmk::RkOut *rk,
                                      hipStream_t st);
}
