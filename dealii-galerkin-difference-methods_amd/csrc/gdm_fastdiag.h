// gdm_fastdiag.h -- argument block and launcher of gdm_fastdiag.hip: the dense
// per-axis transforms of the fast-diagonalisation solve (gdm_system_solve) on
// the FP64 matrix pipe (v_mfma_f64_16x16x4_f64).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace gdmk {

// One transform pass dst[.., i, ..] = sum_j T[i, j] src[.., j, ..] along one
// kernel axis of an x-fastest vector, seen as `batch` row-major (N x cols)
// blocks: cols = extent below the axis, batch = extent above it.  cols == 1
// with row_form set is the x axis (the contraction index is the contiguous
// one): dst = src T^T over `batch` rows of length N.
struct FastdiagPass {
  int N;               // contraction length = output length along the axis
  int64_t cols;        // contiguous extent below the axis
  int64_t batch;       // blocks (strided form) or rows (row form)
  int row_form;        // 1: the x axis
  const double *Tt;    // T transposed, row-major N x N: Tt[j * N + i] = T[i, j]
  // epilogue: dst *= 1 / (alpha + tau (lam0[x] + lam1[y] + lam2[z])) with the
  // kernel-space extents K0, K1 of the whole vector (lam == nullptr: 0);
  // scale == 0: none
  int scale;
  double alpha, tau;
  const double *lam0, *lam1, *lam2;
  int K0, K1;
};

}  // namespace gdmk

extern "C" {
// src and dst must not overlap.  Fixed tiling, ascending k: the bits of dst do
// not depend on the launch or the stream.
hipError_t gdmk_launch_fastdiag_pass(const gdmk::FastdiagPass &P, const double *src, double *dst, hipStream_t st);
}
