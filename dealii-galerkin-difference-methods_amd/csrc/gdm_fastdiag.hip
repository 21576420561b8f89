// gdm_fastdiag.hip -- the dense per-axis transforms of the fast-diagonalisation
// solve (x = (alpha M - tau K)^-1 rhs on an uncut box, gdm_system_solve) on the
// FP64 matrix pipe.
//
// v_mfma_f64_16x16x4_f64 computes D (16 x 16) = A (16 x 4) B (4 x 16) + C per
// wave.  Lane l holds one f64 of A and of B and four of C / D:
//   A[row = l & 15][k = l >> 4],  B[k = l >> 4][col = l & 15],
//   D[row = (l >> 4) + 4 r][col = l & 15]  in register r = 0 .. 3
// (not the f32 row formula).
//
// A wave owns 64 x 32 (strided form) or 32 x 64 (row form) outputs: 4 x 2
// accumulators, six fragment loads for eight matrix instructions per k step
// (with one accumulator column the loads, not the matrix pipe, set the time).
// The table is always read as T transposed, so that 16 consecutive lanes read
// 16 consecutive doubles of it:
//   strided form (y, z): D[i][c] = sum_k T[i][k] X[k][c]
//       A[row][k] = Tt[k][i0 + row]        B[k][col] = X[k][c0 + col]
//   row form (x):        D[r][i] = sum_k X[r][k] T[i][k]
//       A[row][k] = X[r0 + row][k]         B[k][col] = Tt[k][i0 + col]
// Rows, columns and k beyond the extents are predicated off (the fragment
// entry is 0, nothing is read or written there).  k ascends in steps of 4 in a
// tiling that depends on the extents only: the result is bitwise repeatable.
#include "gdm_fastdiag.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int FD_WAVES = 4;   // waves per workgroup, one work item each
constexpr int FD_LONG = 64;   // outputs of a wave along the transformed axis (the table fragments)
constexpr int FD_SHORT = 32;  // and across it (the vector fragments): 4 x 2 accumulators

__device__ inline double fd_scale(const gdmk::FastdiagPass &P, int64_t idx) {
  const int64_t x = idx % P.K0, yz = idx / P.K0;
  const int64_t y = yz % P.K1, z = yz / P.K1;
  double s = 0.0;
  if (P.lam0) s += P.lam0[x];
  if (P.lam1) s += P.lam1[y];
  if (P.lam2) s += P.lam2[z];
  return 1.0 / (P.alpha + P.tau * s);
}

__global__ __launch_bounds__(64 * FD_WAVES) void fastdiag_strided(const gdmk::FastdiagPass P,
                                                                   const double *__restrict__ src,
                                                                   double *__restrict__ dst, int64_t n_ct, int64_t n_rg,
                                                                   int64_t items) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * FD_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= items) return;  // wave-uniform
  const int64_t ct = item % n_ct, t = item / n_ct;
  const int64_t rg = t % n_rg, b = t / n_rg;
  const int N = P.N;
  const int64_t cols = P.cols, base = b * N * cols;
  const int kk = lane >> 4, cc = lane & 15;
  const int i0 = (int)rg * FD_LONG;
  const int64_t c0 = ct * FD_SHORT;
  const int n_r = min(FD_LONG / 16, (N - i0 + 15) / 16);                    // wave-uniform tile counts
  const int n_c = (int)min((int64_t)(FD_SHORT / 16), (cols - c0 + 15) / 16);
  d4 acc[FD_LONG / 16][FD_SHORT / 16] = {};
  for (int k0 = 0; k0 < N; k0 += 4) {
    const int k = k0 + kk;
    const bool k_in = k < N;
    const double *xrow = src + base + (int64_t)k * cols;
    const double *trow = P.Tt + (int64_t)k * N;
    double av[FD_LONG / 16], bv[FD_SHORT / 16];
#pragma unroll
    for (int j = 0; j < FD_SHORT / 16; ++j) {
      const int64_t c = c0 + 16 * j + cc;
      bv[j] = (k_in && c < cols) ? xrow[c] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < FD_LONG / 16; ++r) {
      const int i = i0 + 16 * r + cc;
      av[r] = (k_in && i < N) ? trow[i] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < FD_LONG / 16; ++r)
#pragma unroll
      for (int j = 0; j < FD_SHORT / 16; ++j)
        if (r < n_r && j < n_c) acc[r][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[r], bv[j], acc[r][j], 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < FD_LONG / 16; ++r)
#pragma unroll
    for (int j = 0; j < FD_SHORT / 16; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = i0 + 16 * r + kk + 4 * q;
        const int64_t c = c0 + 16 * j + cc;
        if (row >= N || c >= cols) continue;
        const int64_t idx = base + (int64_t)row * cols + c;
        double v = acc[r][j][q];
        if (P.scale) v *= fd_scale(P, idx);
        dst[idx] = v;
      }
}

__global__ __launch_bounds__(64 * FD_WAVES) void fastdiag_rows(const gdmk::FastdiagPass P,
                                                                const double *__restrict__ src,
                                                                double *__restrict__ dst, int64_t n_ig, int64_t items) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * FD_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= items) return;  // wave-uniform
  const int64_t ig = item % n_ig, rt = item / n_ig;
  const int N = P.N;
  const int64_t rows = P.batch;
  const int kk = lane >> 4, cc = lane & 15;
  const int i0 = (int)ig * FD_LONG;
  const int64_t r0 = rt * FD_SHORT;
  const int n_i = min(FD_LONG / 16, (N - i0 + 15) / 16);                    // wave-uniform tile counts
  const int n_r = (int)min((int64_t)(FD_SHORT / 16), (rows - r0 + 15) / 16);
  d4 acc[FD_SHORT / 16][FD_LONG / 16] = {};
  for (int k0 = 0; k0 < N; k0 += 4) {
    const int k = k0 + kk;
    const bool k_in = k < N;
    const double *trow = P.Tt + (int64_t)k * N;
    double av[FD_SHORT / 16], bv[FD_LONG / 16];
#pragma unroll
    for (int j = 0; j < FD_SHORT / 16; ++j) {
      const int64_t ra = r0 + 16 * j + cc;  // the row this lane loads for A
      av[j] = (k_in && ra < rows) ? src[ra * N + k] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < FD_LONG / 16; ++r) {
      const int i = i0 + 16 * r + cc;
      bv[r] = (k_in && i < N) ? trow[i] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < FD_SHORT / 16; ++j)
#pragma unroll
      for (int r = 0; r < FD_LONG / 16; ++r)
        if (j < n_r && r < n_i) acc[j][r] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[j], bv[r], acc[j][r], 0, 0, 0);
  }
#pragma unroll
  for (int j = 0; j < FD_SHORT / 16; ++j)
#pragma unroll
    for (int r = 0; r < FD_LONG / 16; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + 16 * r + cc;
        const int64_t row = r0 + 16 * j + kk + 4 * q;
        if (i >= N || row >= rows) continue;
        const int64_t idx = row * N + i;
        double v = acc[j][r][q];
        if (P.scale) v *= fd_scale(P, idx);
        dst[idx] = v;
      }
}

}  // namespace

extern "C" hipError_t gdmk_launch_fastdiag_pass(const gdmk::FastdiagPass &P, const double *src, double *dst,
                                                hipStream_t st) {
  if (P.N < 1 || P.cols < 1 || P.batch < 1) return hipErrorInvalidValue;
  const int64_t n_g = (P.N + FD_LONG - 1) / FD_LONG;
  int64_t items;
  if (P.row_form) {
    if (P.cols != 1) return hipErrorInvalidValue;
    items = ((P.batch + FD_SHORT - 1) / FD_SHORT) * n_g;
  } else {
    items = P.batch * n_g * ((P.cols + FD_SHORT - 1) / FD_SHORT);
  }
  const int64_t blocks = (items + FD_WAVES - 1) / FD_WAVES;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (P.row_form)
    fastdiag_rows<<<dim3((unsigned)blocks), dim3(64 * FD_WAVES), 0, st>>>(P, src, dst, n_g, items);
  else
    fastdiag_strided<<<dim3((unsigned)blocks), dim3(64 * FD_WAVES), 0, st>>>(P, src, dst, (P.cols + FD_SHORT - 1) / FD_SHORT, n_g,
                                                                            items);
  return hipGetLastError();
}
