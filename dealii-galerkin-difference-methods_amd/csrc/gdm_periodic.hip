// gdm_periodic.hip -- exact mass inverse with periodicity constraints, the
// device part (gdm_mass_solve_periodic; replaces the SolverCG of
// prototypes/advection_01_gdm.cc:208-217).
//
// Along a periodic direction the condensed 1D mass matrix on the N - 1 free
// vertices is M_per = A + U S U^T with A the leading block of M, U = [e_0, m]
// (m = M[0:N-1, N-1], p non-zeros at its end) and S = [[M[N-1,N-1], 1], [1, 0]].
// The line kernels of gdm_mass.hip solve with A~ = blockdiag(A, 1) (g = A^-1 b,
// the last entry untouched); Woodbury gives
//   M_per^-1 b = g - T (U^T g),  T = Z (S^-1 + U^T Z)^-1, Z = A^-1 U  (host tables),
// a rank-2 update per line, followed by the distribute x_{N-1} = x_0.
//
// The inputs of U^T g (g_0 and the last p free entries) are rows the update
// rewrites, so it runs as two launches: the gather reads every line's inputs
// into w = [2][n_lines], the apply reads w and its own entry only.  Each
// output has one writer; the arithmetic of an entry is the same in the
// in-place and the RK-fused form:  c = fma(T_k0, w_0, T_k1 * w_1), x_k = g_k - c.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gdm_periodic.h"

namespace gdmk {

// one thread per line; strided lines (s > 1): consecutive lanes read
// consecutive addresses.  The p entries of m are wave-uniform loads.
__global__ void __launch_bounds__(256) periodic_gather_kernel(const PeriodicDir d, const double *__restrict__ x,
                                                              double *__restrict__ w) {
  const int64_t n_lines = d.s * d.n_outer;
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n_lines) return;
  const int64_t outer = l / d.s, inner = l - outer * d.s;
  const double *g = x + outer * d.N * d.s + inner;
  double acc = 0.0;
  for (int j = 0; j < d.p; ++j) acc = fma(d.m[j], g[(int64_t)(d.N - 1 - d.p + j) * d.s], acc);
  w[l] = g[0];
  w[n_lines + l] = acc;
}

// row of work item t: the touched rows [0, rows_lo), [N-1-rows_hi, N-1) and
// the constrained row N-1 (in place), or every row (RK form)
template <bool RK>
__device__ inline int periodic_row(const PeriodicDir &d, int t) {
  if (RK) return t;
  if (t < d.rows_lo) return t;
  return d.N - 1 - d.rows_hi + (t - d.rows_lo);
}

template <bool RK, bool WITH_Y>
__device__ inline void periodic_entry(const PeriodicDir &d, int k, double T0, double T1, double w0, double w1,
                                      double *x, int64_t e, const RkOut &rk) {
  const bool touched = k < d.rows_lo || k >= d.N - 1 - d.rows_hi;
  double v;
  if (k == d.N - 1) {
    v = w0 - fma(T0, w0, T1 * w1);  // x_0's value and bits (w_0 = g_0): the distribute
  } else {
    v = x[e];
    if (touched) v = v - fma(T0, w0, T1 * w1);
  }
  if (RK) {
    const double a = __builtin_nontemporal_load(rk.acc_in + e);
    if (WITH_Y) {
      const double y = __builtin_nontemporal_load(rk.y + e);
      __builtin_nontemporal_store(fma(rk.alpha, v, y), rk.Y + e);
    }
    __builtin_nontemporal_store(fma(rk.beta, v, a), rk.acc_out + e);
  } else {
    x[e] = v;
  }
}

// strided lines: grid (line blocks, rows); the row and its T entries are
// block-uniform (scalar loads), lanes run along the contiguous index
template <bool RK, bool WITH_Y>
__global__ void __launch_bounds__(256) periodic_apply_strided_kernel(const PeriodicDir d, double *x,
                                                                     const double *__restrict__ w, const RkOut rk,
                                                                     int nt) {
  const int64_t n_lines = d.s * d.n_outer;
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n_lines) return;
  const int64_t outer = l / d.s, inner = l - outer * d.s;
  const double w0 = w[l], w1 = w[n_lines + l];
  for (int t = blockIdx.y; t < nt; t += gridDim.y) {
    const int k = periodic_row<RK>(d, t);
    const int kt = k == d.N - 1 ? 0 : k;
    const double T0 = d.T[2 * kt], T1 = d.T[2 * kt + 1];
    periodic_entry<RK, WITH_Y>(d, k, T0, T1, w0, w1, x, (outer * d.N + k) * d.s + inner, rk);
  }
}

// contiguous x lines (s = 1): block (64 rows, 4 lines); a wave runs along its
// line, the 64 T rows of the block's row chunk come from LDS
template <bool RK, bool WITH_Y>
__global__ void __launch_bounds__(256) periodic_apply_x_kernel(const PeriodicDir d, double *x,
                                                               const double *__restrict__ w, const RkOut rk, int nt) {
  __shared__ double Ts[64][2];
  const int64_t n_lines = d.n_outer;
  const int t = blockIdx.y * 64 + threadIdx.x;
  const int k = t < nt ? periodic_row<RK>(d, t) : 0;
  if (threadIdx.y == 0) {
    const int kt = k == d.N - 1 ? 0 : k;
    Ts[threadIdx.x][0] = d.T[2 * kt];
    Ts[threadIdx.x][1] = d.T[2 * kt + 1];
  }
  __syncthreads();
  const int64_t l = (int64_t)blockIdx.x * blockDim.y + threadIdx.y;
  if (l >= n_lines || t >= nt) return;
  periodic_entry<RK, WITH_Y>(d, k, Ts[threadIdx.x][0], Ts[threadIdx.x][1], w[l], w[n_lines + l], x, l * d.N + k, rk);
}

}  // namespace gdmk

extern "C" hipError_t gdmk_launch_periodic_gather(const gdmk::PeriodicDir &d, const double *x, double *w,
                                                  hipStream_t st) {
  const int64_t n_lines = d.s * d.n_outer;
  if (n_lines <= 0) return hipSuccess;
  const int64_t blocks = (n_lines + 255) / 256;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gdmk::periodic_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d, x, w);
  return hipGetLastError();
}

extern "C" hipError_t gdmk_launch_periodic_apply(const gdmk::PeriodicDir &d, double *x, const double *w,
                                                 const gdmk::RkOut *rk, hipStream_t st) {
  const int64_t n_lines = d.s * d.n_outer;
  if (n_lines <= 0) return hipSuccess;
  const int nt = rk ? d.N : d.rows_lo + d.rows_hi + 1;
  const gdmk::RkOut r = rk ? *rk : gdmk::RkOut{nullptr, nullptr, nullptr, nullptr, 0.0, 0.0};
  const int mode = rk ? (rk->Y ? 2 : 1) : 0;
  if (d.s == 1) {
    const int64_t bx = (n_lines + 3) / 4;
    if (bx > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)bx, (unsigned)((nt + 63) / 64)), block(64, 4);
    if (grid.y > 65535) return hipErrorInvalidValue;
    if (mode == 0)
      hipLaunchKernelGGL((gdmk::periodic_apply_x_kernel<false, false>), grid, block, 0, st, d, x, w, r, nt);
    else if (mode == 1)
      hipLaunchKernelGGL((gdmk::periodic_apply_x_kernel<true, false>), grid, block, 0, st, d, x, w, r, nt);
    else
      hipLaunchKernelGGL((gdmk::periodic_apply_x_kernel<true, true>), grid, block, 0, st, d, x, w, r, nt);
  } else {
    const int64_t bx = (n_lines + 255) / 256;
    if (bx > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)bx, (unsigned)std::min(nt, 65535)), block(256);
    if (mode == 0)
      hipLaunchKernelGGL((gdmk::periodic_apply_strided_kernel<false, false>), grid, block, 0, st, d, x, w, r, nt);
    else if (mode == 1)
      hipLaunchKernelGGL((gdmk::periodic_apply_strided_kernel<true, false>), grid, block, 0, st, d, x, w, r, nt);
    else
      hipLaunchKernelGGL((gdmk::periodic_apply_strided_kernel<true, true>), grid, block, 0, st, d, x, w, r, nt);
  }
  return hipGetLastError();
}
