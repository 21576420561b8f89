// gdm_vec.hip -- vector kernels of the C ABI: axpby, dot product, zero fill.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_kernels.h"

namespace gdmk {

// ---------------------------------------------------------------------------
// BLAS-1
// ---------------------------------------------------------------------------
// y = a x + b y (gdm_vec_axpby).  MODE bit 0: a != 0, x is read; bit 1:
// b != 0, y is read -- an operand with a zero factor is not loaded, so what
// it holds (uninitialised memory, NaN, Inf) cannot reach the result.  The host
// picks MODE from the scalars.  x may equal y (every entry is loaded before it
// is stored, by the lane that stores it): no __restrict__.
template <int MODE>
__device__ __forceinline__ double axpby_value(double a, double x, double b, double y) {
  if (MODE == 3) return fma(a, x, b * y);
  if (MODE == 1) return a * x;
  if (MODE == 2) return b * y;
  return 0.0;
}

// pairs (double2); host-checked: x and y 16-B aligned.  The odd tail element,
// if any, is done by the first lane.
template <int MODE>
__global__ void __launch_bounds__(256) axpby2_kernel(int64_t n, double a, const double *x, double b, double *y) {
  const int64_t n2 = n / 2;
  const double2 *x2 = reinterpret_cast<const double2 *>(x);
  double2 *y2 = reinterpret_cast<double2 *>(y);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
    double2 xv = {0.0, 0.0}, yv = {0.0, 0.0};
    if (MODE & 1) xv = x2[i];
    if (MODE & 2) yv = y2[i];
    yv.x = axpby_value<MODE>(a, xv.x, b, yv.x);
    yv.y = axpby_value<MODE>(a, xv.y, b, yv.y);
    y2[i] = yv;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1))
    y[n - 1] = axpby_value<MODE>(a, (MODE & 1) ? x[n - 1] : 0.0, b, (MODE & 2) ? y[n - 1] : 0.0);
}

// scalar form for vectors that are not 16-B aligned
template <int MODE>
__global__ void __launch_bounds__(256) axpby_kernel(int64_t n, double a, const double *x, double b, double *y) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = axpby_value<MODE>(a, (MODE & 1) ? x[i] : 0.0, b, (MODE & 2) ? y[i] : 0.0);
}

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(256) dot_partial_kernel(int64_t n, const double *__restrict__ x,
                                                           const double *__restrict__ y,
                                                           double *__restrict__ partial) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    s = fma(x[i], y[i], s);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(256) dot_final_kernel(int n, const double *__restrict__ partial,
                                                         double *__restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(256) zero_kernel(int64_t n, double *__restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = 0.0;
}

}  // namespace gdmk

extern "C" hipError_t gdmk_launch_axpby(int64_t n, double a, const double *x, double b, double *y, hipStream_t st) {
  using namespace gdmk;
  if (n <= 0) return hipSuccess;
  auto al16 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  const bool pairs = al16(x) && al16(y);
  int64_t blocks = ((pairs ? n / 2 : n) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  const int mode = (a != 0.0 ? 1 : 0) | (b != 0.0 ? 2 : 0);
#define GDM_AXPBY(M)                                                                                  \
  case M:                                                                                             \
    if (pairs)                                                                                        \
      hipLaunchKernelGGL(axpby2_kernel<M>, dim3((unsigned)blocks), dim3(256), 0, st, n, a, x, b, y); \
    else                                                                                              \
      hipLaunchKernelGGL(axpby_kernel<M>, dim3((unsigned)blocks), dim3(256), 0, st, n, a, x, b, y);  \
    break;
  switch (mode) {
    GDM_AXPBY(0)
    GDM_AXPBY(1)
    GDM_AXPBY(2)
    GDM_AXPBY(3)
  }
#undef GDM_AXPBY
  return hipGetLastError();
}

extern "C" hipError_t gdmk_launch_dot(int64_t n, const double *x, const double *y, double *partial, int n_partial,
                                     double *out, hipStream_t st) {
  using namespace gdmk;
  hipLaunchKernelGGL(dot_partial_kernel, dim3(n_partial), dim3(256), 0, st, n, x, y, partial);
  hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(256), 0, st, n_partial, partial, out);
  return hipGetLastError();
}

extern "C" hipError_t gdmk_launch_zero(int64_t n, double *y, hipStream_t st) {
  using namespace gdmk;
  if (n <= 0) return hipSuccess;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(zero_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n, y);
  return hipGetLastError();
}
