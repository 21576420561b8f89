// gdm_varmass.hip -- the mass matrix weighted by a separable density
// rho(x) = sum_t prod_d r_td(x_d) (gdm_op_set_density; DESIGN.md "Separable
// density").
//
// One unit per degree: -DGDM_PART=<p> (csrc/Makefile).
//
// wave/mass.h:47-249 with JxW multiplied by rho at the quadrature point: per
// term t
//   (M_x (x) M_y (x) M_z) src,   M_d = M[r_td],
// every band with rows that all differ.  The geometry is gdm_vardiff.hip's, the
// work per term about half of it: one x sweep, one y sweep, one z accumulation.
//   * a workgroup owns a VMASS_TX x VMASS_TY (x, y) tile and VMASS_ZC output
//     planes; it stages the tile's rows of every x table in LDS once,
//   * per input plane the source tile with a p-wide halo goes to LDS; then term
//     by term: a lane takes its column's x coefficients into registers and
//     sweeps the tile's rows, the result goes to LDS, and the y sweep reads a
//     lane's column of it into registers once for the VMASS_RY rows the lane
//     owns,
//   * a wave owns VMASS_RY whole y rows, so the y and the z coefficients are
//     wave-uniform: they come through the scalar cache, not LDS,
//   * the z direction is a march: a register ring of 2p+1 partial output planes
//     per owned row, each output plane written once, with the optional
//     `+ c * add` in that store.
// Zero-padded tables make wall rows, partial tiles and the planes outside the
// box branch-free.  No atomics: every output is summed by one thread in a
// fixed order.
#include <hip/hip_runtime.h>

#include <atomic>

#include "gdm_varmass.h"

#ifndef GDM_PART
#error "gdm_varmass.hip is compiled per degree: -DGDM_PART=<p>"
#endif

namespace {

using gdmk::VMASS_RY;
using gdmk::VMASS_THREADS;
using gdmk::VMASS_TX;
using gdmk::VMASS_TY;
using gdmk::VMASS_ZC;
constexpr int VMASS_WAVES = VMASS_TY / VMASS_RY;
static_assert(VMASS_TX == 64, "a wave owns whole y rows of the tile");

template <int P>
__global__ __launch_bounds__(VMASS_THREADS) void varmass_kernel(const gdmk::VarMassArgs a) {
  constexpr int W = 2 * P + 1, SX = VMASS_TX + 2 * P, SY = VMASS_TY + 2 * P, NR = VMASS_RY + 2 * P;
  extern __shared__ double lds[];
  double *S = lds;                 // [SY][SX] source tile + halo
  double *XM = S + SY * SX;        // [SY][VMASS_TX] M_x sweep of the current term
  double *XT = XM + SY * VMASS_TX; // [n_terms][W][VMASS_TX] x table rows of the tile, column-major
  const int tid = threadIdx.x, lane = tid % VMASS_TX;
  const int wave = __builtin_amdgcn_readfirstlane(tid / VMASS_TX);
  const int x0 = blockIdx.x * VMASS_TX, y0 = blockIdx.y * VMASS_TY, z0 = blockIdx.z * VMASS_ZC;
  const int z1 = min(z0 + VMASS_ZC, a.Nz);
  const int Nx = a.Nx, Ny = a.Ny, Nz = a.Nz, n_terms = a.n_terms;

  // the tile's x table rows (rows past the extent are zero: those outputs are not stored)
  for (int e = tid; e < n_terms * W * VMASS_TX; e += VMASS_THREADS) {
    const int c = e % VMASS_TX, k = (e / VMASS_TX) % W, t = e / (VMASS_TX * W);
    XT[e] = x0 + c < Nx ? a.xm[t][(int64_t)(x0 + c) * W + k] : 0.0;
  }

  const int gx = x0 + lane, gy0 = y0 + wave * VMASS_RY;
  // acc[j][i]: partial sum of output plane zi - P + i, row gy0 + j, while input plane zi is processed
  double acc[VMASS_RY][W];
#pragma unroll
  for (int j = 0; j < VMASS_RY; ++j)
#pragma unroll
    for (int i = 0; i < W; ++i) acc[j][i] = 0.0;

  for (int zi = z0 - P; zi < z1 + P; ++zi) {
    if (zi >= 0 && zi < Nz) {  // workgroup-uniform
      // the previous plane's x sweeps (the readers of S) ended before its last y sweep
      for (int e = tid; e < SY * SX; e += VMASS_THREADS) {
        const int r = e / SX, c = e % SX, sx = x0 - P + c, sy = y0 - P + r;
        S[e] = (sx >= 0 && sx < Nx && sy >= 0 && sy < Ny) ? a.src[((int64_t)zi * Ny + sy) * Nx + sx] : 0.0;
      }
      for (int t = 0; t < n_terms; ++t) {
        // S (first term: and the tables) is staged; the previous y sweep's readers of XM are done
        __syncthreads();
        {
          double cm[W];
          const double *xt = XT + t * W * VMASS_TX + lane;
#pragma unroll
          for (int k = 0; k < W; ++k) cm[k] = xt[k * VMASS_TX];
          for (int r = wave; r < SY; r += VMASS_WAVES) {
            const double *s = S + r * SX + lane;
            double sm = 0.0;
#pragma unroll
            for (int k = 0; k < W; ++k) sm += cm[k] * s[k];
            XM[r * VMASS_TX + lane] = sm;
          }
        }
        __syncthreads();
        double vm[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) vm[i] = XM[(wave * VMASS_RY + i) * VMASS_TX + lane];
        // output plane zo = zi - P + i: M_z(zo, zi) = row zo, entry 2P - i; the z
        // tables have P zero rows in front, so row zo is row zi + i
        const double *zm = a.zm[t] + (int64_t)zi * W;
#pragma unroll
        for (int j = 0; j < VMASS_RY; ++j) {
          const double *my = a.ym[t] + (int64_t)(gy0 + j) * W;
          double p2 = 0.0;
#pragma unroll
          for (int k = 0; k < W; ++k) p2 += my[k] * vm[j + k];
#pragma unroll
          for (int i = 0; i < W; ++i) acc[j][i] += zm[i * W + (2 * P - i)] * p2;
        }
      }
    }
    // plane zi - P has its last contribution
    const int zo = zi - P;
    if (zo >= z0 && zo < z1 && gx < Nx) {
#pragma unroll
      for (int j = 0; j < VMASS_RY; ++j)
        if (gy0 + j < Ny) {
          const int64_t o = ((int64_t)zo * Ny + gy0 + j) * Nx + gx;
          a.dst[o] = a.add ? acc[j][0] + a.c * a.add[o] : acc[j][0];
        }
    }
#pragma unroll
    for (int j = 0; j < VMASS_RY; ++j) {
#pragma unroll
      for (int i = 0; i < W - 1; ++i) acc[j][i] = acc[j][i + 1];
      acc[j][W - 1] = 0.0;
    }
  }
}

std::atomic<size_t> g_lds_max{0};

}  // namespace


extern "C" {

hipError_t GDM_PART_NAME(gdmk_vmass_prepare_p)(size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;  // within the default limit
  // the limit is a property of the kernel, shared by every operator: keep the
  // largest request (set again on every call, so on every device that asks)
  size_t prev = g_lds_max.load();
  while (prev < lds && !g_lds_max.compare_exchange_weak(prev, lds)) {
  }
  return hipFuncSetAttribute((const void *)varmass_kernel<GDM_PART>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)g_lds_max.load());
}

hipError_t GDM_PART_NAME(gdmk_vmass_apply_p)(const gdmk::VarMassArgs &a, size_t lds, hipStream_t st) {
  if (a.Nx <= 0 || a.Ny <= 0 || a.Nz <= 0 || a.n_terms <= 0) return hipSuccess;
  if (a.n_terms > gdmk::VMASS_MAX_TERMS) return hipErrorInvalidValue;
  const dim3 grid((a.Nx + VMASS_TX - 1) / VMASS_TX, (a.Ny + VMASS_TY - 1) / VMASS_TY,
                  (a.Nz + VMASS_ZC - 1) / VMASS_ZC);
  if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(varmass_kernel<GDM_PART>, grid, dim3(VMASS_THREADS), lds, st, a);
  return hipGetLastError();
}

}  // extern "C"
