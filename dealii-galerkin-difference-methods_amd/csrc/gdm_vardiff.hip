// gdm_vardiff.hip -- the wave / heat / Poisson operator with a separable
// coefficient kappa(x) = sum_t prod_d k_td(x_d) (gdm_op_set_coefficient;
// DESIGN.md "Separable coefficient").
//
// One unit per degree: -DGDM_PART=<p> (csrc/Makefile).
//
// wave/stiffness.h:171-181 and :296-310 with JxW multiplied by kappa at the
// quadrature point: per term t
//   (B_x M_y M_z + M_x B_y M_z + M_x M_y B_z) src,   M = M[k_td], B = B[k_td],
// every band with rows that all differ.  The structure saves work over a list
// of 3 T Kronecker terms: per term two x sweeps (M_x, B_x), two y results
//   P1 = M_y (B_x s) + B_y (M_x s),   P2 = M_y (M_x s)
// and two z accumulations, P1 through M_z and P2 through B_z.
//   * a workgroup owns a DIFF_TX x DIFF_TY (x, y) tile and DIFF_ZC output
//     planes; it stages the tile's rows of every x table in LDS once,
//   * per input plane the source tile with a p-wide halo goes to LDS; then term
//     by term: a lane takes its column's x coefficients into registers and
//     sweeps the tile's rows (one LDS read of the source per two FMAs), the two
//     results go to LDS, and the y sweep reads a lane's column of them into
//     registers once for the DIFF_RY rows the lane owns,
//   * a wave owns DIFF_RY whole y rows, so the y and the z coefficients are
//     wave-uniform: they come through the scalar cache, not LDS,
//   * the z direction is a march: a register ring of 2p+1 partial output planes
//     per owned row, each output plane written once.
// Zero-padded tables make wall rows, partial tiles and the planes outside the
// box branch-free.  No atomics: every output is summed by one thread in a
// fixed order.
#include <hip/hip_runtime.h>

#include <atomic>

#include "gdm_vardiff.h"

#ifndef GDM_PART
#error "gdm_vardiff.hip is compiled per degree: -DGDM_PART=<p>"
#endif

namespace {

using gdmk::DIFF_RY;
using gdmk::DIFF_THREADS;
using gdmk::DIFF_TX;
using gdmk::DIFF_TY;
using gdmk::DIFF_ZC;
constexpr int DIFF_WAVES = DIFF_TY / DIFF_RY;
static_assert(DIFF_TX == 64, "a wave owns whole y rows of the tile");

template <int P>
__global__ __launch_bounds__(DIFF_THREADS) void diff_kernel(const gdmk::DiffArgs a) {
  constexpr int W = 2 * P + 1, SX = DIFF_TX + 2 * P, SY = DIFF_TY + 2 * P, NR = DIFF_RY + 2 * P;
  extern __shared__ double lds[];
  double *S = lds;                  // [SY][SX] source tile + halo
  double *XM = S + SY * SX;         // [SY][DIFF_TX] M_x sweep of the current term
  double *XB = XM + SY * DIFF_TX;   // [SY][DIFF_TX] B_x sweep of the current term
  double *XT = XB + SY * DIFF_TX;   // [n_terms][2][W][DIFF_TX] x table rows of the tile, column-major
  const int tid = threadIdx.x, lane = tid % DIFF_TX;
  const int wave = __builtin_amdgcn_readfirstlane(tid / DIFF_TX);
  const int x0 = blockIdx.x * DIFF_TX, y0 = blockIdx.y * DIFF_TY, z0 = blockIdx.z * DIFF_ZC;
  const int z1 = min(z0 + DIFF_ZC, a.Nz);
  const int Nx = a.Nx, Ny = a.Ny, Nz = a.Nz, n_terms = a.n_terms;

  // the tile's x table rows (rows past the extent are zero: those outputs are not stored)
  for (int e = tid; e < n_terms * 2 * W * DIFF_TX; e += DIFF_THREADS) {
    const int c = e % DIFF_TX, k = (e / DIFF_TX) % W, wh = (e / (DIFF_TX * W)) % 2, t = e / (DIFF_TX * W * 2);
    const double *tab = wh ? a.xb[t] : a.xm[t];
    XT[e] = x0 + c < Nx ? tab[(int64_t)(x0 + c) * W + k] : 0.0;
  }

  const int gx = x0 + lane, gy0 = y0 + wave * DIFF_RY;
  // acc[j][i]: partial sum of output plane zi - P + i, row gy0 + j, while input plane zi is processed
  double acc[DIFF_RY][W];
#pragma unroll
  for (int j = 0; j < DIFF_RY; ++j)
#pragma unroll
    for (int i = 0; i < W; ++i) acc[j][i] = 0.0;

  for (int zi = z0 - P; zi < z1 + P; ++zi) {
    if (zi >= 0 && zi < Nz) {  // workgroup-uniform
      // the previous plane's x sweeps (the readers of S) ended before its last y sweep
      for (int e = tid; e < SY * SX; e += DIFF_THREADS) {
        const int r = e / SX, c = e % SX, sx = x0 - P + c, sy = y0 - P + r;
        S[e] = (sx >= 0 && sx < Nx && sy >= 0 && sy < Ny) ? a.src[((int64_t)zi * Ny + sy) * Nx + sx] : 0.0;
      }
      for (int t = 0; t < n_terms; ++t) {
        // S (first term: and the tables) is staged; the previous y sweep's readers of XM / XB are done
        __syncthreads();
        {
          double cm[W], cb[W];
          const double *xt = XT + t * 2 * W * DIFF_TX + lane;
#pragma unroll
          for (int k = 0; k < W; ++k) {
            cm[k] = xt[k * DIFF_TX];
            cb[k] = xt[(W + k) * DIFF_TX];
          }
          for (int r = wave; r < SY; r += DIFF_WAVES) {
            const double *s = S + r * SX + lane;
            double sm = 0.0, sb = 0.0;
#pragma unroll
            for (int k = 0; k < W; ++k) {
              const double v = s[k];
              sm += cm[k] * v;
              sb += cb[k] * v;
            }
            XM[r * DIFF_TX + lane] = sm;
            XB[r * DIFF_TX + lane] = sb;
          }
        }
        __syncthreads();
        double vm[NR], vb[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          vm[i] = XM[(wave * DIFF_RY + i) * DIFF_TX + lane];
          vb[i] = XB[(wave * DIFF_RY + i) * DIFF_TX + lane];
        }
        // output plane zo = zi - P + i: A_z(zo, zi) = row zo, entry 2P - i; the z
        // tables have P zero rows in front, so row zo is row zi + i
        const double *zm = a.zm[t] + (int64_t)zi * W, *zb = a.zb[t] + (int64_t)zi * W;
#pragma unroll
        for (int j = 0; j < DIFF_RY; ++j) {
          const double *my = a.ym[t] + (int64_t)(gy0 + j) * W, *by = a.yb[t] + (int64_t)(gy0 + j) * W;
          double p1 = 0.0, p2 = 0.0;
#pragma unroll
          for (int k = 0; k < W; ++k) {
            p1 += my[k] * vb[j + k];
            p1 += by[k] * vm[j + k];
            p2 += my[k] * vm[j + k];
          }
#pragma unroll
          for (int i = 0; i < W; ++i) {
            acc[j][i] += zm[i * W + (2 * P - i)] * p1;
            acc[j][i] += zb[i * W + (2 * P - i)] * p2;
          }
        }
      }
    }
    // plane zi - P has its last contribution
    const int zo = zi - P;
    if (zo >= z0 && zo < z1 && gx < Nx) {
#pragma unroll
      for (int j = 0; j < DIFF_RY; ++j)
        if (gy0 + j < Ny) a.dst[((int64_t)zo * Ny + gy0 + j) * Nx + gx] = acc[j][0];
    }
#pragma unroll
    for (int j = 0; j < DIFF_RY; ++j) {
#pragma unroll
      for (int i = 0; i < W - 1; ++i) acc[j][i] = acc[j][i + 1];
      acc[j][W - 1] = 0.0;
    }
  }
}

std::atomic<size_t> g_lds_max{0};

}  // namespace


extern "C" {

hipError_t GDM_PART_NAME(gdmk_diff_prepare_p)(size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;  // within the default limit
  // the limit is a property of the kernel, shared by every operator: keep the
  // largest request (set again on every call, so on every device that asks)
  size_t prev = g_lds_max.load();
  while (prev < lds && !g_lds_max.compare_exchange_weak(prev, lds)) {
  }
  return hipFuncSetAttribute((const void *)diff_kernel<GDM_PART>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)g_lds_max.load());
}

hipError_t GDM_PART_NAME(gdmk_diff_apply_p)(const gdmk::DiffArgs &a, size_t lds, hipStream_t st) {
  if (a.Nx <= 0 || a.Ny <= 0 || a.Nz <= 0 || a.n_terms <= 0) return hipSuccess;
  if (a.n_terms > gdmk::DIFF_MAX_TERMS) return hipErrorInvalidValue;
  const dim3 grid((a.Nx + DIFF_TX - 1) / DIFF_TX, (a.Ny + DIFF_TY - 1) / DIFF_TY, (a.Nz + DIFF_ZC - 1) / DIFF_ZC);
  if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(diff_kernel<GDM_PART>, grid, dim3(DIFF_THREADS), lds, st, a);
  return hipGetLastError();
}

}  // extern "C"
