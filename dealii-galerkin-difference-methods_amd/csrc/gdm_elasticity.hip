// gdm_elasticity.hip -- linear elasticity on uncut boxes with zero boundary
// constraints (gdm_apply of a GDM_OP_ELASTICITY operator; DESIGN.md
// "Elasticity").  Replaces the assembled matrix of tests/elasticity_01_gdm.cc:
// 143-184 with the constraints of System::make_zero_boundary_constraints
// (system.h:466-498).
//
// One unit per degree: -DGDM_PART=<p>; -DGDM_PART=0 is the unit of
// the degree-independent kernels (csrc/Makefile).
//
// y = (P A P + I - P) u on component-major vectors.  The block (c, e) of A is
//   c == e:  sum_d w_cd (M (x) .. L_d .. (x) M),  w_cd = 2 mu + lambda (d == c), mu
//   c != e:  mu T(e, c) + lambda T(c, e),  T(a, b) = C in direction a, C^T in b,
//            M elsewhere,
// and P A P is the same sum with row and column 0 and N - 1 of every 1D factor
// zeroed: the constraints are edits of the tables.  One launch computes every
// output component, in the tile / z-march form of gdm_varstencil.hip:
//   * a workgroup owns an ELAS_TX x ELAS_TY (x, y) tile and ELAS_ZC output
//     planes; it stages the tile's rows of the four x and y tables in LDS once,
//   * per input plane and source component: the source tile with a p-wide halo
//     goes to LDS once, one x sweep with the four tables (M, C, C^T, L) writes
//     LDS, the y sweeps of the (x, y) factor pairs that occur for this source
//     are formed in registers and combined with mu / lambda / w into one value
//     per output component and z factor,
//   * the z direction is a march: per output component a register ring of
//     2p+1 partial output planes, the z column coefficients (wave-uniform)
//     from the tables; each output is written once.  2D has no z direction.
// Zero table rows make walls, partial tiles and out-of-box planes branch-free;
// a constrained row returns its source value (the unit diagonal).  No atomics:
// every output is summed by one thread in a fixed order.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "gdm_elasticity.h"

#ifndef GDM_PART
#error "gdm_elasticity.hip is compiled per degree: -DGDM_PART=<p> (0: the shared kernels)"
#endif

namespace {

#if GDM_PART > 0

using gdmk::ELAS_TX;
using gdmk::ELAS_TY;
using gdmk::ELAS_ZC;
constexpr int ELAS_THREADS = ELAS_TX * ELAS_TY;
// unroll factor of the band loops of the x and y sweeps: full unrolling lets the
// scheduler hoist every LDS read of a sweep, which spills the z rings at p = 9
#define ELAS_KUNROLL 3
constexpr int FM = gdmk::ELAS_M, FC = gdmk::ELAS_C, FT = gdmk::ELAS_CT, FL = gdmk::ELAS_L;

// The Kronecker terms of block (c, e): DIM terms for c == e (term t: L in
// direction t), two otherwise (term 0: mu T(e, c), term 1: lambda T(c, e)).
template <int DIM>
constexpr int elas_n_terms(int c, int e) {
  return c == e ? DIM : 2;
}
template <int DIM>
constexpr int elas_factor(int c, int e, int t, int axis) {
  if (axis >= DIM) return FM;
  if (c == e) return axis == t ? FL : FM;
  const int a = t == 0 ? e : c, b = t == 0 ? c : e;  // C in direction a, C^T in b
  return axis == a ? FC : (axis == b ? FT : FM);
}
// does source component e need the y sweep of the pair (fx, fy)?
template <int DIM>
constexpr bool elas_pair_used(int e, int fx, int fy) {
  for (int c = 0; c < DIM; ++c)
    for (int t = 0; t < elas_n_terms<DIM>(c, e); ++t)
      if (elas_factor<DIM>(c, e, t, 0) == fx && elas_factor<DIM>(c, e, t, 1) == fy) return true;
  return false;
}
template <int DIM>
constexpr bool elas_x_used(int e, int fx) {
  return elas_pair_used<DIM>(e, fx, FM) || elas_pair_used<DIM>(e, fx, FC) || elas_pair_used<DIM>(e, fx, FT) ||
         elas_pair_used<DIM>(e, fx, FL);
}
// z column coefficient of factor f: A_f(zo, zi) = A_f^T(zi, zo), a row of the transposed factor's table
constexpr int elas_transposed(int f) { return f == FC ? FT : (f == FT ? FC : f); }

// compile-time loop: f(std::integral_constant<int, I>) for I in [I0, N)
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

template <int P, int DIM>
__global__ __launch_bounds__(ELAS_THREADS) void elasticity_kernel(const gdmk::ElasArgs a) {
  constexpr int W = 2 * P + 1, SX = ELAS_TX + 2 * P, SY = ELAS_TY + 2 * P;
  constexpr int PZ = DIM == 3 ? P : 0, WZ = 2 * PZ + 1;  // z band (2D: none)
  constexpr int XS = SY * ELAS_TX;
  __shared__ double S[SY * SX];             // source tile + halo
  __shared__ double X[4 * XS];              // [4][SY][TX] x sweeps
  __shared__ double XT[4 * ELAS_TX * W];    // [4][TX][W] x table rows of the tile
  __shared__ double YT[4 * ELAS_TY * W];    // [4][TY][W] y table rows of the tile
  static_assert(sizeof(double) * (SY * SX + 4 * XS + 4 * ELAS_TX * W + 4 * ELAS_TY * W) <= 64 * 1024, "LDS");
  const int tid = threadIdx.x, tx = tid % ELAS_TX, ty = tid / ELAS_TX;
  const int x0 = blockIdx.x * ELAS_TX, y0 = blockIdx.y * ELAS_TY, z0 = blockIdx.z * ELAS_ZC;
  const int Nx = a.Nx, Ny = a.Ny, Nz = a.Nz;
  const int z1 = min(z0 + ELAS_ZC, Nz);

  // the tile's table rows (rows past the extent are zero: those outputs are not stored)
  for (int i = tid; i < 4 * ELAS_TX * W; i += ELAS_THREADS) {
    const int f = i / (ELAS_TX * W), r = (i / W) % ELAS_TX, k = i % W, gx = x0 + r;
    XT[i] = gx < Nx ? a.xtab[((int64_t)f * Nx + gx) * W + k] : 0.0;
  }
  for (int i = tid; i < 4 * ELAS_TY * W; i += ELAS_THREADS) {
    const int f = i / (ELAS_TY * W), r = (i / W) % ELAS_TY, k = i % W, gy = y0 + r;
    YT[i] = gy < Ny ? a.ytab[((int64_t)f * Ny + gy) * W + k] : 0.0;
  }

  const int gx = x0 + tx, gy = y0 + ty;
  const bool store = gx < Nx && gy < Ny;
  const bool end_xy = gx == 0 || gx == Nx - 1 || gy == 0 || gy == Ny - 1;
  // acc[c][j]: partial sum of output plane zi - PZ + j of component c while input plane zi is processed
  double acc[DIM][WZ];
#pragma unroll
  for (int c = 0; c < DIM; ++c)
#pragma unroll
    for (int j = 0; j < WZ; ++j) acc[c][j] = 0.0;

  for (int zi = z0 - PZ; zi < z1 + PZ; ++zi) {
    if (zi >= 0 && zi < Nz) {  // workgroup-uniform
      // pv[c][g]: this plane's value for output component c and z factor g
      double pv[DIM][4];
#pragma unroll
      for (int c = 0; c < DIM; ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) pv[c][g] = 0.0;

      static_for<0, DIM>([&](auto E_) {
        constexpr int E = decltype(E_)::value;
        const double *__restrict__ src = a.src + (int64_t)E * a.comp_stride + (int64_t)zi * Ny * Nx;
        __syncthreads();  // the previous readers of S and X are done (first: the tables are staged)
        for (int i = tid; i < SY * SX; i += ELAS_THREADS) {
          const int r = i / SX, c = i % SX, sx = x0 - P + c, sy = y0 - P + r;
          S[i] = (sx >= 0 && sx < Nx && sy >= 0 && sy < Ny) ? src[(int64_t)sy * Nx + sx] : 0.0;
        }
        __syncthreads();
        for (int i = tid; i < XS; i += ELAS_THREADS) {
          const int r = i / ELAS_TX, c = i % ELAS_TX;
          double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll ELAS_KUNROLL
          for (int k = 0; k < W; ++k) {
            const double v = S[r * SX + c + k];
#pragma unroll
            for (int f = 0; f < 4; ++f) s[f] += XT[(f * ELAS_TX + c) * W + k] * v;
          }
#pragma unroll
          for (int f = 0; f < 4; ++f) X[f * XS + i] = s[f];
        }
        __syncthreads();
        // q[fx][fy]: the (x, y) factor pairs of this source
        double q[4][4];
        static_for<0, 4>([&](auto FX_) {
          constexpr int fx = decltype(FX_)::value;
          static_for<0, 4>([&](auto FY_) { q[fx][decltype(FY_)::value] = 0.0; });
          if constexpr (elas_x_used<DIM>(E, fx)) {
            const double *Xf = X + fx * XS + ty * ELAS_TX + tx;
#pragma unroll ELAS_KUNROLL
            for (int k = 0; k < W; ++k) {
              const double v = Xf[k * ELAS_TX];
              static_for<0, 4>([&](auto FY_) {
                constexpr int fy = decltype(FY_)::value;
                if constexpr (elas_pair_used<DIM>(E, fx, fy)) q[fx][fy] += YT[(fy * ELAS_TY + ty) * W + k] * v;
              });
            }
          }
        });
        static_for<0, DIM>([&](auto C_) {
          constexpr int c = decltype(C_)::value;
          static_for<0, elas_n_terms<DIM>(c, E)>([&](auto T_) {
            constexpr int t = decltype(T_)::value;
            constexpr int fx = elas_factor<DIM>(c, E, t, 0), fy = elas_factor<DIM>(c, E, t, 1),
                          fz = elas_factor<DIM>(c, E, t, 2);
            const double coef = c == E ? a.w[c][t] : (t == 0 ? a.mu : a.lambda);
            pv[c][fz] += coef * q[fx][fy];
          });
        });
      });

      if constexpr (DIM == 3) {
        // output plane zo = zi - P + j: A_g(zo, zi) = entry j of row zi of the transposed factor's table
        static_for<0, 4>([&](auto G_) {
          constexpr int g = decltype(G_)::value;
          const double *zt = a.ztab + ((int64_t)elas_transposed(g) * Nz + zi) * W;
#pragma unroll
          for (int j = 0; j < WZ; ++j) {
            const double zc = zt[j];
#pragma unroll
            for (int c = 0; c < DIM; ++c) acc[c][j] += zc * pv[c][g];
          }
        });
      } else {
#pragma unroll
        for (int c = 0; c < DIM; ++c) acc[c][0] += pv[c][FM];
      }
    }
    // plane zi - PZ has its last contribution
    const int zo = zi - PZ;
    if (store && zo >= z0 && zo < z1) {
      const int64_t idx = ((int64_t)zo * Ny + gy) * Nx + gx;
      const bool constrained = end_xy || (DIM == 3 && (zo == 0 || zo == Nz - 1));
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        const int64_t i = (int64_t)c * a.comp_stride + idx;
        a.dst[i] = constrained ? a.src[i] : acc[c][0];
      }
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
#pragma unroll
      for (int j = 0; j < WZ - 1; ++j) acc[c][j] = acc[c][j + 1];
      acc[c][WZ - 1] = 0.0;
    }
  }
}

#else  // GDM_PART == 0

__global__ __launch_bounds__(256) void interleave_kernel(int64_t n, int nc, int to_reference,
                                                         const double *__restrict__ src, double *__restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // output index
  if (i >= n * nc) return;
  if (to_reference) {
    dst[i] = src[(i % nc) * n + i / nc];
  } else {
    dst[i] = src[(i % n) * nc + i / n];
  }
}

#endif

}  // namespace


extern "C" {

#if GDM_PART > 0

hipError_t GDM_PART_NAME(gdmk_elas_apply_p)(const gdmk::ElasArgs &a, int dim, hipStream_t st) {
  if (a.Nx <= 0 || a.Ny <= 0 || a.Nz <= 0) return hipSuccess;
  if (dim != 2 && dim != 3) return hipErrorInvalidValue;
  const dim3 grid((a.Nx + ELAS_TX - 1) / ELAS_TX, (a.Ny + ELAS_TY - 1) / ELAS_TY, (a.Nz + ELAS_ZC - 1) / ELAS_ZC);
  if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
  if (dim == 2)
    hipLaunchKernelGGL((elasticity_kernel<GDM_PART, 2>), grid, dim3(ELAS_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((elasticity_kernel<GDM_PART, 3>), grid, dim3(ELAS_THREADS), 0, st, a);
  return hipGetLastError();
}

#else

hipError_t gdmk_launch_interleave(int64_t n, int nc, int to_reference, const double *src, double *dst,
                                  hipStream_t st) {
  if (n <= 0 || nc <= 0) return hipSuccess;
  const int64_t blocks = (n * nc + 255) / 256;
  if (blocks > 2147483647LL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(interleave_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n, nc, to_reference, src, dst);
  return hipGetLastError();
}

#endif

}  // extern "C"
