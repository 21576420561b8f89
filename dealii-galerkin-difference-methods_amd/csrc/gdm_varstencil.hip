// gdm_varstencil.hip -- advection with a separable, spatially varying velocity
// field (gdm_op_set_advection_field; DESIGN.md "Separable fields").
//
// One unit per degree: -DGDM_PART=<p> (csrc/Makefile).
//
// Volume:  dst = sum_t s_t (A^t_x (x) A^t_y (x) A^t_z) src, the quadrature sums
// of advection/stiffness.h:395-417 reordered, with A = C[f] along the term's
// component and M[f] elsewhere.  The bands are not Toeplitz: every row has its
// own 2p+1 coefficients, read from tables.
//   * a workgroup owns a VAR_TX x VAR_TY (x, y) tile and VAR_ZC output planes;
//     it stages the tile's rows of every x and y table in LDS once,
//   * per input plane: the source tile with a p-wide halo goes to LDS, one x
//     sweep per distinct x table writes LDS, one y sweep per distinct (x, y)
//     pair reads it back into a register,
//   * the z direction is a march: a register ring of 2p+1 partial output
//     planes, the z column coefficients (wave-uniform) from the zero-padded
//     table, each output plane written once.
// Zero-padded tables make wall rows, partial tiles and the planes outside the
// box branch-free.  No atomics: every output is summed by one thread in a
// fixed order.
//
// Faces: the upwind selection max(a.n, 0) acts on the SUM of the terms, so the
// face term is not separable; it is (dim-1)-dimensional and touches the
// boundary node plane only.  Three launches per face: the points (a.n from the
// 1D factor samples, u interpolated from the plane's nodes, u or u+ selected,
// G = -(a.n) u_upwind), the projection along t0, the projection along t1 with
// the add into dst.  Gather form, one thread per output, fixed order; the
// faces run one after the other on the stream, so the box edges' sums have a
// fixed order too.
#include <hip/hip_runtime.h>

#include <atomic>

#include "gdm_varstencil.h"

#ifndef GDM_PART
#error "gdm_varstencil.hip is compiled per degree: -DGDM_PART=<p>"
#endif

namespace {

using gdmk::VAR_TX;
using gdmk::VAR_TY;
using gdmk::VAR_ZC;
constexpr int VAR_THREADS = VAR_TX * VAR_TY;

template <int P>
__global__ __launch_bounds__(VAR_THREADS) void var_volume_kernel(const gdmk::VarArgs a) {
  constexpr int W = 2 * P + 1, SX = VAR_TX + 2 * P, SY = VAR_TY + 2 * P;
  extern __shared__ double lds[];
  double *S = lds;                              // [SY][SX] source tile + halo
  double *X = S + SY * SX;                      // [n_x][SY][VAR_TX] x sweeps
  double *XT = X + a.n_x * SY * VAR_TX;         // [n_x][VAR_TX][W] x table rows of the tile
  double *YT = XT + a.n_x * VAR_TX * W;         // [n_xy][VAR_TY][W] y table rows of the tile
  const int tid = threadIdx.x, tx = tid % VAR_TX, ty = tid / VAR_TX;
  const int x0 = blockIdx.x * VAR_TX, y0 = blockIdx.y * VAR_TY, z0 = blockIdx.z * VAR_ZC;
  const int z1 = min(z0 + VAR_ZC, a.Nz);
  const int Nx = a.Nx, Ny = a.Ny, Nz = a.Nz;

  // the tile's table rows (rows past the extent are zero: those outputs are not stored)
  for (int e = tid; e < a.n_x * VAR_TX * W; e += VAR_THREADS) {
    const int u = e / (VAR_TX * W), r = (e / W) % VAR_TX, k = e % W, gx = x0 + r;
    XT[e] = gx < Nx ? a.xtab[u][(int64_t)gx * W + k] : 0.0;
  }
  for (int e = tid; e < a.n_xy * VAR_TY * W; e += VAR_THREADS) {
    const int v = e / (VAR_TY * W), r = (e / W) % VAR_TY, k = e % W, gy = y0 + r;
    YT[e] = gy < Ny ? a.ytab[v][(int64_t)gy * W + k] : 0.0;
  }

  const int gx = x0 + tx, gy = y0 + ty;
  const bool store = gx < Nx && gy < Ny;
  // acc[j]: partial sum of output plane zi - P + j while input plane zi is processed
  double acc[W];
#pragma unroll
  for (int j = 0; j < W; ++j) acc[j] = 0.0;

  for (int zi = z0 - P; zi < z1 + P; ++zi) {
    if (zi >= 0 && zi < Nz) {  // workgroup-uniform
      __syncthreads();  // the previous plane's readers of S and X are done (first plane: the tables are staged)
      for (int e = tid; e < SY * SX; e += VAR_THREADS) {
        const int r = e / SX, c = e % SX, sx = x0 - P + c, sy = y0 - P + r;
        S[e] = (sx >= 0 && sx < Nx && sy >= 0 && sy < Ny) ? a.src[((int64_t)zi * Ny + sy) * Nx + sx] : 0.0;
      }
      __syncthreads();
      for (int u = 0; u < a.n_x; ++u) {
        const double *xt = XT + u * VAR_TX * W;
        double *Xu = X + u * SY * VAR_TX;
        for (int e = tid; e < SY * VAR_TX; e += VAR_THREADS) {
          const int r = e / VAR_TX, c = e % VAR_TX;
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < W; ++k) s += xt[c * W + k] * S[r * SX + c + k];
          Xu[e] = s;
        }
      }
      __syncthreads();
      for (int v = 0; v < a.n_xy; ++v) {
        const double *Xu = X + a.xy_x[v] * SY * VAR_TX;
        const double *yt = YT + (v * VAR_TY + ty) * W;
        double pv = 0.0;
#pragma unroll
        for (int k = 0; k < W; ++k) pv += yt[k] * Xu[(ty + k) * VAR_TX + tx];
        for (int t = 0; t < a.n_terms; ++t) {
          if (a.term_xy[t] != v) continue;  // uniform
          // output plane zo = zi - P + j: A_z(zo, zi) = row zo, entry 2P - j;
          // the table has P zero rows in front, so row zo is row zi + j
          const double *zt = a.ztab[t] + (int64_t)zi * W;
          const double s = a.scale[t];
#pragma unroll
          for (int j = 0; j < W; ++j) acc[j] += (s * zt[j * W + (2 * P - j)]) * pv;
        }
      }
    }
    // plane zi - P has its last contribution
    const int zo = zi - P;
    if (store && zo >= z0 && zo < z1) a.dst[((int64_t)zo * Ny + gy) * Nx + gx] = acc[0];
#pragma unroll
    for (int j = 0; j < W - 1; ++j) acc[j] = acc[j + 1];
    acc[W - 1] = 0.0;
  }
}

// category / DoF-box offset of a 1D cell (include/gdm/system.h:195-246)
__device__ inline int var_category(int c, int p, int n) {
  const int half = p / 2;
  if (c < half) return c;
  if (c < n - half) return half;
  return p + c - n;
}
__device__ inline int var_offset(int c, int p, int n) {
  const int half = p / 2;
  if (c < half) return 0;
  return min(n, c + half + 1) - p;
}

// G[q1][q0] = -(a.n) * (a.n >= 0 ? u : u+) at every face quadrature point
template <int P>
__global__ __launch_bounds__(256) void var_face_points_kernel(const gdmk::VarFaceArgs f) {
  constexpr int n1 = P + 1;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)f.Q0 * f.Q1) return;
  const int q0 = (int)(idx % f.Q0), q1 = (int)(idx / f.Q0);
  double an = 0.0;
  for (int t = 0; t < f.n_terms; ++t)
    an += f.coef[t] * (f.f0[t] ? f.f0[t][q0] : 1.0) * (f.f1[t] ? f.f1[t][q1] : 1.0);
  double upw = 0.0;
  if (an >= 0.0) {
    if (f.u) {
      // u at the point from the boundary plane's nodes (the trace of the basis
      // on a box face is the boundary node's shape function alone)
      int off0 = 0, m0 = 1, off1 = 0, m1 = 1;
      const double *s0 = nullptr, *s1 = nullptr;
      if (f.nc0 > 0) {
        const int c = q0 / n1;
        off0 = var_offset(c, P, f.nc0);
        m0 = n1;
        s0 = f.shape + (var_category(c, P, f.nc0) * n1) * n1 + q0 % n1;
      }
      if (f.nc1 > 0) {
        const int c = q1 / n1;
        off1 = var_offset(c, P, f.nc1);
        m1 = n1;
        s1 = f.shape + (var_category(c, P, f.nc1) * n1) * n1 + q1 % n1;
      }
      for (int l1 = 0; l1 < m1; ++l1) {
        const double *row = f.u + f.base + (int64_t)(off1 + l1) * f.stride1 + (int64_t)off0 * f.stride0;
        double r = 0.0;
        for (int l0 = 0; l0 < m0; ++l0) r += (s0 ? s0[l0 * n1] : 1.0) * row[(int64_t)l0 * f.stride0];
        upw += (s1 ? s1[l1 * n1] : 1.0) * r;
      }
    }
  } else if (f.bc) {
    upw = f.bc[idx];
  }
  f.G[idx] = -an * upw;
}

// T[q1][i0] = sum over the points q0 of node i0: w0 G
__global__ __launch_bounds__(256) void var_face_t0_kernel(const gdmk::VarFaceArgs f) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)f.n0 * f.Q1) return;
  const int i0 = (int)(idx % f.n0), q1 = (int)(idx / f.n0);
  const double *g = f.G + (int64_t)q1 * f.Q0 + f.qs0[i0];
  const double *w = f.w0 + (int64_t)i0 * f.wmax0;
  const int m = f.qc0[i0];
  double s = 0.0;
  for (int k = 0; k < m; ++k) s += w[k] * g[k];
  f.T[idx] = s;
}

// dst[node (i0, i1)] += sum over the points q1 of node i1: w1 T
__global__ __launch_bounds__(256) void var_face_t1_kernel(const gdmk::VarFaceArgs f) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)f.n0 * f.n1) return;
  const int i0 = (int)(idx % f.n0), i1 = (int)(idx / f.n0);
  const double *t = f.T + (int64_t)f.qs1[i1] * f.n0 + i0;
  const double *w = f.w1 + (int64_t)i1 * f.wmax1;
  const int m = f.qc1[i1];
  double s = 0.0;
  for (int k = 0; k < m; ++k) s += w[k] * t[(int64_t)k * f.n0];
  f.dst[f.base + (int64_t)i0 * f.stride0 + (int64_t)i1 * f.stride1] += s;
}

std::atomic<size_t> g_lds_max{0};

}  // namespace


extern "C" {

hipError_t GDM_PART_NAME(gdmk_var_prepare_p)(size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;  // within the default limit
  // the limit is a property of the kernel, shared by every operator: keep the
  // largest request (set again on every call, so on every device that asks)
  size_t prev = g_lds_max.load();
  while (prev < lds && !g_lds_max.compare_exchange_weak(prev, lds)) {
  }
  return hipFuncSetAttribute((const void *)var_volume_kernel<GDM_PART>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)g_lds_max.load());
}

hipError_t GDM_PART_NAME(gdmk_var_volume_p)(const gdmk::VarArgs &a, size_t lds, hipStream_t st) {
  if (a.Nx <= 0 || a.Ny <= 0 || a.Nz <= 0) return hipSuccess;
  const dim3 grid((a.Nx + VAR_TX - 1) / VAR_TX, (a.Ny + VAR_TY - 1) / VAR_TY, (a.Nz + VAR_ZC - 1) / VAR_ZC);
  if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(var_volume_kernel<GDM_PART>, grid, dim3(VAR_THREADS), lds, st, a);
  return hipGetLastError();
}

hipError_t GDM_PART_NAME(gdmk_var_face_p)(const gdmk::VarFaceArgs &f, hipStream_t st) {
  auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
  const int64_t npts = (int64_t)f.Q0 * f.Q1, nT = (int64_t)f.n0 * f.Q1, nn = (int64_t)f.n0 * f.n1;
  if (npts <= 0 || nn <= 0) return hipSuccess;
  hipLaunchKernelGGL(var_face_points_kernel<GDM_PART>, blocks(npts), dim3(256), 0, st, f);
  hipLaunchKernelGGL(var_face_t0_kernel, blocks(nT), dim3(256), 0, st, f);
  hipLaunchKernelGGL(var_face_t1_kernel, blocks(nn), dim3(256), 0, st, f);
  return hipGetLastError();
}

}  // extern "C"
