// gdm_massgrid.hip -- the mass matrix weighted by a general density rho on the
// tensor Gauss grid (gdm_op_set_density_grid; DESIGN.md "Grid density").
//
// One unit per degree, -DGDM_PART=<p>, next to the unit of the
// degree-independent kernel (-DGDM_PART=0: W^-1/2 of the preconditioner).
//
// wave/mass.h:47-249 with JxW multiplied by rho at the quadrature point, as
// sweeps over the whole grid instead of a cell loop:
//   M[rho] u = (B_z (x) B_y (x) B_x)^T diag(w rho) (B_z (x) B_y (x) B_x) u.
//   * a workgroup owns a TX x TY tile of nodes and ZC node planes and marches
//     the z Gauss planes whose boxes reach those planes;
//   * per Gauss plane: (1) the z contraction on the tile's nodes and halo from
//     the p + 1 node planes of the cell layer's box; (2) the x sweep to the
//     tile's quadrature columns; (3) per quadrature column one thread marches
//     the y Gauss points: forward y contraction over the cell's p + 1 node rows,
//     times w rho streamed from rq (MG_AHEAD cells in flight, the first of them
//     loaded before step 1), and the transposed y contraction into a
//     register ring of the box's p + 1 node rows, written back in place once the
//     boxes have moved past a row; (4) one thread per node gathers the
//     transposed x sweep and adds the plane into a register ring of the p + 1
//     node planes of the box.
//   * one node plane and one sweep plane in LDS (the stiffness form of
//     gdm_coefgrid.hip needs two and three): two or three workgroups share a CU
//     and fill the lanes that the column march of step 3 leaves idle.
//   * the diagonal (DIAG) is the transposed half alone with squared tables:
//     steps 1 and 2 fall away and step 3 spreads w rho itself.
// Gather form throughout: every sum is formed by one thread in a fixed order,
// no atomics; the bits do not depend on the launch.  The guards on node indices
// make trivial axes (N = Q = 1) and partial tiles run the same code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_massgrid.h"

#ifndef GDM_PART
#error "gdm_massgrid.hip is compiled per degree: -DGDM_PART=<p> (0: the degree-independent kernel)"
#endif

#if GDM_PART == 0

namespace {

__global__ __launch_bounds__(256) void mg_wisqrt_kernel(int64_t n, const double *__restrict__ diag,
                                                        const double *__restrict__ mdiag, double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double w = diag[i] / mdiag[i];
  // a density that is not positive is the caller's error: the CG reports the breakdown
  out[i] = w > 0.0 && w < 1.7e308 ? 1.0 / sqrt(w) : 1.0;
}

}  // namespace

extern "C" hipError_t gdmk_mg_wisqrt(int64_t n, const double *diag, const double *mdiag, double *out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(mg_wisqrt_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, diag, mdiag, out);
  return hipGetLastError();
}

#else  // GDM_PART > 0

namespace {

template <int P, bool DIAG>
__global__ __launch_bounds__(gdmk::MG_THREADS) void mg_kernel(const gdmk::MgArgs a) {
  constexpr int N1 = P + 1, TX = gdmk::mg_tx(P), TY = gdmk::mg_ty(P), AH = gdmk::MG_AHEAD;
  constexpr int NT = gdmk::MG_THREADS, SX = gdmk::mg_sx(P), SY = gdmk::mg_sy(P), NQ = gdmk::mg_nqx(P);
  constexpr int NQY = gdmk::mg_nqy(P);
  constexpr bool XT = gdmk::mg_xt(P);
  static_assert(TX * TY <= NT, "one thread per node of the tile");
  extern __shared__ double lds[];
  double *A = lds;             // [SY][SX] z contraction
  double *X = A + SY * SX;     // [SY][NQ] x sweep; after step 3 its y-transposed result
  double *YV = X + SY * NQ;    // [NQY][N1] y basis values of the tile's footprint (DIAG: squared)
  double *YW = YV + NQY * N1;  // [NQY] y weights
  double *XV = YW + NQY;       // [NQ][N1] x basis values of the tile's footprint (XT: degrees that have the LDS)
  int *FX = reinterpret_cast<int *>(XV + (XT ? NQ * N1 : 0));  // [NQ] first node of the x footprint's points, relative to nx0
  int *FY = FX + NQ;                                           // [NQY] the same along y, relative to ny0
  const int tid = threadIdx.x;
  const gdmk::CgAxis ax = a.ax[0], ay = a.ax[1], az = a.ax[2];
  const int Nx = ax.N, Ny = ay.N, Nz = az.N;
  const int X0 = blockIdx.x * TX, Y0 = blockIdx.y * TY, z0 = blockIdx.z * a.zc;
  const int xl = min(X0 + TX, Nx) - 1, yl = min(Y0 + TY, Ny) - 1, z1 = min(z0 + a.zc, Nz);
  // quadrature footprint and node halo of the tile
  const int qx0 = ax.qlo[X0], qx1 = ax.qhi[xl], nqx = qx1 - qx0;
  const int qy0 = ay.qlo[Y0], qy1 = ay.qhi[yl];
  const int qz0 = az.qlo[z0], qz1 = az.qhi[z1 - 1];
  const int nx0 = ax.first[qx0], sx = min(ax.first[qx1 - 1] + P, Nx - 1) - nx0 + 1;
  const int ny0 = ay.first[qy0], sy = min(ay.first[qy1 - 1] + P, Ny - 1) - ny0 + 1;
  const int nqy = qy1 - qy0;
  if (nqx > NQ || nqy > NQY || sx > SX || sy > SY) return;  // checked on the host when the density is set; block-uniform
  // the footprint's y table and box offsets, once per workgroup (the first barrier of the march orders them)
  for (int e = tid; e < nqy * N1; e += NT) {
    const double v = ay.val[(size_t)qy0 * N1 + e];
    YV[e] = DIAG ? v * v : v;
  }
  for (int e = tid; e < nqy; e += NT) {
    YW[e] = ay.w[qy0 + e];
    FY[e] = ay.first[qy0 + e] - ny0;
  }
  for (int e = tid; e < nqx; e += NT) FX[e] = ax.first[qx0 + e] - nx0;
  if (XT)
    for (int e = tid; e < nqx * N1; e += NT) XV[e] = ax.val[(size_t)qx0 * N1 + e];
  // the x table of the footprint: staged, or read from global memory through the same pointer
  const double *xvt = XT ? XV : ax.val + (size_t)qx0 * N1;

  const int ix = tid % TX, iy = tid / TX, nx = X0 + ix, ny = Y0 + iy;
  const bool valid = tid < TX * TY && nx <= xl && ny <= yl;
  const int qa = valid ? ax.qlo[nx] : 0, qb = valid ? ax.qhi[nx] : 0;
  const int64_t plane = (int64_t)Nx * Ny, node_xy = (int64_t)ny * Nx + nx;
  auto store = [&](int zp, double v) {
    const int64_t i = node_xy + plane * zp;
    a.dst[i] = (!DIAG && a.add) ? fma(a.c, a.add[i], v) : v;
  };

  double ring[N1];  // partial sums of the node planes off_cur .. off_cur + P
#pragma unroll
  for (int k = 0; k < N1; ++k) ring[k] = 0.0;
  int off_cur = az.first[qz0];

  for (int qz = qz0; qz < qz1; ++qz) {
    const int fz = az.first[qz];
    while (fz > off_cur) {  // the boxes moved on: the lowest plane is complete
      if (valid && off_cur >= z0 && off_cur < z1) store(off_cur, ring[0]);
#pragma unroll
      for (int k = 0; k < P; ++k) ring[k] = ring[k + 1];
      ring[P] = 0.0;
      ++off_cur;
    }
    double vz[N1];
#pragma unroll
    for (int k = 0; k < N1; ++k) {
      const double v = az.val[(size_t)qz * N1 + k];
      vz[k] = DIAG ? v * v : v;
    }
    // rho of the column's first AH cells, in flight across steps 1 and 2; the march keeps AH cells in flight
    const int nq = ay.Q == 1 ? 1 : N1;  // points per cell (a trivial axis: its one point)
    const double *kp = a.rq + ((int64_t)qz * ay.Q + qy0) * ax.Q + qx0 + min(tid, nqx - 1);
    const int64_t ks = ax.Q;
    double kn[AH][N1];
    if (tid < nqx) {  // the lanes that march in step 3
#pragma unroll
      for (int d = 0; d < AH; ++d)
#pragma unroll
        for (int q = 0; q < N1; ++q) kn[d][q] = kp[ks * min(d * nq + q, nqy - 1)];
    }
    if (!DIAG) {
      // (1) z contraction on the tile's nodes and halo; a plane past the extent (a trivial axis) has zero
      // weight: it is read at the last plane instead
      for (int e = tid; e < sy * sx; e += NT) {
        const int r = e / sx, c = e - r * sx;
        const double *s = a.src + plane * fz + (int64_t)(ny0 + r) * Nx + nx0 + c;
        double v[N1];
#pragma unroll
        for (int k = 0; k < N1; ++k) v[k] = s[plane * min(k, Nz - 1 - fz)];
        double sa = 0.0;
#pragma unroll
        for (int k = 0; k < N1; ++k) sa = fma(vz[k], v[k], sa);
        A[r * SX + c] = sa;
      }
      __syncthreads();
      // (2) x sweep: node rows to quadrature columns
      for (int e = tid; e < sy * nqx; e += NT) {
        const int r = e / nqx, j = e - r * nqx;
        const int c0 = FX[j];
        double xv = 0.0;
#pragma unroll
        for (int i = 0; i < N1; ++i)  // a column past the extent (a trivial axis) has zero weight
          xv = fma(xvt[j * N1 + i], A[r * SX + min(c0 + i, sx - 1)], xv);
        X[r * NQ + j] = xv;
      }
    }
    __syncthreads();  // DIAG: step 4 of the plane before has read X
    // (3) per column: y forward, times w rho, y transposed, in place
    if (tid < nqx) {
      const int j = tid;
      double *Xc = X + j;
      const double wxz = ax.w[qx0 + j] * az.w[qz];
      double acc[N1], xin[N1], kk[N1];
#pragma unroll
      for (int k = 0; k < N1; ++k) acc[k] = 0.0;
      int off = 0;  // rows relative to ny0
      for (int jc0 = 0; jc0 < nqy; jc0 += AH * nq) {
#pragma unroll
        for (int d = 0; d < AH; ++d) {
          const int jc = jc0 + d * nq;
          if (jc >= nqy) break;
#pragma unroll
          for (int q = 0; q < N1; ++q) kk[q] = kn[d][q];
#pragma unroll
          for (int q = 0; q < N1; ++q) kn[d][q] = kp[ks * min(jc + AH * nq + q, nqy - 1)];
          const int fy = FY[jc];
          while (fy > off) {
            Xc[off * NQ] = acc[0];
#pragma unroll
            for (int k = 0; k < P; ++k) acc[k] = acc[k + 1];
            acc[P] = 0.0;
            ++off;
          }
          if (!DIAG) {
#pragma unroll
            for (int k = 0; k < N1; ++k) xin[k] = Xc[min(fy + k, sy - 1) * NQ];  // rows past the extent: zero weight
          }
#pragma unroll
          for (int q = 0; q < N1; ++q) {
            if (q < nq) {
              const double *t = YV + (jc + q) * N1;
              double g = 1.0;
              if (!DIAG) {
                g = 0.0;
#pragma unroll
                for (int k = 0; k < N1; ++k) g = fma(t[k], xin[k], g);
              }
              const double f = wxz * YW[jc + q] * kk[q] * g;
#pragma unroll
              for (int k = 0; k < N1; ++k) acc[k] = fma(t[k], f, acc[k]);
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < N1; ++k)
        if (off + k < sy) Xc[(off + k) * NQ] = acc[k];
    }
    __syncthreads();
    // (4) x transposed, one thread per node, and the z transposed into the ring
    if (valid) {
      const double *R = X + (ny - ny0) * NQ - qx0;
      double an = 0.0;
      for (int q = qa; q < qb; ++q) {
        const double v = xvt[(q - qx0) * N1 + (nx - nx0 - FX[q - qx0])];
        an = fma(DIAG ? v * v : v, R[q], an);
      }
#pragma unroll
      for (int k = 0; k < N1; ++k) ring[k] = fma(vz[k], an, ring[k]);
    }
    // the next plane's step 1 writes A only; its barrier orders step 4 before the next step 2
  }
  if (valid) {
#pragma unroll
    for (int k = 0; k < N1; ++k) {
      const int zp = off_cur + k;
      if (zp >= z0 && zp < z1) store(zp, ring[k]);
    }
  }
}

template <bool DIAG>
hipError_t mg_launch(const gdmk::MgArgs &a, hipStream_t st) {
  constexpr int P = GDM_PART, TX = gdmk::mg_tx(P), TY = gdmk::mg_ty(P);
  const int Nx = a.ax[0].N, Ny = a.ax[1].N, Nz = a.ax[2].N;
  if (Nx <= 0 || Ny <= 0 || Nz <= 0) return hipSuccess;
  if (a.zc < 1 || a.zc > gdmk::mg_zc(P)) return hipErrorInvalidValue;
  const dim3 grid((Nx + TX - 1) / TX, (Ny + TY - 1) / TY, (Nz + a.zc - 1) / a.zc);
  if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL((mg_kernel<P, DIAG>), grid, dim3(gdmk::MG_THREADS), gdmk::mg_lds(P), st, a);
  return hipGetLastError();
}

}  // namespace


extern "C" {

hipError_t GDM_PART_NAME(gdmk_mg_prepare_p)(void) {
  constexpr size_t lds = gdmk::mg_lds(GDM_PART);
  if (lds <= 64 * 1024) return hipSuccess;  // within the default limit
  hipError_t e = hipFuncSetAttribute((const void *)mg_kernel<GDM_PART, false>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute((const void *)mg_kernel<GDM_PART, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)lds);
}

hipError_t GDM_PART_NAME(gdmk_mg_apply_p)(const gdmk::MgArgs &a, hipStream_t st) { return mg_launch<false>(a, st); }

hipError_t GDM_PART_NAME(gdmk_mg_diag_p)(const gdmk::MgArgs &a, hipStream_t st) { return mg_launch<true>(a, st); }

}  // extern "C"

#endif
