// gdm_coefgrid.hip -- the wave / heat / Poisson operator with a general
// coefficient kappa on the tensor Gauss grid (gdm_op_set_coefficient_grid;
// DESIGN.md "Grid coefficient").
//
// One unit per degree, -DGDM_PART=<p>, next to the unit of the
// degree-independent kernels (-DGDM_PART=0: the reduction of the set call and
// the box-face part).
//
// Volume part: wave/stiffness.h:171-181 with JxW multiplied by kappa at the
// quadrature point, as sweeps over the whole grid instead of a cell loop:
//   K u = - sum_e G_e^T diag(w kappa) G_e u,  G_e = (x)_d (D_d if d == e else B_d).
//   * a workgroup owns a TX x TY tile of nodes and ZC node planes and marches
//     the z Gauss planes whose boxes reach those planes;
//   * per Gauss plane: (1) the z contraction on the tile's nodes and halo, value
//     and derivative, from the p + 1 node planes of the cell layer's box;
//     (2) the x sweep to the tile's quadrature columns: d/dx, value, d/dz;
//     (3) per quadrature column and component one thread marches the y Gauss
//     points: forward y contraction over the cell's p + 1 node rows (held in
//     registers per cell), times -w kappa streamed from kq, and the transposed
//     y contraction into a register ring of the box's p + 1 node rows, written
//     back in place once the boxes have moved past a row; (4) one thread per
//     node gathers the transposed x sweep and adds the plane into a register
//     ring of the p + 1 node planes of the box.
//   * the footprint's y tables and box offsets are staged in LDS once per
//     workgroup (broadcast reads: a component's columns fill whole waves);
//     kappa of the next cell is in flight while a cell is processed; the z
//     and x sweeps issue their loads together: rows and columns past the
//     extent of a trivial axis carry zero weights and are read clamped.
// Gather form throughout: every sum is formed by one thread in a fixed order,
// no atomics; the bits do not depend on the launch.  The guards on node indices
// make trivial axes (N = Q = 1) and partial tiles run the same code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_coefgrid.h"

#ifndef GDM_PART
#error "gdm_coefgrid.hip is compiled per degree: -DGDM_PART=<p> (0: the degree-independent kernels)"
#endif

#if GDM_PART == 0

namespace {

constexpr int RED_THREADS = 256;

__global__ __launch_bounds__(RED_THREADS) void cg_reduce_kernel(const double *__restrict__ k, int64_t n,
                                                                const gdmk::CgAxis *__restrict__ ax,
                                                                double *__restrict__ partial,
                                                                double *__restrict__ bad) {
  __shared__ double ss[RED_THREADS], sb[RED_THREADS];
  double s = 0.0, b = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * RED_THREADS) {
    const double v = k[i];
    double w = 1.0;
    if (ax) {
      const int64_t r = i / ax[0].Q;
      w = ax[0].w[i - r * ax[0].Q] * ax[1].w[r % ax[1].Q] * ax[2].w[r / ax[1].Q];
    }
    if (!(v > 0.0) || !(v < 1.7e308))
      b += 1.0;
    else
      s += w * v;
  }
  ss[threadIdx.x] = s;
  sb[threadIdx.x] = b;
  __syncthreads();
  for (int o = RED_THREADS / 2; o > 0; o /= 2) {
    if ((int)threadIdx.x < o) {
      ss[threadIdx.x] += ss[threadIdx.x + o];
      sb[threadIdx.x] += sb[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = ss[0];
    bad[blockIdx.x] = sb[0];
  }
}

// Box face, step 1: at every face Gauss point the wall trace U and the normal
// derivative D of u, times kappa: av = kappa (D - gamma U), adv = kappa U
// (wave/stiffness.h:296-310; the face JxW is in step 2's weights).
__global__ __launch_bounds__(256) void cg_face_eval_kernel(gdmk::CgFace F, const double *__restrict__ u,
                                                           const double *__restrict__ kbc,
                                                           double *__restrict__ scratch) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nq = (int64_t)F.Q0 * F.Q1;
  if (id >= nq) return;
  const int q0 = (int)(id % F.Q0), q1 = (int)(id / F.Q0);
  const int f0 = F.first0[q0], f1 = F.first1[q1];
  double U = 0.0, D = 0.0;
  for (int b = 0; b < F.nk; ++b) {
    const int i1 = f1 + b;
    if (i1 >= F.n1) break;
    for (int a = 0; a < F.nk; ++a) {
      const int i0 = f0 + a;
      if (i0 >= F.n0) break;
      const double *un = u + F.base + i0 * F.stride0 + i1 * F.stride1;
      double uw = 0.0, dn = 0.0;
      for (int k = 0; k < F.nk; ++k) {
        const double v = un[k * F.stride_d];
        uw = fma(F.tr[k], v, uw);
        dn = fma(F.dk[k], v, dn);
      }
      const double c = F.val1[q1 * F.nk + b] * F.val0[q0 * F.nk + a];
      U = fma(c, uw, U);
      D = fma(c, dn, D);
    }
  }
  const double kap = kbc[F.goff + id];
  scratch[id] = kap * (D - F.gamma * U);
  scratch[nq + id] = kap * U;
}

// step 2: the face-JxW-weighted projection of av and adv onto face node
// (i0, i1), then dst[node + k stride_d] += tr_k Pv + dk_k Pdv on the p + 1
// planes behind the wall.  One thread per face node, faces one after the other.
__global__ __launch_bounds__(256) void cg_face_add_kernel(gdmk::CgFace F, const double *__restrict__ scratch,
                                                          double *__restrict__ dst) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nq = (int64_t)F.Q0 * F.Q1;
  if (id >= (int64_t)F.n0 * F.n1) return;
  const int i0 = (int)(id % F.n0), i1 = (int)(id / F.n0);
  const int s0 = F.qs0[i0], m0 = F.qc0[i0], s1 = F.qs1[i1], m1 = F.qc1[i1];
  const double *w0 = F.w0 + (size_t)i0 * F.wmax0, *w1 = F.w1 + (size_t)i1 * F.wmax1;
  double Pv = 0.0, Pd = 0.0;
  for (int b = 0; b < m1; ++b) {
    const double *row = scratch + (int64_t)(s1 + b) * F.Q0 + s0;
    double rv = 0.0, rd = 0.0;
    for (int a = 0; a < m0; ++a) {
      rv = fma(w0[a], row[a], rv);
      rd = fma(w0[a], row[nq + a], rd);
    }
    Pv = fma(w1[b], rv, Pv);
    Pd = fma(w1[b], rd, Pd);
  }
  double *o = dst + F.base + i0 * F.stride0 + i1 * F.stride1;
  for (int k = 0; k < F.nk; ++k) o[k * F.stride_d] += F.tr[k] * Pv + F.dk[k] * Pd;
}

}  // namespace

extern "C" hipError_t gdmk_cg_reduce(const double *k, int64_t n, const gdmk::CgAxis *ax, double *partial, double *bad,
                                     int blocks, hipStream_t st) {
  hipLaunchKernelGGL(cg_reduce_kernel, dim3((unsigned)blocks), dim3(RED_THREADS), 0, st, k, n, ax, partial, bad);
  return hipGetLastError();
}

extern "C" hipError_t gdmk_cg_face(const gdmk::CgFace &F, const double *u, const double *kbc, double *scratch,
                                   double *dst, hipStream_t st) {
  const int64_t nq = (int64_t)F.Q0 * F.Q1, nn = (int64_t)F.n0 * F.n1;
  hipLaunchKernelGGL(cg_face_eval_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, F, u, kbc, scratch);
  hipLaunchKernelGGL(cg_face_add_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, F, scratch, dst);
  return hipGetLastError();
}

#else  // GDM_PART > 0

namespace {

template <int P>
__global__ __launch_bounds__(gdmk::cg_threads(P)) void cg_kernel(const gdmk::CgArgs a) {
  constexpr int N1 = P + 1, TX = gdmk::cg_tx(P), TY = gdmk::cg_ty(P), ZC = gdmk::cg_zc(P);
  constexpr int NT = gdmk::cg_threads(P), SX = gdmk::cg_sx(P), SY = gdmk::cg_sy(P), NQ = gdmk::cg_nqx(P);
  constexpr int CW = gdmk::cg_cw(P), NQY = gdmk::cg_nqy(P);
  constexpr bool XT = gdmk::cg_xt(P);
  static_assert(TX * TY <= NT, "one thread per node of the tile");
  extern __shared__ double lds[];
  double *A = lds;            // [SY][SX] z contraction with values
  double *B = A + SY * SX;    // [SY][SX] z contraction with derivatives
  double *X = B + SY * SX;    // [3][SY][NQ] x sweeps: d/dx, value, d/dz; after step 3 their y-transposed results
  double *YV = X + 3 * SY * NQ;  // [NQY][N1] y basis values of the tile's footprint
  double *YD = YV + NQY * N1;    // [NQY][N1] y derivatives
  double *YW = YD + NQY * N1;    // [NQY] y weights
  double *XV = YW + NQY;         // [NQ][N1] x basis values of the tile's footprint (XT: degrees that have the LDS)
  double *XD = XV + (XT ? NQ * N1 : 0);  // [NQ][N1] x derivatives
  int *FX = reinterpret_cast<int *>(XD + (XT ? NQ * N1 : 0));  // [NQ] first node of the x footprint's points, relative to nx0
  int *FY = FX + NQ;                            // [NQY] the same along y, relative to ny0
  const int tid = threadIdx.x;
  const gdmk::CgAxis ax = a.ax[0], ay = a.ax[1], az = a.ax[2];
  const int Nx = ax.N, Ny = ay.N, Nz = az.N;
  const int X0 = blockIdx.x * TX, Y0 = blockIdx.y * TY, z0 = blockIdx.z * ZC;
  const int xl = min(X0 + TX, Nx) - 1, yl = min(Y0 + TY, Ny) - 1, z1 = min(z0 + ZC, Nz);
  // quadrature footprint and node halo of the tile
  const int qx0 = ax.qlo[X0], qx1 = ax.qhi[xl], nqx = qx1 - qx0;
  const int qy0 = ay.qlo[Y0], qy1 = ay.qhi[yl];
  const int qz0 = az.qlo[z0], qz1 = az.qhi[z1 - 1];
  const int nx0 = ax.first[qx0], sx = min(ax.first[qx1 - 1] + P, Nx - 1) - nx0 + 1;
  const int ny0 = ay.first[qy0], sy = min(ay.first[qy1 - 1] + P, Ny - 1) - ny0 + 1;
  const int nqy = qy1 - qy0;
  if (nqx > NQ || nqy > NQY || sx > SX || sy > SY) return;  // checked on the host when the coefficient is set; block-uniform
  // the footprint's y tables and box offsets, once per workgroup (the first barrier of the march orders them)
  for (int e = tid; e < nqy * N1; e += NT) {
    YV[e] = ay.val[(size_t)qy0 * N1 + e];
    YD[e] = ay.der[(size_t)qy0 * N1 + e];
  }
  for (int e = tid; e < nqy; e += NT) {
    YW[e] = ay.w[qy0 + e];
    FY[e] = ay.first[qy0 + e] - ny0;
  }
  for (int e = tid; e < nqx; e += NT) FX[e] = ax.first[qx0 + e] - nx0;
  if (XT)
    for (int e = tid; e < nqx * N1; e += NT) {
      XV[e] = ax.val[(size_t)qx0 * N1 + e];
      XD[e] = ax.der[(size_t)qx0 * N1 + e];
    }
  // the x tables of the footprint: staged, or read from global memory through the same pointers
  const double *xvt = XT ? XV : ax.val + (size_t)qx0 * N1, *xdt = XT ? XD : ax.der + (size_t)qx0 * N1;

  const int ix = tid % TX, iy = tid / TX, nx = X0 + ix, ny = Y0 + iy;
  const bool valid = tid < TX * TY && nx <= xl && ny <= yl;
  const int qa = valid ? ax.qlo[nx] : 0, qb = valid ? ax.qhi[nx] : 0;
  const int64_t plane = (int64_t)Nx * Ny, node_xy = (int64_t)ny * Nx + nx;

  double ring[N1];  // partial sums of the node planes off_cur .. off_cur + P
#pragma unroll
  for (int k = 0; k < N1; ++k) ring[k] = 0.0;
  int off_cur = az.first[qz0];

  for (int qz = qz0; qz < qz1; ++qz) {
    const int fz = az.first[qz];
    while (fz > off_cur) {  // the boxes moved on: the lowest plane is complete
      if (valid && off_cur >= z0 && off_cur < z1) a.dst[node_xy + plane * off_cur] = ring[0];
#pragma unroll
      for (int k = 0; k < P; ++k) ring[k] = ring[k + 1];
      ring[P] = 0.0;
      ++off_cur;
    }
    double vz[N1], dz[N1];
#pragma unroll
    for (int k = 0; k < N1; ++k) {
      vz[k] = az.val[(size_t)qz * N1 + k];
      dz[k] = az.der[(size_t)qz * N1 + k];
    }
    // (1) z contraction on the tile's nodes and halo; a plane past the extent (a trivial axis) has zero
    // weights: it is read at the last plane instead
    for (int e = tid; e < sy * sx; e += NT) {
      const int r = e / sx, c = e - r * sx;
      const double *s = a.src + plane * fz + (int64_t)(ny0 + r) * Nx + nx0 + c;
      double v[N1];
#pragma unroll
      for (int k = 0; k < N1; ++k) v[k] = s[plane * min(k, Nz - 1 - fz)];
      double sa = 0.0, sb = 0.0;
#pragma unroll
      for (int k = 0; k < N1; ++k) {
        sa = fma(vz[k], v[k], sa);
        sb = fma(dz[k], v[k], sb);
      }
      A[r * SX + c] = sa;
      B[r * SX + c] = sb;
    }
    __syncthreads();
    // (2) x sweep: node rows to quadrature columns
    for (int e = tid; e < sy * nqx; e += NT) {
      const int r = e / nqx, j = e - r * nqx;
      const int c0 = FX[j];
      double vx[N1], dx[N1];
#pragma unroll
      for (int i = 0; i < N1; ++i) {
        vx[i] = xvt[j * N1 + i];
        dx[i] = xdt[j * N1 + i];
      }
      double xd = 0.0, xv = 0.0, zv = 0.0;
#pragma unroll
      for (int i = 0; i < N1; ++i) {  // a column past the extent (a trivial axis) has zero weights
        const int c = min(c0 + i, sx - 1);
        const double va = A[r * SX + c], vb = B[r * SX + c];
        xd = fma(dx[i], va, xd);
        xv = fma(vx[i], va, xv);
        zv = fma(vx[i], vb, zv);
      }
      X[(0 * SY + r) * NQ + j] = xd;
      X[(1 * SY + r) * NQ + j] = xv;
      X[(2 * SY + r) * NQ + j] = zv;
    }
    __syncthreads();
    // (3) per column and component: y forward, times -w kappa, y transposed, in place
    {
      const double wz = az.w[qz];
      for (int item = tid; item < 3 * CW; item += NT) {
        const int comp = __builtin_amdgcn_readfirstlane(item / CW), j = item % CW;
        if (j >= nqx) continue;
        const double *ty = comp == 1 ? YD : YV;
        double *Xc = X + (size_t)comp * SY * NQ + j;
        const double wxz = -ax.w[qx0 + j] * wz;
        const double *kp = a.kq + ((int64_t)qz * ay.Q + qy0) * ax.Q + qx0 + j;
        const int64_t ks = ax.Q;
        const int nq = ay.Q == 1 ? 1 : N1;  // points per cell (a trivial axis: its one point)
        double acc[N1], xin[N1], kk[N1], kn[N1];
#pragma unroll
        for (int k = 0; k < N1; ++k) acc[k] = 0.0;
        // kappa of the first cell; the next cell's is in flight while a cell is processed
#pragma unroll
        for (int q = 0; q < N1; ++q) kn[q] = kp[ks * min(q, nqy - 1)];
        int off = 0;  // rows relative to ny0
        for (int jc = 0; jc < nqy; jc += nq) {
#pragma unroll
          for (int q = 0; q < N1; ++q) kk[q] = kn[q];
#pragma unroll
          for (int q = 0; q < N1; ++q) kn[q] = kp[ks * min(jc + nq + q, nqy - 1)];
          const int fy = FY[jc];
          while (fy > off) {
            Xc[off * NQ] = acc[0];
#pragma unroll
            for (int k = 0; k < P; ++k) acc[k] = acc[k + 1];
            acc[P] = 0.0;
            ++off;
          }
#pragma unroll
          for (int k = 0; k < N1; ++k) xin[k] = Xc[min(fy + k, sy - 1) * NQ];  // rows past the extent: zero weights
#pragma unroll
          for (int q = 0; q < N1; ++q) {
            if (q < nq) {
              const double *t = ty + (jc + q) * N1;
              double g = 0.0;
#pragma unroll
              for (int k = 0; k < N1; ++k) g = fma(t[k], xin[k], g);
              const double f = wxz * YW[jc + q] * kk[q] * g;
#pragma unroll
              for (int k = 0; k < N1; ++k) acc[k] = fma(t[k], f, acc[k]);
            }
          }
        }
#pragma unroll
        for (int k = 0; k < N1; ++k)
          if (off + k < sy) Xc[(off + k) * NQ] = acc[k];
      }
    }
    __syncthreads();
    // (4) x transposed, one thread per node, and the z transposed into the ring
    if (valid) {
      const int r = ny - ny0;
      const double *R0 = X + (0 * SY + r) * NQ - qx0, *R1 = X + (1 * SY + r) * NQ - qx0,
                   *R2 = X + (2 * SY + r) * NQ - qx0;
      double an = 0.0, bn = 0.0;
      for (int q = qa; q < qb; ++q) {
        const int k = nx - nx0 - FX[q - qx0];
        const double v = xvt[(q - qx0) * N1 + k], d = xdt[(q - qx0) * N1 + k];
        an = fma(d, R0[q], an);
        an = fma(v, R1[q], an);
        bn = fma(v, R2[q], bn);
      }
#pragma unroll
      for (int k = 0; k < N1; ++k) ring[k] = fma(vz[k], an, fma(dz[k], bn, ring[k]));
    }
    // the next plane's step 1 writes A / B only; its barrier orders step 4 before the next step 2
  }
  if (valid) {
#pragma unroll
    for (int k = 0; k < N1; ++k) {
      const int zp = off_cur + k;
      if (zp >= z0 && zp < z1) a.dst[node_xy + plane * zp] = ring[k];
    }
  }
}

}  // namespace


extern "C" {

hipError_t GDM_PART_NAME(gdmk_cg_prepare_p)(void) {
  constexpr size_t lds = gdmk::cg_lds(GDM_PART);
  if (lds <= 64 * 1024) return hipSuccess;  // within the default limit
  return hipFuncSetAttribute((const void *)cg_kernel<GDM_PART>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)lds);
}

hipError_t GDM_PART_NAME(gdmk_cg_apply_p)(const gdmk::CgArgs &a, hipStream_t st) {
  constexpr int P = GDM_PART, TX = gdmk::cg_tx(P), TY = gdmk::cg_ty(P), ZC = gdmk::cg_zc(P);
  const int Nx = a.ax[0].N, Ny = a.ax[1].N, Nz = a.ax[2].N;
  if (Nx <= 0 || Ny <= 0 || Nz <= 0) return hipSuccess;
  const dim3 grid((Nx + TX - 1) / TX, (Ny + TY - 1) / TY, (Nz + ZC - 1) / ZC);
  if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cg_kernel<P>, grid, dim3(gdmk::cg_threads(P)), gdmk::cg_lds(P), st, a);
  return hipGetLastError();
}

}  // extern "C"

#endif
