// gdm_evalgrid.hip -- a GDM field on the tensor Gauss grid and back (DESIGN.md
// "Grid evaluation"): what FEValues::get_function_values / get_function_gradients
// give the reference's cell loops (wave/stiffness.h:151-203,
// advection/problem.h:330-425), for the whole mesh at once.
//
// One unit per degree, -DGDM_PART=<p>, next to the unit of the
// degree-independent trace kernel (-DGDM_PART=0).
//
// Evaluation (ev_kernel): sum factorisation per run of CX cells along x at one
// (cell_y, cell_z).  The node rows of the run's DoF boxes are staged in LDS
// once; per z Gauss point the rows are contracted along z (values, derivatives)
// and along y into the three rows (B_z, B_y), (D_z, B_y), (B_z, D_y); then one
// thread per pair of neighbouring x points contracts x with B_x on all three
// and with D_x on the first: u, du/dx, du/dy, du/dz.  The pair is one 16-byte
// store per output where the alignment allows; the lanes of a wave write one
// contiguous run of a Gauss row.  MODE (values, gradients, both) is a template
// parameter: an output that is not asked for costs neither FMAs nor bytes.
// Trivial axes (2D, 1D) run the same code through their N = Q = 1 tables.
//
// Flux load (ev_flux_kernel): gdm_load.hip's load_kernel with, per direction e,
// the derivative table along e and the value tables elsewhere, the dim
// contributions summed into the same register ring inside one launch.  Gather
// form: one thread per node, cells and directions in ascending order, no
// atomics.
//
// Every output value is formed by one thread in a fixed order and stored once:
// the bits do not depend on the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_evalgrid.h"

#ifndef GDM_PART
#error "gdm_evalgrid.hip is compiled per degree: -DGDM_PART=<p> (0: the degree-independent kernels)"
#endif

#if GDM_PART == 0

namespace {

// cg_face_eval_kernel (gdm_coefgrid.hip) without kappa: the wall trace U and
// the outward normal derivative D of u at the face's Gauss points, written at
// the face's block(0) offset
__global__ __launch_bounds__(256) void ev_trace_kernel(gdmk::EvFace F, const double *__restrict__ u,
                                                       double *__restrict__ u_bc, double *__restrict__ dn_bc) {
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
  if (u_bc) u_bc[F.goff + id] = U;
  if (dn_bc) dn_bc[F.goff + id] = D;
}

}  // namespace

extern "C" hipError_t gdmk_ev_trace(const gdmk::EvFace &F, const double *u, double *u_bc, double *dn_bc,
                                    hipStream_t st) {
  const int64_t nq = (int64_t)F.Q0 * F.Q1;
  if (nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(ev_trace_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, F, u, u_bc, dn_bc);
  return hipGetLastError();
}

#else  // GDM_PART > 0

namespace {

// MODE: 1 values, 2 gradients, 3 both
template <int P, int MODE>
__global__ __launch_bounds__(gdmk::EV_THREADS) void ev_kernel(const gdmk::EvArgs a) {
  constexpr int N1 = P + 1, CX = gdmk::ev_cx(P), W = CX + P, NQ = CX * N1, NT = gdmk::EV_THREADS;
  constexpr bool VAL = (MODE & 1) != 0, GRAD = (MODE & 2) != 0;
  extern __shared__ double lds[];
  double *A = lds;            // [N1][N1][W] node rows of the run's boxes
  double *Bv = A + N1 * N1 * W;  // [N1][W] z contraction with values
  double *Bd = Bv + N1 * W;      // [N1][W] ... with derivatives
  double *R0 = Bd + N1 * W;      // [N1][W] (B_z, B_y), by y Gauss point of the cell
  double *R1 = R0 + N1 * W;      // (D_z, B_y)
  double *R2 = R1 + N1 * W;      // (B_z, D_y)
  double *XV = R2 + N1 * W;      // [NQ][N1] x basis values of the run
  double *XD = XV + NQ * N1;     // [NQ][N1] x derivatives
  int *FX = reinterpret_cast<int *>(XD + NQ * N1);  // [NQ] first node of the point's box, relative to xb
  const int tid = threadIdx.x;
  const gdmk::CgAxis ax = a.ax[0], ay = a.ax[1], az = a.ax[2];
  const int Nx = ax.N, Ny = ay.N, Nz = az.N;
  // points per cell and box rows per direction (a trivial axis: its one point and node)
  const int nqx = ax.Q == 1 ? 1 : N1, nqy = ay.Q == 1 ? 1 : N1, nqz = az.Q == 1 ? 1 : N1;
  const int nby = Ny == 1 ? 1 : N1, nbz = Nz == 1 ? 1 : N1;
  const int ncy = ay.Q / nqy, ncz = az.Q / nqz;
  const int q0 = (int)blockIdx.x * CX * nqx;
  if (q0 >= ax.Q) return;  // block-uniform
  const int nq = min(CX * nqx, ax.Q - q0);
  const int xb = ax.first[q0];
  const int wdt = min(ax.first[q0 + nq - 1] + P, Nx - 1) - xb + 1;
  if (wdt > W) return;  // cannot happen: the boxes move by at most one node per cell; block-uniform
  // the x tables of the run, once per workgroup (the first barriers of the march order them)
  for (int e = tid; e < nq * N1; e += NT) {
    XV[e] = ax.val[(size_t)q0 * N1 + e];
    if (GRAD) XD[e] = ax.der[(size_t)q0 * N1 + e];
  }
  for (int e = tid; e < nq; e += NT) FX[e] = ax.first[q0 + e] - xb;
  const int npairs = (nq + 1) / 2;
  const int64_t Qx = ax.Q, Qy = ay.Q;

  for (int r = (int)blockIdx.y; r < ncy * ncz; r += (int)gridDim.y) {
    const int cy = r % ncy, cz = r / ncy;
    const int qy0 = cy * nqy, qz0 = cz * nqz;
    const int oy = ay.first[qy0], oz = az.first[qz0];
    __syncthreads();  // the previous item's reads of A are done
    // stage the node rows (x contiguous: coalesced)
    for (int i = tid; i < nbz * nby * wdt; i += NT) {
      const int x = i % wdt, yz = i / wdt, iy = yz % nby, iz = yz / nby;
      A[(iz * N1 + iy) * W + x] = a.u[((int64_t)(oz + iz) * Ny + (oy + iy)) * Nx + xb + x];
    }
    __syncthreads();
    for (int qz = 0; qz < nqz; ++qz) {
      const int gz = qz0 + qz;
      const double *vz = az.val + (size_t)gz * N1, *dz = az.der + (size_t)gz * N1;
      // z contraction
      for (int i = tid; i < nby * wdt; i += NT) {
        const int x = i % wdt, iy = i / wdt;
        double sv = 0.0, sd = 0.0;
#pragma unroll
        for (int iz = 0; iz < N1; ++iz)
          if (iz < nbz) {
            const double v = A[(iz * N1 + iy) * W + x];
            sv = fma(vz[iz], v, sv);
            if (GRAD) sd = fma(dz[iz], v, sd);
          }
        Bv[iy * W + x] = sv;
        if (GRAD) Bd[iy * W + x] = sd;
      }
      __syncthreads();
      // y contraction: the three rows of every y Gauss point of the cell
      for (int i = tid; i < nqy * wdt; i += NT) {
        const int x = i % wdt, qy = i / wdt;
        const double *vy = ay.val + (size_t)(qy0 + qy) * N1, *dy = ay.der + (size_t)(qy0 + qy) * N1;
        double r0 = 0.0, r1 = 0.0, r2 = 0.0;
#pragma unroll
        for (int iy = 0; iy < N1; ++iy)
          if (iy < nby) {
            const double bv = Bv[iy * W + x];
            r0 = fma(vy[iy], bv, r0);
            if (GRAD) {
              r1 = fma(vy[iy], Bd[iy * W + x], r1);
              r2 = fma(dy[iy], bv, r2);
            }
          }
        R0[qy * W + x] = r0;
        if (GRAD) {
          R1[qy * W + x] = r1;
          R2[qy * W + x] = r2;
        }
      }
      __syncthreads();
      // x contraction and the stores: one thread per pair of points of a Gauss row
      for (int item = tid; item < nqy * npairs; item += NT) {
        const int j = item % npairs, qy = item / npairs, qa = 2 * j;
        const bool two = qa + 1 < nq;
        const int ox = FX[qa];  // both points lie in one cell (p + 1 is even)
        double w0[N1], w1[N1], w2[N1];
#pragma unroll
        for (int i = 0; i < N1; ++i) {  // a column past the extent (a trivial axis) has zero weights
          const int c = min(ox + i, wdt - 1);
          w0[i] = R0[qy * W + c];
          if (GRAD) {
            w1[i] = R1[qy * W + c];
            w2[i] = R2[qy * W + c];
          }
        }
        double uv[2] = {0.0, 0.0}, gx[2] = {0.0, 0.0}, gy[2] = {0.0, 0.0}, gzv[2] = {0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (t == 1 && !two) break;
          const double *xv = XV + (qa + t) * N1, *xd = XD + (qa + t) * N1;
#pragma unroll
          for (int i = 0; i < N1; ++i) {
            const double v = xv[i];
            if (VAL) uv[t] = fma(v, w0[i], uv[t]);
            if (GRAD) {
              gx[t] = fma(xd[i], w0[i], gx[t]);
              gy[t] = fma(v, w2[i], gy[t]);
              gzv[t] = fma(v, w1[i], gzv[t]);
            }
          }
        }
        const int64_t o = ((int64_t)gz * Qy + (qy0 + qy)) * Qx + q0 + qa;
        const bool vec = a.vec && two;
        auto store = [&](double *out, double v0, double v1) {
          if (!out) return;  // a trivial axis has no derivative
          if (vec) {
            *reinterpret_cast<double2 *>(out + o) = make_double2(v0, v1);
          } else {
            out[o] = v0;
            if (two) out[o + 1] = v1;
          }
        };
        if (VAL) store(a.uq, uv[0], uv[1]);
        if (GRAD) {
          store(a.g[0], gx[0], gx[1]);
          store(a.g[1], gy[0], gy[1]);
          store(a.g[2], gzv[0], gzv[1]);
        }
      }
      // the next z point's barriers order these reads of R before its writes
    }
  }
}

// dst += scale sum_e (d_e v, F_e): load_kernel (gdm_load.hip) once per direction e
// inside the march, the derivative table along e
template <int P>
__global__ void __launch_bounds__(gdmk::LOAD_TX *gdmk::LOAD_TY)
    ev_flux_kernel(gdmk::LoadGeom g, const double *__restrict__ Sw, const double *__restrict__ Dw,
                   const double *__restrict__ Fq, int64_t comp_stride, double scale, double *__restrict__ dst) {
  constexpr int N1 = P + 1, NCAT = P > 1 ? P : 1, NS = NCAT * N1 * N1;
  constexpr int TX = gdmk::LOAD_TX, TY = gdmk::LOAD_TY, NT = TX * TY, R = gdmk::load_rows(P);
  constexpr int QF = gdmk::ev_flux_qf(P);
  static_assert(TX == TY, "the footprint bound QF serves both directions");
  extern __shared__ double lds[];
  double *Sl = lds;          // [NCAT][N1][N1] values times weights
  double *Dl = Sl + NS;      // ... derivatives times weights
  double *F = Dl + NS;       // [R][QF]
  double *T = F + R * QF;    // [QF][TX]
  const int tid = threadIdx.x;
  for (int i = tid; i < NS; i += NT) {
    Sl[i] = Sw[i];
    Dl[i] = Dw[i];
  }

  const int n1x = g.on[0] ? N1 : 1, n1y = g.on[1] ? N1 : 1, n1z = g.on[2] ? N1 : 1;
  const int tiles_x = (g.K[0] + TX - 1) / TX;
  const int X0 = (int)(blockIdx.x % tiles_x) * TX, Y0 = (int)(blockIdx.x / tiles_x) * TY;
  const int z0 = (int)blockIdx.y * gdmk::LOAD_ZC, z1 = min(z0 + gdmk::LOAD_ZC, g.K[2]);
  const int xl = min(X0 + TX, g.K[0]) - 1, yl = min(Y0 + TY, g.K[1]) - 1;  // last nodes of the tile
  // footprint cells
  const int cxf0 = g.on[0] ? gdmk::ld_first(X0, P, g.nc[0]) : 0, cxf1 = g.on[0] ? gdmk::ld_last(xl, P, g.nc[0]) : 0;
  const int cyf0 = g.on[1] ? gdmk::ld_first(Y0, P, g.nc[1]) : 0, cyf1 = g.on[1] ? gdmk::ld_last(yl, P, g.nc[1]) : 0;
  const int czf0 = g.on[2] ? gdmk::ld_first(z0, P, g.nc[2]) : 0, czf1 = g.on[2] ? gdmk::ld_last(z1 - 1, P, g.nc[2]) : 0;
  const int qxb = cxf0 * n1x, nqx = (cxf1 - cxf0 + 1) * n1x;
  const int qyb = cyf0 * n1y, nqy = (cyf1 - cyf0 + 1) * n1y;
  if (nqx > QF || nqy > QF) return;  // cannot happen (the bound of gdm_load.hip); block-uniform

  const int ix = tid % TX, iy = tid / TX;
  const int nx = X0 + ix, ny = Y0 + iy;
  const bool valid = nx < g.K[0] && ny < g.K[1];
  const int cy_a = g.on[1] && valid ? gdmk::ld_first(ny, P, g.nc[1]) : 0;
  const int cy_b = g.on[1] && valid ? gdmk::ld_last(ny, P, g.nc[1]) : 0;

  double ring[N1];
#pragma unroll
  for (int k = 0; k < N1; ++k) ring[k] = 0.0;
  int off_cur = g.on[2] ? gdmk::ld_off(czf0, P, g.nc[2]) : 0;
  const double sj = scale * g.jxw;
  const int64_t node_xy = (int64_t)nx + (int64_t)g.K[0] * ny, plane = (int64_t)g.K[0] * g.K[1];

  for (int cz = czf0; cz <= czf1; ++cz) {
    const int noff = g.on[2] ? gdmk::ld_off(cz, P, g.nc[2]) : 0;
    if (noff > off_cur) {  // the boxes moved one plane on: the lowest plane is complete
      if (valid && off_cur >= z0 && off_cur < z1) dst[node_xy + plane * off_cur] += sj * ring[0];
#pragma unroll
      for (int k = 0; k < P; ++k) ring[k] = ring[k + 1];
      ring[P] = 0.0;
      off_cur = noff;
    }
    const int catz = (g.on[2] ? gdmk::ld_cat(cz, P, g.nc[2]) : 0) * N1 * N1;
    for (int qz = 0; qz < n1z; ++qz) {
      const int64_t gq2 = (int64_t)cz * n1z + qz;
      for (int e = 0; e < 3; ++e) {
        if (!g.on[e]) continue;  // block-uniform
        const double *Fe = Fq + (int64_t)g.rdir[e] * comp_stride;
        const double *Tx = e == 0 ? Dl : Sl, *Ty = e == 1 ? Dl : Sl, *Tz = (e == 2 ? Dl : Sl) + catz;
        const double inv_h = 1.0 / g.h[e];
        // x contraction, R quadrature rows at a time: T[qy][ix] = sum_c sum_q Tx F_e
        for (int r0 = 0; r0 < nqy; r0 += R) {
          const int nr = min(R, nqy - r0);
          __syncthreads();  // the previous strip's reads of F and the previous pass's reads of T are done
          for (int i = tid; i < nr * nqx; i += NT) {
            const int r = i / nqx, j = i - r * nqx;
            const int gq1 = qyb + r0 + r, gq0 = qxb + j;
            F[r * QF + j] = Fe[(gq2 * g.Q[1] + gq1) * (int64_t)g.Q[0] + gq0];
          }
          __syncthreads();
          for (int o = tid; o < nr * TX; o += NT) {
            const int r = o / TX, jx = o % TX, i = X0 + jx;
            if (i >= g.K[0]) continue;
            double s = 0.0;
            if (g.on[0]) {
              const int ca = gdmk::ld_first(i, P, g.nc[0]), cb = gdmk::ld_last(i, P, g.nc[0]);
              for (int c = ca; c <= cb; ++c) {
                const double *Sx = Tx + (gdmk::ld_cat(c, P, g.nc[0]) * N1 + (i - gdmk::ld_off(c, P, g.nc[0]))) * N1;
                const double *Fr = &F[r * QF + (c - cxf0) * N1];
#pragma unroll
                for (int q = 0; q < N1; ++q) s = fma(Sx[q], Fr[q], s);
              }
            } else {
              s = F[r * QF];
            }
            T[(r0 + r) * TX + jx] = s;
          }
        }
        __syncthreads();
        if (valid) {
          double val = 0.0;
          if (g.on[1]) {
            for (int c = cy_a; c <= cy_b; ++c) {
              const double *Sy = Ty + (gdmk::ld_cat(c, P, g.nc[1]) * N1 + (ny - gdmk::ld_off(c, P, g.nc[1]))) * N1;
              const int rb = (c - cyf0) * N1;
#pragma unroll
              for (int q = 0; q < N1; ++q) val = fma(Sy[q], T[(rb + q) * TX + ix], val);
            }
          } else {
            val = T[ix];
          }
          val *= inv_h;
          if (g.on[2]) {
#pragma unroll
            for (int k = 0; k < N1; ++k) ring[k] = fma(Tz[k * N1 + qz], val, ring[k]);
          } else {
            ring[0] += val;
          }
        }
      }
    }
  }
  if (valid) {
#pragma unroll
    for (int k = 0; k < N1; ++k) {
      const int zp = off_cur + k;
      if (k < n1z && zp >= z0 && zp < z1) dst[node_xy + plane * zp] += sj * ring[k];
    }
  }
}

template <int MODE>
void launch_mode(const gdmk::EvArgs &a, hipStream_t st) {
  constexpr int P = GDM_PART, CX = gdmk::ev_cx(P);
  const int nqx = a.ax[0].Q == 1 ? 1 : P + 1;
  const int chunks = (a.ax[0].Q + CX * nqx - 1) / (CX * nqx);
  const int64_t rows = (int64_t)(a.ax[1].Q / (a.ax[1].Q == 1 ? 1 : P + 1)) * (a.ax[2].Q / (a.ax[2].Q == 1 ? 1 : P + 1));
  // a workgroup keeps its x run (the staged x tables) and strides over the (y, z) cells: about 4096 workgroups
  int64_t gy = rows < 1 ? 1 : rows;
  const int64_t cap = chunks >= 4096 ? 1 : 4096 / chunks;
  if (gy > cap) gy = cap;
  hipLaunchKernelGGL((ev_kernel<P, MODE>), dim3((unsigned)chunks, (unsigned)gy), dim3(gdmk::EV_THREADS),
                     gdmk::ev_lds(P), st, a);
}

}  // namespace

extern "C" {

hipError_t GDM_PART_NAME(gdmk_ev_prepare_p)(void) {
  constexpr size_t lds = gdmk::ev_flux_lds(GDM_PART);
  if (lds <= 64 * 1024) return hipSuccess;  // within the default limit
  return hipFuncSetAttribute((const void *)ev_flux_kernel<GDM_PART>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)lds);
}

hipError_t GDM_PART_NAME(gdmk_ev_eval_p)(const gdmk::EvArgs &a, hipStream_t st) {
  if (a.ax[0].Q <= 0 || a.ax[1].Q <= 0 || a.ax[2].Q <= 0) return hipSuccess;
  const bool grad = a.g[0] || a.g[1] || a.g[2];
  if (a.uq && grad)
    launch_mode<3>(a, st);
  else if (a.uq)
    launch_mode<1>(a, st);
  else if (grad)
    launch_mode<2>(a, st);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t GDM_PART_NAME(gdmk_ev_flux_p)(const gdmk::LoadGeom &g, const double *Sw, const double *Dw, const double *Fq,
                                         int64_t comp_stride, double scale, double *dst, hipStream_t st) {
  constexpr int P = GDM_PART;
  const int tiles = ((g.K[0] + gdmk::LOAD_TX - 1) / gdmk::LOAD_TX) * ((g.K[1] + gdmk::LOAD_TY - 1) / gdmk::LOAD_TY);
  const dim3 grid((unsigned)tiles, (unsigned)((g.K[2] + gdmk::LOAD_ZC - 1) / gdmk::LOAD_ZC));
  hipLaunchKernelGGL(ev_flux_kernel<P>, grid, dim3(gdmk::LOAD_TX * gdmk::LOAD_TY), gdmk::ev_flux_lds(P), st, g, Sw, Dw,
                     Fq, comp_stride, scale, dst);
  return hipGetLastError();
}

}  // extern "C"

#endif
