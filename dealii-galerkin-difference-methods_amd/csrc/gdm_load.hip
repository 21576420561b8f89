// gdm_load.hip -- the data terms of the uncut wave / heat right-hand side
// (applications/wave/include/gdm/wave/stiffness.h:151-330):
//   the source term (v, f(., t)) over QGauss(p+1)            (:196-200)
//   the Nitsche Dirichlet data <gamma_D / h v - dv/dn, g_D>  (:320-326)
// Both add into the owned vector, as compute_rhs accumulates.
//
// General load kernel: b = (E_z (x) E_y (x) E_x)^T (w . f_q), the transpose of
// gdm_post.hip's evaluation.  A workgroup owns a LOAD_TX x LOAD_TY tile of
// nodes and LOAD_ZC node planes, and marches the cell layers whose DoF boxes
// reach those planes.  Per layer and z quadrature point it takes f on the
// tile's quadrature footprint (the cells outside the tile whose boxes reach
// its nodes included) strip by strip through LDS, contracts x, then y, and
// adds the plane into a register ring of the p + 1 node planes of the layer's
// box; a plane leaves the ring with one read-modify-write of dst once the
// boxes have moved past it.  Gather form: one thread per node, cells in
// ascending order, no atomics -- the bits do not depend on the launch.
//
// Rank-1 path (GDM_FN_CONSTANT, GDM_FN_SINE_PRODUCT): tensor Gauss quadrature
// of a product f = prod_d f_d(x_d) factorises, (v, f) = b_z (x) b_y (x) b_x with
// b_d[i] = sum_q w_q h phi_i(x_q) f_d(x_q); one small launch builds the per-axis
// (sin, cos) load vectors at time t, one streaming launch adds the product.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_bcfn.h"
#include "gdm_load.h"

namespace gdmk {

template <int P, int MODE>
__global__ void __launch_bounds__(LOAD_TX *LOAD_TY) load_kernel(LoadGeom g, BcFn f, const double *__restrict__ Sw,
                                                                  const double *__restrict__ fq, double scale,
                                                                  double *__restrict__ dst) {
  constexpr int N1 = P + 1, NCAT = P > 1 ? P : 1;
  constexpr int TX = LOAD_TX, TY = LOAD_TY, NT = TX * TY, R = load_rows(P);
  // quadrature points of a tile's footprint along x or y: the nodes [i0, i0 + TX) lie in the boxes of the
  // cells [i0 - p + p/2, i0 + TX - 1 + p/2] in the interior (TX + p cells); next to the upper wall the last
  // node may be n - p, which every cell up to n - 1 = (n - p) + p - 1 holds: p/2 cells more
  constexpr int QF = (TX + P + P / 2) * N1;
  static_assert(TX == TY, "the footprint bound QF serves both directions");
  __shared__ double Sl[NCAT * N1 * N1];
  __shared__ double F[R][QF];
  __shared__ double T[QF][TX];
  const int tid = threadIdx.x;
  for (int i = tid; i < NCAT * N1 * N1; i += NT) Sl[i] = Sw[i];

  const int n1x = g.on[0] ? N1 : 1, n1y = g.on[1] ? N1 : 1, n1z = g.on[2] ? N1 : 1;
  const int tiles_x = (g.K[0] + TX - 1) / TX;
  const int X0 = (int)(blockIdx.x % tiles_x) * TX, Y0 = (int)(blockIdx.x / tiles_x) * TY;
  const int z0 = (int)blockIdx.y * LOAD_ZC, z1 = min(z0 + LOAD_ZC, g.K[2]);
  const int xl = min(X0 + TX, g.K[0]) - 1, yl = min(Y0 + TY, g.K[1]) - 1;  // last nodes of the tile
  // footprint cells
  const int cxf0 = g.on[0] ? ld_first(X0, P, g.nc[0]) : 0, cxf1 = g.on[0] ? ld_last(xl, P, g.nc[0]) : 0;
  const int cyf0 = g.on[1] ? ld_first(Y0, P, g.nc[1]) : 0, cyf1 = g.on[1] ? ld_last(yl, P, g.nc[1]) : 0;
  const int czf0 = g.on[2] ? ld_first(z0, P, g.nc[2]) : 0, czf1 = g.on[2] ? ld_last(z1 - 1, P, g.nc[2]) : 0;
  const int qxb = cxf0 * n1x, nqx = (cxf1 - cxf0 + 1) * n1x;
  const int qyb = cyf0 * n1y, nqy = (cyf1 - cyf0 + 1) * n1y;
  if (nqx > QF || nqy > QF) return;  // cannot happen (bound above); block-uniform

  const int ix = tid % TX, iy = tid / TX;
  const int nx = X0 + ix, ny = Y0 + iy;
  const bool valid = nx < g.K[0] && ny < g.K[1];
  const int cy_a = g.on[1] && valid ? ld_first(ny, P, g.nc[1]) : 0;
  const int cy_b = g.on[1] && valid ? ld_last(ny, P, g.nc[1]) : 0;

  double ring[N1];
#pragma unroll
  for (int k = 0; k < N1; ++k) ring[k] = 0.0;
  int off_cur = g.on[2] ? ld_off(czf0, P, g.nc[2]) : 0;
  const double sj = scale * g.jxw;
  const int64_t node_xy = (int64_t)nx + (int64_t)g.K[0] * ny, plane = (int64_t)g.K[0] * g.K[1];

  for (int cz = czf0; cz <= czf1; ++cz) {
    const int noff = g.on[2] ? ld_off(cz, P, g.nc[2]) : 0;
    if (noff > off_cur) {  // the boxes moved one plane on: the lowest plane is complete
      if (valid && off_cur >= z0 && off_cur < z1) dst[node_xy + plane * off_cur] += sj * ring[0];
#pragma unroll
      for (int k = 0; k < P; ++k) ring[k] = ring[k + 1];
      ring[P] = 0.0;
      off_cur = noff;
    }
    const double *Sz = Sl + (g.on[2] ? ld_cat(cz, P, g.nc[2]) : 0) * N1 * N1;
    for (int qz = 0; qz < n1z; ++qz) {
      const int64_t gq2 = (int64_t)cz * n1z + qz;
      // x contraction, R quadrature rows at a time: T[qy][ix] = sum_c sum_q Sw_x f
      for (int r0 = 0; r0 < nqy; r0 += R) {
        const int nr = min(R, nqy - r0);
        __syncthreads();  // the previous strip's reads of F and the previous plane's reads of T are done
        for (int i = tid; i < nr * nqx; i += NT) {
          const int r = i / nqx, j = i - r * nqx;
          const int gq1 = qyb + r0 + r, gq0 = qxb + j;
          double v;
          if (MODE == 0) {
            v = fq[(gq2 * g.Q[1] + gq1) * (int64_t)g.Q[0] + gq0];
          } else {  // GDM_FN_CONE: max(0, r0 - |x - c|)
            double r2 = 0.0;
            if (g.on[0]) {
              const double d = g.lo[0] + (gq0 / N1 + g.xq[gq0 % N1]) * g.h[0] - f.prm[1 + g.rdir[0]];
              r2 += d * d;
            }
            if (g.on[1]) {
              const double d = g.lo[1] + (gq1 / N1 + g.xq[gq1 % N1]) * g.h[1] - f.prm[1 + g.rdir[1]];
              r2 += d * d;
            }
            if (g.on[2]) {
              const double d = g.lo[2] + (cz + g.xq[qz]) * g.h[2] - f.prm[1 + g.rdir[2]];
              r2 += d * d;
            }
            v = fmax(0.0, f.prm[0] - sqrt(r2));
          }
          F[r][j] = v;
        }
        __syncthreads();
        for (int o = tid; o < nr * TX; o += NT) {
          const int r = o / TX, jx = o % TX, i = X0 + jx;
          if (i >= g.K[0]) continue;
          double s = 0.0;
          if (g.on[0]) {
            const int ca = ld_first(i, P, g.nc[0]), cb = ld_last(i, P, g.nc[0]);
            for (int c = ca; c <= cb; ++c) {
              const double *Sx = Sl + (ld_cat(c, P, g.nc[0]) * N1 + (i - ld_off(c, P, g.nc[0]))) * N1;
              const double *Fr = &F[r][(c - cxf0) * N1];
#pragma unroll
              for (int q = 0; q < N1; ++q) s = fma(Sx[q], Fr[q], s);
            }
          } else {
            s = F[r][0];
          }
          T[r0 + r][jx] = s;
        }
      }
      __syncthreads();
      if (valid) {
        double val = 0.0;
        if (g.on[1]) {
          for (int c = cy_a; c <= cy_b; ++c) {
            const double *Sy = Sl + (ld_cat(c, P, g.nc[1]) * N1 + (ny - ld_off(c, P, g.nc[1]))) * N1;
            const int rb = (c - cyf0) * N1;
#pragma unroll
            for (int q = 0; q < N1; ++q) val = fma(Sy[q], T[rb + q][ix], val);
          }
        } else {
          val = T[0][ix];
        }
        if (g.on[2]) {
#pragma unroll
          for (int k = 0; k < N1; ++k) ring[k] = fma(Sz[k * N1 + qz], val, ring[k]);
        } else {
          ring[0] += val;
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

// per-axis load vectors of the separable factor at time t: bvec[(2 ax + 0) ld
// + i] = sum_q w_q h phi_i(x_q) sin(.), [(2 ax + 1) ld + i] the same with cos;
// GDM_FN_CONSTANT: the factor is 1 (sin slot) and 0.  One node per thread,
// cells in ascending order.
__global__ void __launch_bounds__(64) load_vec_kernel(LoadGeom g, BcFn f, double t, const double *__restrict__ Sw,
                                                      double *__restrict__ bvec, int ld) {
  const int ax = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.K[ax]) return;
  double bs = 1.0, bc = 0.0;
  if (g.on[ax]) {
    const int p = g.p, n1 = p + 1, n = g.nc[ax];
    bs = 0.0;
    for (int c = ld_first(i, p, n); c <= ld_last(i, p, n); ++c) {
      const double *S = Sw + (ld_cat(c, p, n) * n1 + (i - ld_off(c, p, n))) * n1;
      for (int q = 0; q < n1; ++q) {
        double s = 1.0, co = 0.0;
        if (f.kind == 2) bc_sine_factor(f, g.rdir[ax], g.lo[ax] + (c + g.xq[q]) * g.h[ax], t, s, co);
        bs = fma(S[q], s, bs);
        bc = fma(S[q], co, bc);
      }
    }
    bs *= g.h[ax];
    bc *= g.h[ax];
  }
  bvec[(size_t)(2 * ax) * ld + i] = bs;
  bvec[(size_t)(2 * ax + 1) * ld + i] = bc;
}

// dst[i, j, k] += coef bx[i] by[j] bz[k] (derivative 0) or the d/dt sum
// coef sum_e w_e cos_e prod_{d != e} sin_d; two entries per thread, 16-byte
// accesses when dst is 16-byte aligned (VEC)
template <bool VEC>
__global__ void __launch_bounds__(256) load_rank1_kernel(int64_t n, int K0, int K1, const double *__restrict__ b,
                                                         int ld, double coef, double w0, double w1, double w2,
                                                         int derivative, double *__restrict__ dst) {
  const int64_t i0 = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  if (i0 >= n) return;
  double v[2] = {0.0, 0.0};
  const int m = i0 + 1 < n ? 2 : 1;
  for (int e = 0; e < m; ++e) {
    const int64_t fl = i0 + e, r = fl / K0;
    const int i = (int)(fl - r * K0), j = (int)(r % K1);
    const int64_t k = r / K1;
    const double s0 = b[i], s1 = b[(size_t)2 * ld + j], s2 = b[(size_t)4 * ld + k];
    if (!derivative) {
      v[e] = coef * (s0 * s1 * s2);
    } else {
      const double c0 = b[(size_t)ld + i], c1 = b[(size_t)3 * ld + j], c2 = b[(size_t)5 * ld + k];
      v[e] = coef * (w0 * c0 * s1 * s2 + w1 * s0 * c1 * s2 + w2 * s0 * s1 * c2);
    }
  }
  if (VEC && m == 2) {
    double2 *p2 = reinterpret_cast<double2 *>(dst + i0);
    double2 d = *p2;
    d.x += v[0];
    d.y += v[1];
    *p2 = d;
  } else {
    for (int e = 0; e < m; ++e) dst[i0 + e] += v[e];
  }
}

// Dirichlet data of one box face, step 1: the face-JxW-weighted projection of
// g along t0, tmp[q1][i0] = sum_a w0[i0][a] g[q1][qs0[i0] + a]
__global__ void __launch_bounds__(256) dirichlet_project_kernel(DirFace F, const double *__restrict__ g,
                                                                double *__restrict__ tmp) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)F.n0 * F.Q1) return;
  const int i0 = (int)(id % F.n0);
  const int64_t q1 = id / F.n0;
  const int m0 = F.qc0[i0];
  const double *w0 = F.w0 + (size_t)i0 * F.wmax0, *gr = g + F.goff + q1 * F.Q0 + F.qs0[i0];
  double s = 0.0;
  for (int a = 0; a < m0; ++a) s = fma(w0[a], gr[a], s);
  tmp[id] = s;
}

// step 2: P = the projection along t1 onto node (i0, i1) of the face, then
// dst[node + k stride_d] += c_k P for the p + 1 planes behind the face.  One
// thread per face node; the faces run one launch pair after the other, they
// share the edge and corner columns and the scratch.
__global__ void __launch_bounds__(256) dirichlet_face_kernel(DirFace F, const double *__restrict__ tmp,
                                                             double *__restrict__ dst) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)F.n0 * F.n1) return;
  const int i0 = (int)(id % F.n0), i1 = (int)(id / F.n0);
  const int q1 = F.qs1[i1], m1 = F.qc1[i1];
  const double *w1 = F.w1 + (size_t)i1 * F.wmax1;
  double P = 0.0;
  for (int b = 0; b < m1; ++b) P = fma(w1[b], tmp[(int64_t)(q1 + b) * F.n0 + i0], P);
  double *o = dst + F.base + i0 * F.stride0 + i1 * F.stride1;
  for (int k = 0; k < F.nk; ++k) o[k * F.stride_d] += F.ck[k] * P;
}

}  // namespace gdmk

namespace {
template <int P>
void launch_load_p(const gdmk::LoadGeom &g, const gdmk::BcFn &f, int mode, const double *Sw, const double *fq,
                   double scale, double *dst, hipStream_t st) {
  const int tiles = ((g.K[0] + gdmk::LOAD_TX - 1) / gdmk::LOAD_TX) * ((g.K[1] + gdmk::LOAD_TY - 1) / gdmk::LOAD_TY);
  const dim3 grid((unsigned)tiles, (unsigned)((g.K[2] + gdmk::LOAD_ZC - 1) / gdmk::LOAD_ZC));
  const dim3 block(gdmk::LOAD_TX * gdmk::LOAD_TY);
  if (mode == 0)
    hipLaunchKernelGGL((gdmk::load_kernel<P, 0>), grid, block, 0, st, g, f, Sw, fq, scale, dst);
  else
    hipLaunchKernelGGL((gdmk::load_kernel<P, 1>), grid, block, 0, st, g, f, Sw, fq, scale, dst);
}
}  // namespace

extern "C" hipError_t gdmk_launch_load(const gdmk::LoadGeom &g, const gdmk::BcFn &f, int mode, const double *Sw,
                                      const double *fq, double scale, double *dst, hipStream_t st) {
  switch (g.p) {
    case 1: launch_load_p<1>(g, f, mode, Sw, fq, scale, dst, st); break;
    case 3: launch_load_p<3>(g, f, mode, Sw, fq, scale, dst, st); break;
    case 5: launch_load_p<5>(g, f, mode, Sw, fq, scale, dst, st); break;
    case 7: launch_load_p<7>(g, f, mode, Sw, fq, scale, dst, st); break;
    case 9: launch_load_p<9>(g, f, mode, Sw, fq, scale, dst, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

extern "C" hipError_t gdmk_launch_load_rank1(const gdmk::LoadGeom &g, const gdmk::BcFn &f, double t, int derivative,
                                            double scale, const double *Sw, double *bvec, int ld, double *dst,
                                            hipStream_t st) {
  int kmax = 1;
  for (int ax = 0; ax < 3; ++ax) kmax = kmax > g.K[ax] ? kmax : g.K[ax];
  if (kmax > ld) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gdmk::load_vec_kernel, dim3((unsigned)((kmax + 63) / 64), 3), dim3(64), 0, st, g, f, t, Sw, bvec,
                     ld);
  double w[3] = {0.0, 0.0, 0.0};
  for (int ax = 0; ax < 3; ++ax)
    if (g.on[ax] && f.kind == 2) w[ax] = -2.0 * M_PI * f.prm[3 + g.rdir[ax]] * f.prm[g.rdir[ax]];
  const double coef = f.kind == 0 ? scale * f.prm[0] : scale;
  const int64_t n = (int64_t)g.K[0] * g.K[1] * g.K[2];
  const unsigned blocks = (unsigned)(((n + 1) / 2 + 255) / 256);
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0)
    hipLaunchKernelGGL((gdmk::load_rank1_kernel<true>), dim3(blocks), dim3(256), 0, st, n, g.K[0], g.K[1], bvec, ld,
                       coef, w[0], w[1], w[2], derivative, dst);
  else
    hipLaunchKernelGGL((gdmk::load_rank1_kernel<false>), dim3(blocks), dim3(256), 0, st, n, g.K[0], g.K[1], bvec, ld,
                       coef, w[0], w[1], w[2], derivative, dst);
  return hipGetLastError();
}

extern "C" hipError_t gdmk_launch_dirichlet_face(const gdmk::DirFace &F, const double *g, double *tmp, double *dst,
                                                hipStream_t st) {
  const int64_t n = (int64_t)F.n0 * F.n1, nt = (int64_t)F.n0 * F.Q1;
  hipLaunchKernelGGL(gdmk::dirichlet_project_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, F, g, tmp);
  hipLaunchKernelGGL(gdmk::dirichlet_face_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, F, tmp, dst);
  return hipGetLastError();
}
