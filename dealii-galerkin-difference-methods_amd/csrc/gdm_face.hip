// gdm_face.hip -- the inflow boundary-data term (gdm_face.h): the step-1 and
// step-2 kernels of the faces and their launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "gdm_face.h"
#include "gdm_kernels.h"
#include "gdm_parts.h"

namespace gdmk {

template <int ROWS, class Src>
__global__ void __launch_bounds__(FACE_CHUNK) face_step1_kernel(const Src U, int Q0, int Q1,
                                                                 int i0_begin, int n0,
                                                                 const int *__restrict__ qs0,
                                                                 const double *__restrict__ w0T, int wmax0,
                                                                 int ldw0, int qmax, double *__restrict__ T) {
  extern __shared__ double sh[];  // [ROWS][qmax]
  const int c0 = blockIdx.x * FACE_CHUNK;
  const int q1b = blockIdx.y * ROWS;
  const int nc = min(FACE_CHUNK, n0 - c0);
  const int ia = i0_begin + c0;
  const int qa = qs0[ia];
  const int nq = min(Q0, qs0[ia + nc - 1] + wmax0) - qa;  // <= qmax (host-checked)
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    if (q1b + r < Q1) {
      for (int e = threadIdx.x; e < nq; e += FACE_CHUNK) sh[r * qmax + e] = U(qa + e, q1b + r);
    }
  }
  __syncthreads();
  if ((int)threadIdx.x >= nc) return;
  const int i0 = ia + threadIdx.x;
  const int b = qs0[i0] - qa;
  const int mend = min(wmax0, nq - b);  // weights past the node's own count are 0
  double s[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) s[r] = 0.0;
  for (int m = 0; m < mend; ++m) {
    const double w = w0T[(int64_t)m * ldw0 + i0];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) s[r] = fma(w, sh[r * qmax + b + m], s[r]);
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
    if (q1b + r < Q1) T[(int64_t)(q1b + r) * n0 + c0 + threadIdx.x] = s[r];
}

template <int P, class Src>
__global__ void __launch_bounds__(512) face_cell_step1_kernel(const Src U, int Q0, int Q1, int rpb,
                                                               int i0_begin, int n0, const int *__restrict__ crange,
                                                               const double *__restrict__ phi, int ncell_total,
                                                               int cell_begin, double *__restrict__ T) {
  face_cell_step1_body<P>(U, Q0, Q1, rpb, i0_begin, n0, crange, phi, ncell_total, cell_begin, T, blockIdx.x);
}

template <int P, class Src>
__global__ void __launch_bounds__(512) face_cell_step1_multi_kernel(const Step1Set<Src> set) {
  const Step1Face<Src> &F = set.f[blockIdx.y];
  if ((int)blockIdx.x * set.rpb >= F.Q1) return;
  face_cell_step1_body<P>(F.U, F.Q0, F.Q1, set.rpb, F.i0_begin, F.n0, F.crange, F.phi, F.ncell_total, F.cell_begin,
                          F.T, blockIdx.x);
}

// scale sum_m w1[i1][m] T[q + m][t], the product rounded on its own: the
// compiler may not fuse it into the later add (one FMA would round
// differently from the face-by-face path's dst + G)
__device__ __forceinline__ double face_step2_value(const double *__restrict__ T, int n0, int t, int i1,
                                                   const int *__restrict__ qs1, const int *__restrict__ qc1,
                                                   const double *__restrict__ w1, int wmax1, double scale) {
  const double *w = w1 + (int64_t)i1 * wmax1;
  const int n = qc1[i1], q = qs1[i1];
  const double *Tc = T + (int64_t)q * n0 + t;
  double s = 0.0;
  int m = 0;
  // groups of 6 loads in flight, the FMAs in increasing m (the order of the
  // one-at-a-time loop: same bits)
  for (; m + 6 <= n; m += 6) {
    double tv[6];
#pragma unroll
    for (int u = 0; u < 6; ++u) tv[u] = Tc[(int64_t)(m + u) * n0];
#pragma unroll
    for (int u = 0; u < 6; ++u) s = fma(w[m + u], tv[u], s);
  }
  for (; m < n; ++m) s = fma(w[m], Tc[(int64_t)m * n0], s);
  double v;
  {
#pragma clang fp contract(off)
    v = scale * s;
  }
  asm volatile("" : "+v"(v));
  return v;
}

// dst node (t, i1) += scale sum_m w1[i1][m] T[q + m][t]: one face (face by face, in face order)
__global__ void __launch_bounds__(256) face_step2_kernel(const double *__restrict__ T, int n0, int i1_begin,
                                                          int i1_end, const int *__restrict__ qs1,
                                                          const int *__restrict__ qc1,
                                                          const double *__restrict__ w1, int wmax1,
                                                          double *__restrict__ dst, int64_t base,
                                                          int64_t stride0, int64_t stride1, double scale) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i1 = i1_begin + (int)blockIdx.y;
  if (t >= n0 || i1 >= i1_end) return;
  const double v = face_step2_value(T, n0, t, i1, qs1, qc1, w1, wmax1, scale);
  double *d = dst + base + (int64_t)t * stride0 + (int64_t)(i1 - i1_begin) * stride1;
  *d = *d + v;
}

// step-2 data of one face for face_step2_add_kernel
struct Step2Face {
  const double *T;
  int n0, i1_begin, i1_end;
  const int *qs1, *qc1;
  const double *w1;
  int wmax1;
  double scale;
};
__device__ __forceinline__ bool face_add_member(const FaceAddFace &g, const int c[3]) {
  return c[g.d] == g.plane && (g.a0 < 0 || (c[g.a0] >= g.b0 && c[g.a0] < g.e0)) &&
         (g.a1 < 0 || (c[g.a1] >= g.b1 && c[g.a1] < g.e1));
}
// step 2 of every inflow face fused with the ordered adds (one launch, face =
// blockIdx.z): a node is handled by the thread of the first face containing
// it, which adds its own face's G = scale sum_m w1 T and then every later
// containing face's G, in face order -- the sums (and roundings) of the
// per-face step-2 launches, without the G buffers and the separate add launch
struct Step2AddSet {
  Step2Face f[BcStage::kMaxFaces];
  FaceAddFace g[BcStage::kMaxFaces];
  int n;
  int64_t N0, N1, own_off;
};
// One thread per node column t and R1 consecutive i1 rows: the rows' T
// windows overlap (consecutive nodes shift by one cell), so the thread walks
// the union of their q ranges once and feeds each row's sum in increasing m
// -- the same FMA sequence per node as face_step2_value, with ~R1 / 4 of its
// T loads.  Weights and q ranges are wave-uniform (scalar loads).
template <int R1>
__global__ void __launch_bounds__(64) face_step2_add_kernel(const Step2AddSet set, double *__restrict__ dst) {
  const int f = blockIdx.z;
  const Step2Face &F = set.f[f];
  const FaceAddFace &A = set.g[f];
  const int r0 = blockIdx.y * R1, nr = min(R1, F.i1_end - F.i1_begin - r0);
  if (nr <= 0) return;
  const int t = blockIdx.x * 64 + threadIdx.x;
  const bool on = t < F.n0;
  const int tt = on ? t : F.n0 - 1;  // idle lanes repeat a valid column (no divergence in the q walk)
  const int i1a = F.i1_begin + r0;
  int qlo = F.qs1[i1a], qhi = qlo;
#pragma unroll
  for (int j = 0; j < R1; ++j)
    if (j < nr) {
      qlo = min(qlo, F.qs1[i1a + j]);
      qhi = max(qhi, F.qs1[i1a + j] + F.qc1[i1a + j]);
    }
  double sum[R1];
  int qs[R1], qe[R1];
  const double *wr[R1];
#pragma unroll
  for (int j = 0; j < R1; ++j) {
    sum[j] = 0.0;
    qs[j] = j < nr ? F.qs1[i1a + j] : 0;
    qe[j] = j < nr ? qs[j] + F.qc1[i1a + j] : 0;
    wr[j] = F.w1 + (int64_t)(i1a + j) * F.wmax1 - qs[j];  // wr[j][q] = w1[i1][q - qs]
  }
  const double *Tc = F.T + tt;
  int q = qlo;
  for (; q + 6 <= qhi; q += 6) {
    double tv[6];
#pragma unroll
    for (int u = 0; u < 6; ++u) tv[u] = Tc[(int64_t)(q + u) * F.n0];
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
      for (int j = 0; j < R1; ++j)
        if (q + u >= qs[j] && q + u < qe[j]) sum[j] = fma(wr[j][q + u], tv[u], sum[j]);
  }
  for (; q < qhi; ++q) {
    const double tv = Tc[(int64_t)q * F.n0];
#pragma unroll
    for (int j = 0; j < R1; ++j)
      if (q >= qs[j] && q < qe[j]) sum[j] = fma(wr[j][q], tv, sum[j]);
  }
  if (!on) return;
#pragma unroll
  for (int j = 0; j < R1; ++j) {
    if (j >= nr) break;
    const int r = r0 + j;
    const int64_t o = A.base + (int64_t)t * A.stride0 + (int64_t)r * A.stride1;
    const int64_t gi = o + set.own_off;
    const int c[3] = {(int)(gi % set.N0), (int)((gi / set.N0) % set.N1), (int)(gi / (set.N0 * set.N1))};
    bool mine = true;
    for (int g = 0; g < f; ++g)
      if (face_add_member(set.g[g], c)) mine = false;
    if (!mine) continue;  // the node's first face adds every face's term
    double gv;
    {
#pragma clang fp contract(off)
      gv = F.scale * sum[j];
    }
    asm volatile("" : "+v"(gv));
    double v = dst[o];
    v = v + gv;
    for (int g = f + 1; g < set.n; ++g) {
      const FaceAddFace &H = set.g[g];
      if (!face_add_member(H, c)) continue;
      const Step2Face &S = set.f[g];
      const int u0 = H.a0 < 0 ? 0 : c[H.a0] - H.b0, u1 = H.a1 < 0 ? 0 : c[H.a1] - H.b1;
      v = v + face_step2_value(S.T, S.n0, u0, S.i1_begin + u1, S.qs1, S.qc1, S.w1, S.wmax1, S.scale);
    }
    dst[o] = v;
  }
}

}  // namespace gdmk

template <class Src, class Step2>
static hipError_t face_launch(const gdmk::FaceArgs &f, const Src &U, hipStream_t st, Step2 &step2) {
  using namespace gdmk;
  const int n0 = f.i0_end - f.i0_begin;
  const size_t cell_lds = sizeof(double) * ((size_t)f.p * (f.p + 1) * (f.p + 1) + (size_t)f.Q0);
  if (f.phi0 && cell_lds <= 48 * 1024) {
    // cell form of step 1, then the usual step 2
    const int rpb = 4;
    dim3 g1c((f.Q1 + rpb - 1) / rpb);
    if (f.phase != 2) switch (f.p) {
#define GDM_FACE_CELL(PP, ...)                                                                                           \
  case PP:                                                                                                         \
    hipLaunchKernelGGL((face_cell_step1_kernel<PP, Src>), g1c, dim3(512), cell_lds, st, U, f.Q0, f.Q1, rpb, f.i0_begin, \
                       n0, f.crange0, f.phi0, f.ncell0_total, f.cell0_begin, f.T);                                 \
    break;
      GDM_FOR_EACH_DEGREE(GDM_FACE_CELL)
#undef GDM_FACE_CELL
      default: return hipErrorInvalidValue;
    }
    dim3 g2((n0 + 255) / 256, f.i1_end - f.i1_begin);
    if (f.phase != 1) step2(g2);
    return hipGetLastError();
  }
  // rows per workgroup: as many as fit 48 KiB of LDS (up to 4)
  const size_t row_bytes = sizeof(double) * (size_t)f.qmax0;
  const int rows = row_bytes * 4 <= 48 * 1024 ? 4 : (row_bytes * 2 <= 48 * 1024 ? 2 : 1);
  if (row_bytes > 48 * 1024) return hipErrorInvalidValue;  // <= (FACE_CHUNK + 2p) (p + 1) doubles in practice
  dim3 g1((n0 + FACE_CHUNK - 1) / FACE_CHUNK, (f.Q1 + rows - 1) / rows);
  const size_t lds = row_bytes * rows;
  if (f.phase == 2)
    ;
  else if (rows == 4)
    hipLaunchKernelGGL((face_step1_kernel<4, Src>), g1, dim3(FACE_CHUNK), lds, st, U, f.Q0, f.Q1, f.i0_begin, n0, f.qs0,
                       f.w0T, f.wmax0, f.ldw0, f.qmax0, f.T);
  else if (rows == 2)
    hipLaunchKernelGGL((face_step1_kernel<2, Src>), g1, dim3(FACE_CHUNK), lds, st, U, f.Q0, f.Q1, f.i0_begin, n0, f.qs0,
                       f.w0T, f.wmax0, f.ldw0, f.qmax0, f.T);
  else
    hipLaunchKernelGGL((face_step1_kernel<1, Src>), g1, dim3(FACE_CHUNK), lds, st, U, f.Q0, f.Q1, f.i0_begin, n0, f.qs0,
                       f.w0T, f.wmax0, f.ldw0, f.qmax0, f.T);
  dim3 g2((n0 + 255) / 256, f.i1_end - f.i1_begin);
  if (f.phase != 1) step2(g2);
  return hipGetLastError();
}

extern "C" hipError_t gdmk_launch_face(const gdmk::FaceArgs &f, hipStream_t st) {
  using namespace gdmk;
  const int n0 = f.i0_end - f.i0_begin;
  if (n0 <= 0 || f.Q1 <= 0 || f.i1_end <= f.i1_begin) return hipSuccess;
  if (f.phase < 0 || f.phase > 2) return hipErrorInvalidValue;
  auto step2 = [&](dim3 g2) {
    hipLaunchKernelGGL(face_step2_kernel, g2, dim3(256), 0, st, f.T, n0, f.i1_begin, f.i1_end, f.qs1, f.qc1, f.w1,
                       f.wmax1, f.dst, f.base, f.stride0, f.stride1, f.scale);
  };
  return face_launch(f, BcArr{f.U, f.Q0}, st, step2);
}

// step 1 (cell form) of n inflow faces in one launch (each face its own T)
extern "C" hipError_t gdmk_launch_faces_step1(const gdmk::FaceArgs *fa, int n, hipStream_t st) {
  using namespace gdmk;
  if (n <= 0) return hipSuccess;
  if (n > BcStage::kMaxFaces) return hipErrorNotSupported;
  Step1Set<BcArr> s1{};
  s1.rpb = 4;
  size_t lds = 0;
  int g1 = 0;
  for (int i = 0; i < n; ++i) {
    const FaceArgs &f = fa[i];
    const size_t cell_lds = sizeof(double) * ((size_t)f.p * (f.p + 1) * (f.p + 1) + (size_t)f.Q0);
    if (!f.phi0 || cell_lds > 48 * 1024 || !f.T || f.p != fa[0].p || f.Q1 <= 0 || f.i0_end <= f.i0_begin)
      return hipErrorNotSupported;
    for (int j = 0; j < i; ++j)
      if (fa[j].T == f.T) return hipErrorNotSupported;  // faces must not share T
    s1.f[i] = Step1Face<BcArr>{BcArr{f.U, f.Q0}, f.Q0, f.Q1, f.i0_begin, f.i0_end - f.i0_begin, f.crange0, f.phi0,
                               f.ncell0_total, f.cell0_begin, f.T};
    lds = std::max(lds, cell_lds);
    g1 = std::max(g1, (f.Q1 + s1.rpb - 1) / s1.rpb);
  }
  switch (fa[0].p) {
#define GDM_FACES_S1(PP, ...)                                                                                      \
  case PP:                                                                                                   \
    hipLaunchKernelGGL((face_cell_step1_multi_kernel<PP, BcArr>), dim3(g1, n), dim3(512), lds, st, s1); \
    break;
    GDM_FOR_EACH_DEGREE(GDM_FACES_S1)
#undef GDM_FACES_S1
    default: return hipErrorNotSupported;
  }
  return hipGetLastError();
}

// step 2 of n inflow faces (their T from gdmk_launch_faces_step1) with the
// ordered adds into dst, one launch (face_step2_add_kernel)
extern "C" hipError_t gdmk_launch_faces_step2_add(const gdmk::FaceArgs *fa, const gdmk::FaceAddFace *fg, int n,
                                                  int64_t N0, int64_t N1, int64_t own_off, double *dst,
                                                  hipStream_t st) {
  using namespace gdmk;
  // rows per thread: 1 / 2 / 4 / 8 measured 41.5 / 37.0 / 45.6 / 74.9 us at C3
  // (three 512^2 faces, profiles/r5_experiments/face_step2_rows.txt)
  constexpr int kRows = 2;
  if (n <= 0) return hipSuccess;
  if (n > BcStage::kMaxFaces || N0 <= 0 || N1 <= 0) return hipErrorNotSupported;
  Step2AddSet set{};
  set.n = n;
  set.N0 = N0;
  set.N1 = N1;
  set.own_off = own_off;
  int gx = 0, gy = 0;
  for (int i = 0; i < n; ++i) {
    const FaceArgs &f = fa[i];
    const int n0 = f.i0_end - f.i0_begin;
    if (!f.T || fg[i].e0 - fg[i].b0 != n0 || fg[i].e1 - fg[i].b1 != f.i1_end - f.i1_begin) return hipErrorNotSupported;
    set.f[i] = Step2Face{f.T, n0, f.i1_begin, f.i1_end, f.qs1, f.qc1, f.w1, f.wmax1, f.scale};
    set.g[i] = fg[i];
    gx = std::max(gx, (n0 + 63) / 64);
    gy = std::max(gy, (f.i1_end - f.i1_begin + kRows - 1) / kRows);
  }
  if (gx <= 0 || gy <= 0) return hipSuccess;
  hipLaunchKernelGGL(face_step2_add_kernel<kRows>, dim3(gx, gy, n), dim3(64), 0, st, set, dst);
  return hipGetLastError();
}
