// gdm_face.h -- device code of the inflow faces' step 1 that the face kernels
// (gdm_face.hip) and the tail of the v8 stencil (gdm_stencil.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdm_device.h"
#include "gdm_kernels.h"

namespace gdmk {

// ---------------------------------------------------------------------------
// Inflow boundary-data term (advection/stiffness.h:473-532 with a.n < 0):
//   rhs(node) += |a.n| sum_{q on face} u+_q phi_node(x_q) JxW_q
// factorised over the two tangential directions of the face:
//   step 1: T[q1][i0] = sum_m U[q1][qs0(i0) + m] w0[i0][m]
//   step 2: dst(i0, i1) += scale * sum_m w1[i1][m] T[qs1(i1) + m][i0]
// Step 1 stages ROWS rows of U (the q-range of FACE_CHUNK consecutive nodes)
// in LDS with coalesced loads; each lane then owns one node and reads its
// weights node-minor (w0T), so every global access is a contiguous wave row.
// ---------------------------------------------------------------------------
// boundary values U(i0, i1) of the face ([Q1][Q0] array).  (Evaluating the
// stage values of a built-in function here instead, per point, measured 2-3x
// slower than reading them: each lane's six consecutive points make every
// table read touch 64 cache lines; gdm_apply_bc_fn fills the array first.)
struct BcArr {
  const double *__restrict__ U;
  int Q0;
  __device__ __forceinline__ double operator()(int i0, int i1) const { return U[(int64_t)i1 * Q0 + i0]; }
};

// Step 1 in cell form: for one row q1 of the face, every local cell c reduces
// its p + 1 contiguous boundary values with its category's (p+1) x (p+1) table
// (S_c[l] = sum_q Phi[cat(c)][l][q] U[q1][c (p+1) + q], one contiguous read per
// cell, no per-node weight rows), then every owned node gathers the S_c of the
// cells whose DoF boxes contain it (system.h:195-246 box offsets).
__device__ __forceinline__ int face_category(int c, int p, int n) {
  const int half = p / 2;
  return c < half ? c : (c < n - half ? half : p + c - n);
}
__device__ __forceinline__ int face_box_offset(int c, int p, int n) {
  const int half = p / 2;
  return c < half ? 0 : min(n, c + half + 1) - p;
}

template <int P, class Src>
__device__ __forceinline__ void face_cell_step1_body(const Src &U, int Q0, int Q1, int rpb, int i0_begin, int n0,
                                                     const int *__restrict__ crange, const double *__restrict__ phi,
                                                     int ncell_total, int cell_begin, double *__restrict__ T,
                                                     int block) {
  constexpr int N1 = P + 1;
  extern __shared__ double sh[];  // [P][N1][N1] Phi, then [ncells][N1] S
  double *sphi = sh, *S = sh + P * N1 * N1;
  const int ncells = Q0 / N1;
  for (int e = threadIdx.x; e < P * N1 * N1; e += blockDim.x) sphi[e] = phi[e];
  const int r0 = block * rpb, r1 = min(Q1, r0 + rpb);
  for (int row = r0; row < r1; ++row) {
    __syncthreads();  // Phi ready / previous row's gather done
    for (int c = threadIdx.x; c < ncells; c += blockDim.x) {
      const int cat = face_category(cell_begin + c, P, ncell_total);
      double v[N1];
#pragma unroll
      for (int q = 0; q < N1; ++q) v[q] = U(c * N1 + q, row);
      const double *ph = sphi + cat * N1 * N1;
#pragma unroll
      for (int l = 0; l < N1; ++l) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < N1; ++q) s = fma(ph[l * N1 + q], v[q], s);
        S[c * N1 + l] = s;
      }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < n0; t += blockDim.x) {
      const int i0 = i0_begin + t;
      const int cf = crange[2 * i0], cl = crange[2 * i0 + 1];
      double acc = 0.0;
      for (int c = cf; c <= cl; ++c) acc += S[c * N1 + (i0 - face_box_offset(cell_begin + c, P, ncell_total))];
      T[(int64_t)row * n0 + t] = acc;
    }
  }
}

// Step 1 of the rows [block rpb, block rpb + rpb) at once, all threads of the
// workgroup (the stencil's tail): the rows (contiguous in U) are staged in LDS
// with coalesced 16-B loads, all of them in flight together; each (row, cell)
// reduction then reads its N1 values from LDS and writes its N1 results over
// them (the same positions: in place, no barrier); one barrier; every
// (row, node) gather.  The same sums in the same order as
// face_cell_step1_body.  LDS: Phi, then [rpb][Q0] (U rows, then S).
template <int P>
__device__ __forceinline__ void face_cell_step1_rows(const BcArr &U, int Q0, int Q1, int rpb, int i0_begin, int n0,
                                                     const int *__restrict__ crange, const double *__restrict__ phi,
                                                     int ncell_total, int cell_begin, double *__restrict__ T,
                                                     int block) {
  constexpr int N1 = P + 1, MAXLD = 8;
  extern __shared__ double sh[];
  double *sphi = sh, *S = sh + ((P * N1 * N1 + 1) & ~1);  // 16-B aligned rows
  const int ncells = Q0 / N1;
  for (int e = threadIdx.x; e < P * N1 * N1; e += blockDim.x) sphi[e] = phi[e];
  const int r0 = block * rpb, nr = min(Q1, r0 + rpb) - r0;
  // stage rows r0 .. r0 + nr - 1 (nr * Q0 contiguous doubles of U)
  const double *src = U.U + (int64_t)r0 * Q0;
  const int n = nr * Q0;
  if ((((uintptr_t)src) & 15) == 0 && (n & 1) == 0) {
    const dpair *s2 = (const dpair *)src;
    ldouble2 *d2 = (ldouble2 *)S;
    for (int eb = 0; eb < n / 2; eb += MAXLD * (int)blockDim.x) {
      dpair v[MAXLD];
#pragma unroll
      for (int k = 0; k < MAXLD; ++k) {
        const int e = eb + k * (int)blockDim.x + (int)threadIdx.x;
        if (e < n / 2) v[k] = __builtin_nontemporal_load(s2 + e);
      }
#pragma unroll
      for (int k = 0; k < MAXLD; ++k) {
        const int e = eb + k * (int)blockDim.x + (int)threadIdx.x;
        if (e < n / 2) d2[e] = v[k];
      }
    }
  } else {
    for (int e = threadIdx.x; e < n; e += blockDim.x) S[e] = src[e];
  }
  __syncthreads();  // Phi and the rows staged
  for (int e = threadIdx.x; e < nr * ncells; e += blockDim.x) {
    const int r = e / ncells, c = e - r * ncells;
    double *Sc = S + (int64_t)r * Q0 + c * N1;
    double v[N1];
#pragma unroll
    for (int q = 0; q < N1; ++q) v[q] = Sc[q];
    const double *ph = sphi + face_category(cell_begin + c, P, ncell_total) * N1 * N1;
#pragma unroll
    for (int l = 0; l < N1; ++l) {
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < N1; ++q) acc = fma(ph[l * N1 + q], v[q], acc);
      Sc[l] = acc;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nr * n0; e += blockDim.x) {
    const int r = e / n0, t = e - r * n0;
    const int i0 = i0_begin + t;
    const int cf = crange[2 * i0], cl = crange[2 * i0 + 1];
    const double *Sr = S + (int64_t)r * Q0;
    double acc = 0.0;
    for (int c = cf; c <= cl; ++c) acc += Sr[c * N1 + (i0 - face_box_offset(cell_begin + c, P, ncell_total))];
    T[(int64_t)(r0 + r) * n0 + t] = acc;
  }
}

// every inflow face's step 1 (cell form) in one launch, face = blockIdx.y:
// the faces are independent (own T), so their rows share the GPU instead of
// running one face after the other (gdmk_launch_faces_step1)
template <class Src>
struct Step1Face {
  Src U;
  int Q0, Q1, i0_begin, n0;
  const int *crange;
  const double *phi;
  int ncell_total, cell_begin;
  double *T;
};
template <class Src>
struct Step1Set {
  Step1Face<Src> f[BcStage::kMaxFaces];
  int rpb;
};

}  // namespace gdmk
