// gdm_pcg.h -- the preconditioned conjugate gradient of the library, once.
//
// SolverCG with ReductionControl(max_it, abs_tol, rel_tol), x the initial
// guess.  Header only and free of HIP: the vectors are opaque handles (device
// pointers in the C ABI, host arrays in host/pcg_check.cc) and every operation
// on them is a callable of the caller, which also knows their length:
//   apply(src, dst)         dst = A src
//   precondition(r, z)      z = B^-1 r
//   dot(u, v) -> double     the value on the host
//   axpby(a, x, b, y)       y = a x + b y
//   copy(dst, src)
// The loop reads host scalars only and allocates nothing; r, p, Ap, z are the
// caller's work vectors.  The order of the operations is fixed (the callers'
// results are compared bit by bit):
//   r = b - A x, res = |r|, tol = max(abs_tol, rel_tol res), z, p = z, rz;
//   per iteration Ap, pAp, step = rz / pAp, x += step p, r -= step Ap, res,
//   the convergence test, then the non-finite test, z, rz_new,
//   p = z + (rz_new / rz) p.
#ifndef GDM_PCG_H
#define GDM_PCG_H

#include <algorithm>
#include <cmath>

namespace gdm {

enum class PcgStatus {
  converged,
  max_it,      // res > tol after max_it iterations (SolverControl::NoConvergence)
  breakdown,   // p^T A p <= 0 (or not a number): A is not positive definite
  non_finite,  // the residual norm is not finite
};

struct PcgResult {
  PcgStatus status;
  int its;     // iterations begun
  double res;  // the last residual norm
};

template <typename Vec, typename CVec, typename Apply, typename Precondition, typename Dot, typename Axpby,
          typename Copy>
PcgResult pcg(Apply &&apply, Precondition &&precondition, Dot &&dot, Axpby &&axpby, Copy &&copy, Vec r, Vec p, Vec Ap,
              Vec z, CVec rhs, Vec x, double rel_tol, double abs_tol, int max_it) {
  apply(x, r);
  axpby(1.0, rhs, -1.0, r);
  double res = std::sqrt(dot(r, r));
  const double tol = std::max(abs_tol, rel_tol * res);
  int it = 0;
  if (!std::isfinite(res)) return {PcgStatus::non_finite, it, res};
  if (!(res > tol)) return {PcgStatus::converged, it, res};
  precondition(r, z);
  copy(p, z);
  double rz = dot(r, z);
  while (true) {
    if (it >= max_it) return {PcgStatus::max_it, it, res};
    ++it;
    apply(p, Ap);
    const double pAp = dot(p, Ap);
    if (!(pAp > 0.0)) return {PcgStatus::breakdown, it, res};
    const double step = rz / pAp;
    axpby(step, p, 1.0, x);
    axpby(-step, Ap, 1.0, r);
    res = std::sqrt(dot(r, r));
    if (res <= tol) return {PcgStatus::converged, it, res};
    if (!std::isfinite(res)) return {PcgStatus::non_finite, it, res};
    precondition(r, z);
    const double rz_new = dot(r, z);
    axpby(1.0, z, rz_new / rz, p);
    rz = rz_new;
  }
}

}  // namespace gdm

#endif
