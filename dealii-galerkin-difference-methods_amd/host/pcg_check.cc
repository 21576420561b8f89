// pcg_check -- host check of the library's CG template (csrc/gdm_pcg.h) on
// std::vector<double> with a dense matrix; no GPU, no libgdm_hip.  Built with
// -fsanitize=address,undefined (host/Makefile) and run by tests/test_pcg_cpu.py,
// which restates the systems in numpy:
//
//   A[i][j] = 1 / (1 + |i - j|) + (i == j ? i + 1 : 0)   (symmetric positive definite)
//   b[i]    = 1 + (i % 3) / 2 - (i % 5) / 4,  x0 = 0
//
// usage: pcg_check ORDER [--precond none|jacobi|exact] [--mode solve|entry|nan|indefinite]
//                        [--max-it K] [--rel-tol T]
//   entry       abs_tol above |b|: res <= tol at entry
//   nan         b[ORDER / 2] is not a number
//   indefinite  A = diag(1, -1, 1, ...), b[i] = 1 (i even), 2 (i odd): p^T A p <= 0 at the first step
// prints: status, its, applies (calls of apply), hist (the residual norms), x
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../csrc/gdm_pcg.h"

namespace {

using Vector = std::vector<double>;

// x = A^-1 b by Cholesky (A symmetric positive definite, row-major n x n)
struct Cholesky {
  int n;
  Vector L;
  Cholesky(const Vector &A, int n_) : n(n_), L(A) {
    for (int j = 0; j < n; ++j) {
      for (int k = 0; k < j; ++k) L[(size_t)j * n + j] -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
      L[(size_t)j * n + j] = std::sqrt(L[(size_t)j * n + j]);
      for (int i = j + 1; i < n; ++i) {
        for (int k = 0; k < j; ++k) L[(size_t)i * n + j] -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
        L[(size_t)i * n + j] /= L[(size_t)j * n + j];
      }
    }
  }
  void solve(const Vector &b, Vector &x) const {
    x = b;
    for (int i = 0; i < n; ++i) {
      for (int k = 0; k < i; ++k) x[i] -= L[(size_t)i * n + k] * x[k];
      x[i] /= L[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
      for (int k = i + 1; k < n; ++k) x[i] -= L[(size_t)k * n + i] * x[k];
      x[i] /= L[(size_t)i * n + i];
    }
  }
};

const char *status_name(gdm::PcgStatus s) {
  switch (s) {
    case gdm::PcgStatus::converged: return "converged";
    case gdm::PcgStatus::max_it: return "max_it";
    case gdm::PcgStatus::breakdown: return "breakdown";
    default: return "non_finite";
  }
}

void print_vector(const char *name, const Vector &v) {
  std::printf("%s", name);
  for (double e : v) std::printf(" %.17g", e);
  std::printf("\n");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: pcg_check ORDER [--precond P] [--mode M] [--max-it K] [--rel-tol T]\n");
    return 2;
  }
  const int n = std::atoi(argv[1]);
  std::string precond = "none", mode = "solve";
  int max_it = 1000;
  double rel_tol = 1e-10, abs_tol = 0.0;
  for (int i = 2; i + 1 < argc; i += 2) {
    if (!std::strcmp(argv[i], "--precond")) precond = argv[i + 1];
    else if (!std::strcmp(argv[i], "--mode")) mode = argv[i + 1];
    else if (!std::strcmp(argv[i], "--max-it")) max_it = std::atoi(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--rel-tol")) rel_tol = std::atof(argv[i + 1]);
    else {
      std::fprintf(stderr, "pcg_check: unknown option %s\n", argv[i]);
      return 2;
    }
  }
  if (n < 1 || (precond != "none" && precond != "jacobi" && precond != "exact") ||
      (mode != "solve" && mode != "entry" && mode != "nan" && mode != "indefinite")) {
    std::fprintf(stderr, "pcg_check: bad argument\n");
    return 2;
  }

  Vector A((size_t)n * n, 0.0), b((size_t)n), x((size_t)n, 0.0);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) A[(size_t)i * n + j] = 1.0 / (1 + std::abs(i - j)) + (i == j ? i + 1.0 : 0.0);
    b[i] = 1.0 + (i % 3) / 2.0 - (i % 5) / 4.0;
  }
  if (mode == "indefinite") {
    A.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) {
      A[(size_t)i * n + i] = i % 2 ? -1.0 : 1.0;
      b[i] = i % 2 ? 2.0 : 1.0;
    }
    precond = "none";
  }
  if (mode == "nan") b[n / 2] = std::numeric_limits<double>::quiet_NaN();
  if (mode == "entry") abs_tol = 1e3 * n;  // above |b| <= 2 sqrt(n)

  Vector r((size_t)n), p((size_t)n), Ap((size_t)n), z((size_t)n), hist;
  const Cholesky *chol = precond == "exact" ? new Cholesky(A, n) : nullptr;
  int applies = 0;
  auto apply = [&](const Vector *src, Vector *dst) {
    ++applies;
    for (int i = 0; i < n; ++i) {
      double s = 0.0;
      for (int j = 0; j < n; ++j) s += A[(size_t)i * n + j] * (*src)[j];
      (*dst)[i] = s;
    }
  };
  auto precondition = [&](const Vector *rr, Vector *zz) {
    if (chol)
      chol->solve(*rr, *zz);
    else
      for (int i = 0; i < n; ++i) (*zz)[i] = precond == "jacobi" ? (*rr)[i] / A[(size_t)i * n + i] : (*rr)[i];
  };
  // the residual history: every dot(r, r) of the loop is a residual norm squared
  auto dot = [&](const Vector *u, const Vector *v) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += (*u)[i] * (*v)[i];
    if (u == &r && v == &r) hist.push_back(std::sqrt(s));
    return s;
  };
  auto axpby = [&](double a, const Vector *xx, double c, Vector *yy) {
    for (int i = 0; i < n; ++i) (*yy)[i] = a * (*xx)[i] + c * (*yy)[i];
  };
  auto copy = [](Vector *dst, const Vector *src) { *dst = *src; };

  const gdm::PcgResult res = gdm::pcg(apply, precondition, dot, axpby, copy, &r, &p, &Ap, &z,
                                      static_cast<const Vector *>(&b), &x, rel_tol, abs_tol, max_it);
  delete chol;
  std::printf("status %s\nits %d\napplies %d\nres %.17g\n", status_name(res.status), res.its, applies, res.res);
  print_vector("hist", hist);
  print_vector("x", x);
  return 0;
}
