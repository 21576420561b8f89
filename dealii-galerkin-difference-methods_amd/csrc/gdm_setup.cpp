// gdm_setup.cpp -- host-side setup of the GDM operator engine (see gdm_setup.h).
#include "gdm_setup.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <utility>

namespace gdm {

void gauss_unit(int n, std::vector<double> &x, std::vector<double> &w) {
  // Newton iteration on the Legendre polynomial P_n, started from the
  // asymptotic root estimate; deal.II's QGauss gives the same rule.
  x.assign(n, 0.0);
  w.assign(n, 0.0);
  const double pi = 3.14159265358979323846;
  for (int r = 0; r < n; ++r) {
    double t = std::cos(pi * (r + 0.75) / (n + 0.5));
    double dp = 1.0;
    for (int it = 0; it < 200; ++it) {
      double p0 = 1.0, p1 = t;
      for (int k = 2; k <= n; ++k) {
        const double pk = ((2 * k - 1) * t * p1 - (k - 1) * p0) / k;
        p0 = p1;
        p1 = pk;
      }
      if (n == 1) { p1 = t; p0 = 1.0; }
      dp = n * (t * p1 - p0) / (t * t - 1.0);
      const double dt = p1 / dp;
      t -= dt;
      if (std::abs(dt) < 1e-17) break;
    }
    double p0 = 1.0, p1 = t;
    for (int k = 2; k <= n; ++k) {
      const double pk = ((2 * k - 1) * t * p1 - (k - 1) * p0) / k;
      p0 = p1;
      p1 = pk;
    }
    if (n == 1) { p1 = t; p0 = 1.0; }
    dp = n * (t * p1 - p0) / (t * t - 1.0);
    x[r] = 0.5 * (1.0 - t);  // r = 0 is the largest root -> smallest x
    w[r] = 1.0 / ((1.0 - t * t) * dp * dp);
  }
}

double shape_1d(int p, int cat, int i, double x, int d) {
  // Expand prod_{j != i} (x - t_j) / (t_i - t_j) into monomials, then
  // differentiate d times and evaluate with Horner (the reference stores the
  // same polynomials as monomial coefficient tables, fe.h:323-333).
  std::vector<double> c(p + 2, 0.0);
  c[0] = 1.0;
  int deg = 0;
  double denom = 1.0;
  for (int j = 0; j <= p; ++j) {
    if (j == i) continue;
    const double tj = double(j - cat);
    for (int k = deg + 1; k >= 1; --k) c[k] = c[k - 1] - tj * c[k];
    c[0] *= -tj;
    ++deg;
    denom *= double(i - j);
  }
  for (int k = 0; k <= deg; ++k) c[k] /= denom;
  for (int o = 0; o < d; ++o) {
    for (int k = 0; k < deg; ++k) c[k] = c[k + 1] * double(k + 1);
    --deg;
  }
  if (deg < 0) return 0.0;
  double r = c[deg];
  for (int k = deg - 1; k >= 0; --k) r = r * x + c[k];
  return r;
}

unsigned category(unsigned cell, unsigned p, unsigned n_cells) {
  const unsigned half = p / 2;
  if (cell < half) return cell;
  if (cell < n_cells - half) return half;
  return p + cell - n_cells;
}

unsigned box_offset(unsigned cell, unsigned p, unsigned n_cells) {
  const unsigned half = p / 2;
  if (cell < half) return 0;
  return std::min(n_cells, cell + half + 1) - p;
}

Matrices1D assemble_1d(int p, unsigned n_cells, double h) {
  if (n_cells < (unsigned)p) throw std::invalid_argument("n_subdivisions must be >= fe_degree");
  const int n1 = p + 1, N = int(n_cells) + 1;
  Matrices1D m{Band(N, p), Band(N, p), Band(N, p)};
  std::vector<double> xq, wq;
  gauss_unit(n1, xq, wq);
  const int ncat = std::max(1, p);
  // per category: values and derivatives at the quadrature points
  std::vector<double> val((size_t)ncat * n1 * n1), der((size_t)ncat * n1 * n1);
  for (int cat = 0; cat < ncat; ++cat)
    for (int i = 0; i < n1; ++i)
      for (int q = 0; q < n1; ++q) {
        val[((size_t)cat * n1 + i) * n1 + q] = shape_1d(p, cat, i, xq[q], 0);
        der[((size_t)cat * n1 + i) * n1 + q] = shape_1d(p, cat, i, xq[q], 1) / h;
      }
  for (unsigned c = 0; c < n_cells; ++c) {
    const int cat = int(category(c, p, n_cells));
    const int off = int(box_offset(c, p, n_cells));
    const double *v = &val[(size_t)cat * n1 * n1];
    const double *g = &der[(size_t)cat * n1 * n1];
    for (int i = 0; i < n1; ++i)
      for (int j = 0; j < n1; ++j) {
        double mm = 0, cc = 0, ll = 0;
        for (int q = 0; q < n1; ++q) {
          const double jxw = wq[q] * h;
          mm += v[i * n1 + q] * v[j * n1 + q] * jxw;
          cc += g[i * n1 + q] * v[j * n1 + q] * jxw;
          ll += g[i * n1 + q] * g[j * n1 + q] * jxw;
        }
        m.M(off + i, off + j) += mm;
        m.C(off + i, off + j) += cc;
        m.L(off + i, off + j) += ll;
      }
  }
  return m;
}

WeightedMatrices1D assemble_1d_weighted(int p, unsigned n_cells, double h, const double *f) {
  if (n_cells < (unsigned)p) throw std::invalid_argument("n_subdivisions must be >= fe_degree");
  const int n1 = p + 1, N = int(n_cells) + 1;
  WeightedMatrices1D m{Band(N, p), Band(N, p), Band(N, p)};
  std::vector<double> xq, wq;
  gauss_unit(n1, xq, wq);
  const int ncat = std::max(1, p);
  std::vector<double> val((size_t)ncat * n1 * n1), der((size_t)ncat * n1 * n1);
  for (int cat = 0; cat < ncat; ++cat)
    for (int i = 0; i < n1; ++i)
      for (int q = 0; q < n1; ++q) {
        val[((size_t)cat * n1 + i) * n1 + q] = shape_1d(p, cat, i, xq[q], 0);
        der[((size_t)cat * n1 + i) * n1 + q] = shape_1d(p, cat, i, xq[q], 1) / h;
      }
  for (unsigned c = 0; c < n_cells; ++c) {
    const int cat = int(category(c, p, n_cells));
    const int off = int(box_offset(c, p, n_cells));
    const double *v = &val[(size_t)cat * n1 * n1];
    const double *g = &der[(size_t)cat * n1 * n1];
    const double *fc = f ? f + (size_t)c * n1 : nullptr;
    for (int i = 0; i < n1; ++i)
      for (int j = 0; j < n1; ++j) {
        double mm = 0, cc = 0, ll = 0;
        for (int q = 0; q < n1; ++q) {
          // f == 1 takes assemble_1d's arithmetic, so its bits
          const double jxw = wq[q] * h;
          if (fc) {
            mm += v[i * n1 + q] * v[j * n1 + q] * (jxw * fc[q]);
            cc += g[i * n1 + q] * v[j * n1 + q] * (jxw * fc[q]);
            ll += g[i * n1 + q] * g[j * n1 + q] * (jxw * fc[q]);
          } else {
            mm += v[i * n1 + q] * v[j * n1 + q] * jxw;
            cc += g[i * n1 + q] * v[j * n1 + q] * jxw;
            ll += g[i * n1 + q] * g[j * n1 + q] * jxw;
          }
        }
        m.M(off + i, off + j) += mm;
        m.C(off + i, off + j) += cc;
        m.L(off + i, off + j) += ll;
      }
  }
  return m;
}

std::vector<double> load_vector_1d(int p, unsigned n_cells, double h, const double *f) {
  if (n_cells < (unsigned)p) throw std::invalid_argument("n_subdivisions must be >= fe_degree");
  const int n1 = p + 1;
  std::vector<double> xq, wq, b((size_t)n_cells + 1, 0.0);
  gauss_unit(n1, xq, wq);
  const int ncat = std::max(1, p);
  std::vector<double> val((size_t)ncat * n1 * n1);
  for (int cat = 0; cat < ncat; ++cat)
    for (int i = 0; i < n1; ++i)
      for (int q = 0; q < n1; ++q) val[((size_t)cat * n1 + i) * n1 + q] = shape_1d(p, cat, i, xq[q], 0) * wq[q];
  for (unsigned c = 0; c < n_cells; ++c) {
    const double *v = &val[(size_t)category(c, p, n_cells) * n1 * n1];
    const int off = int(box_offset(c, p, n_cells));
    for (int i = 0; i < n1; ++i) {
      double s = 0.0;
      for (int q = 0; q < n1; ++q) s += v[i * n1 + q] * (f ? f[(size_t)c * n1 + q] : 1.0);
      b[off + i] += s * h;
    }
  }
  return b;
}

std::vector<double> field_points_1d(int p, unsigned n_cells, double lo, double hi) {
  const int n1 = p + 1;
  std::vector<double> xq, wq, x;
  gauss_unit(n1, xq, wq);
  const double h = (hi - lo) / n_cells;
  x.reserve((size_t)n_cells * n1 + 2);
  x.push_back(lo);
  for (unsigned c = 0; c < n_cells; ++c)
    for (int q = 0; q < n1; ++q) x.push_back(lo + (c + xq[q]) * h);
  x.push_back(hi);
  return x;
}

void cholesky_band(const Band &M, std::vector<double> &lrow, std::vector<double> &inv_diag) {
  const int n = M.n, hb = M.hb, wl = hb + 1;
  lrow.assign((size_t)n * wl, 0.0);
  inv_diag.assign(n, 0.0);
  auto Lij = [&](int i, int j) -> double & { return lrow[(size_t)i * wl + (j - i + hb)]; };
  for (int i = 0; i < n; ++i) {
    for (int j = std::max(0, i - hb); j <= i; ++j) {
      double s = M(i, j);
      for (int k = std::max(0, i - hb); k < j; ++k) s -= Lij(i, k) * Lij(j, k);
      if (j == i) {
        if (s <= 0.0) throw std::runtime_error("mass matrix not positive definite");
        Lij(i, i) = std::sqrt(s);
        inv_diag[i] = 1.0 / Lij(i, i);
      } else {
        Lij(i, j) = s / Lij(j, j);
      }
    }
  }
}

Band wave_band_1d(int p, unsigned n_cells, double h, double nitsche_over_hmin, const Matrices1D &m) {
  const int n = m.M.n, last = n - 1;
  Band b(n, p);
  for (int i = 0; i < n; ++i)
    for (int j = std::max(0, i - p); j <= std::min(last, i + p); ++j) b(i, j) = -m.L(i, j);
  if (nitsche_over_hmin > 0.0) {
    // traces of the boundary cells
    const unsigned cl = 0, cr = n_cells - 1;
    const int catl = (int)category(cl, p, n_cells), catr = (int)category(cr, p, n_cells);
    const int offl = (int)box_offset(cl, p, n_cells), offr = (int)box_offset(cr, p, n_cells);
    for (int side = 0; side < 2; ++side) {
      const int cat = side ? catr : catl, off = side ? offr : offl;
      const double x = side ? 1.0 : 0.0, nrm = side ? 1.0 : -1.0;
      for (int ii = 0; ii <= p; ++ii)
        for (int jj = 0; jj <= p; ++jj) {
          const double vi = shape_1d(p, cat, ii, x, 0), vj = shape_1d(p, cat, jj, x, 0);
          const double di = shape_1d(p, cat, ii, x, 1) / h * nrm;
          const double dj = shape_1d(p, cat, jj, x, 1) / h * nrm;
          b(off + ii, off + jj) -= (-di * vj - vi * dj + nitsche_over_hmin * vi * vj);
        }
    }
  }
  return b;
}

Band wave_band_1d_weighted(int p, unsigned n_cells, double h, double nitsche_over_hmin, const double *f) {
  const WeightedMatrices1D m = assemble_1d_weighted(p, n_cells, h, f ? f + 1 : nullptr);
  const int n = m.M.n, last = n - 1;
  Band b(n, p);
  for (int i = 0; i < n; ++i)
    for (int j = std::max(0, i - p); j <= std::min(last, i + p); ++j) b(i, j) = -m.L(i, j);
  if (nitsche_over_hmin > 0.0) {
    const unsigned cl = 0, cr = n_cells - 1;
    const int catl = (int)category(cl, p, n_cells), catr = (int)category(cr, p, n_cells);
    const int offl = (int)box_offset(cl, p, n_cells), offr = (int)box_offset(cr, p, n_cells);
    const size_t n_samples = (size_t)n_cells * (p + 1) + 2;
    for (int side = 0; side < 2; ++side) {
      const int cat = side ? catr : catl, off = side ? offr : offl;
      const double x = side ? 1.0 : 0.0, nrm = side ? 1.0 : -1.0;
      for (int ii = 0; ii <= p; ++ii)
        for (int jj = 0; jj <= p; ++jj) {
          const double vi = shape_1d(p, cat, ii, x, 0), vj = shape_1d(p, cat, jj, x, 0);
          const double di = shape_1d(p, cat, ii, x, 1) / h * nrm;
          const double dj = shape_1d(p, cat, jj, x, 1) / h * nrm;
          // f == 1 takes wave_band_1d's arithmetic, so its bits
          const double blk = -di * vj - vi * dj + nitsche_over_hmin * vi * vj;
          b(off + ii, off + jj) -= f ? f[side ? n_samples - 1 : 0] * blk : blk;
        }
    }
  }
  return b;
}

// Householder tridiagonalisation followed by the implicit QL iteration (the
// classic tred2 / tql2 pair).  V(k, j) = a[j * n + k]: every inner loop of
// both phases then runs along contiguous memory.
void symmetric_eigen(int n, std::vector<double> &a, std::vector<double> &d) {
  d.assign(n, 0.0);
  if (n == 0) return;
  std::vector<double> e(n, 0.0);
  auto V = [&](int k, int j) -> double & { return a[(size_t)j * n + k]; };
  // -- tridiagonalise -------------------------------------------------------
  for (int j = 0; j < n; ++j) d[j] = V(n - 1, j);
  for (int i = n - 1; i > 0; --i) {
    double scale = 0.0, h = 0.0;
    for (int k = 0; k < i; ++k) scale += std::fabs(d[k]);
    if (scale == 0.0) {
      e[i] = d[i - 1];
      for (int j = 0; j < i; ++j) {
        d[j] = V(i - 1, j);
        V(i, j) = 0.0;
        V(j, i) = 0.0;
      }
    } else {
      for (int k = 0; k < i; ++k) {
        d[k] /= scale;
        h += d[k] * d[k];
      }
      double f = d[i - 1];
      double g = std::sqrt(h);
      if (f > 0) g = -g;
      e[i] = scale * g;
      h -= f * g;
      d[i - 1] = f - g;
      for (int j = 0; j < i; ++j) e[j] = 0.0;
      for (int j = 0; j < i; ++j) {
        f = d[j];
        V(j, i) = f;
        g = e[j] + V(j, j) * f;
        for (int k = j + 1; k <= i - 1; ++k) {
          g += V(k, j) * d[k];
          e[k] += V(k, j) * f;
        }
        e[j] = g;
      }
      f = 0.0;
      for (int j = 0; j < i; ++j) {
        e[j] /= h;
        f += e[j] * d[j];
      }
      const double hh = f / (h + h);
      for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
      for (int j = 0; j < i; ++j) {
        f = d[j];
        g = e[j];
        for (int k = j; k <= i - 1; ++k) V(k, j) -= (f * e[k] + g * d[k]);
        d[j] = V(i - 1, j);
        V(i, j) = 0.0;
      }
    }
    d[i] = h;
  }
  // accumulate the transformations
  for (int i = 0; i < n - 1; ++i) {
    V(n - 1, i) = V(i, i);
    V(i, i) = 1.0;
    const double h = d[i + 1];
    if (h != 0.0) {
      for (int k = 0; k <= i; ++k) d[k] = V(k, i + 1) / h;
      for (int j = 0; j <= i; ++j) {
        double g = 0.0;
        for (int k = 0; k <= i; ++k) g += V(k, i + 1) * V(k, j);
        for (int k = 0; k <= i; ++k) V(k, j) -= g * d[k];
      }
    }
    for (int k = 0; k <= i; ++k) V(k, i + 1) = 0.0;
  }
  for (int j = 0; j < n; ++j) {
    d[j] = V(n - 1, j);
    V(n - 1, j) = 0.0;
  }
  V(n - 1, n - 1) = 1.0;
  e[0] = 0.0;
  // -- implicit QL ------------------------------------------------------------
  for (int i = 1; i < n; ++i) e[i - 1] = e[i];
  e[n - 1] = 0.0;
  double f = 0.0, tst1 = 0.0;
  const double eps = std::ldexp(1.0, -52);
  for (int l = 0; l < n; ++l) {
    tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
    int m = l;
    while (m < n - 1 && std::fabs(e[m]) > eps * tst1) ++m;
    if (m > l) {
      int iter = 0;
      do {
        if (++iter > 200) throw std::runtime_error("symmetric_eigen: the QL iteration did not converge");
        double g = d[l];
        double p = (d[l + 1] - g) / (2.0 * e[l]);
        double r = std::hypot(p, 1.0);
        if (p < 0) r = -r;
        d[l] = e[l] / (p + r);
        d[l + 1] = e[l] * (p + r);
        const double dl1 = d[l + 1];
        double h = g - d[l];
        for (int i = l + 2; i < n; ++i) d[i] -= h;
        f += h;
        p = d[m];
        double c = 1.0, c2 = c, c3 = c;
        const double el1 = e[l + 1];
        double s = 0.0, s2 = 0.0;
        for (int i = m - 1; i >= l; --i) {
          c3 = c2;
          c2 = c;
          s2 = s;
          g = c * e[i];
          h = c * p;
          r = std::hypot(p, e[i]);
          e[i + 1] = s * r;
          s = e[i] / r;
          c = p / r;
          p = c * d[i] - s * g;
          d[i + 1] = h + s * (c * g + s * d[i]);
          double *vi = &a[(size_t)i * n], *vi1 = &a[(size_t)(i + 1) * n];
          for (int k = 0; k < n; ++k) {
            h = vi1[k];
            vi1[k] = s * vi[k] + c * h;
            vi[k] = c * vi[k] - s * h;
          }
        }
        p = -s * s2 * c3 * el1 * e[l] / dl1;
        e[l] = s * p;
        d[l] = c * p;
      } while (std::fabs(e[l]) > eps * tst1);
    }
    d[l] = d[l] + f;
    e[l] = 0.0;
  }
  // ascending order
  for (int i = 0; i < n - 1; ++i) {
    int k = i;
    for (int j = i + 1; j < n; ++j)
      if (d[j] < d[k]) k = j;
    if (k != i) {
      std::swap(d[k], d[i]);
      std::swap_ranges(&a[(size_t)i * n], &a[(size_t)i * n] + n, &a[(size_t)k * n]);
    }
  }
}

void fastdiag_1d(int p, unsigned n_cells, double h, double nitsche_over_hmin, std::vector<double> &S,
                 std::vector<double> &lambda) {
  const Matrices1D m = assemble_1d(p, n_cells, h);
  Band B = wave_band_1d(p, n_cells, h, nitsche_over_hmin, m);
  for (double &v : B.a) v = -v;
  fastdiag_pencil(B, m.M, S, lambda);
}

void fastdiag_pencil(const Band &A, const Band &M, std::vector<double> &S, std::vector<double> &lambda) {
  const int n = M.n, hb = M.hb, wl = hb + 1;
  if (n == 0) {
    S.clear();
    lambda.clear();
    return;
  }
  std::vector<double> lrow, invd;
  cholesky_band(M, lrow, invd);
  auto R = [&](int i, int j) { return lrow[(size_t)i * wl + (j - i + hb)]; };  // i - hb <= j <= i
  // forward substitution R y = x in place, x a contiguous vector
  auto forward = [&](double *x) {
    for (int i = 0; i < n; ++i) {
      double s = x[i];
      for (int j = std::max(0, i - hb); j < i; ++j) s -= R(i, j) * x[j];
      x[i] = s * invd[i];
    }
  };
  // c[j * n + i]: column j of A, then of R^-1 A; transposed, again: R^-1 (R^-1 A)^T = R^-1 A R^-T
  std::vector<double> c((size_t)n * n, 0.0), t((size_t)n * n);
  for (int j = 0; j < n; ++j) {
    for (int i = std::max(0, j - hb); i <= std::min(n - 1, j + hb); ++i) c[(size_t)j * n + i] = A(i, j);
    forward(&c[(size_t)j * n]);
  }
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) t[(size_t)i * n + j] = c[(size_t)j * n + i];
  for (int j = 0; j < n; ++j) forward(&t[(size_t)j * n]);
  for (int j = 0; j < n; ++j)
    for (int i = 0; i <= j; ++i) {
      const double v = 0.5 * (t[(size_t)j * n + i] + t[(size_t)i * n + j]);
      t[(size_t)j * n + i] = t[(size_t)i * n + j] = v;
    }
  symmetric_eigen(n, t, lambda);
  // S = R^-T Q column by column (back substitution), signs fixed
  S.assign((size_t)n * n, 0.0);
  for (int j = 0; j < n; ++j) {
    double *x = &t[(size_t)j * n];
    for (int i = n - 1; i >= 0; --i) {
      double s = x[i];
      for (int k = i + 1; k <= std::min(n - 1, i + hb); ++k) s -= R(k, i) * x[k];
      x[i] = s * invd[i];
    }
    int big = 0;
    for (int i = 1; i < n; ++i)
      if (std::fabs(x[i]) > std::fabs(x[big])) big = i;
    const double sg = x[big] < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < n; ++i) S[(size_t)i * n + j] = sg * x[i];
  }
}

ElasticityBands1D elasticity_bands_1d(int p, unsigned n_cells, double h) {
  const Matrices1D m = assemble_1d(p, n_cells, h);
  const int n = m.M.n, last = n - 1;
  ElasticityBands1D b;
  b.M = Band(n, p);
  b.C = Band(n, p);
  b.Ct = Band(n, p);
  b.L = Band(n, p);
  // P A P: rows and columns 0 and n - 1 stay zero
  for (int i = 1; i < last; ++i)
    for (int j = std::max(1, i - p); j <= std::min(last - 1, i + p); ++j) {
      b.M(i, j) = m.M(i, j);
      b.C(i, j) = m.C(i, j);
      b.Ct(i, j) = m.C(j, i);
      b.L(i, j) = m.L(i, j);
    }
  return b;
}

void elasticity_fastdiag_1d(int p, unsigned n_cells, double h, std::vector<double> &S, std::vector<double> &lambda) {
  const ElasticityBands1D b = elasticity_bands_1d(p, n_cells, h);
  const int n = b.M.n, ni = std::max(0, n - 2);
  Band Mi(ni, p), Li(ni, p);
  for (int i = 0; i < ni; ++i)
    for (int j = std::max(0, i - p); j <= std::min(ni - 1, i + p); ++j) {
      Mi(i, j) = b.M(i + 1, j + 1);
      Li(i, j) = b.L(i + 1, j + 1);
    }
  std::vector<double> Si, li;
  fastdiag_pencil(Li, Mi, Si, li);
  S.assign((size_t)n * n, 0.0);
  lambda.assign((size_t)n, 1.0);
  for (int i = 0; i < ni; ++i) {
    lambda[i + 1] = li[i];
    for (int j = 0; j < ni; ++j) S[(size_t)(i + 1) * n + (j + 1)] = Si[(size_t)i * ni + j];
  }
}

FaceTable face_table_1d(int p, unsigned n_cells, double h, unsigned cell_begin, unsigned cell_end) {
  FaceTable t;
  const int n1 = p + 1;
  const unsigned N = n_cells + 1;
  t.n_nodes = int(N);
  t.qstart.assign(N, 0);
  t.qcount.assign(N, 0);
  // A node near a wall lies in the boxes of up to p + p/2 + 1 cells (the
  // first p/2 + 1 cells all use the box [0, p], system.h:228-233), so the row
  // width is the largest count, not (p + 1)^2.
  std::vector<std::pair<unsigned, unsigned>> range(N, {1u, 0u});
  int maxc = 1;
  for (unsigned i = 0; i < N; ++i) {
    unsigned first = ~0u, last = 0;
    for (unsigned c = cell_begin; c < cell_end; ++c) {
      const unsigned off = box_offset(c, p, n_cells);
      if (i < off || i > off + unsigned(p)) continue;
      first = std::min(first, c);
      last = std::max(last, c);
    }
    if (first != ~0u) {
      range[i] = {first, last};
      maxc = std::max(maxc, int(last - first + 1));
    }
  }
  t.wmax = maxc * n1;
  t.w.assign((size_t)N * t.wmax, 0.0);
  std::vector<double> xq, wq;
  gauss_unit(n1, xq, wq);
  for (unsigned i = 0; i < N; ++i) {
    if (range[i].first > range[i].second) continue;
    int m = 0;
    for (unsigned c = range[i].first; c <= range[i].second; ++c) {
      const unsigned off = box_offset(c, p, n_cells);
      const int cat = int(category(c, p, n_cells));
      for (int q = 0; q < n1; ++q)
        t.w[(size_t)i * t.wmax + m++] = shape_1d(p, cat, int(i - off), xq[q], 0) * wq[q] * h;
    }
    t.qstart[i] = int(range[i].first - cell_begin) * n1;
    t.qcount[i] = m;
  }
  return t;
}

Slab slab_partition(unsigned n_cells_last, unsigned n_ranks, unsigned rank) {
  const unsigned stride = (n_cells_last + n_ranks - 1) / n_ranks;
  Slab s;
  s.plane_begin = std::min(rank == 0 ? 0u : stride * rank + 1, n_cells_last + 1);
  s.plane_end = std::min(stride * (rank + 1) + 1, n_cells_last + 1);
  s.cell_begin = std::min(stride * rank, n_cells_last);
  s.cell_end = std::min(stride * (rank + 1), n_cells_last);
  return s;
}

}  // namespace gdm
