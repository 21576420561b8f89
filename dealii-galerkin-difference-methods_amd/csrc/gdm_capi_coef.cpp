// gdm_capi_coef.cpp -- C ABI of the variable coefficient kappa and density rho of
// the wave operator (separable and on the Gauss grid), their solves, and the
// fast diagonalisation that preconditions them (declared in include/gdm_hip.h).
#include <cmath>
#include <cstdio>
#include <utility>

#include "gdm_capi_internal.h"
#include "gdm_fastdiag.h"

using namespace gdm_detail;

namespace {

// samples of a factor along direction d
size_t coef_samples(const gdm_mesh_desc *mesh, int d) {
  return (size_t)mesh->n_subdivisions[d] * (mesh->fe_degree + 1) + 2;
}

// the domain mean of a separable function: sum_t prod_d mean(f_td), the Gauss
// weights sum to 1 per cell
double separable_mean(const gdm_op *op, int n_terms, const gdm_coef_term *terms) {
  const int n1 = op->p + 1;
  std::vector<double> xq, wq;
  gdm::gauss_unit(n1, xq, wq);
  double mean = 0.0;
  for (int t = 0; t < n_terms; ++t) {
    double prod = 1.0;
    for (int d = 0; d < op->dim; ++d) {
      const double *f = terms[t].factor[d];
      if (!f) continue;
      const int ncell = op->mesh.n_subdivisions[d];
      double s = 0.0;
      for (int c = 0; c < ncell; ++c)
        for (int q = 0; q < n1; ++q) s += wq[q] * f[1 + (size_t)c * n1 + q];
      prod *= s / ncell;
    }
    mean += prod;
  }
  return mean;
}

}  // namespace

// ---- separable coefficient of the wave operator (gdm_vardiff.hip) -----------

void gdm_detail::coef_apply(gdm_op *op, const double *src, double *dst) {
  if (op->coef.grid) {
    gdmk::CgArgs g = op->coef.grid_args;
    g.src = src;
    g.dst = dst;
    hip_check(gdmk::launch_cg(op->p, g, op->stream), "grid coefficient apply launch");
    // the box faces one after the other: they share the edge and corner columns and the scratch
    for (const gdmk::CgFace &F : op->coef.grid_faces)
      hip_check(gdmk_cg_face(F, src, op->coef.kappa_bc, op->coef.face_scratch, dst, op->stream),
                "grid coefficient face launch");
    return;
  }
  gdmk::DiffArgs a = op->coef.args;
  a.src = src;
  a.dst = dst;
  hip_check(gdmk::launch_diff(op->p, a, op->coef.lds, op->stream), "coefficient apply launch");
}

namespace {

// Build the launch plan, tables and scratch of a coefficient into `nc` (every
// device allocation is recorded in nc.allocations as it is made).
void build_coef(gdm_op *op, int n_terms, const gdm_coef_term *terms, gdm_op::Coef &nc) {
  const int p = op->p;
  std::vector<void *> &made = nc.allocations;
  nc.n_terms = n_terms;
  const double noh = nitsche_over_hmin(&op->mesh, op->nitsche);
  // distinct device tables: (kernel axis, M or B, factor array); terms that
  // pass the same array share them
  struct Table {
    int ax, which;
    const double *f;
    double *dev;
  };
  std::vector<Table> tabs;
  auto table = [&](int ax, int which, const double *f) -> const double * {
    const int d = op->kdir[ax];
    if (d < 0) f = nullptr;
    for (const Table &T : tabs)
      if (T.ax == ax && T.which == which && T.f == f) return T.dev;
    gdm::Band B(1, p);
    if (d < 0) {
      if (which == 0) B(0, 0) = 1.0;  // a trivial axis: M = (1), B = (0)
    } else {
      const unsigned ncell = (unsigned)op->mesh.n_subdivisions[d];
      const double h = (op->mesh.hi[d] - op->mesh.lo[d]) / ncell;
      B = which ? gdm::wave_band_1d_weighted(p, ncell, h, noh, f)
                : gdm::assemble_1d_weighted(p, ncell, h, f ? f + 1 : nullptr).M;
    }
    tabs.push_back(Table{ax, which, f, up(made, padded_table(B, ax, gdmk::diff_y_rows(B.n)))});
    return tabs.back().dev;
  };
  gdmk::DiffArgs &a = nc.args;
  a = gdmk::DiffArgs{};
  a.Nx = op->K[0];
  a.Ny = op->K[1];
  a.Nz = op->K[2];
  a.n_terms = n_terms;
  for (int t = 0; t < n_terms; ++t) {
    const double *f[3];
    for (int ax = 0; ax < 3; ++ax) f[ax] = op->kdir[ax] < 0 ? nullptr : terms[t].factor[op->kdir[ax]];
    a.xm[t] = table(0, 0, f[0]);
    a.xb[t] = table(0, 1, f[0]);
    a.ym[t] = table(1, 0, f[1]);
    a.yb[t] = table(1, 1, f[1]);
    a.zm[t] = table(2, 0, f[2]);
    a.zb[t] = table(2, 1, f[2]);
  }
  nc.lds = gdmk::diff_lds(p, n_terms);
  if (nc.lds > 160 * 1024) throw std::runtime_error("coefficient: the launch plan exceeds the LDS of a CU");
  hip_check(gdmk::diff_prepare(p, nc.lds), "coefficient: LDS limit");

  nc.mean = separable_mean(op, n_terms, terms);

  // kappa at the boundary points: Gauss entries in the tangential directions,
  // the lo / hi entry in the normal one
  const int64_t nbc = op->layout.n_bc_points;
  std::vector<double> kbc((size_t)std::max<int64_t>(nbc, 1), 0.0);
  for (const Face &F : op->faces) {
    const int e0 = F.t0.dim_index, e1 = F.t1.dim_index;
    for (int t = 0; t < n_terms; ++t) {
      const double *fn = terms[t].factor[F.d];
      const double end = fn ? fn[F.side ? coef_samples(&op->mesh, F.d) - 1 : 0] : 1.0;
      const double *f0 = e0 < 0 ? nullptr : terms[t].factor[e0], *f1 = e1 < 0 ? nullptr : terms[t].factor[e1];
      for (int64_t i1 = 0; i1 < F.t1.Q; ++i1)
        for (int64_t i0 = 0; i0 < F.t0.Q; ++i0)
          kbc[(size_t)(F.offset + i1 * F.t0.Q + i0)] += end * (f0 ? f0[1 + i0] : 1.0) * (f1 ? f1[1 + i1] : 1.0);
    }
  }
  nc.kappa_bc = up(made, kbc);
  nc.g_scaled = up(made, std::vector<double>(kbc.size(), 0.0));
  const size_t n = (size_t)std::max<int64_t>(op->layout.n_owned, 1);
  for (double *&v : nc.cg) v = up(made, std::vector<double>(n, 0.0));
  nc.active = true;
}

// ---- general coefficient on the Gauss grid (gdm_coefgrid.hip) ---------------

// the kernel's tables of one direction: per Gauss point the first node of the
// cell's DoF box, the p + 1 basis values and physical derivatives, w_q h
struct CoefGridTables {
  std::vector<int32_t> first;
  std::vector<double> val, der, w;
};
void coef_grid_tables(int p, unsigned ncell, double h, CoefGridTables &T) {
  const int n1 = p + 1;
  std::vector<double> xq, wq;
  gdm::gauss_unit(n1, xq, wq);
  const size_t Q = (size_t)ncell * n1;
  T.first.resize(Q);
  T.w.resize(Q);
  T.val.resize(Q * n1);
  T.der.resize(Q * n1);
  for (unsigned c = 0; c < ncell; ++c) {
    const int cat = (int)gdm::category(c, (unsigned)p, ncell), off = (int)gdm::box_offset(c, (unsigned)p, ncell);
    for (int q = 0; q < n1; ++q) {
      const size_t g = (size_t)c * n1 + q;
      T.first[g] = off;
      T.w[g] = wq[q] * h;
      for (int i = 0; i < n1; ++i) {
        T.val[g * n1 + i] = gdm::shape_1d(p, cat, i, xq[q], 0);
        T.der[g * n1 + i] = gdm::shape_1d(p, cat, i, xq[q], 1) / h;
      }
    }
  }
}

}  // namespace

// The kernel axes of the tensor Gauss grid, built once per operator by
// gdm_op_create (single rank, non-periodic) into op->ev: the device tables that
// gdm_coefgrid.hip, gdm_massgrid.hip and gdm_evalgrid.hip share, host copies of
// the box offsets and point ranges for the footprint checks, the box volume.
void gdm_detail::build_grid_axes(gdm_op *op) {
  const int p = op->p, n1 = p + 1;
  gdm_op::Eval &ev = op->ev;
  ev.volume = 1.0;
  for (int k = 0; k < 3; ++k) {
    const int d = op->kdir[k];
    CoefGridTables T;
    int N = 1;
    if (d < 0) {
      T.first.assign(1, 0);
      T.w.assign(1, 1.0);
      T.val.assign((size_t)n1, 0.0);
      T.der.assign((size_t)n1, 0.0);
      T.val[0] = 1.0;
    } else {
      const unsigned ncell = (unsigned)op->mesh.n_subdivisions[d];
      coef_grid_tables(p, ncell, (op->mesh.hi[d] - op->mesh.lo[d]) / ncell, T);
      N = op->N[d];
      ev.volume *= op->mesh.hi[d] - op->mesh.lo[d];
    }
    const int Q = (int)T.first.size();
    // the Gauss points whose box holds node i: a contiguous range (the boxes move monotonically)
    std::vector<int32_t> qlo((size_t)N, Q), qhi((size_t)N, 0);
    for (int q = 0; q < Q; ++q)
      for (int i = T.first[q]; i <= std::min(N - 1, T.first[q] + p); ++i) {
        qlo[(size_t)i] = std::min(qlo[(size_t)i], q);
        qhi[(size_t)i] = std::max(qhi[(size_t)i], q + 1);
      }
    gdmk::CgAxis &A = ev.ax[k];
    A.N = N;
    A.Q = Q;
    A.first = keep(op, dev_upload(T.first));
    A.val = keep(op, dev_upload(T.val));
    A.der = keep(op, dev_upload(T.der));
    A.w = keep(op, dev_upload(T.w));
    A.qlo = keep(op, dev_upload(qlo));
    A.qhi = keep(op, dev_upload(qhi));
    ev.first[k] = std::move(T.first);
    ev.qlo[k] = std::move(qlo);
    ev.qhi[k] = std::move(qhi);
  }
}

// The operator's kernel axes into ax[3] for a kernel with compile-time bounds
// on a tile's footprint (tile, Gauss points and node span of kernel axes x and
// y), which are checked here.  Returns the volume of the box.
double gdm_detail::grid_axes(const gdm_op *op, const int tile[2], const int nq_max[2], const int span_max[2],
                             const char *what, gdmk::CgAxis ax[3]) {
  const gdm_op::Eval &ev = op->ev;
  if (ev.first[0].empty()) throw std::runtime_error(std::string(what) + ": the operator has no grid axes");
  for (int k = 0; k < 3; ++k) {
    const int N = ev.ax[k].N, p = op->p;
    const std::vector<int32_t> &first = ev.first[k], &qlo = ev.qlo[k], &qhi = ev.qhi[k];
    for (int i0 = 0; i0 < N && k < 2; i0 += tile[k]) {
      const int il = std::min(N, i0 + tile[k]) - 1;
      const int q0 = qlo[(size_t)i0], q1 = qhi[(size_t)il];
      const int span = std::min(first[(size_t)q1 - 1] + p, N - 1) - first[(size_t)q0] + 1;
      if (q1 <= q0 || q1 - q0 > nq_max[k] || span > span_max[k])
        throw std::runtime_error(std::string(what) + ": a tile's footprint exceeds the kernel's bounds");
    }
    ax[k] = ev.ax[k];
  }
  return ev.volume;
}

namespace {

// One reduction over n samples on the operator's stream: the Gauss-weighted sum
// into *sum (axes_dev NULL: the samples carry no weights, the sum means nothing)
// through the device scratch partial[2][kGridBlocks] (1024 block partials,
// summed here in a fixed order); false = a sample is not finite or not positive
constexpr int kGridBlocks = 1024;
bool grid_reduce(gdm_op *op, const double *samples, int64_t n, const gdmk::CgAxis *axes_dev, double *partial,
                 const char *what, double *sum) {
  hip_check(gdmk_cg_reduce(samples, n, axes_dev, partial, partial + kGridBlocks, kGridBlocks, op->stream), what);
  std::vector<double> host((size_t)2 * kGridBlocks);
  hip_check(hipMemcpyAsync(host.data(), partial, sizeof(double) * host.size(), hipMemcpyDeviceToHost, op->stream),
            "copy");
  hip_check(hipStreamSynchronize(op->stream), "hipStreamSynchronize");
  double bad = 0.0;
  *sum = 0.0;
  for (int b = 0; b < kGridBlocks; ++b) {
    *sum += host[(size_t)b];
    bad += host[(size_t)kGridBlocks + b];
  }
  return bad == 0.0;
}

// Build the launch plan, tables and scratch of a grid coefficient into `nc`,
// and run the reduction over kq (and kbc): false = a sample is not finite or
// not positive.
bool build_coef_grid(gdm_op *op, const double *kq, const double *kbc, gdm_op::Coef &nc) {
  const int p = op->p, n1 = p + 1;
  std::vector<void *> &made = nc.allocations;
  nc.grid = true;
  gdmk::CgArgs &a = nc.grid_args;
  a = gdmk::CgArgs{};
  a.kq = kq;
  const int tile[2] = {gdmk::cg_tx(p), gdmk::cg_ty(p)}, nq_max[2] = {gdmk::cg_nqx(p), gdmk::cg_nqy(p)},
            span_max[2] = {gdmk::cg_sx(p), gdmk::cg_sy(p)};
  const double volume = grid_axes(op, tile, nq_max, span_max, "grid coefficient", a.ax);
  hip_check(gdmk::cg_prepare(p), "grid coefficient: LDS limit");

  // the box faces (Nitsche part)
  const int64_t nbc = op->layout.n_bc_points;
  int64_t max_face = 1;
  if (op->nitsche > 0.0) {
    const int64_t stride[3] = {1, op->N[0], (int64_t)op->N[0] * op->N[1]};
    auto axis_of = [&](int e) {  // kernel axis of reference direction e (-1: any trivial axis)
      for (int k = 0; k < 3; ++k)
        if (op->kdir[k] == e) return k;
      throw std::runtime_error("grid coefficient: direction without a kernel axis");
    };
    for (const Face &F : op->faces) {
      gdmk::CgFace f{};
      const gdmk::CgAxis &A0 = a.ax[axis_of(F.t0.dim_index)], &A1 = a.ax[axis_of(F.t1.dim_index)];
      f.n0 = F.t0.n_nodes;
      f.n1 = F.t1.n_nodes;
      f.Q0 = F.t0.Q;
      f.Q1 = F.t1.Q;
      f.nk = n1;
      f.first0 = A0.first;
      f.val0 = A0.val;
      f.first1 = A1.first;
      f.val1 = A1.val;
      f.qs0 = F.t0.qs;
      f.qc0 = F.t0.qc;
      f.w0 = F.t0.w;
      f.wmax0 = F.t0.wmax;
      f.qs1 = F.t1.qs;
      f.qc1 = F.t1.qc;
      f.w1 = F.t1.w;
      f.wmax1 = F.t1.wmax;
      f.stride0 = F.t0.stride;
      f.stride1 = F.t1.stride;
      f.stride_d = stride[F.d];
      f.base = (F.side ? (int64_t)(op->N[F.d] - 1 - p) : 0) * stride[F.d];
      f.goff = F.offset;
      f.gamma = nitsche_over_hmin(&op->mesh, op->nitsche);
      const unsigned ncd = (unsigned)op->mesh.n_subdivisions[F.d];
      const double hd = (op->mesh.hi[F.d] - op->mesh.lo[F.d]) / ncd;
      const int cat = F.side ? (int)gdm::category(ncd - 1, (unsigned)p, ncd) : 0;
      const double xs = F.side ? 1.0 : 0.0, nrm = F.side ? 1.0 : -1.0;
      for (int k = 0; k < n1; ++k) {
        f.tr[k] = gdm::shape_1d(p, cat, k, xs, 0);
        f.dk[k] = nrm * gdm::shape_1d(p, cat, k, xs, 1) / hd;
      }
      if (f.Q0 != A0.Q || f.Q1 != A1.Q || f.n0 != A0.N || f.n1 != A1.N)
        throw std::runtime_error("grid coefficient: face and volume tables disagree");
      max_face = std::max(max_face, (int64_t)f.Q0 * f.Q1);
      nc.grid_faces.push_back(f);
    }
    nc.kappa_bc = const_cast<double *>(kbc);  // borrowed, read only
    nc.g_scaled = up(made, std::vector<double>((size_t)std::max<int64_t>(nbc, 1), 0.0));
    nc.face_scratch = up(made, std::vector<double>((size_t)(2 * max_face), 0.0));
  }
  const size_t n = (size_t)std::max<int64_t>(op->layout.n_owned, 1);
  for (double *&v : nc.cg) v = up(made, std::vector<double>(n, 0.0));

  // one reduction over kq (and kbc): the Gauss-weighted mean, and the samples that are not finite or not positive
  std::vector<gdmk::CgAxis> axes(a.ax, a.ax + 3);
  const gdmk::CgAxis *axes_dev = up(made, axes);
  double *part = up(made, std::vector<double>((size_t)4 * kGridBlocks, 0.0));
  const int64_t nq = (int64_t)a.ax[0].Q * a.ax[1].Q * a.ax[2].Q;
  double sum = 0.0, sum_bc = 0.0;
  bool ok = grid_reduce(op, kq, nq, axes_dev, part, "grid coefficient reduction", &sum);
  if (op->nitsche > 0.0 && nbc > 0)
    ok &= grid_reduce(op, kbc, nbc, nullptr, part + 2 * kGridBlocks, "grid coefficient reduction", &sum_bc);
  nc.mean = sum / volume;
  nc.active = true;
  return ok;
}

// ---- separable density of the wave operator (gdm_varmass.hip) ---------------

// dst = M[rho] src (+ c * add)
void density_apply(gdm_op *op, const double *src, double *dst, const double *add = nullptr, double c = 0.0) {
  if (op->dens.grid) {
    gdmk::MgArgs g = op->dens.grid_args;
    g.src = src;
    g.dst = dst;
    g.add = add;
    g.c = c;
    hip_check(gdmk::launch_mg(op->p, g, op->stream), "grid density apply launch");
    return;
  }
  gdmk::VarMassArgs a = op->dens.args;
  a.src = src;
  a.dst = dst;
  a.add = add;
  a.c = c;
  hip_check(gdmk::launch_varmass(op->p, a, op->dens.lds, op->stream), "density apply launch");
}

// M_d[f] of reference direction d, f sampled at gdm_field_points (NULL: 1)
void density_band(const gdm_mesh_desc *mesh, int d, const double *f, gdm::Band &M) {
  const unsigned ncell = (unsigned)mesh->n_subdivisions[d];
  const double h = (mesh->hi[d] - mesh->lo[d]) / ncell;
  M = gdm::assemble_1d_weighted(mesh->fe_degree, ncell, h, f ? f + 1 : nullptr).M;
}

// Build the launch plan, tables and scratch of a density into `nd` (every
// device allocation is recorded in nd.allocations as it is made).
void build_density(gdm_op *op, int n_terms, const gdm_coef_term *terms, gdm_op::Density &nd) {
  const int p = op->p;
  std::vector<void *> &made = nd.allocations;
  nd.n_terms = n_terms;
  // distinct tables: (kernel axis, factor array); terms that pass the same
  // array share them
  struct Table {
    int ax;
    const double *f;
    double *dev;
    gdm::Band B;
  };
  std::vector<Table> tabs;
  auto table = [&](int ax, const double *f) -> size_t {
    const int d = op->kdir[ax];
    if (d < 0) f = nullptr;
    for (size_t i = 0; i < tabs.size(); ++i)
      if (tabs[i].ax == ax && tabs[i].f == f) return i;
    gdm::Band B = identity_band(p);
    if (d >= 0) density_band(&op->mesh, d, f, B);
    tabs.push_back(Table{ax, f, up(made, padded_table(B, ax, gdmk::varmass_y_rows(B.n))), B});
    return tabs.size() - 1;
  };
  gdmk::VarMassArgs &a = nd.args;
  a = gdmk::VarMassArgs{};
  a.Nx = op->K[0];
  a.Ny = op->K[1];
  a.Nz = op->K[2];
  a.n_terms = n_terms;
  size_t term_tab[gdmk::VMASS_MAX_TERMS][3];
  for (int t = 0; t < n_terms; ++t) {
    for (int ax = 0; ax < 3; ++ax)
      term_tab[t][ax] = table(ax, op->kdir[ax] < 0 ? nullptr : terms[t].factor[op->kdir[ax]]);
    a.xm[t] = tabs[term_tab[t][0]].dev;
    a.ym[t] = tabs[term_tab[t][1]].dev;
    a.zm[t] = tabs[term_tab[t][2]].dev;
  }
  nd.lds = gdmk::varmass_lds(p, n_terms);
  if (nd.lds > 160 * 1024) throw std::runtime_error("density: the launch plan exceeds the LDS of a CU");
  hip_check(gdmk::varmass_prepare(p, nd.lds), "density: LDS limit");

  nd.mean = separable_mean(op, n_terms, terms);

  // diag(M_d[r_td]) per term and kernel axis (gdm_density_diag)
  nd.band_diag.assign((size_t)n_terms * 3, std::vector<double>());
  for (int t = 0; t < n_terms; ++t)
    for (int ax = 0; ax < 3; ++ax) {
      std::vector<double> &v = nd.band_diag[(size_t)t * 3 + ax];
      v.assign((size_t)op->K[ax], 1.0);
      if (op->kdir[ax] < 0) continue;
      const gdm::Band &B = tabs[term_tab[t][ax]].B;
      for (int i = 0; i < op->K[ax]; ++i) v[(size_t)i] = B(i, i);
    }

  const size_t n = (size_t)std::max<int64_t>(op->layout.n_owned, 1);
  if (n_terms == 1) {
    // M[rho]^-1 = (x)_d M_d[r_d]^-1: the two-sweep line tables of every factor;
    // a negative factor is factored as -M_d[r_d] (the signs multiply to +1)
    for (int ax = 0; ax < 3; ++ax) {
      if (op->kdir[ax] < 0) continue;
      gdm::Band B = tabs[term_tab[0][ax]].B;
      if (B(0, 0) < 0.0)
        for (double &v : B.a) v = -v;
      std::vector<double> lrow, invd;
      gdm::cholesky_band(B, lrow, invd);
      lrow.resize(lrow.size() + (size_t)p * (p + 1), 0.0);  // zero pad for the backward sweep
      nd.tab[ax].lrow = up(made, lrow);
      nd.tab[ax].invd = up(made, invd);
      nd.axis_tab[ax] = &nd.tab[ax];
    }
  } else {
    // W = diag(M[rho]) / diag(M) = sum_t prod_d diag(M_d[r_td]) / prod_d diag(M_d)
    std::vector<std::vector<double>> dg((size_t)n_terms * 3);
    for (int t = 0; t < n_terms; ++t)
      for (int ax = 0; ax < 3; ++ax) {
        std::vector<double> &v = dg[(size_t)t * 3 + ax];
        v.assign((size_t)op->K[ax], 1.0);
        if (op->kdir[ax] < 0) continue;
        const gdm::Band &B = tabs[term_tab[t][ax]].B;
        const gdm::Band M = mesh_mass_1d(&op->mesh, op->kdir[ax]);
        for (int i = 0; i < op->K[ax]; ++i) v[(size_t)i] = B(i, i) / M(i, i);
      }
    std::vector<double> w(n, 1.0);
    const int Nx = op->K[0], Ny = op->K[1], Nz = op->K[2];
    if (op->layout.n_owned == (int64_t)Nx * Ny * Nz)
      for (int z = 0; z < Nz; ++z)
        for (int y = 0; y < Ny; ++y)
          for (int x = 0; x < Nx; ++x) {
            double s = 0.0;
            for (int t = 0; t < n_terms; ++t)
              s += dg[(size_t)t * 3][(size_t)x] * dg[(size_t)t * 3 + 1][(size_t)y] * dg[(size_t)t * 3 + 2][(size_t)z];
            // a density that is not positive is the caller's error: the CG reports the breakdown
            w[((size_t)z * Ny + y) * Nx + x] = s > 0.0 ? 1.0 / std::sqrt(s) : 1.0;
          }
    nd.w_isqrt = up(made, w);
  }
  for (double *&v : nd.cg) v = up(made, std::vector<double>(n, 0.0));
  nd.active = true;
}

// ---- general density on the Gauss grid (gdm_massgrid.hip) -------------------

// W^-1/2 = (diag M[rho] / diag M)^-1/2 of a grid density from the samples as they are
// now: the kernel's diagonal mode into a CG vector, then the ratio (two launches)
void density_grid_scaling(gdm_op *op, gdm_op::Density &D) {
  gdmk::MgArgs g = D.grid_args;
  g.dst = D.cg[2];
  hip_check(gdmk::launch_mg_diag(op->p, g, op->stream), "grid density diagonal launch");
  hip_check(gdmk_mg_wisqrt(op->layout.n_owned, D.cg[2], D.mdiag, D.w_isqrt, op->stream), "grid density scaling");
}

// One reduction over the samples of a grid density: the Gauss-weighted mean into
// *mean; false = a sample is not finite or not positive
bool density_grid_reduce(gdm_op *op, const gdm_op::Density &D, double *mean) {
  const gdmk::MgArgs &a = D.grid_args;
  const int64_t nq = (int64_t)a.ax[0].Q * a.ax[1].Q * a.ax[2].Q;
  double sum = 0.0;
  const bool ok = grid_reduce(op, a.rq, nq, D.grid_axes_dev, D.grid_partial, "grid density reduction", &sum);
  *mean = sum / D.volume;
  return ok;
}

// Build the launch plan, tables and scratch of a grid density into `nd`, run the
// reduction over rq (false = a sample is not finite or not positive) and form
// W^-1/2 = (diag M[rho] / diag M)^-1/2 of the preconditioner on the device.
bool build_density_grid(gdm_op *op, const double *rq, gdm_op::Density &nd) {
  const int p = op->p;
  std::vector<void *> &made = nd.allocations;
  nd.grid = true;
  nd.n_terms = 0;
  gdmk::MgArgs &a = nd.grid_args;
  a = gdmk::MgArgs{};
  a.rq = rq;
  const int tile[2] = {gdmk::mg_tx(p), gdmk::mg_ty(p)}, nq_max[2] = {gdmk::mg_nqx(p), gdmk::mg_nqy(p)},
            span_max[2] = {gdmk::mg_sx(p), gdmk::mg_sy(p)};
  const double volume = grid_axes(op, tile, nq_max, span_max, "grid density", a.ax);
  if ((int64_t)a.ax[0].N * a.ax[1].N * a.ax[2].N != op->layout.n_owned)
    throw std::runtime_error("grid density: the kernel axes do not cover the owned DoFs");
  int n_cu = 0;
  hip_check(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, op->device), "hipDeviceGetAttribute");
  nd.zc_auto = a.zc = gdmk::mg_pick_zc(p, a.ax[0].N, a.ax[1].N, a.ax[2].N, n_cu);
  hip_check(gdmk::mg_prepare(p), "grid density: LDS limit");
  const size_t n = (size_t)std::max<int64_t>(op->layout.n_owned, 1);
  for (double *&v : nd.cg) v = up(made, std::vector<double>(n, 0.0));
  nd.w_isqrt = up(made, std::vector<double>(n, 1.0));
  nd.mdiag = up(made, mass_diagonal_owned(op));

  std::vector<gdmk::CgAxis> axes(a.ax, a.ax + 3);
  nd.grid_axes_dev = up(made, axes);
  nd.grid_partial = up(made, std::vector<double>((size_t)2 * kGridBlocks, 0.0));
  nd.volume = volume;
  double mean = 0.0;
  if (!density_grid_reduce(op, nd, &mean)) return false;
  nd.mean = mean;
  density_grid_scaling(op, nd);
  hip_check(hipStreamSynchronize(op->stream), "hipStreamSynchronize");
  nd.active = true;
  return true;
}

// the refusals shared by the gdm_op_set_* calls of the coefficient and the density
// (assembled_for: what the cut-cell rows of a cut handle are assembled for); 0 = ok
int check_set_op(gdm_op *op, const char *what, const char *assembled_for) {
  const std::string w(what);
  if (!op) return fail(GDM_ERR_ARG, "op is NULL");
  if (op->kind != GDM_OP_WAVE) return fail(GDM_ERR_UNSUPPORTED, w + ": wave operators only");
  if (op->cut_inner)
    return fail(GDM_ERR_UNSUPPORTED, w + ": the cut-cell rows of a cut handle are assembled for " + assembled_for);
  if (op->mesh.n_ranks != 1) return fail(GDM_ERR_UNSUPPORTED, w + ": single rank only");
  if (op->mesh.periodic) return fail(GDM_ERR_UNSUPPORTED, w + ": not with periodic constraints");
  return GDM_OK;
}

// the screening of (n_terms, terms) shared by gdm_op_set_coefficient and
// gdm_op_set_density: the factor samples are finite, and the factors of a
// one-term `noun` keep their sign and never vanish; 0 = ok
int check_factors(const gdm_op *op, int n_terms, const gdm_coef_term *terms, const char *what, const char *noun) {
  const std::string w(what);
  if (n_terms < 0 || n_terms > GDM_COEF_MAX_TERMS)
    return fail(GDM_ERR_ARG, w + ": n_terms must be in [0, GDM_COEF_MAX_TERMS]");
  if (n_terms > 0 && !terms) return fail(GDM_ERR_ARG, w + ": terms is NULL");
  for (int t = 0; t < n_terms; ++t)
    for (int d = 0; d < op->dim; ++d) {
      const double *f = terms[t].factor[d];
      if (!f) continue;
      const size_t n = coef_samples(&op->mesh, d);
      for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(f[i])) return fail(GDM_ERR_ARG, w + ": a factor sample is not finite");
        if (n_terms == 1 && !(f[i] * f[0] > 0.0))
          return fail(GDM_ERR_ARG, w + ": a factor of a one-term " + noun + " vanishes or changes sign");
      }
    }
  return GDM_OK;
}

// install `nc` as the operator's coefficient (applies in flight read the old tables)
void install_coef(gdm_op *op, gdm_op::Coef &nc) {
  hip_check(hipStreamSynchronize(op->stream), "hipStreamSynchronize");
  for (void *ptr : op->coef.allocations) (void)hipFree(ptr);
  op->coef = std::move(nc);
}

// install `nd` as the operator's density (applies in flight read the old tables)
void install_density(gdm_op *op, gdm_op::Density &nd) {
  hip_check(hipStreamSynchronize(op->stream), "hipStreamSynchronize");
  for (void *ptr : op->dens.allocations) (void)hipFree(ptr);
  op->dens = std::move(nd);
  // the pointers into the moved-from object
  for (int ax = 0; ax < 3; ++ax) op->dens.axis_tab[ax] = op->dens.axis_tab[ax] ? &op->dens.tab[ax] : nullptr;
}

}  // namespace

extern "C" {

int gdm_coef_matrix_1d(const gdm_mesh_desc *mesh, double nitsche, int axis, int which, const double *f,
                       double *band_host) {
  if (int rc = check_field_mesh(mesh, axis)) return rc;
  if (!band_host) return fail(GDM_ERR_ARG, "band_host is NULL");
  if (which != 0 && which != 1) return fail(GDM_ERR_ARG, "which: 0 = M[f], 1 = B[f]");
  if (!std::isfinite(nitsche)) return fail(GDM_ERR_ARG, "nitsche is not finite");
  for (int d = 0; d < mesh->dim; ++d)
    if (mesh->n_subdivisions[d] < 1 || !(mesh->hi[d] > mesh->lo[d])) return fail(GDM_ERR_ARG, "empty box");
  GDM_GUARD_BEGIN
  const unsigned nc = (unsigned)mesh->n_subdivisions[axis];
  const double h = (mesh->hi[axis] - mesh->lo[axis]) / nc;
  const gdm::Band B = which ? gdm::wave_band_1d_weighted(mesh->fe_degree, nc, h, nitsche_over_hmin(mesh, nitsche), f)
                            : gdm::assemble_1d_weighted(mesh->fe_degree, nc, h, f ? f + 1 : nullptr).M;
  std::copy(B.a.begin(), B.a.end(), band_host);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_coef_tile(int fe_degree, int dim, int *tile_x, int *tile_y, int *z_chunk) {
  if (int rc = check_tile_query(fe_degree, dim)) return rc;
  return tile_answer(gdmk::DIFF_TX, gdmk::DIFF_TY, gdmk::DIFF_ZC, tile_x, tile_y, z_chunk);
}

int gdm_op_set_coefficient(gdm_op *op, int n_terms, const gdm_coef_term *terms) {
  if (int rc = check_set_op(op, "gdm_op_set_coefficient", "the constant coefficient")) return rc;
  if (int rc = check_factors(op, n_terms, terms, "gdm_op_set_coefficient", "coefficient")) return rc;
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  return build_and_install<gdm_op::Coef>(op, n_terms > 0, [&](gdm_op::Coef &nc) {
    build_coef(op, n_terms, terms, nc);
    return true;
  }, install_coef, "");
  GDM_GUARD_END
}

int gdm_coef_grid_tile(int fe_degree, int dim, int *tile_x, int *tile_y, int *z_chunk) {
  if (int rc = check_tile_query(fe_degree, dim)) return rc;
  return tile_answer(gdmk::cg_tx(fe_degree), gdmk::cg_ty(fe_degree), gdmk::cg_zc(fe_degree), tile_x, tile_y, z_chunk);
}

int gdm_coef_grid_tables_1d(const gdm_mesh_desc *mesh, int axis, double *val_host, double *der_host,
                            int32_t *first_host) {
  if (int rc = check_field_mesh(mesh, axis)) return rc;
  if (!val_host || !der_host || !first_host) return fail(GDM_ERR_ARG, "NULL argument");
  GDM_GUARD_BEGIN
  const unsigned nc = (unsigned)mesh->n_subdivisions[axis];
  CoefGridTables T;
  coef_grid_tables(mesh->fe_degree, nc, (mesh->hi[axis] - mesh->lo[axis]) / nc, T);
  std::copy(T.val.begin(), T.val.end(), val_host);
  std::copy(T.der.begin(), T.der.end(), der_host);
  std::copy(T.first.begin(), T.first.end(), first_host);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_op_set_coefficient_grid(gdm_op *op, const double *kq, const double *kbc) {
  if (int rc = check_set_op(op, "gdm_op_set_coefficient_grid", "the constant coefficient")) return rc;
  if (kq && op->nitsche > 0.0 && op->layout.n_bc_points > 0 && !kbc)
    return fail(GDM_ERR_ARG, "gdm_op_set_coefficient_grid: an operator with nitsche > 0 needs kbc");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  return build_and_install<gdm_op::Coef>(
      op, kq != nullptr, [&](gdm_op::Coef &nc) { return build_coef_grid(op, kq, kbc, nc); }, install_coef,
      "gdm_op_set_coefficient_grid: a sample of kappa is not finite or not positive");
  GDM_GUARD_END
}

int gdm_density_tile(int fe_degree, int dim, int *tile_x, int *tile_y, int *z_chunk) {
  if (int rc = check_tile_query(fe_degree, dim)) return rc;
  return tile_answer(gdmk::VMASS_TX, gdmk::VMASS_TY, gdmk::VMASS_ZC, tile_x, tile_y, z_chunk);
}

int gdm_density_cholesky_1d(const gdm_mesh_desc *mesh, int axis, const double *f, double *lrow_host,
                            double *invd_host) {
  if (const char *e = host_mesh_error(mesh, axis)) return fail(GDM_ERR_ARG, e);
  if (!lrow_host || !invd_host) return fail(GDM_ERR_ARG, "NULL argument");
  if (f) {
    const size_t n = coef_samples(mesh, axis);
    for (size_t i = 0; i < n; ++i)
      if (!std::isfinite(f[i])) return fail(GDM_ERR_ARG, "gdm_density_cholesky_1d: a factor sample is not finite");
  }
  GDM_GUARD_BEGIN
  std::vector<double> lrow, invd;
  try {
    gdm::Band M;
    density_band(mesh, axis, f, M);
    gdm::cholesky_band(M, lrow, invd);
  } catch (const std::runtime_error &) {
    return fail(GDM_ERR_ARG, "gdm_density_cholesky_1d: M[f] is not positive definite");
  }
  std::copy(lrow.begin(), lrow.end(), lrow_host);
  std::copy(invd.begin(), invd.end(), invd_host);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_op_set_density(gdm_op *op, int n_terms, const gdm_coef_term *terms) {
  if (int rc = check_set_op(op, "gdm_op_set_density", "the unit density")) return rc;
  if (int rc = check_factors(op, n_terms, terms, "gdm_op_set_density", "density")) return rc;
  // one term: the factors keep their signs, which multiply to the sign of rho
  double sign = 1.0;
  for (int d = 0; d < op->dim && n_terms == 1; ++d)
    if (terms[0].factor[d] && terms[0].factor[d][0] < 0.0) sign = -sign;
  if (sign < 0.0) return fail(GDM_ERR_ARG, "gdm_op_set_density: the one-term density is negative");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  return build_and_install<gdm_op::Density>(op, n_terms > 0, [&](gdm_op::Density &nd) {
    build_density(op, n_terms, terms, nd);
    return true;
  }, install_density, "");
  GDM_GUARD_END
}

int gdm_density_grid_tile(int fe_degree, int dim, int *tile_x, int *tile_y, int *z_chunk) {
  if (int rc = check_tile_query(fe_degree, dim)) return rc;
  return tile_answer(gdmk::mg_tx(fe_degree), gdmk::mg_ty(fe_degree), gdmk::mg_zc(fe_degree), tile_x, tile_y, z_chunk);
}

int gdm_op_set_density_grid(gdm_op *op, const double *rq) {
  if (int rc = check_set_op(op, "gdm_op_set_density_grid", "the unit density")) return rc;
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  // the reduction and the diagonal run on the operator's stream behind whatever wrote rq there
  hip_check(hipStreamSynchronize(op->stream), "hipStreamSynchronize");
  const char *bad_sample = "gdm_op_set_density_grid: a sample of rho is not finite or not positive";
  if (rq && op->dens.active && op->dens.grid && op->dens.grid_args.rq == rq) {
    // the same pointer: the tables and the scratch stand, the mean and W follow the samples
    double mean = 0.0;
    if (!density_grid_reduce(op, op->dens, &mean)) return fail(GDM_ERR_ARG, bad_sample);
    op->dens.mean = mean;
    density_grid_scaling(op, op->dens);
    hip_check(hipStreamSynchronize(op->stream), "hipStreamSynchronize");
    return GDM_OK;
  }
  return build_and_install<gdm_op::Density>(
      op, rq != nullptr, [&](gdm_op::Density &nd) { return build_density_grid(op, rq, nd); }, install_density,
      bad_sample);
  GDM_GUARD_END
}

int gdm_op_set_density_grid_z_chunk(gdm_op *op, int z_chunk) {
  if (!op) return fail(GDM_ERR_ARG, "op is NULL");
  if (!op->dens.active || !op->dens.grid)
    return fail(GDM_ERR_STATE, "gdm_op_set_density_grid_z_chunk: no grid density is set (gdm_op_set_density_grid)");
  if (z_chunk == 0 || z_chunk < -1 || z_chunk > gdmk::mg_zc(op->p))
    return fail(GDM_ERR_ARG, "gdm_op_set_density_grid_z_chunk: z_chunk must be -1 or in [1, the chunk of "
                             "gdm_density_grid_tile]");
  op->dens.grid_args.zc = z_chunk < 0 ? op->dens.zc_auto : z_chunk;
  return GDM_OK;
}

int gdm_density_diag(gdm_op *op, double *dst_owned) {
  if (!op) return fail(GDM_ERR_ARG, "op is NULL");
  if (!op->dens.active) return fail(GDM_ERR_STATE, "gdm_density_diag: no density is set (gdm_op_set_density[_grid])");
  if (!dst_owned) return fail(GDM_ERR_ARG, "NULL vector");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  const gdm_op::Density &D = op->dens;
  if (D.grid) {
    gdmk::MgArgs g = D.grid_args;
    g.dst = dst_owned;
    hip_check(gdmk::launch_mg_diag(op->p, g, op->stream), "grid density diagonal launch");
    return GDM_OK;
  }
  // separable: sum_t prod_d diag(M_d[r_td]), 1D tables from the set call
  const int Nx = op->K[0], Ny = op->K[1], Nz = op->K[2];
  std::vector<double> h((size_t)Nx * Ny * Nz);
  for (int z = 0; z < Nz; ++z)
    for (int y = 0; y < Ny; ++y)
      for (int x = 0; x < Nx; ++x) {
        double s = 0.0;
        for (int t = 0; t < D.n_terms; ++t)
          s += D.band_diag[(size_t)t * 3][(size_t)x] * D.band_diag[(size_t)t * 3 + 1][(size_t)y] *
               D.band_diag[(size_t)t * 3 + 2][(size_t)z];
        h[((size_t)z * Ny + y) * Nx + x] = s;
      }
  hip_check(hipMemcpyAsync(dst_owned, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, op->stream), "copy");
  hip_check(hipStreamSynchronize(op->stream), "hipStreamSynchronize");
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_density_apply(gdm_op *op, const double *src, double *dst) {
  if (!op) return fail(GDM_ERR_ARG, "op is NULL");
  if (!op->dens.active) return fail(GDM_ERR_STATE, "gdm_density_apply: no density is set (gdm_op_set_density)");
  if (!src || !dst || src == dst) return fail(GDM_ERR_ARG, "src and dst: distinct device vectors");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  density_apply(op, src, dst);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_density_apply_add(gdm_op *op, const double *src, double c, const double *add, double *dst) {
  if (!op) return fail(GDM_ERR_ARG, "op is NULL");
  if (!op->dens.active) return fail(GDM_ERR_STATE, "gdm_density_apply_add: no density is set (gdm_op_set_density)");
  if (!src || !dst || src == dst || add == dst) return fail(GDM_ERR_ARG, "src, add and dst: distinct device vectors");
  if (!std::isfinite(c)) return fail(GDM_ERR_ARG, "gdm_density_apply_add: c is not finite");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  density_apply(op, src, dst, add, c);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_density_solve(gdm_op *op, const double *rhs, double *x, double rel_tol, double abs_tol, int max_it,
                      int *its_host, double *res_host) {
  if (!op) return fail(GDM_ERR_ARG, "op is NULL");
  if (!op->dens.active) return fail(GDM_ERR_STATE, "gdm_density_solve: no density is set (gdm_op_set_density)");
  if (!rhs || !x) return fail(GDM_ERR_ARG, "NULL vector");
  if (op->dens.n_terms != 1 && rhs == x)
    return fail(GDM_ERR_ARG, "gdm_density_solve: a sum of terms or a grid density needs rhs != x");
  if (max_it < 0) return fail(GDM_ERR_ARG, "max_it < 0");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  const int64_t n = op->layout.n_owned;
  gdm_op::Density &D = op->dens;
  if (D.n_terms == 1) {
    // exact: M[rho]^-1 = (x)_d M_d[r_d]^-1, two-sweep line solves with the weighted factors
    mass_solve_passes(op, rhs, x, nullptr, nullptr, D.axis_tab);
    if (its_host) *its_host = 0;
    if (res_host) *res_host = 0.0;
    return GDM_OK;
  }
  // the caller may have overwritten a borrowed grid in place: W follows the samples of this solve
  if (D.grid) density_grid_scaling(op, D);
  auto apply = [&](const double *src, double *dst) { density_apply(op, src, dst); };
  // z = W^-1/2 M^-1 W^-1/2 r
  auto precondition = [&](const double *rr, double *zz) {
    hip_check(gdmk_launch_vmul(n, D.w_isqrt, rr, D.cg[4], op->stream), "scale");
    mass_solve_passes(op, D.cg[4], D.cg[4], nullptr);
    hip_check(gdmk_launch_vmul(n, D.w_isqrt, D.cg[4], zz, op->stream), "scale");
  };
  const gdm::PcgResult res = device_pcg(op, n, apply, precondition, D.cg[0], D.cg[1], D.cg[2], D.cg[3], rhs, x,
                                        rel_tol, abs_tol, max_it);
  return finish_pcg(res, "gdm_density_solve", its_host, res_host,
                    "(p^T M[rho] p <= 0): rho must be positive on the box");
  GDM_GUARD_END
}
}  // extern "C"

namespace {

// shared refusals of the fast-diagonalisation entry points; 0 = ok
int check_fastdiag_op(gdm_op *op, const char *what, bool need_setup) {
  if (!op) return fail(GDM_ERR_ARG, "op is NULL");
  if (op->kind != GDM_OP_WAVE)
    return fail(GDM_ERR_UNSUPPORTED, std::string(what) + ": wave operators only (the stiffness matrix must be symmetric)");
  if (op->mesh.n_ranks > 1) return fail(GDM_ERR_UNSUPPORTED, std::string(what) + ": single rank only");
  if (op->mesh.periodic) return fail(GDM_ERR_UNSUPPORTED, std::string(what) + ": not with periodic constraints");
  if (op->cut_inner) return fail(GDM_ERR_UNSUPPORTED, std::string(what) + ": not on the inner operator of a cut handle");
  if (need_setup && !op->fd.built)
    return fail(GDM_ERR_STATE, std::string(what) + ": call gdm_system_solve_setup first");
  return GDM_OK;
}

void fastdiag_host_tables(const gdm_mesh_desc *mesh, double nitsche, int axis, std::vector<double> &S,
                          std::vector<double> &lambda) {
  const unsigned nc = (unsigned)mesh->n_subdivisions[axis];
  const double h = (mesh->hi[axis] - mesh->lo[axis]) / nc;
  gdm::fastdiag_1d(mesh->fe_degree, nc, h, nitsche_over_hmin(mesh, nitsche), S, lambda);
}

}  // namespace

// one pass along kernel axis ax: dst = T src, Tt the row-major transpose of T
gdmk::FastdiagPass gdm_detail::fastdiag_pass(const gdm_op *op, int ax, const double *Tt) {
  gdmk::FastdiagPass P{};
  P.N = op->K[ax];
  P.Tt = Tt;
  P.K0 = op->K[0];
  P.K1 = op->K[1];
  if (ax == 0) {
    P.row_form = 1;
    P.cols = 1;
    P.batch = (int64_t)op->K[1] * op->K[2];
  } else {
    P.cols = ax == 1 ? op->K[0] : (int64_t)op->K[0] * op->K[1];
    P.batch = ax == 1 ? op->K[2] : 1;
  }
  return P;
}

extern "C" {

int gdm_fastdiag_tables(const gdm_mesh_desc *mesh, double nitsche, int axis, double *S_host, double *lambda_host) {
  if (int rc = check_field_mesh(mesh, axis)) return rc;
  if (!S_host || !lambda_host) return fail(GDM_ERR_ARG, "S_host / lambda_host is NULL");
  if (!std::isfinite(nitsche)) return fail(GDM_ERR_ARG, "nitsche is not finite");
  for (int d = 0; d < mesh->dim; ++d)
    if (mesh->n_subdivisions[d] < 1 || !(mesh->hi[d] > mesh->lo[d])) return fail(GDM_ERR_ARG, "empty box");
  GDM_GUARD_BEGIN
  std::vector<double> S, lambda;
  fastdiag_host_tables(mesh, nitsche, axis, S, lambda);
  std::copy(S.begin(), S.end(), S_host);
  std::copy(lambda.begin(), lambda.end(), lambda_host);
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_system_solve_setup(gdm_op *op) {
  if (int rc = check_fastdiag_op(op, "gdm_system_solve_setup", false)) return rc;
  if (op->fd.built) return GDM_OK;
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  // everything is uploaded before the handle changes: a failure leaves it as it was
  gdm_op::FastDiag nf;
  std::vector<void *> made;
  try {
    for (int ax = 0; ax < 3; ++ax) {
      const int d = op->kdir[ax];
      if (d < 0) continue;
      std::vector<double> S, lambda;
      fastdiag_host_tables(&op->mesh, op->nitsche, d, S, lambda);
      const int n = (int)lambda.size();
      std::vector<double> St((size_t)n * n);
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) St[(size_t)j * n + i] = S[(size_t)i * n + j];
      nf.S[ax] = up(made, S);
      nf.St[ax] = up(made, St);
      nf.lam[ax] = up(made, lambda);
      nf.lam_min[ax] = lambda.front();
      nf.lam_max[ax] = lambda.back();
    }
    for (int i = 0; i < 2; ++i) {
      double *t = nullptr;
      hip_check(hipMalloc(&t, std::max<size_t>((size_t)op->layout.n_owned, 1) * sizeof(double)), "hipMalloc");
      made.push_back(t);
      nf.tmp[i] = t;
    }
  } catch (...) {
    for (void *ptr : made) (void)hipFree(ptr);
    throw;
  }
  for (void *ptr : made) op->allocations.push_back(ptr);
  nf.built = true;
  op->fd = nf;
  return GDM_OK;
  GDM_GUARD_END
}

int gdm_fastdiag_transform(gdm_op *op, int axis, int transpose, const double *src_owned, double *dst_owned) {
  if (int rc = check_fastdiag_op(op, "gdm_fastdiag_transform", true)) return rc;
  if (!src_owned || !dst_owned) return fail(GDM_ERR_ARG, "NULL vector");
  if (src_owned == dst_owned) return fail(GDM_ERR_ARG, "gdm_fastdiag_transform: src and dst must be distinct vectors");
  if (axis < 0 || axis >= op->dim) return fail(GDM_ERR_ARG, "axis outside [0, dim)");
  if (transpose != 0 && transpose != 1) return fail(GDM_ERR_ARG, "transpose must be 0 or 1");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  int ax = 0;
  while (op->kdir[ax] != axis) ++ax;
  const double *Tt = transpose ? op->fd.S[ax] : op->fd.St[ax];
  hip_check(gdmk_launch_fastdiag_pass(fastdiag_pass(op, ax, Tt), src_owned, dst_owned, op->stream), "fastdiag pass");
  return GDM_OK;
  GDM_GUARD_END
}

}  // extern "C"

namespace {

// x = (alpha M + tau S)^-1 rhs of the constant-coefficient operator by fast
// diagonalisation: gdm_system_solve, and the preconditioner of gdm_coef_solve
int fastdiag_solve(gdm_op *op, double alpha, double tau, const double *rhs_owned, double *x_owned) {
  // the spectrum of alpha M + tau S in the M-orthonormal eigenbasis is alpha + tau sum_d lambda_d
  double smin = 0.0, smax = 0.0;
  int axes[3], n_axes = 0;
  for (int ax = 0; ax < 3; ++ax) {
    if (op->kdir[ax] < 0) continue;
    axes[n_axes++] = ax;
    smin += op->fd.lam_min[ax];
    smax += op->fd.lam_max[ax];
  }
  const double e0 = alpha + tau * smin, e1 = alpha + tau * smax;
  const double lo = std::min(e0, e1), hi = std::max(e0, e1);
  const double near0 = std::min(std::fabs(lo), std::fabs(hi)), far0 = std::max(std::fabs(lo), std::fabs(hi));
  if ((lo <= 0.0 && hi >= 0.0) || near0 < 1e-12 * far0) {
    char msg[320];
    const double tiny = 1e-10 * std::max(std::fabs(smin), std::fabs(smax));
    if (smin < -tiny)
      std::snprintf(msg, sizeof msg,
                    "gdm_system_solve: the stiffness matrix is indefinite (smallest eigenvalue %.6g): the Nitsche "
                    "penalty %g is too small for degree %d; alpha M + tau S has eigenvalues in [%.6g, %.6g]",
                    smin, op->nitsche, op->p, lo, hi);
    else
      std::snprintf(msg, sizeof msg,
                    "gdm_system_solve: alpha M + tau S is singular (eigenvalues in [%.6g, %.6g]); without Nitsche "
                    "terms the stiffness matrix has the constants in its kernel (pure Neumann problem)",
                    lo, hi);
    return fail(GDM_ERR_ARG, msg);
  }
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  // forward S^T along x, y, z (the last one scales by the inverse eigenvalues),
  // backward S along z, y, x; ping-pong between the two scratch vectors, so rhs
  // is read by the first pass only and x written by the last only
  const int n_pass = 2 * n_axes;
  const double *src = rhs_owned;
  for (int i = 0; i < n_pass; ++i) {
    const bool fwd = i < n_axes;
    const int ax = fwd ? axes[i] : axes[n_pass - 1 - i];
    gdmk::FastdiagPass P = fastdiag_pass(op, ax, fwd ? op->fd.S[ax] : op->fd.St[ax]);
    if (i == n_axes - 1) {
      P.scale = 1;
      P.alpha = alpha;
      P.tau = tau;
      P.lam0 = op->fd.lam[0];
      P.lam1 = op->fd.lam[1];
      P.lam2 = op->fd.lam[2];
    }
    double *dst = i == n_pass - 1 ? x_owned : op->fd.tmp[i & 1];
    hip_check(gdmk_launch_fastdiag_pass(P, src, dst, op->stream), "fastdiag pass");
    src = dst;
  }
  return GDM_OK;
  GDM_GUARD_END
}

}  // namespace

extern "C" {

int gdm_system_solve(gdm_op *op, double alpha, double tau, const double *rhs_owned, double *x_owned) {
  if (int rc = check_fastdiag_op(op, "gdm_system_solve", true)) return rc;
  if (!rhs_owned || !x_owned) return fail(GDM_ERR_ARG, "NULL vector");
  if (!std::isfinite(alpha) || !std::isfinite(tau)) return fail(GDM_ERR_ARG, "gdm_system_solve: alpha / tau is not finite");
  if (op->coef.active)
    return fail(GDM_ERR_STATE, "gdm_system_solve: the direct solve is the constant-coefficient one; with a "
                               "coefficient set use gdm_coef_solve");
  return fastdiag_solve(op, alpha, tau, rhs_owned, x_owned);
}

int gdm_coef_solve(gdm_op *op, double alpha, double tau, const double *rhs, double *x, double rel_tol, double abs_tol,
                   int max_it, int *its_host, double *res_host) {
  if (int rc = check_fastdiag_op(op, "gdm_coef_solve", false)) return rc;
  const bool dens = op->dens.active;
  if (!op->coef.active && !dens)
    return fail(GDM_ERR_STATE, "gdm_coef_solve: no coefficient is set (gdm_op_set_coefficient)");
  if (!op->fd.built) return fail(GDM_ERR_STATE, "gdm_coef_solve: call gdm_system_solve_setup first (the preconditioner)");
  if (!rhs || !x || rhs == x) return fail(GDM_ERR_ARG, "rhs and x: distinct device vectors");
  if (!std::isfinite(alpha) || !std::isfinite(tau)) return fail(GDM_ERR_ARG, "gdm_coef_solve: alpha / tau is not finite");
  if (max_it < 0) return fail(GDM_ERR_ARG, "max_it < 0");
  GDM_GUARD_BEGIN
  hip_check(hipSetDevice(op->device), "hipSetDevice");
  const int64_t n = op->layout.n_owned;
  // with a density its own vectors serve (a coefficient need not be set)
  double *const *cg = dens ? op->dens.cg : op->coef.cg;
  double *Mp = cg[4];
  const double ptau = tau * (op->coef.active ? op->coef.mean : 1.0);
  const double palpha = alpha * (dens ? op->dens.mean : 1.0);
  // dst = (alpha M - tau K[kappa]) src
  auto apply = [&](const double *src, double *dst) {
    if (dens) {
      // (alpha M[rho] - tau K) src: K src first, then the weighted mass with the
      // fused `+ c * add`; K = K_0 (the plain stencil) without a coefficient
      double *Ks = alpha != 0.0 ? Mp : dst;
      if (op->coef.active)
        coef_apply(op, src, Ks);
      else
        hip_check(launch_stencil(op, false, src, Ks), "stencil launch");
      if (alpha != 0.0) {
        density_apply(op, src, dst, Ks, -tau / alpha);
        if (alpha != 1.0) hip_check(gdmk_launch_axpby(n, 0.0, src, alpha, dst, op->stream), "axpby");
      } else {
        hip_check(gdmk_launch_axpby(n, 0.0, src, -tau, dst, op->stream), "axpby");
      }
      return;
    }
    coef_apply(op, src, dst);
    if (alpha != 0.0) {
      any_stencil(op, true, src, Mp);
      hip_check(gdmk_launch_axpby(n, alpha, Mp, -tau, dst, op->stream), "axpby");
    } else {
      hip_check(gdmk_launch_axpby(n, 0.0, src, -tau, dst, op->stream), "axpby");
    }
  };
  // SolverCG with ReductionControl(max_it, abs_tol, rel_tol), x the initial
  // guess, preconditioned by (alpha mean(rho) M - tau mean(kappa) K_0)^-1 (a mean is 1 where nothing is set)
  // a refusal of the preconditioner (its spectrum check, with its own error) ends the solve with its code
  struct Refused {
    int code;
  };
  auto precondition = [&](const double *rr, double *zz) {
    if (int rc = fastdiag_solve(op, palpha, ptau, rr, zz)) throw Refused{rc};
  };
  gdm::PcgResult res{};
  try {
    res = device_pcg(op, n, apply, precondition, cg[0], cg[1], cg[2], cg[3], rhs, x, rel_tol, abs_tol, max_it);
  } catch (const Refused &e) {
    return e.code;
  }
  return finish_pcg(res, "gdm_coef_solve", its_host, res_host,
                    "(p^T A p <= 0): alpha M - tau K[kappa] is not positive definite; kappa must be positive on the box");
  GDM_GUARD_END
}

}  // extern "C"
