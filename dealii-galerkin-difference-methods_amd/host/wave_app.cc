// wave_app.cc -- the uncut wave-rk driver on the MI355X engine, written against
// the C++ mirror of the reference's wave operator surface (gdm/hip/wave.h), in
// the shape of applications/wave/wave-app.cc:222-285 + problem.h:280-346.
//
//   wave_app DIM P N STEPS CFL OUT [NITSCHE] [DEVICE] [DATA] [SIMULATION_TYPE]
//
// Box [-1.21, 1.21]^dim, initial displacement u0 = prod_d cos(0.75 pi x_d /
// 1.21 + 0.2 d), v0 = 0, natural boundary (NITSCHE = 0) or box Nitsche with
// gamma_D = NITSCHE.  DATA = 1 (needs NITSCHE > 0) drives the problem with
// function_rhs = 3 w and function_domain_dbc = w, w(x, t) = prod_d sin(2 pi
// k_d (x_d - a_d t) + phi_d), a = (0.8, 0, 0), k = (0.4, 0.3, 0.35), phi =
// (0.3, 0.5, 0.2), and starts from u0 = w(., 0).  SIMULATION_TYPE = wave-rk
// (default), heat-rk, heat-impl or poisson (the latter two solve with the
// stiffness matrix: NITSCHE > 0; poisson takes no steps, v stays 0 for all
// three).  Writes u then v after STEPS steps to OUT (raw little-endian
// doubles, reference global order).
#include <gdm/hip/wave.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>

namespace {

const double kPi = 3.14159265358979323846;

template <int dim>
double sine_product(const GDM::HIP::Point &x, double t) {
  const double a[3] = {0.8, 0.0, 0.0}, k[3] = {0.4, 0.3, 0.35}, phi[3] = {0.3, 0.5, 0.2};
  double v = 1.0;
  for (int d = 0; d < dim; ++d) v *= std::sin(2.0 * kPi * k[d] * (x[d] - a[d] * t) + phi[d]);
  return v;
}

template <int dim>
int run(int p, int n, int steps, double cfl, const char *out, double nitsche, int device, int data,
        const char *simulation_type) {
  GDM::HIP::Wave::Parameters<dim> params;
  params.fe_degree = p;
  params.n_subdivisions_1D = n;
  params.nitsche_parameter = nitsche;
  params.exact_solution = [](const GDM::HIP::Point &x, double) {
    double v = 1.0;
    for (int d = 0; d < dim; ++d) v *= std::cos(0.75 * kPi * x[d] / 1.21 + 0.2 * d);
    return v;
  };
  if (data) {
    params.exact_solution = sine_product<dim>;
    params.function_rhs = [](const GDM::HIP::Point &x, double t) { return 3.0 * sine_product<dim>(x, t); };
    params.function_domain_dbc = sine_product<dim>;
  }
  params.cfl = cfl;
  params.end_t = 1e9;
  params.device = device;
  params.simulation_type = simulation_type;
  GDM::HIP::Wave::WaveProblem<dim> problem(params);
  const unsigned int done = problem.run(steps);
  std::vector<double> u = problem.get_solution();
  const std::vector<double> v = problem.get_velocity();
  double s = 0.0;
  for (double x : u) s += x * x;
  std::printf("steps %u  |u|_2 %.15e\n", done, std::sqrt(s));
  u.insert(u.end(), v.begin(), v.end());
  std::ofstream f(out, std::ios::binary);
  f.write(reinterpret_cast<const char *>(u.data()), sizeof(double) * u.size());
  return f.good() ? 0 : 3;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 7) {
    std::fprintf(stderr, "usage: %s DIM P N STEPS CFL OUT [NITSCHE] [DEVICE] [DATA] [SIMULATION_TYPE]\n", argv[0]);
    return 2;
  }
  const int dim = std::atoi(argv[1]), p = std::atoi(argv[2]), n = std::atoi(argv[3]), steps = std::atoi(argv[4]);
  const double cfl = std::atof(argv[5]);
  const double nitsche = argc > 7 ? std::atof(argv[7]) : 0.0;
  const int device = argc > 8 ? std::atoi(argv[8]) : 0;
  const int data = argc > 9 ? std::atoi(argv[9]) : 0;
  const char *type = argc > 10 ? argv[10] : "wave-rk";
  try {
    switch (dim) {
      case 1: return run<1>(p, n, steps, cfl, argv[6], nitsche, device, data, type);
      case 2: return run<2>(p, n, steps, cfl, argv[6], nitsche, device, data, type);
      case 3: return run<3>(p, n, steps, cfl, argv[6], nitsche, device, data, type);
      default: std::fprintf(stderr, "dim must be 1, 2 or 3\n"); return 2;
    }
  } catch (const GDM::HIP::Error &e) {
    std::fprintf(stderr, "GDM::HIP::Error: %s\n", e.what());
    return 1;
  }
}
