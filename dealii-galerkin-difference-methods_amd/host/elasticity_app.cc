// elasticity_app.cc -- tests/elasticity_01_gdm.cc on the MI355X engine, written
// against the C++ mirror gdm/hip/elasticity.h.
//
//   elasticity_app [PRECOND]
//
// 2D, two components, p = 3 on 40^2 cells of [0, 1]^2, 2 (eps(u), eps(v)), zero
// boundary constraints, CG with ReductionControl(100, 1e-10, 1e-8).  PRECOND =
// jacobi (default, the reference's PreconditionJacobi), fastdiag (the block
// fast-diagonalisation preconditioner) or none.  Prints the reference's output
// line "error : <L2 error>" and, on stderr, the iteration count.
//
// Manufactured solution u = (sin^2(pi x) sin(pi y) cos(pi y), -sin(pi x) cos(pi x)
// sin^2(pi y)) = ((1 - cos 2 pi x) sin(2 pi y) / 4, -sin(2 pi x) (1 - cos 2 pi y) / 4);
// div u = 0, so the force is f = -div(2 eps(u)) = -laplace u:
//   f_0 = pi^2 sin(2 pi y) (1 - 2 cos 2 pi x),  f_1 = -pi^2 sin(2 pi x) (1 - 2 cos 2 pi y).
#include <gdm/hip/elasticity.h>

#include <cstdio>
#include <cstring>
#include <iostream>

namespace {

const double kPi = 3.14159265358979323846;

double exact_solution(const GDM::HIP::Point &x, unsigned int c) {
  const double a = 2.0 * kPi;
  return c == 0 ? 0.25 * (1.0 - std::cos(a * x[0])) * std::sin(a * x[1])
                : -0.25 * std::sin(a * x[0]) * (1.0 - std::cos(a * x[1]));
}

double force(const GDM::HIP::Point &x, unsigned int c) {
  const double a = 2.0 * kPi;
  return c == 0 ? kPi * kPi * std::sin(a * x[1]) * (1.0 - 2.0 * std::cos(a * x[0]))
                : -kPi * kPi * std::sin(a * x[0]) * (1.0 - 2.0 * std::cos(a * x[1]));
}

}  // namespace

int main(int argc, char **argv) {
  using namespace GDM::HIP;
  const char *name = argc > 1 ? argv[1] : "jacobi";
  Elasticity::Preconditioner precond;
  if (!std::strcmp(name, "jacobi"))
    precond = Elasticity::Preconditioner::jacobi;
  else if (!std::strcmp(name, "fastdiag"))
    precond = Elasticity::Preconditioner::fastdiag;
  else if (!std::strcmp(name, "none"))
    precond = Elasticity::Preconditioner::none;
  else {
    std::fprintf(stderr, "usage: %s [jacobi | fastdiag | none]\n", argv[0]);
    return 2;
  }
  try {
    const unsigned int n_subdivisions = 40, fe_degree = 3;
    Elasticity::ElasticityOperator<2> matrix(fe_degree, n_subdivisions);
    DeviceVector rhs, solution;
    matrix.initialize_dof_vector(rhs);
    matrix.initialize_dof_vector(solution);
    matrix.assemble_rhs(rhs, force);
    // the unpreconditioned iteration needs more than the reference's 100 steps
    const unsigned int its = matrix.solve(solution, rhs, precond, precond == Elasticity::Preconditioner::none ? 1000 : 100);
    const double error = matrix.l2_error(solution, exact_solution);
    std::cerr << "iterations: " << its << std::endl;
    std::cout << "error : " << error << std::endl;
  } catch (const Error &e) {
    std::fprintf(stderr, "GDM::HIP::Error: %s\n", e.what());
    return 1;
  }
  return 0;
}
