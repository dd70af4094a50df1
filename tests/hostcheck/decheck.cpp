// TEST-ONLY harness: the host side of w0-wa dark energy -- the pressure integrand, the knot
// abscissae, the spline and E0 as chomp_math.h has them -- built for the CPU (g++) by
// tests/test_dark_energy_cpu.py.  Never loaded by the chomp_amd package.
//
// The Romberg loop here is scipy's (oracle/romberg.py) run serially; the device runs the same
// stopping rule on wavefront sums (chomp_romberg.h).
#include <cmath>
#include <vector>

#include "../../include/chomp_mi355x.h"
#include "../../chomp_amd/csrc/chomp_math.h"

namespace {
// numpy's pairwise summation is not reproduced bit for bit; a pairwise sum keeps the rounding
// at the level of the reference's (~1e-16 relative), far below the stopping tolerances.
double pairwise(const double* v, size_t n) {
  if (n <= 8) {
    double s = 0.0;
    for (size_t i = 0; i < n; ++i) s += v[i];
    return s;
  }
  const size_t h = n / 2;
  return pairwise(v, h) + pairwise(v + h, n - h);
}

template <class F>
double romberg(const F& f, double a, double b, double tol, double rtol, int divmax, int* level,
               int* converged) {
  const double intrange = b - a;
  double ordsum = 0.5 * (f(a) + f(b));
  std::vector<double> last{intrange * ordsum}, row;
  std::vector<double> pts;
  double result = last[0];
  *level = 0;
  *converged = 0;
  long n = 1;
  for (int i = 1; i <= divmax; ++i) {
    n *= 2;
    const long m = n / 2;
    const double h = intrange / (double)m;
    const double lox = a + 0.5 * h;
    pts.resize(m);
    for (long j = 0; j < m; ++j) pts[j] = f(lox + h * (double)j);
    ordsum = ordsum + pairwise(pts.data(), (size_t)m);
    row.assign(1, intrange * ordsum / (double)n);
    for (int k = 0; k < i; ++k) {
      const double t = std::pow(4.0, k + 1);
      row.push_back((t * row[k] - last[k]) / (t - 1.0));
    }
    result = row[i];
    const double err = std::fabs(result - last[i - 1]);
    *level = i;
    if (err < tol || err < rtol * std::fabs(result)) {
      *converged = 1;
      break;
    }
    last = row;
  }
  return result;
}
}  // namespace

extern "C" {
void dc_knots(double cosmo_precision, int n, double* ln_a, double* z) {
  for (int i = 0; i < n; ++i) chomp::de_knot(cosmo_precision, n, i, &ln_a[i], &z[i]);
}
void dc_integrand(double w0, double wa, const double* z, int n, double* out) {
  const chomp::DePressureIntegrand f{w0, wa};
  for (int i = 0; i < n; ++i) out[i] = f(z[i]);
}
// P_i = 3 romberg((1 + w) / (1 + z), 0, z_i) with its level and whether it converged.
void dc_pressure(double w0, double wa, const double* z, int n, double tol, double rtol,
                 int divmax, double* p, int* level, int* converged) {
  const chomp::DePressureIntegrand f{w0, wa};
  for (int i = 0; i < n; ++i)
    p[i] = 3.0 * romberg(f, 0.0, z[i], tol, rtol, divmax, &level[i], &converged[i]);
}
// E0(z) from the knots (ln a, P): the library's spline and E0_de.
void dc_e0(double om0, double ol0, double or0, const double* ln_a, const double* p, int n,
           const double* z, int m, double* out) {
  std::vector<double> pp(4 * (size_t)(n - 1)), work(2 * (size_t)n);
  chomp::spline_build(ln_a, p, n, pp.data(), work.data());
  const chomp::DeSpline de{ln_a, pp.data(), n};
  for (int i = 0; i < m; ++i) out[i] = chomp::E0_de(om0, ol0, or0, de, z[i]);
}
}
