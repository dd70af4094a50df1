// TEST-ONLY harness: the general-slope halo profile of chomp_math.h -- the profile's mass
// integral, the halo normalisation and the y_general integrand with its normalisation rule --
// built for the CPU (g++) by tests/test_halo_profile_cpu.py.  Never loaded by the chomp_amd package.
#include "../../chomp_amd/csrc/chomp_math.h"

extern "C" {
void hc_profile_mass_integral(const double* alpha, const double* c, int n, double* out) {
  for (int i = 0; i < n; ++i) out[i] = chomp::profile_mass_integral(alpha[i], c[i]);
}
void hc_halo_normalization(double rho_bar, double delta_v, double alpha, const double* c, int n,
                           double* out) {
  for (int i = 0; i < n; ++i) out[i] = chomp::halo_normalization(rho_bar, delta_v, alpha, c[i]);
}
double hc_y_general_norm(double alpha, double k, double r_vir, double con) {
  return chomp::y_general_norm(alpha, k, r_vir, con);
}
void hc_y_general_integrand(double alpha, double k, double r_vir, double con, double norm,
                            const double* x, int n, double* out) {
  const chomp::YGeneralIntegrand f{alpha, k, r_vir, con, norm};
  for (int i = 0; i < n; ++i) out[i] = f(x[i]);
}
double hc_y_general_scale(double r_vir, double con, double halo_norm, double mass) {
  return chomp::y_general_scale(r_vir, con, halo_norm, mass);
}
}
