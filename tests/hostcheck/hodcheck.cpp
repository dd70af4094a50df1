// TEST-ONLY harness: the host side of the tagged HOD model -- the layout of chomp_hod_model as
// the C header declares it and the Mandelbaum constants as chomp_math.h derives them -- built
// for the CPU (g++) by tests/test_hod_mandelbaum_cpu.py.  Never loaded by the chomp_amd package.
#include <cstddef>
#include "../../include/chomp_mi355x.h"
#include "../../chomp_amd/csrc/chomp_math.h"

extern "C" {
void hc_hod_model_layout(size_t* out) {
  out[0] = sizeof(chomp_hod_model);
  out[1] = offsetof(chomp_hod_model, kind);
  out[2] = offsetof(chomp_hod_model, reserved);
  out[3] = offsetof(chomp_hod_model, zheng);
  out[4] = offsetof(chomp_hod_model, log_M_0);
  out[5] = offsetof(chomp_hod_model, w);
  out[6] = CHOMP_HOD_ZHENG;
  out[7] = CHOMP_HOD_MANDELBAUM;
}
void hc_mandelbaum_constants(const double* log_M_0, int n, double* log_M_min, double* M_min) {
  for (int i = 0; i < n; ++i) chomp::mandelbaum_constants(log_M_0[i], &log_M_min[i], &M_min[i]);
}
void hc_mandelbaum_moments(double log_M_0, double w, const double* mass, int n, double* out) {
  chomp::Epoch e{};
  e.hod_model = chomp::kHodMandelbaum;
  e.hod_log_M_0 = log_M_0;
  chomp::mandelbaum_constants(log_M_0, &e.hod_log_M_min, &e.hod_M_min);
  e.hod_w = w;
  for (int i = 0; i < n; ++i) {
    out[4 * i] = chomp::hod_first(e, mass[i]);
    out[4 * i + 1] = chomp::hod_second(e, mass[i]);
    out[4 * i + 2] = chomp::hod_central(e, mass[i]);
    out[4 * i + 3] = chomp::hod_satellite(e, mass[i]);
  }
}
}
