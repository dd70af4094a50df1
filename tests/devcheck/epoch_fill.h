// TEST-ONLY: the Epoch record filled on the device by the product's own functions from raw
// inputs, shared by the harnesses that need one (devphys.hip, devpower.hip).  Includes the
// product's headers themselves; no part of the package.
#pragma once

#include "../../chomp_amd/csrc/chomp_cov_kernels.h"

namespace devcheck {

static_assert(sizeof(chomp::Epoch) % sizeof(double) == 0, "Epoch is staged as doubles");
constexpr int kEpochD = (int)(sizeof(chomp::Epoch) / sizeof(double));

// in: 0-7 om0 ob0 ol0 or0 tcmb h sigma8 ns, 8 z, 9 cosmo_precision, 10 k_min, 11 k_max,
//     12 with_bao, 13 sigma_norm, 14 mf_kind, 15 stq, 16 st_a, 17 f_norm, 18 bias_norm,
//     19 mf_delta_v, 20-24 t_alpha t_beta t_gamma t_phi t_eta, 25 m_star, 26 c0, 27 beta,
//     28 delta_v_in, 29 hod_model, 30 log_M_min, 31 sigma, 32 log_M_0, 33 log_M_1p, 34 alpha,
//     35 w, 36 shape_only
constexpr int kEpochIn = 37;
__device__ inline void fill_epoch(const double* in, chomp::Epoch& e) {
  double* raw = reinterpret_cast<double*>(&e);
  for (int i = 0; i < kEpochD; ++i) raw[i] = 0.0;
  e.om0 = in[0]; e.ob0 = in[1]; e.ol0 = in[2]; e.or0 = in[3];
  e.tcmb = in[4]; e.h = in[5]; e.sigma8 = in[6]; e.ns = in[7];
  e.z = in[8];
  if (in[36] != 0.0) {
    chomp::epoch_shape_only(e, in[10], in[11], (int)in[12]);
  } else {
    chomp::epoch_background(e, in[9], in[10], in[11], (int)in[12]);
    e.sigma_norm = in[13];
    // the mass-function scalars as the set-up kernel stores them (chomp_mass_kernels.h)
    e.mf_kind = (int)in[14];
    e.stq = in[15]; e.st_a = in[16]; e.f_norm = in[17]; e.bias_norm = in[18];
    e.mf_delta_v = in[19];
    e.ln_st_a = log(e.st_a);
    e.ln_t_beta = 0.0;
    e.m_star = in[25];
    if (e.mf_kind == 1) {
      e.t_alpha = in[20]; e.t_beta = in[21]; e.t_gamma = in[22]; e.t_phi = in[23];
      e.t_eta = in[24];
      e.ln_t_beta = log(e.t_beta);
      chomp::tinker_bias_constants(e);
    }
    // halo and HOD constants as apply_halo_hod stores them (chomp_halo_kernels.h)
    chomp::halo_constants(e, in[26], in[27], in[28]);
    e.hod_model = (int)in[29];
    e.hod_log_M_min = in[30]; e.hod_sigma = in[31]; e.hod_log_M_0 = in[32];
    e.hod_log_M_1p = in[33]; e.hod_alpha = in[34];
    e.hod_w = in[35];
    if (e.hod_model == chomp::kHodMandelbaum)
      chomp::mandelbaum_constants(e.hod_log_M_0, &e.hod_log_M_min, &e.hod_M_min);
    e.hod_M0 = pow(10.0, e.hod_log_M_0);
    e.hod_M1p = pow(10.0, e.hod_log_M_1p);
  }
}

}  // namespace devcheck
