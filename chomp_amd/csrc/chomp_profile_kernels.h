// chomp_profile_kernels.h -- halo profiles with a general inner slope, halo_dict["alpha"] != -1
// (gfx950, fp64 throughout): a path of its own beside the NFW one of chomp_halo_kernels.h, taken
// only with chomp_set_general_profile(ctx, 1) and some epoch's alpha != -1.
//
//   k_y_general_table     y(k, M) of Halo._initialize_y_spline (halo.py:500-529): one Romberg
//                         integral of the profile against sinc(k r) per (epoch, ln k row, mass
//                         knot), a wavefront each, the level of every integral beside its value
//   k_y_general_splines   the not-a-knot cubic of every row over ln M (halo.py:527-528) and of
//                         ln halo_normalization over ln M (halo.py:848-855; its knot values by
//                         k_halo_normalization_knots)
//   k_halo_knots_general  the knot integrals h_m, pp_mm, h_g, pp_gm, pp_gg, I_1^2 and n_bar with
//                         the literal integrands, y taken from the row's spline (an epoch with
//                         alpha = -1: y_nfw), a wavefront group per (epoch, group, knot)
//   k_halo_finalize_general  the epochs' normalisations and splines over ln k
//                         (halo_finalize_block), after which everything downstream is unchanged
//   k_y_general_eval, k_halo_normalization_eval  Halo.y / Halo.halo_normalization at given masses
#pragma once

#include "chomp_halo_kernels.h"

namespace chomp {

// Per-epoch block of the general-profile tables (doubles).  Rows 0..NK-1 are the ln k knots of
// the halo tables; row NK is the scratch row of chomp_y_general (an arbitrary scalar ln k).
struct ProfLayout {
  int NM, NK;
  int off_y, off_level, off_pp;     // [NK + 1][NM], [NK + 1][NM], [NK + 1][4 (NM - 1)]
  int off_ln_hn, off_hn_pp;         // ln halo_normalization at the mass knots, its spline
  int stride;
};
inline ProfLayout make_prof_layout(int NM, int NK) {
  ProfLayout P;
  P.NM = NM; P.NK = NK;
  int o = 0;
  P.off_y = o; o += (NK + 1) * NM;
  P.off_level = o; o += (NK + 1) * NM;
  P.off_pp = o; o += (NK + 1) * 4 * (NM - 1);
  P.off_ln_hn = o; o += NM;
  P.off_hn_pp = o; o += 4 * (NM - 1);
  P.stride = (o + 7) & ~7;
  return P;
}

// Status bit of a y(k, M) integral that exhausted divmax (scipy's AccuracyWarning): the bit of
// the family the row feeds first, h_m.
constexpr unsigned kStProfileDivmax = kStHaloDivmax0 << F_HM;

// The one-argument face of YGeneralIntegrand for romberg_group.
struct YGeneralNode {
  YGeneralIntegrand f;
  __device__ __forceinline__ void operator()(double x, double (&out)[1]) const { out[0] = f(x); }
};

// grid (NM, rows, n_epoch), block 64: row blockIdx.y + row0 of epoch blockIdx.z + epoch0, mass
// knot blockIdx.x.  ln_k_row: the ln k of row NK (rows < NK take the halo tables' knots).
// skip_nfw: leave the rows of an epoch with alpha = -1 alone (a mixed set-up integrates it with
// y_nfw).  At the knots the reference's splines of ln c, ln r_vir and ln halo_normalization
// return the knot values, so the closed forms stand for them.
__global__ __launch_bounds__(64) void k_y_general_table(
    chomp_config cfg, TabLayout L, ProfLayout P, const Epoch* __restrict__ epochs, int epoch0,
    const double* __restrict__ tab, const chomp_halo_par* __restrict__ profile, int row0,
    double ln_k_row, int skip_nfw, double* __restrict__ prof, unsigned* __restrict__ status) {
  const int m = blockIdx.x, row = row0 + (int)blockIdx.y, e = epoch0 + (int)blockIdx.z;
  const double alpha = profile[e].alpha;
  if (skip_nfw && alpha == -1.0) return;
  const Epoch& E = epochs[e];
  const double ln_k = row < L.NK ? linspace_at(log(cfg.k_min), log(cfg.k_max), L.NK, row) : ln_k_row;
  const double lnm = tab[(size_t)e * L.stride + L.off_ln_mass + m];
  const double mass = exp(lnm);
  const double con = exp(E.ln_c_const + E.beta * lnm);
  const double r_vir = exp((E.ln_rv_const + lnm) * (1.0 / 3.0));
  const double k = exp(ln_k);
  const double norm = y_general_norm(alpha, k, r_vir, con);
  const YGeneralNode f{YGeneralIntegrand{alpha, k, r_vir, con, norm}};
  const RombergOut<1> r = romberg_group<1, 1>(f, 1e-8, con, cfg.global_precision,
                                              cfg.halo_precision, cfg.divmax, nullptr);
  if (threadIdx.x != 0) return;
  const double hn = halo_normalization(E.rho_bar, E.prof_delta_v, alpha, con);
  double* p = prof + (size_t)e * P.stride;
  p[P.off_y + row * P.NM + m] = r.value[0] / norm * y_general_scale(r_vir, con, hn, mass);
  p[P.off_level + row * P.NM + m] = (double)r.level[0];
  if (!r.converged[0] && row < L.NK) atomicOr(&status[e], kStProfileDivmax);
}

// grid n_epoch, block 64: ln halo_normalization of epoch blockIdx.x + epoch0 at the mass knots
// (halo.py:848), for k_y_general_splines' last block.
__global__ __launch_bounds__(64) void k_halo_normalization_knots(
    TabLayout L, ProfLayout P, const Epoch* __restrict__ epochs, int epoch0,
    const double* __restrict__ tab, const chomp_halo_par* __restrict__ profile,
    double* __restrict__ prof) {
  const int e = epoch0 + (int)blockIdx.x;
  const Epoch& E = epochs[e];
  for (int m = threadIdx.x; m < P.NM; m += 64) {
    const double lnm = tab[(size_t)e * L.stride + L.off_ln_mass + m];
    const double con = exp(E.ln_c_const + E.beta * lnm);
    prof[(size_t)e * P.stride + P.off_ln_hn + m] =
        log(halo_normalization(E.rho_bar, E.prof_delta_v, profile[e].alpha, con));
  }
}

// grid (rows + with_hn, n_epoch), block 64, LDS 11 NM doubles: the spline of row blockIdx.x + row0
// over ln M; with_hn: the last block of an epoch builds the spline of ln halo_normalization.
__global__ __launch_bounds__(64) void k_y_general_splines(
    TabLayout L, ProfLayout P, int epoch0, const double* __restrict__ tab,
    const chomp_halo_par* __restrict__ profile, int row0, int skip_nfw, int with_hn,
    double* __restrict__ prof) {
  extern __shared__ __align__(16) double sm[];
  const int NM = P.NM;
  const int e = epoch0 + (int)blockIdx.y;
  if (skip_nfw && profile[e].alpha == -1.0) return;
  const bool hn = with_hn && blockIdx.x + 1 == gridDim.x;
  const int row = row0 + (int)blockIdx.x;
  double* x = sm;
  double* y = x + NM;
  double* work = y + NM;               // [9 NM]
  double* p = prof + (size_t)e * P.stride;
  for (int i = threadIdx.x; i < NM; i += 64) {
    x[i] = tab[(size_t)e * L.stride + L.off_ln_mass + i];
    y[i] = hn ? p[P.off_ln_hn + i] : p[P.off_y + row * NM + i];
  }
  __syncthreads();
  spline_build_pcr(x, y, NM, hn ? p + P.off_hn_pp : p + P.off_pp + (size_t)row * 4 * (NM - 1), work,
                   (int)threadIdx.x, 64, true);
}

// y(k, M) of a row's spline: zero outside the mass table (halo.py:496-498).
struct YRow {
  const double* lnm_knots;   // [NM]
  const double* pp;          // [4 (NM - 1)]
  int NM;
  double lnm_min, lnm_max;
  __device__ __forceinline__ double operator()(double lnm) const {
    if (!(lnm >= lnm_min && lnm <= lnm_max)) return 0.0;
    return spline_eval(lnm_knots, pp, NM, lnm);
  }
};

// The integrands of halo.py:922-927, 964-969, 989-994, 1032-1041, 1078-1086, 1194-1199 and
// HaloExclusion's (:1208-1221) as IntegrandMM .. IntegrandI12 state them, with Halo.y's dispatch
// (halo.py:487-489) in place of y_nfw: the row's spline, or -- general == false, an epoch with
// alpha = -1 in a mixed set-up -- y_nfw itself.
struct ProfileY {
  HaloCtx c;
  YRow row;
  bool general;
  __device__ __forceinline__ double operator()(double lnm) const {
    return general ? row(lnm) : y_nfw(*c.e, *c.sici, c.ln_k, lnm);
  }
};

struct IntegrandMMProfile {       // out[0] = h_m, out[1] = pp_mm (x rho_bar)
  ProfileY y;
  __device__ __forceinline__ void operator()(double ln_nu, double (&out)[2]) const {
    const HaloCtx& c = y.c;
    const double nu = exp(ln_nu);
    const double lnm = spline_eval(c.nu_knots, c.lnm_pp, c.NM, nu);
    const double yv = y(lnm);
    double nf, b;
    mf_node(*c.e, nu, ln_nu, true, &nf, &b);
    out[0] = nf * b * yv * c.window(lnm);
    out[1] = nf * exp(lnm) * yv * yv;
  }
};

struct IntegrandI12Profile {      // out[0] = I_1^2 (x rho_bar)
  ProfileY y;
  __device__ __forceinline__ void operator()(double ln_nu, double (&out)[1]) const {
    const HaloCtx& c = y.c;
    const double nu = exp(ln_nu);
    const double lnm = spline_eval(c.nu_knots, c.lnm_pp, c.NM, nu);
    const double yv = y(lnm);
    double nf, b;
    mf_node(*c.e, nu, ln_nu, true, &nf, &b);
    out[0] = nf * b * exp(lnm) * yv * yv;
  }
};

struct IntegrandGMProfile {       // out[0] = h_g, out[1] = pp_gm
  ProfileY y;
  bool want_hg;
  __device__ __forceinline__ void operator()(double ln_nu, double (&out)[2]) const {
    const HaloCtx& c = y.c;
    const double nu = exp(ln_nu);
    const double lnm = spline_eval(c.nu_knots, c.lnm_pp, c.NM, nu);
    const double mass = exp(lnm);
    const double yv = y(lnm);
    double nf, b = 0.0, n1, n2;
    mf_node(*c.e, nu, ln_nu, want_hg, &nf, &b);
    hod_node(*c.e, mass, lnm, &n1, &n2);
    out[0] = nf * b * yv * n1 / mass * (want_hg ? c.window(lnm) : 1.0);
    out[1] = (n1 < 1.0) ? nf * n1 * yv : nf * n1 * yv * yv;
  }
};

struct IntegrandGGProfile {       // out[0] = pp_gg
  ProfileY y;
  __device__ __forceinline__ void operator()(double ln_nu, double (&out)[1]) const {
    const HaloCtx& c = y.c;
    const double nu = exp(ln_nu);
    const double lnm = spline_eval(c.nu_knots, c.lnm_pp, c.NM, nu);
    const double mass = exp(lnm);
    const double yv = y(lnm);
    double nf, b, n1, n2;
    mf_node(*c.e, nu, ln_nu, false, &nf, &b);
    hod_node(*c.e, mass, lnm, &n1, &n2);
    out[0] = (n2 < 1.0) ? nf * n2 * yv / mass : nf * n2 * yv * yv / mass;
  }
};

// LDS doubles of a k_halo_knots_general block: HaloLds' tables, the row's knots and spline, the
// Romberg scratch of a four-wavefront group.
__host__ __device__ inline int knots_general_lds_doubles(int NM) {
  return NM + 8 * (NM - 1) + NM + 4 * (NM - 1) + kKnotScratch;
}

// grid (n_epoch, NK + 1, n_groups), block 256 = one wavefront group per (epoch, group, knot); the
// extra y-block of z == 0 integrates n_bar (halo.py:674-700).  Limits and stopping rule as the
// literal evaluation of the NFW path (deep_literal); values and levels go into the epoch's knot
// tables, un-normalised, for k_halo_finalize_general.  No node tables, no fast sums, no lists.
__global__ __launch_bounds__(256) void k_halo_knots_general(
    chomp_config cfg, TabLayout L, ProfLayout P, const Epoch* __restrict__ epochs,
    double* __restrict__ tab, const chomp_halo_par* __restrict__ profile,
    const HodDev* __restrict__ hod, const SiCiTab* __restrict__ sici_g,
    const double* __restrict__ prof, int g0, int g1, int g2, int g3, unsigned mask,
    unsigned* __restrict__ status) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ SiCiTab S;
  constexpr int NWV = 4;
  const int NK = L.NK, NM = L.NM;
  const int e = blockIdx.x, ik = blockIdx.y;
  const int group = pick_group((int)blockIdx.z, g0, g1, g2, g3);
  const bool nbar_block = ik == NK;
  if (nbar_block ? blockIdx.z != 0 : (group < 0 || group > 3)) return;
  double* t = tab + (size_t)e * L.stride;
  HaloLds H;
  H.stage(L, E, S, epochs, e, t, profile, hod, sici_g, sm);
  if (nbar_block) {
    HaloCtx c{&E, &S, H.nu_knots, H.lnm_pp, NM, 0.0, false};
    IntegrandNbar f{c};
    double* red = H.rest + NM + 4 * (NM - 1);
    const double v = romberg1<NWV>(f, E.ln_nu_lo_first, log(E.nu_max), cfg.global_precision,
                                   cfg.halo_precision, cfg.divmax, red);
    if (threadIdx.x == 0) t[L.off_misc] = v;
    return;
  }
  const bool general = profile[e].alpha != -1.0;
  double* row_x = H.rest;                  // [NM]
  double* row_pp = row_x + NM;             // [4 (NM - 1)]
  double* red = row_pp + 4 * (NM - 1);
  if (general) {
    const double* p = prof + (size_t)e * P.stride;
    copy_doubles(row_x, t + L.off_ln_mass, NM);
    copy_doubles(row_pp, p + P.off_pp + (size_t)ik * 4 * (NM - 1), 4 * (NM - 1));
  }
  __syncthreads();
  const HaloCtx c{&E, &S, H.nu_knots, H.lnm_pp, NM,
                  linspace_at(log(cfg.k_min), log(cfg.k_max), NK, ik), (mask & kMaskExclusion) != 0};
  const ProfileY y{c, YRow{row_x, row_pp, NM, E.ln_mass_min, E.ln_mass_max}, general};
  const int fa = group_fa(group), fb = group_fb(group);
  const bool pa = !group_single(group) && (mask & (1u << fa));
  const bool pb = (mask & (1u << fb)) != 0;
  const double hi = log(E.nu_max), lo = group_lower(E, group);
  double val[2] = {0.0, 0.0};
  int lev[2] = {0, 0};
  bool conv[2] = {true, true};
  if (group == 0 || group == 1) {
    RombergOut<2> r;
    if (group == 0)
      r = romberg_group<NWV, 2>(IntegrandMMProfile{y}, lo, hi, cfg.global_precision,
                                cfg.halo_precision, cfg.divmax, red);
    else
      r = romberg_group<NWV, 2>(IntegrandGMProfile{y, pa}, lo, hi, cfg.global_precision,
                                cfg.halo_precision, cfg.divmax, red);
    val[0] = r.value[0]; val[1] = r.value[1]; lev[0] = r.level[0]; lev[1] = r.level[1];
    conv[0] = r.converged[0]; conv[1] = r.converged[1];
  } else {
    RombergOut<1> r;
    if (group == 3)
      r = romberg_group<NWV, 1>(IntegrandI12Profile{y}, lo, hi, cfg.global_precision,
                                cfg.halo_precision, cfg.divmax, red);
    else
      r = romberg_group<NWV, 1>(IntegrandGGProfile{y}, lo, hi, cfg.global_precision,
                                cfg.halo_precision, cfg.divmax, red);
    val[1] = r.value[0]; lev[1] = r.level[0]; conv[1] = r.converged[0];
  }
  if (threadIdx.x != 0) return;
  double* levs = t + L.off_levels;
  if (pa) { t[L.off_knot[fa] + ik] = val[0]; levs[fa * NK + ik] = (double)lev[0]; }
  if (pb) { t[L.off_knot[fb] + ik] = val[1]; levs[fb * NK + ik] = (double)lev[1]; }
  unsigned st = 0u;                  // divmax exhausted (halo.py:1065-1071 and alike)
  if (pa && !conv[0]) st |= kStHaloDivmax0 << fa;
  if (pb && !conv[1]) st |= kStHaloDivmax0 << fb;
  if (st) atomicOr(&status[e], st);
}

// grid n_epoch, block 256, LDS finalize_lds_doubles(NK) doubles: behind k_halo_knots_general.
__global__ __launch_bounds__(256) void k_halo_finalize_general(
    chomp_config cfg, TabLayout L, Epoch* __restrict__ epochs, double* __restrict__ tab,
    unsigned fam_mask, unsigned* __restrict__ status) {
  extern __shared__ __align__(16) double sm[];
  halo_finalize_block(cfg, L, epochs, tab, (int)blockIdx.x, fam_mask, status, sm);
}

// Halo.y_general at n masses from row `row` of epoch e (halo.py:495-498).  LDS 5 NM - 4 doubles.
__global__ __launch_bounds__(256) void k_y_general_eval(
    TabLayout L, ProfLayout P, const Epoch* __restrict__ epochs, int e,
    const double* __restrict__ tab, const double* __restrict__ prof, int row,
    const double* __restrict__ mass, int n, double* __restrict__ out) {
  extern __shared__ __align__(16) double sm[];
  const int NM = P.NM;
  double* x = sm;
  double* pp = x + NM;
  copy_doubles(x, tab + (size_t)e * L.stride + L.off_ln_mass, NM);
  copy_doubles(pp, prof + (size_t)e * P.stride + P.off_pp + (size_t)row * 4 * (NM - 1), 4 * (NM - 1));
  __syncthreads();
  const YRow y{x, pp, NM, epochs[e].ln_mass_min, epochs[e].ln_mass_max};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = y(log(mass[i]));
}

// Halo.halo_normalization at n masses (halo.py:465-474): exp of the spline of its logarithm over
// ln M, extrapolated by the end pieces as FITPACK does.  LDS 5 NM - 4 doubles.
__global__ __launch_bounds__(256) void k_halo_normalization_eval(
    TabLayout L, ProfLayout P, int e, const double* __restrict__ tab,
    const double* __restrict__ prof, const double* __restrict__ mass, int n,
    double* __restrict__ out) {
  extern __shared__ __align__(16) double sm[];
  const int NM = P.NM;
  double* x = sm;
  double* pp = x + NM;
  copy_doubles(x, tab + (size_t)e * L.stride + L.off_ln_mass, NM);
  copy_doubles(pp, prof + (size_t)e * P.stride + P.off_hn_pp, 4 * (NM - 1));
  __syncthreads();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = exp(spline_eval(x, pp, NM, log(mass[i])));
}

}  // namespace chomp
