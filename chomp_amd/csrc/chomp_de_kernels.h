// chomp_de_kernels.h -- w0-wa dark energy on the device (cosmology.py:96-104, 165-213).
//
//   k_de_table     the pressure integrals P_i = 3 int_0^{z_i} (1 + w) / (1 + z) dz of every
//                  distinct (w0, wa) of a set-up, one workgroup per (knot, table)
//   k_de_spline    their not-a-knot spline in ln a, one wavefront per table
//   k_de_epochs    E0(z) and what follows from it (omega_m, omega_l, delta_c, delta_v, rho_bar)
//                  of the epochs with dark energy, and their CHOMP_ST_DE_DIVMAX bit
//   k_de_chi       chi(z) of those epochs (cosmology.py:105-109 with the pressure in E)
//
// Only set-ups with a w0-wa cosmology launch any of them; Lambda-CDM epochs keep the path and
// the bits they always had.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "chomp_buffers.h"
#include "chomp_mass_kernels.h"

namespace chomp {

constexpr unsigned kStDeDivmax = CHOMP_ST_DE_DIVMAX;

// One (w0, wa) pair per table.
struct DePar {
  double w0, wa;
};

// Dark-energy pressure tables of one kind of set-up (the epochs', the projection's or the
// projection sets'): one per distinct (w0, wa), in the order `keys` lists them, valid while the
// keys stay the same.
struct DeTables {
  std::vector<DePar> keys;
  DeviceBuffer<double> d_tab;
  StagedBuffer<DePar> d_par;
  bool valid = false;
};

// Knots in the order the reference lists them: a ascending, so z_i descending and knot 0 the
// deepest integral (with the default precision knots 0..21 exhaust divmax = 20).  Blocks are
// dispatched x-major, i.e. the deep knots of every table first.  knots: ln a [n], then z [n]
// (computed on the host with numpy's formulas).
constexpr int kDeNW = 16;
__global__ __launch_bounds__(64 * kDeNW) void k_de_table(chomp_config cfg,
                                                        const DePar* __restrict__ par,
                                                        const double* __restrict__ knots,
                                                        double* __restrict__ tab) {
  __shared__ double red[romberg_scratch<kDeNW, 1>()];
  const int n = cfg.cosmo_npoints, i = blockIdx.x, s = blockIdx.y;
  const DePressureIntegrand f{par[s].w0, par[s].wa};
  Scalar1<DePressureIntegrand> w{f};
  const RombergOut<1> r = romberg_group<kDeNW, 1>(
      w, 0.0, knots[n + i], cfg.global_precision, cfg.cosmo_precision, cfg.divmax, red);
  if (threadIdx.x == 0) {
    double* t = tab + (size_t)s * de_stride(n);
    t[de_off_ln_a(n) + i] = knots[i];
    t[de_off_p(n) + i] = 3.0 * r.value[0];
    t[de_off_level(n) + i] = (double)r.level[0];
    t[de_off_conv(n) + i] = r.converged[0] ? 1.0 : 0.0;
  }
}

// grid n_tables, block 64: InterpolatedUnivariateSpline(ln a, P) (cosmology.py:103-104).
// lds: 11 n doubles.
__global__ __launch_bounds__(64) void k_de_spline(chomp_config cfg, double* __restrict__ tab) {
  extern __shared__ __align__(16) double sm_de[];
  const int n = cfg.cosmo_npoints;
  double* t = tab + (size_t)blockIdx.x * de_stride(n);
  double* lx = sm_de;
  double* ly = lx + n;
  for (int i = threadIdx.x; i < n; i += 64) {
    lx[i] = t[de_off_ln_a(n) + i];
    ly[i] = t[de_off_p(n) + i];
  }
  __syncthreads();
  spline_build_pcr(lx, ly, n, t + de_off_pp(n), ly + n, (int)threadIdx.x, 64, true);
}

// grid ceil(n_epoch / 64), block 64: thread e fixes up epoch e if its cosmology has dark
// energy (de_slot[e] >= 0), behind k_sigma_nodes (which wrote the Lambda-CDM values and cleared
// the status word) and ahead of the mass-limit search (which reads delta_c).
__global__ __launch_bounds__(64) void k_de_epochs(chomp_config cfg, const int* __restrict__ de_slot,
                                                  int n_epoch, const double* __restrict__ tab,
                                                  Epoch* __restrict__ epochs,
                                                  unsigned* __restrict__ status) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= n_epoch || de_slot[e] < 0) return;
  const int n = cfg.cosmo_npoints;
  const double* t = tab + (size_t)de_slot[e] * de_stride(n);
  Epoch& E = epochs[e];
  E.E0z = E0_de(E.om0, E.ol0, E.or0, de_spline(t, n), E.z);
  epoch_e0_dependents(E);
  bool conv = true;
  for (int i = 0; i < n; ++i) conv = conv && t[de_off_conv(n) + i] != 0.0;
  if (!conv) atomicOr(&status[e], kStDeDivmax);        // scipy: AccuracyWarning, last row kept
}

// grid n_epoch, block 64: chi of the epochs with dark energy, after the mass-limit search (whose
// chi role integrates the Lambda-CDM E: this replaces that value).
__global__ __launch_bounds__(64) void k_de_chi(chomp_config cfg, const int* __restrict__ de_slot,
                                               const double* __restrict__ tab,
                                               Epoch* __restrict__ epochs) {
  const int e = blockIdx.x;
  if (de_slot[e] < 0) return;
  const int n = cfg.cosmo_npoints;
  const Epoch& E = epochs[e];
  const EIntegrandDE f{E.om0, E.ol0, E.or0, E.H0,
                       de_spline(tab + (size_t)de_slot[e] * de_stride(n), n)};
  const double chi = romberg1<1>(f, 0.0, E.z, cfg.global_precision, cfg.cosmo_precision,
                                 cfg.divmax, nullptr);
  if (threadIdx.x == 0) epochs[e].chi = chi;
}

}  // namespace chomp
