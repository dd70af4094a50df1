// TEST-ONLY harness: the fourth device counterpart of tests/hostcheck.  One HIP translation unit
// that compiles the product's header chain (chomp_cov_kernels.h down to chomp_math.h) FOR THE
// DEVICE, with the product's compiler flags, and drives the layer that turns the knot tables into
// P(k): k_power (PowerEval::eval_t), PowerEval::at_ln, the Stage E launch shapes (k_power_grid;
// k_power_prep + k_power_stream + k_power_grid_lanes), k_power_extrap, k_cell_ptab and the
// 6-point stencil CellTabIntegrand::from_table -- on epochs, knot tables and piecewise-cubic
// coefficients handed in (no halo set-up runs).  It launches the product's own __global__ kernels
// with the product's block sizes and dynamic-LDS sizes; the thin kernels below exist only where
// the product has no kernel of its own around a device function.  It includes the headers
// themselves, never copies of their functions.  Never loaded by the chomp_amd package, not in
// _lib.UNITS, no part of the C ABI.  Built and loaded by tests/devcheck_build.py.
//
// Every entry point allocates its buffers, launches, synchronises, returns the HIP error code
// (0: success; -1: an argument outside what the buffers were sized for) and frees its buffers,
// unless it is a plain getter.  Every output and work buffer is filled with NaN bytes before the
// launch (a sample a kernel never wrote poisons the result), but for the list of slow k groups,
// which is zeroed as the product's is, and the node table of the stencil kernel, whose values the
// harness supplies.
//
// Inputs common to the entry points ("the set-up"):
//   ein      n_epoch records of dw_epoch_inputs() doubles: the kEpochIn inputs of epoch_fill.h, then
//            hf_k_s hf_a_n hf_b_n hf_c_n hf_alpha_n hf_beta_n hf_gamma_n hf_mu_n hf_nu_n hf_f1
//            hf_f2 hf_f3
//   tab      n_epoch table blocks of dw_layout(NK)'s stride: off_knot[f], off_kpp[f], misc[2..7]
//            as the caller wants them; misc[1] = amp sigma_norm^2 is written on the device, as
//            k_halo_knots writes it
//   k_min, k_max, delta_b[n_epoch]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../chomp_amd/csrc/chomp_cov_kernels.h"
#include "power_setup.h"

using chomp::Epoch;
using chomp::PowerEval;
using chomp::TabLayout;

namespace {

// the host plumbing and the set-up (epochs and table blocks on the device): power_setup.h
using devcheck::Dev;
using devcheck::DevI;
using devcheck::Setup;
using devcheck::setup_ok;
using devcheck::kIn;
using devcheck::kNM;
using devcheck::kMinNK;
using devcheck::kMaxNK;
constexpr size_t kMaxK = (size_t)1 << 22;

// ---------------------------------------------------------------------------------------
// test-only kernels: the product has none around these device functions
// ---------------------------------------------------------------------------------------
// log(k_min), log(k_max) as the device's log gives them (every evaluator forms its knots from them)
__global__ void k_logs(double k_min, double k_max, double* out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { out[0] = log(k_min); out[1] = log(k_max); }
}

// grid ceil(n / 256), block 256, dynamic LDS 12 (NK - 1) doubles: PowerEval staged as k_power
// stages it, then at_ln<HF, BAO>(log k, k); beside it what the reference needs to isolate the
// evaluator's own arithmetic: out[f * n + i], f = 0 at_ln, 1 log(k), 2 power_shape_t(log k),
// 3 fast_log(k), 4 power_shape_t(fast_log k) (the shape Stage E's launch shapes multiply by)
template <bool HF, bool BAO>
__global__ __launch_bounds__(256) void k_at_ln(chomp_config cfg, TabLayout L, const Epoch* epochs,
                                               int e, const double* tab, int which,
                                               const double* delta_b, const double* k, int n,
                                               double* out) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  chomp::copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
                      chomp::kEpochDoubles);
  PowerEval P;
  P.stage(cfg, L, &E, tab + (size_t)e * L.stride, which, sm);
  if (chomp::is_ssc(which & 15)) P.delta_b = delta_b[e];
  __syncthreads();
  P.template finish_t<BAO>();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double kv = k[i], lk = log(kv), fl = chomp::fast_log(kv);
  out[i] = P.template at_ln<HF, BAO>(lk, kv);
  out[(size_t)n + i] = lk;
  out[(size_t)2 * n + i] = chomp::power_shape_t<BAO>(E, lk, kv);
  out[(size_t)3 * n + i] = fl;
  out[(size_t)4 * n + i] = chomp::power_shape_t<BAO>(E, fl, kv);
}

// grid ceil(n / 256), block 256, dynamic LDS 12 (NK - 1) doubles: from_table at lk[i] on the
// table handed in (out[i], ok in out[n + i]) and operator() at level 0 on a neutral node table
// (F = 1, ln chi = 0, chi = 1: with ell = k_i, ln ell = lk_i it evaluates ln k = lk_i, k = k_i --
// the table's value, or at_ln where from_table declines) in out[2 n + i]
template <bool HF>
__global__ __launch_bounds__(256) void k_stencil(chomp_config cfg, TabLayout L, const Epoch* epochs,
                                                 const double* tab, int which, const double* ptab,
                                                 const double* lk, const double* kk, int n,
                                                 const double* nodes, double* out) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  chomp::copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[0]),
                      chomp::kEpochDoubles);
  PowerEval P;
  P.stage(cfg, L, &E, tab, which, sm);
  __syncthreads();
  P.finish();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double px0 = log(cfg.k_min), pdx = (log(cfg.k_max) - px0) / (double)chomp::kPTabN;
  const chomp::CellTabIntegrand<HF, false, false> f{&P, nodes, 2L, 0, kk[i], lk[i], ptab, px0, pdx,
                                                    1.0 / pdx, {&P, nullptr, kk[i], 1.0}};
  bool ok = false;
  const double v = f.from_table(lk[i], &ok);
  double o[1] = {0.0};
  f(1.0, o, 0, 0L);
  out[i] = v;
  out[(size_t)n + i] = ok ? 1.0 : 0.0;
  out[(size_t)2 * n + i] = o[0];
}

bool ssc_code(int w) { return w == CHOMP_P_SSC_RESPONSE || w == CHOMP_P_MM_SSC; }   // (is_ssc, host)
bool code_ok(int w) { return w >= CHOMP_P_LIN && w <= CHOMP_P_MM_SSC; }
bool which_ok(int which) {
  return code_ok(which & 15) && (which & ~(15 | CHOMP_P_HALOFIT | CHOMP_P_EXTRAPOLATE)) == 0;
}

template <class F>
void with_bao(int bao, F f) {
  if (bao) f(std::true_type{}); else f(std::false_type{});
}
template <class F>
void with2(int a, int b, F f) {
  if (a) { if (b) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
  else { if (b) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
}

}  // namespace

// ---------------------------------------------------------------------------------------
// C entry points
// ---------------------------------------------------------------------------------------
extern "C" {

int dw_ptab_n() { return chomp::kPTabN; }
int dw_sizeof_epoch() { return (int)sizeof(Epoch); }
int dw_epoch_inputs() { return kIn; }
// out: kWaveIdxMask, kWaveSlow, kWaveTwo
void dw_wave_bits(int* out) {
  out[0] = chomp::kWaveIdxMask; out[1] = chomp::kWaveSlow; out[2] = chomp::kWaveTwo;
}
// make_layout(NM, NK) of the table blocks: out[0..5] off_knot, [6..11] off_kpp, [12] off_misc,
// [13] stride
int dw_layout(int NK, int* out) {
  if (NK < kMinNK || NK > kMaxNK) return -1;
  const TabLayout L = chomp::make_layout(kNM, NK);
  for (int f = 0; f < 6; ++f) { out[f] = L.off_knot[f]; out[6 + f] = L.off_kpp[f]; }
  out[12] = L.off_misc;
  out[13] = L.stride;
  return 0;
}

// out[0] = log(k_min), out[1] = log(k_max) by the device's log
int dw_logs(double k_min, double k_max, double* out) {
  Dev d_o(2, nullptr);
  DW_TRY(d_o.err);
  DW_TRY(d_o.nan_fill());
  k_logs<<<1, 64>>>(k_min, k_max, d_o.p);
  DW_SYNC();
  DW_TRY(d_o.back(out, 2));
  return 0;
}

// the Epoch records as filled on the device (n_epoch * dw_sizeof_epoch() bytes) and every
// epoch's misc[1]
int dw_epochs(int n_epoch, const double* ein, const double* tab, int NK, double k_min, double k_max,
              void* epochs_out, double* misc1_out) {
  if (!setup_ok(n_epoch, NK, k_min, k_max)) return -1;
  std::vector<double> zero(n_epoch, 0.0);
  Setup S(n_epoch, ein, tab, NK, k_min, k_max, zero.data());
  if (const int rc = S.init()) return rc;
  DW_TRY(hipMemcpy(epochs_out, S.d_ep.p, (size_t)n_epoch * sizeof(Epoch), hipMemcpyDeviceToHost));
  for (int e = 0; e < n_epoch; ++e)
    DW_TRY(hipMemcpy(misc1_out + e, S.d_tab.p + (size_t)e * S.L.stride + S.L.off_misc + 1,
                     sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// k_power<BAO> (PowerEval::eval_t) of `which` (a code | CHOMP_P_HALOFIT | CHOMP_P_EXTRAPOLATE)
// with the product's launch shape; out[e * nk + i]
int dw_eval(int n_epoch, const double* ein, const double* tab, int NK, double k_min, double k_max,
            const double* delta_b, int bao, int which, const double* k, int nk, double* out) {
  if (!setup_ok(n_epoch, NK, k_min, k_max) || !which_ok(which) || nk < 1 || (size_t)nk > kMaxK)
    return -1;
  Setup S(n_epoch, ein, tab, NK, k_min, k_max, delta_b);
  if (const int rc = S.init()) return rc;
  Dev d_k(nk, k), d_o((size_t)n_epoch * nk, nullptr);
  DW_TRY(d_k.err); DW_TRY(d_o.err);
  DW_TRY(d_o.nan_fill());
  const unsigned gx = (unsigned)std::min<size_t>(((size_t)nk + 255) / 256, 2048);   // (chomp_power)
  with_bao(bao, [&](auto BAO) {
    chomp::k_power<BAO><<<dim3(gx, (unsigned)n_epoch), dim3(256), S.lds()>>>(
        S.cfg, S.L, S.ep(), S.d_tab.p, which, 0, d_k.p, (size_t)nk, d_o.p, S.d_db.p);
  });
  DW_SYNC();
  DW_TRY(d_o.back(out, (size_t)n_epoch * nk));
  return 0;
}

// at_ln<HF, BAO> of epoch e (HF from `which`; the halo-model and HaloFit codes LIN..GG only: at_ln
// has no super-sample branch); out: 5 nk doubles (k_at_ln)
int dw_at_ln(int n_epoch, const double* ein, const double* tab, int NK, double k_min, double k_max,
             const double* delta_b, int bao, int which, int e, const double* k, int nk,
             double* out) {
  if (!setup_ok(n_epoch, NK, k_min, k_max) || !which_ok(which) || (which & 15) > CHOMP_P_GG ||
      e < 0 || e >= n_epoch || nk < 1 || (size_t)nk > kMaxK)
    return -1;
  Setup S(n_epoch, ein, tab, NK, k_min, k_max, delta_b);
  if (const int rc = S.init()) return rc;
  Dev d_k(nk, k), d_o((size_t)5 * nk, nullptr);
  DW_TRY(d_k.err); DW_TRY(d_o.err);
  DW_TRY(d_o.nan_fill());
  with2((which & CHOMP_P_HALOFIT) != 0, bao, [&](auto HF, auto BAO) {
    k_at_ln<HF, BAO><<<dim3((unsigned)((nk + 255) / 256)), dim3(256), S.lds()>>>(
        S.cfg, S.L, S.ep(), e, S.d_tab.p, which, S.d_db.p, d_k.p, nk, d_o.p);
  });
  DW_SYNC();
  DW_TRY(d_o.back(out, (size_t)5 * nk));
  return 0;
}

// k_power_grid<BAO, SSC> with explicit epochs_per_y, grid (ceil(nk / 512), ceil(n / epochs_per_y));
// out[e * nk + i]
int dw_grid(int n_epoch, const double* ein, const double* tab, int NK, double k_min, double k_max,
            const double* delta_b, int bao, int w, int extrap, int epochs_per_y, const double* k,
            int nk, double* out) {
  if (!setup_ok(n_epoch, NK, k_min, k_max) || !code_ok(w) || nk < 1 || (size_t)nk > kMaxK ||
      epochs_per_y < 1 || epochs_per_y > n_epoch)
    return -1;
  Setup S(n_epoch, ein, tab, NK, k_min, k_max, delta_b);
  if (const int rc = S.init()) return rc;
  Dev d_k(nk, k), d_o((size_t)n_epoch * nk, nullptr);
  DW_TRY(d_k.err); DW_TRY(d_o.err);
  DW_TRY(d_o.nan_fill());
  const unsigned gx = (unsigned)(((size_t)nk + 511) / 512);
  const unsigned gy = (unsigned)((n_epoch + epochs_per_y - 1) / epochs_per_y);
  with2(bao, ssc_code(w), [&](auto BAO, auto SSC) {
    chomp::k_power_grid<BAO, SSC><<<dim3(gx, gy), dim3(256)>>>(
        S.cfg, S.L, S.ep(), S.d_tab.p, w, 0, n_epoch, epochs_per_y, d_k.p, (size_t)nk, d_o.p,
        extrap != 0, S.d_db.p);
  });
  DW_SYNC();
  DW_TRY(d_o.back(out, (size_t)n_epoch * nk));
  return 0;
}

// The streaming shape as chomp_power runs it: per call c of n_call (<= 4) k grids of nk (even)
// values, k_power_prep<BAO> (shapes of epoch 0: the epochs share one cosmology),
// k_power_stream<PER, SSC> (PER = 2 for an even n_epoch, else 1), k_power_grid_lanes<BAO, SSC> on
// lanes_blocks blocks (the product: 1024) -- on ONE set of ktab / winfo / slow buffers sized as
// stage_e_prep sizes them, parity 0, 1, 0, 1.  out[(c * n_epoch + e) * nk + i];
// winfo_out[c * gx8 * 4 + g] (gx8 = roundup8(ceil(nk / 512))); slow_out[2 c + {0, 1}] the two
// counters after call c.
int dw_stream(int n_epoch, const double* ein, const double* tab, int NK, double k_min, double k_max,
              const double* delta_b, int bao, int w, int extrap, int lanes_blocks, const double* k,
              int n_call, int nk, double* out, int* winfo_out, int* slow_out) {
  if (!setup_ok(n_epoch, NK, k_min, k_max) || !code_ok(w) || w == CHOMP_P_LIN || nk < 2 ||
      (nk & 1) != 0 || (size_t)nk > kMaxK || n_call < 1 || n_call > 4 || lanes_blocks < 1 ||
      lanes_blocks > 1024)
    return -1;
  Setup S(n_epoch, ein, tab, NK, k_min, k_max, delta_b);
  if (const int rc = S.init()) return rc;
  const unsigned gx = (unsigned)(((size_t)nk + 511) / 512);
  const unsigned gx8 = (gx + 7) / 8 * 8;
  const size_t groups = ((size_t)nk + 127) / 128;
  Dev d_k((size_t)n_call * nk, k), d_o((size_t)n_epoch * nk, nullptr), d_ktab((size_t)gx8 * 1024, nullptr);
  DevI d_winfo((size_t)gx8 * 4, nullptr), d_slow(groups + 2, nullptr);       // (slow: zeroed)
  DW_TRY(d_k.err); DW_TRY(d_o.err); DW_TRY(d_ktab.err); DW_TRY(d_winfo.err); DW_TRY(d_slow.err);
  DW_TRY(d_ktab.nan_fill());
  DW_TRY(d_winfo.nan_fill());
  const bool pairs = n_epoch % 2 == 0;
  for (int c = 0; c < n_call; ++c) {
    const int parity = c & 1;
    const double* dk = d_k.p + (size_t)c * nk;
    DW_TRY(d_o.nan_fill());
    with_bao(bao, [&](auto BAO) {
      chomp::k_power_prep<BAO><<<dim3(gx8), dim3(256)>>>(S.cfg, S.L, S.ep(), 0, w, dk, (size_t)nk,
                                                         d_ktab.p, d_winfo.p, d_slow.p, parity);
    });
    with2(pairs, ssc_code(w), [&](auto PAIRS, auto SSC) {
      constexpr int PER = PAIRS ? 2 : 1;
      chomp::k_power_stream<PER, SSC><<<dim3(gx8, (unsigned)(n_epoch / PER)), dim3(256)>>>(
          S.L, S.d_tab.p, w, 0, d_ktab.p, d_winfo.p, (size_t)nk, d_o.p, S.d_db.p);
    });
    with2(bao, ssc_code(w), [&](auto BAO, auto SSC) {
      chomp::k_power_grid_lanes<BAO, SSC><<<dim3((unsigned)lanes_blocks), dim3(256)>>>(
          S.cfg, S.L, S.ep(), S.d_tab.p, w, extrap != 0, 0, n_epoch, dk, (size_t)nk, d_o.p,
          d_slow.p, parity, S.d_db.p);
    });
    DW_SYNC();
    DW_TRY(d_o.back(out + (size_t)c * n_epoch * nk, (size_t)n_epoch * nk));
    DW_TRY(d_winfo.back(winfo_out + (size_t)c * gx8 * 4, (size_t)gx8 * 4));
    DW_TRY(d_slow.back(slow_out + 2 * c, 2));
  }
  return 0;
}

// k_power_extrap<BAO> of spectrum w (MM, GM or GG) on the knots handed in; misc_out[5 e + j] =
// misc[3 + j] of epoch e afterwards (NaN where the kernel wrote nothing)
int dw_extrap(int n_epoch, const double* ein, const double* tab, int NK, double k_min, double k_max,
              int bao, int w, double* misc_out) {
  if (!setup_ok(n_epoch, NK, k_min, k_max) || w < CHOMP_P_MM || w > CHOMP_P_GG) return -1;
  std::vector<double> zero(n_epoch, 0.0);
  Setup S(n_epoch, ein, tab, NK, k_min, k_max, zero.data());
  if (const int rc = S.init()) return rc;
  for (int e = 0; e < n_epoch; ++e)
    DW_TRY(hipMemset(S.d_tab.p + (size_t)e * S.L.stride + S.L.off_misc + 3, 0xFF, 5 * sizeof(double)));
  with_bao(bao, [&](auto BAO) {
    chomp::k_power_extrap<BAO><<<dim3((unsigned)n_epoch), dim3(64)>>>(S.cfg, S.L, S.ep(), S.d_tab.p,
                                                                      w, 0);
  });
  DW_SYNC();
  for (int e = 0; e < n_epoch; ++e)
    DW_TRY(hipMemcpy(misc_out + 5 * e, S.d_tab.p + (size_t)e * S.L.stride + S.L.off_misc + 3,
                     5 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// k_cell_ptab<HF, false> of epoch 0 (one epoch handed in; codes LIN..GG); out: kPTabN + 1 doubles
int dw_ptab(const double* ein, const double* tab, int NK, double k_min, double k_max, int which,
            double* out) {
  if (!setup_ok(1, NK, k_min, k_max) || !which_ok(which) || (which & 15) > CHOMP_P_GG) return -1;
  const double zero = 0.0;
  Setup S(1, ein, tab, NK, k_min, k_max, &zero);
  if (const int rc = S.init()) return rc;
  Dev d_o((size_t)chomp::kPTabN + 1, nullptr);
  DW_TRY(d_o.err);
  DW_TRY(d_o.nan_fill());
  with_bao((which & CHOMP_P_HALOFIT) != 0, [&](auto HF) {
    chomp::k_cell_ptab<HF, false><<<dim3((chomp::kPTabN + 256) / 256), dim3(256), S.lds()>>>(
        S.cfg, S.L, S.ep(), 0, S.d_tab.p, which, d_o.p);
  });
  DW_SYNC();
  DW_TRY(d_o.back(out, (size_t)chomp::kPTabN + 1));
  return 0;
}

// CellTabIntegrand<HF, false, false>::from_table on the table ptab (kPTabN + 1 doubles) handed in,
// at lk[i] (with k[i], for the fall-back to at_ln); out: 3 n doubles (k_stencil)
int dw_stencil(const double* ein, const double* tab, int NK, double k_min, double k_max, int which,
               const double* ptab, const double* lk, const double* k, int n, double* out) {
  if (!setup_ok(1, NK, k_min, k_max) || !which_ok(which) || (which & 15) > CHOMP_P_GG || n < 1 ||
      (size_t)n > kMaxK)
    return -1;
  const double zero = 0.0;
  Setup S(1, ein, tab, NK, k_min, k_max, &zero);
  if (const int rc = S.init()) return rc;
  const double nodes[6] = {1.0, 1.0, 0.0, 0.0, 1.0, 1.0};     // F_j, ln chi_j, chi_j; LT = 0
  Dev d_p((size_t)chomp::kPTabN + 1, ptab), d_l(n, lk), d_k(n, k), d_n(6, nodes),
      d_o((size_t)3 * n, nullptr);
  DW_TRY(d_p.err); DW_TRY(d_l.err); DW_TRY(d_k.err); DW_TRY(d_n.err); DW_TRY(d_o.err);
  DW_TRY(d_o.nan_fill());
  with_bao((which & CHOMP_P_HALOFIT) != 0, [&](auto HF) {
    k_stencil<HF><<<dim3((unsigned)((n + 255) / 256)), dim3(256), S.lds()>>>(
        S.cfg, S.L, S.ep(), S.d_tab.p, which, d_p.p, d_l.p, d_k.p, n, d_n.p, d_o.p);
  });
  DW_SYNC();
  DW_TRY(d_o.back(out, (size_t)3 * n));
  return 0;
}

}  // extern "C"
