// chomp_power_kernels.h -- Stage E (gfx950): evaluation of the spectra from the tables.
//
//   k_power         generic per-sample kernel: Halo.linear_power/power_mm/power_gm/power_gg
//                   (halo.py:266-439), HaloFit.power_* (halo.py:1325-1413)
//   k_power_prep + k_power_stream   row-major streaming of a large (k, z) grid
//   k_power_grid_lanes  per-lane pass of that shape for unsorted / ragged / out-of-range k groups
//   k_power_grid    row-walking streaming kernel (epochs of different cosmologies, small grids);
//                   it takes such k groups on the per-lane path itself
//   k_power_extrap  constants of Halo(extrapolate=True) above k_max
//   k_sigma_r, k_y_nfw, k_eval   point lookups of the mirror classes
#pragma once

#include "chomp_halo_kernels.h"

namespace chomp {

// ---------------------------------------------------------------------------
// Stage E.  grid (ceil(nk / (256*KPT)), n_epoch), block 256.  Each block stages
// its epoch's scalars and the pp-coefficients of the (up to 3) knot splines it
// needs in LDS, then streams k -> P with coalesced 8-byte accesses.
// ---------------------------------------------------------------------------
struct PowerFam { int fa, fb, fp; };
__device__ __forceinline__ bool is_ssc(int w) {
  return w == CHOMP_P_SSC_RESPONSE || w == CHOMP_P_MM_SSC;
}
// (the super-sample codes read h_m, I_1^2 and pp_mm: I_1^2 rides in the second 2-halo slot)
__device__ __forceinline__ PowerFam power_families(int w) {
  if (w == CHOMP_P_GM) return PowerFam{F_HG, F_HM, F_PPGM};
  if (w == CHOMP_P_GG) return PowerFam{F_HG, F_HG, F_PPGG};
  if (is_ssc(w)) return PowerFam{F_HM, F_I12, F_PPMM};
  return PowerFam{F_HM, F_HM, F_PPMM};
}

// HaloSuperSampleCovariance inside [k_min, k_max] (halo.py:1136-1169), from the linear spectrum
// As = P_lin(k), h = h_m(k), i12 = I_1^2(k), pp = pp_mm(k) and the epoch's delta_b:
//   P_mm = P_lin h^2 + pp (the very operations of P_mm's streaming shapes: the same bits),
//   dlnP/ddelta_b = (68/21 P_lin h^2 + I_1^2) / P_mm,  P_mm_ssc = P_mm (1 + delta_b dlnP/ddelta_b).
// Every launch shape evaluates this one function, so the shapes agree bit for bit.
constexpr double kSscBeat = 68.0 / 21.0;
__device__ __forceinline__ double ssc_in_range(int w, double As, double h, double i12, double pp,
                                               double delta_b) {
  const double h2 = h * h;
  const double pmm = fma(As, h2, pp);
  const double resp = fma(kSscBeat * As, h2, i12) / pmm;
  return w == CHOMP_P_SSC_RESPONSE ? resp : pmm * fma(resp, delta_b, 1.0);
}

// Above k_max with Halo(extrapolate=True) (halo.py:300-312, 341-367, 405-431); x[] are
// the epoch's misc[3..7] written by k_power_extrap.
// BAO (here and below): the context's transfer function, a compile-time choice in device
// code (chomp_set_transfer; transfer_t in chomp_math.h).
template <bool BAO>
__device__ __forceinline__ double power_tail(const Epoch& E, const double* x, int w, double kv,
                                             double k_max) {
  if (w == CHOMP_P_MM) return linear_power_t<BAO>(E, kv) * x[0];
  const double* vs = w == CHOMP_P_GM ? x + 1 : x + 3;          // value at k_max, log-slope
  return pow(kv / k_max, vs[1]) * vs[0];
}

template <bool BAO>
__device__ __forceinline__ double halofit_mm(const Epoch& E, double k) {
  // halo.py:1339-1360
  const double lk = log(k);
  const double dk = delta_k_ln_t<BAO>(E, lk, k);
  const double y = k / E.hf_k_s;
  const double d2q = dk * (pow(1.0 + dk, E.hf_beta_n) / (1.0 + E.hf_alpha_n * dk) *
                           exp(-(y / 4.0 + y * y / 8.0)));
  const double d2h = (E.hf_a_n * pow(y, 3.0 * E.hf_f1) /
                      (1.0 + E.hf_b_n * pow(y, E.hf_f2) +
                       pow(E.hf_c_n * E.hf_f3 * y, 3.0 - E.hf_gamma_n))) /
                     (1.0 + E.hf_mu_n / y + E.hf_nu_n / (y * y));
  return 2.0 * kPi * kPi / (k * k * k) * (d2q + d2h);
}

// halofit_mm for a caller that holds ln k as well: every power becomes one exp of a
// linear form in ln k, the linear spectrum comes from power_shape (halo.py:1339-1360).
template <bool BAO>
__device__ __forceinline__ double halofit_mm_ln(const Epoch& E, double amp2, double lk, double k) {
  const double k3 = k * k * k;
  const double dk = amp2 * power_shape_t<BAO>(E, lk, k) * k3 * (1.0 / (2.0 * kPi * kPi));
  const double ln_y = lk - log(E.hf_k_s);               // (log of a per-epoch constant)
  const double y = exp(ln_y);
  const double d2q = dk * exp(E.hf_beta_n * fast_log(1.0 + dk) - (y * 0.25 + y * y * 0.125)) /
                     (1.0 + E.hf_alpha_n * dk);
  const double t_b = exp(E.hf_f2 * ln_y);
  const double t_c = exp((3.0 - E.hf_gamma_n) * (log(E.hf_c_n * E.hf_f3) + ln_y));
  const double inv_y = 1.0 / y;
  const double d2h = E.hf_a_n * exp(3.0 * E.hf_f1 * ln_y) /
                     ((1.0 + E.hf_b_n * t_b + t_c) *
                      (1.0 + E.hf_mu_n * inv_y + E.hf_nu_n * inv_y * inv_y));
  return 2.0 * kPi * kPi / k3 * (d2q + d2h);
}

// P(k) of one epoch from tables staged in LDS: shared by k_power and by the
// projection integrands (correlation.py:270-275, 387-392 call halo.power_*).
struct PowerEval {
  const Epoch* E;
  const double *ca, *cb, *cp;     // pp coefficients: h_a, h_b, 1-halo term
  int NK, w;
  bool halofit, extrap;
  const double* tail;             // misc[3..7] of the epoch (k_power_extrap)
  double x0, dx, inv_dx, amp2, k_min, k_max, c_lo;
  double delta_b = 0.0;           // the epoch's delta_b (CHOMP_P_MM_SSC; set by the caller)

  // Stage the coefficient sets of spectrum `which` of epoch table `t` into `sm`
  // (needs 12 (NK-1) doubles) and set the evaluator up.  All threads call it;
  // __syncthreads() must follow before use.
  __device__ __forceinline__ void stage(const chomp_config& cfg, const TabLayout& L,
                                        const Epoch* Els, const double* t, int which,
                                        double* sm) {
    E = Els;
    NK = L.NK;
    halofit = (which & CHOMP_P_HALOFIT) != 0;
    extrap = (which & CHOMP_P_EXTRAPOLATE) != 0 && !halofit;   // HaloFit ignores it
    tail = t + L.off_misc + 3;
    w = which & 15;
    const PowerFam F = power_families(w);
    double* a = sm;
    double* b = a + 4 * (NK - 1);
    double* p = b + 4 * (NK - 1);
    if (needs_tables()) {
      copy_doubles(a, t + L.off_kpp[F.fa], 4 * (NK - 1));
      copy_doubles(b, t + L.off_kpp[F.fb], 4 * (NK - 1));
      copy_doubles(p, t + L.off_kpp[F.fp], 4 * (NK - 1));
    }
    ca = a; cb = b; cp = p;
    k_min = cfg.k_min;
    k_max = cfg.k_max;
    x0 = log(cfg.k_min);
    dx = (log(cfg.k_max) - x0) / (double)(NK - 1);
    inv_dx = 1.0 / dx;
    amp2 = 0.0;                     // set by finish(): *Els may still be being staged
    c_lo = 0.0;
  }
  __device__ __forceinline__ bool needs_tables() const {
    return w != CHOMP_P_LIN && !(halofit && w == CHOMP_P_MM);
  }
  // after the barrier: k < k_min constant (halo.py:314-317)
  template <bool BAO>
  __device__ __forceinline__ void finish_t() {
    amp2 = E->amp * E->sigma_norm * E->sigma_norm;
    if (w != CHOMP_P_LIN && !halofit) {
      const double ha = pp_poly(ca, 0, 0.0), p0 = pp_poly(cp, 0, 0.0);
      const double hb = is_ssc(w) ? ha : pp_poly(cb, 0, 0.0);   // (P_mm's constant)
      c_lo = ha * hb + p0 / linear_power_t<BAO>(*E, k_min);
    }
  }
  // (the projection kernels only run on no-wiggle contexts)
  __device__ __forceinline__ void finish() { finish_t<false>(); }
  __device__ __forceinline__ double operator()(double kv) const { return eval_t<false>(kv); }
  template <bool BAO>
  __device__ __forceinline__ double eval_t(double kv) const {
    if (w == CHOMP_P_LIN) return linear_power_t<BAO>(*E, kv);
    if (halofit) {
      const double pmm = halofit_mm<BAO>(*E, kv);
      if (w == CHOMP_P_MM) return pmm;
      double ha = 0.0, hb = 0.0, pp = 0.0;               // halo.py:649-672 range rule
      if (kv >= k_min && kv <= k_max) {
        const double lk = log(kv);
        ha = spline_eval_uniform(x0, dx, ca, NK, lk);
        hb = spline_eval_uniform(x0, dx, cb, NK, lk);
        pp = spline_eval_uniform(x0, dx, cp, NK, lk);
      }
      return pmm * ha * hb + pp;
    }
    if (is_ssc(w)) {                                      // halo.py:1136-1169
      if (kv < k_min) return w == CHOMP_P_SSC_RESPONSE ? 0.0 : linear_power_t<BAO>(*E, kv) * c_lo;
      if (!(kv <= k_max)) return 0.0;
      const double lk = log(kv);
      const double h = spline_eval_uniform(x0, dx, ca, NK, lk);
      const double i12 = spline_eval_uniform(x0, dx, cb, NK, lk);
      const double pp = spline_eval_uniform(x0, dx, cp, NK, lk);
      return ssc_in_range(w, amp2 * power_shape_t<BAO>(*E, lk, kv), h, i12, pp, delta_b);
    }
    if (kv < k_min) return linear_power_t<BAO>(*E, kv) * c_lo;
    if (extrap ? kv < k_max : kv <= k_max) {
      const double lk = log(kv);
      const double ha = spline_eval_uniform(x0, dx, ca, NK, lk);
      const double hb = spline_eval_uniform(x0, dx, cb, NK, lk);
      const double pp = spline_eval_uniform(x0, dx, cp, NK, lk);
      const double plin = 2.0 * kPi * kPi * delta_k_ln_t<BAO>(*E, lk, kv) / (kv * kv * kv);
      return plin * ha * hb + pp;
    }
    if (extrap) return power_tail<BAO>(*E, tail, w, kv, k_max);
    return 0.0;                                           // k > k_max (or NaN)
  }
  // The same spectrum for callers that integrate over ln k (w(theta), xi(r)) and so hold
  // both ln k and k: no logarithm is retaken, the three splines share one interval
  // lookup, and the linear spectrum uses the two-division arrangement of Stage E
  // (power_shape).  Agrees with operator() to rounding.
  // HF: compile-time copy of `halofit`, so that each instance carries one formula only.
  // BAO: the context's transfer function (compile time, as in eval_t).
  template <bool HF, bool BAO = false>
  __device__ __forceinline__ double at_ln(double lk, double kv) const {
    const bool in = kv >= k_min && kv <= k_max;
    if (HF) {
      if (w != CHOMP_P_MM && !in) return 0.0;             // halo.py:649-672 range rule
      const double pmm = halofit_mm_ln<BAO>(*E, amp2, lk, kv);
      if (w == CHOMP_P_MM) return pmm;
      int i = (int)floor((lk - x0) * inv_dx);
      i = i < 0 ? 0 : (i > NK - 2 ? NK - 2 : i);
      const double d = lk - (x0 + dx * (double)i);
      return pmm * pp_poly(ca, i, d) * pp_poly(cb, i, d) + pp_poly(cp, i, d);
    }
    if (w == CHOMP_P_LIN || !in || (extrap && !(kv < k_max))) {
      // the rarely taken branches (eval_t's, without the HaloFit formula this instance never uses)
      if (w == CHOMP_P_LIN) return linear_power_t<BAO>(*E, kv);
      if (kv < k_min) return linear_power_t<BAO>(*E, kv) * c_lo;
      if (extrap && kv >= k_max) return power_tail<BAO>(*E, tail, w, kv, k_max);
      return 0.0;                                         // k > k_max (or NaN)
    }
    int i = (int)floor((lk - x0) * inv_dx);
    i = i < 0 ? 0 : (i > NK - 2 ? NK - 2 : i);
    const double d = lk - (x0 + dx * (double)i);
    const double ha = pp_poly(ca, i, d), hb = pp_poly(cb, i, d), pp = pp_poly(cp, i, d);
    return amp2 * power_shape_t<BAO>(*E, lk, kv) * ha * hb + pp;
  }
};

// Halo(extrapolate=True): the constants of the continuation above k_max, from the knot
// tables of spectrum w (halo.py:300-312: misc[3]; :341-352 / :405-416: value at k_max and
// mean log-slope over knots -7..-1 into misc[4,5] (gm) / misc[6,7] (gg)).  grid n, block 64.
template <bool BAO>
__global__ void k_power_extrap(chomp_config cfg, TabLayout L, const Epoch* __restrict__ epochs,
                               double* __restrict__ tab, int w, int epoch0) {
  __shared__ double lv[6], lx[6];
  const int e = epoch0 + blockIdx.x;
  const Epoch& E = epochs[e];
  double* t = tab + (size_t)e * L.stride;
  const PowerFam F = power_families(w);
  const int NK = L.NK;
  const double* ka = t + L.off_knot[F.fa];
  const double* kb = t + L.off_knot[F.fb];
  const double* kp = t + L.off_knot[F.fp];
  const int i = threadIdx.x;
  if (i < 6) {
    const int j = NK - 7 + i;
    const double x = linspace_at(log(cfg.k_min), log(cfg.k_max), NK, j);
    lx[i] = x;
    lv[i] = log(linear_power_t<BAO>(E, exp(x)) * ka[j] * kb[j] + kp[j]);
  }
  __syncthreads();
  if (i == 0) {
    const double plin = linear_power_t<BAO>(E, cfg.k_max);
    const double ha = ka[NK - 1], hb = kb[NK - 1], pp = kp[NK - 1];
    if (w == CHOMP_P_MM) {
      t[L.off_misc + 3] = ha * hb + pp / plin;
    } else {
      double slope = 0.0;
      for (int m = 0; m < 5; ++m) slope += (lv[m + 1] - lv[m]) / (lx[m + 1] - lx[m]);
      double* vs = t + L.off_misc + (w == CHOMP_P_GM ? 4 : 6);
      vs[0] = plin * ha * hb + pp;
      vs[1] = slope / 5.0;
    }
  }
}

template <bool BAO>
__global__ __launch_bounds__(256) void k_power(chomp_config cfg, TabLayout L,
                                               const Epoch* __restrict__ epochs,
                                               const double* __restrict__ tab, int which,
                                               int epoch0, const double* __restrict__ k,
                                               size_t nk, double* __restrict__ out,
                                               const double* __restrict__ delta_b) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  const int e = epoch0 + blockIdx.y;
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  PowerEval P;
  P.stage(cfg, L, &E, tab + (size_t)e * L.stride, which, sm);
  if (is_ssc(which & 15)) P.delta_b = delta_b[e];
  __syncthreads();
  P.template finish_t<BAO>();
  double* o = out + (size_t)blockIdx.y * nk;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nk;
       i += (size_t)gridDim.x * blockDim.x)
    o[i] = P.template eval_t<BAO>(k[i]);
}

// ---------------------------------------------------------------------------
// k_power_grid (+ k_power_grid_lanes): Stage E over a whole (k, epoch) grid, built to
// run at HBM speed on large grids.  grid ceil(nk / 512), block 256; a thread owns two
// consecutive k (16-byte loads / stores) and walks the epochs:
//   * ln k, the knot interval and the Eisenstein-Hu shape (k/H0)^(3+n) T(k)^2 / k^3
//     are computed once per k and re-used for every epoch that shares the previous
//     epoch's cosmology (the z-axis of a (k, z) grid): per (k, z) sample that leaves
//     three cubic evaluations and one multiply;
//   * when all 128 k of a wavefront fall into one knot interval (the usual case for
//     a sorted grid) the 12 spline coefficients of an epoch are wave-uniform and
//     come through the scalar cache; any other wavefront takes the per-lane path.
// Algorithmic traffic: 8 B read per k + 8 B written per (k, epoch) sample.
// ---------------------------------------------------------------------------
// P(k) of epoch table t where the knot tables do not reach: k < k_min, k > k_max or NaN
// (halo.py:314-320, the tail of Halo(extrapolate=True); 0 for the super-sample codes above
// k_max and for the response below k_min), and every k of the linear spectrum.
template <bool BAO>
__device__ __forceinline__ double power_outside_knots(const chomp_config& cfg, const TabLayout& L,
                                                      const Epoch& E, const double* t,
                                                      const PowerFam& F, int w, bool extrap,
                                                      double kv) {
  if (w == CHOMP_P_LIN) return linear_power_t<BAO>(E, kv);
  if (kv < cfg.k_min) {
    if (w == CHOMP_P_SSC_RESPONSE) return 0.0;
    const int fb = is_ssc(w) ? F.fa : F.fb;               // (fb holds I_1^2: P_mm's constant)
    const double c_lo = t[L.off_kpp[F.fa]] * t[L.off_kpp[fb]] +
                        t[L.off_kpp[F.fp]] / linear_power_t<BAO>(E, cfg.k_min);
    return linear_power_t<BAO>(E, kv) * c_lo;
  }
  if (extrap && !is_ssc(w)) return power_tail<BAO>(E, t + L.off_misc + 3, w, kv, cfg.k_max);
  return 0.0;
}

// What one wavefront knows about its 128 k (two per lane).
struct KLanes {
  size_t i0;
  bool have0, have1, vec, in0, in1;
  double k0, k1, lk0, lk1;
  int idx0, idx1;
};

__device__ __forceinline__ KLanes load_k_lanes(const chomp_config& cfg, int NK,
                                               const double* __restrict__ k, size_t nk,
                                               size_t thread_index) {
  KLanes s;
  s.i0 = 2 * thread_index;
  s.have0 = s.i0 < nk;
  s.have1 = s.i0 + 1 < nk;
  s.vec = s.have1 && ((nk & 1) == 0);            // rows stay 16-byte aligned
  s.k0 = 1.0;
  s.k1 = 1.0;
  if (s.vec) {
    const double2 kk = *reinterpret_cast<const double2*>(k + s.i0);
    s.k0 = kk.x; s.k1 = kk.y;
  } else {
    if (s.have0) s.k0 = k[s.i0];
    if (s.have1) s.k1 = k[s.i0 + 1];
  }
  const double x0 = log(cfg.k_min);
  const double dx = (log(cfg.k_max) - x0) / (double)(NK - 1);
  const double inv_dx = 1.0 / dx;
  s.lk0 = fast_log(s.k0);
  s.lk1 = fast_log(s.k1);
  s.idx0 = (int)floor((s.lk0 - x0) * inv_dx);
  s.idx1 = (int)floor((s.lk1 - x0) * inv_dx);
  s.idx0 = s.idx0 < 0 ? 0 : (s.idx0 > NK - 2 ? NK - 2 : s.idx0);
  s.idx1 = s.idx1 < 0 ? 0 : (s.idx1 > NK - 2 ? NK - 2 : s.idx1);
  s.in0 = s.k0 >= cfg.k_min && s.k0 <= cfg.k_max;
  s.in1 = s.k1 >= cfg.k_min && s.k1 <= cfg.k_max;
  return s;
}

// How a wavefront's k sit on the knots: worked out by k_power_prep and k_power_grid with
// classify_wave, read back by k_power_stream from winfo / ktab.
struct WaveKnots {
  int idxu;           // the wavefront's lower knot interval (wave-uniform)
  bool fast, two;     // takes the fast path; straddles the knot idxu + 1 (both wave-uniform)
  bool s0, s1;        // this lane's k lies in the upper interval idxu + 1
  double d0, d1;      // ln k - the lower knot of its interval
};

__device__ __forceinline__ WaveKnots classify_wave(const chomp_config& cfg, int NK, const KLanes& s,
                                                   int w) {
  WaveKnots v;
  v.idxu = __builtin_amdgcn_readfirstlane(s.idx0);
  // Fast path: every k of the wavefront present, in range and in knot interval idxu or
  // idxu + 1 (a sorted grid straddles at most one knot per wavefront once nk >~ 6500;
  // indices are clamped to NK - 2, so idxu + 1 never runs past the last piece).
  v.fast = __all(s.have0 && s.have1 && s.in0 && s.in1 &&
                 (s.idx0 == v.idxu || s.idx0 == v.idxu + 1) &&
                 (s.idx1 == v.idxu || s.idx1 == v.idxu + 1)) &&
           w != CHOMP_P_LIN;
  v.two = !__all(s.idx0 == v.idxu && s.idx1 == v.idxu);
  v.s0 = s.idx0 != v.idxu;
  v.s1 = s.idx1 != v.idxu;
  v.d0 = v.d1 = 0.0;
  return v;
}
// ... and, for a wavefront on the fast path, the lanes' offsets d0 / d1 (k_power_prep takes them
// after the shapes: held across power_shape they cost k_power_prep<true> two VGPRs).
__device__ __forceinline__ void knot_offsets(const chomp_config& cfg, int NK, const KLanes& s,
                                             WaveKnots& v) {
  const double x0 = log(cfg.k_min);
  const double dx = (log(cfg.k_max) - x0) / (double)(NK - 1);
  const double xa = x0 + dx * (double)v.idxu, xb = x0 + dx * (double)(v.idxu + 1);
  v.d0 = s.lk0 - (v.s0 ? xb : xa);
  v.d1 = s.lk1 - (v.s1 ? xb : xa);
}

// The fast path's wave-uniform operands of one epoch (through the scalar cache): the
// amplitude and the pp coefficients of h_a, h_b and the 1-halo term on knot interval idxu.
struct Cubic {
  double c0, c1, c2, c3;
  __device__ __forceinline__ double at(double d) const { return fma(fma(fma(c3, d, c2), d, c1), d, c0); }
};
__device__ __forceinline__ Cubic cubic_at(const double* c) { return Cubic{c[0], c[1], c[2], c[3]}; }

struct PowerRow { double A; Cubic a, b, p; };

// Where those operands sit in an epoch table (the next interval's coefficients follow at +4).
struct RowCols {
  bool same_ab;       // P_mm and P_gg multiply a 2-halo factor by itself
  int oa, ob, op;
};
__device__ __forceinline__ RowCols row_cols(const TabLayout& L, int w, int idxu) {
  const PowerFam F = power_families(w);
  return RowCols{F.fa == F.fb, L.off_kpp[F.fa] + 4 * idxu, L.off_kpp[F.fb] + 4 * idxu,
                 L.off_kpp[F.fp] + 4 * idxu};
}
__device__ __forceinline__ PowerRow fetch_row(const TabLayout& L, const RowCols& o, const double* t) {
  return PowerRow{t[L.off_misc + 1], cubic_at(t + o.oa), cubic_at(t + o.ob), cubic_at(t + o.op)};
}

// The fast path's two samples of one epoch (row c of epoch table t), sh0 / sh1 the lanes'
// shapes.  k_power_grid and k_power_stream both evaluate this one function, so the launch
// shapes agree bit for bit.
template <bool SSC>
__device__ __forceinline__ void power_fast_pair(const PowerRow& c, const double* t, const RowCols& o,
                                                const WaveKnots& v, double sh0, double sh1, int w,
                                                double db, double& r0, double& r1) {
  const double d0 = v.d0, d1 = v.d1;
  double ha0 = c.a.at(d0), pp0 = c.p.at(d0);
  double ha1 = c.a.at(d1), pp1 = c.p.at(d1);
  // (hb1 declared first: in the other order k_power_stream<1, false> takes 24 VGPRs, not 22)
  double hb1 = ha1, hb0 = ha0;
  if (!o.same_ab) {                // wave-uniform
    hb0 = c.b.at(d0);
    hb1 = c.b.at(d1);
  }
  if (v.two) {     // the wavefront straddles a knot: lanes above it use the next piece
    const Cubic a = cubic_at(t + o.oa + 4), b = cubic_at(t + o.ob + 4), p = cubic_at(t + o.op + 4);
    if (v.s0) {
      ha0 = a.at(d0);
      hb0 = b.at(d0);
      pp0 = p.at(d0);
    }
    if (v.s1) {
      ha1 = a.at(d1);
      hb1 = b.at(d1);
      pp1 = p.at(d1);
    }
  }
  if constexpr (SSC) {
    r0 = ssc_in_range(w, c.A * sh0, ha0, hb0, pp0, db);
    r1 = ssc_in_range(w, c.A * sh1, ha1, hb1, pp1, db);
  } else {
    r0 = fma(c.A * sh0, ha0 * hb0, pp0);
    r1 = fma(c.A * sh1, ha1 * hb1, pp1);
  }
}

// 16-byte write-through store (sc1).  Issued from inline asm, so the compiler's hazard
// recogniser does not see a VMEM store: a store of more than 64 bits must not be
// followed directly by a VALU write of its data registers, hence the trailing s_nop.
__device__ __forceinline__ void store_wt16(double* p, double r0, double r1) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  typedef double v2d __attribute__((ext_vector_type(2)));
  v2d rr = {r0, r1};
  v4f bits = __builtin_bit_cast(v4f, rr);
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 2" : : "v"(p), "v"(bits) : "memory");
}

// Wavefronts (groups of 128 consecutive k) that cannot take the streaming kernel are
// collected by k_power_prep in a compact list for k_power_grid_lanes.  slow[0..1] are two
// counters used by alternate launches (`parity`): a launch appends through slow[parity] and
// clears slow[parity ^ 1] for the next one, so no separate memset is needed (launches of one
// context are stream-ordered).  slow[2...] is the list.
__device__ __forceinline__ void slow_list_begin(int* slow, int parity) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) slow[parity ^ 1] = 0;
}
__device__ __forceinline__ void slow_list_append(int* slow, int parity, int k_group) {
  const int at = atomicAdd(&slow[parity], 1);
  slow[2 + at] = k_group;
}

// One wavefront's 128 k (two per lane) for the epochs [q_lo, q_hi) on the per-lane path: any
// k, any knot interval, any order.  In-range k still re-use the Eisenstein-Hu shape across
// epochs of one cosmology; k outside [k_min, k_max] take the full formula (halo.py:314-320).
// SSC: w is one of the super-sample codes (a compile-time copy: P_mm's instances carry none of it).
template <bool BAO, bool SSC = false>
__device__ __forceinline__ void power_lanes_range(const chomp_config& cfg, const TabLayout& L,
                                                  const Epoch* __restrict__ epochs,
                                                  const double* __restrict__ tab, int w,
                                                  bool extrap, int epoch0, int q_lo, int q_hi,
                                                  const KLanes& s, size_t nk,
                                                  double* __restrict__ out,
                                                  const double* __restrict__ delta_b = nullptr) {
  const PowerFam F = power_families(w);
  const int NK = L.NK;
  const double x0 = log(cfg.k_min);
  const double dx = (log(cfg.k_max) - x0) / (double)(NK - 1);
  const double e0 = s.lk0 - (x0 + dx * (double)s.idx0), e1 = s.lk1 - (x0 + dx * (double)s.idx1);
  double sh0 = 0.0, sh1 = 0.0;
  for (int q = q_lo; q < q_hi; ++q) {
    const int e = epoch0 + q;
    const Epoch& E = epochs[e];
    const double* t = tab + (size_t)e * L.stride;
    double* o = out + (size_t)q * nk + s.i0;
    const bool same = q > q_lo && t[L.off_misc + 2] != 0.0;
    const double A = t[L.off_misc + 1];
    const double db = SSC ? delta_b[e] : 0.0;
    if (!same && w != CHOMP_P_LIN) {
      sh0 = power_shape_t<BAO>(E, s.lk0, s.k0);
      sh1 = power_shape_t<BAO>(E, s.lk1, s.k1);
    }
    auto lane = [&](bool have, bool in, int idx, double d, double sh, double kv, double* ol) {
      if (!have) return;
      if (in && w != CHOMP_P_LIN) {
        const double ha = pp_poly(t + L.off_kpp[F.fa], idx, d);
        const double hb = pp_poly(t + L.off_kpp[F.fb], idx, d);
        const double pp = pp_poly(t + L.off_kpp[F.fp], idx, d);
        *ol = SSC ? ssc_in_range(w, A * sh, ha, hb, pp, db) : fma(A * sh, ha * hb, pp);
      } else {
        *ol = power_outside_knots<BAO>(cfg, L, E, t, F, w, extrap, kv);
      }
    };
    lane(s.have0, s.in0, s.idx0, e0, sh0, s.k0, o);
    lane(s.have1, s.in1, s.idx1, e1, sh1, s.k1, o + 1);
  }
}

// The row-walking streaming pass (epochs of different cosmologies, or small grids).
// grid (ceil(nk / 512), ceil(n_epoch / epochs_per_y)), block 256.  A wavefront whose k
// do not qualify for the fast path evaluates its epochs on the per-lane path itself.
template <bool BAO, bool SSC = false>
__global__ __launch_bounds__(256) void k_power_grid(chomp_config cfg, TabLayout L,
                                                    const Epoch* __restrict__ epochs,
                                                    const double* __restrict__ tab, int w,
                                                    int epoch0, int n_epoch, int epochs_per_y,
                                                    const double* __restrict__ k, size_t nk,
                                                    double* __restrict__ out, bool extrap,
                                                    const double* __restrict__ delta_b) {
  const int k_group = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
  const KLanes s = load_k_lanes(cfg, L.NK, k, nk, (size_t)blockIdx.x * blockDim.x + threadIdx.x);
  WaveKnots v = classify_wave(cfg, L.NK, s, w);
  const int q_lo = blockIdx.y * epochs_per_y;
  int q_hi = q_lo + epochs_per_y;
  if (q_hi > n_epoch) q_hi = n_epoch;
  if (!v.fast) {
    if ((size_t)k_group * 128 < nk)
      power_lanes_range<BAO, SSC>(cfg, L, epochs, tab, w, extrap, epoch0, q_lo, q_hi, s, nk, out,
                                  delta_b);
    return;
  }
  knot_offsets(cfg, L.NK, s, v);
  const RowCols o = row_cols(L, w, v.idxu);
  double shape0 = 0.0, shape1 = 0.0;             // 2 pi^2 (k/H0)^(3+n) T^2 / k^3
  // Blocks start their walk at different rows (rows of a large grid are a power-of-two
  // stride apart: in lockstep every wavefront would hit the same HBM channels).
  const int cnt = q_hi - q_lo;
  int q = q_lo + (int)(blockIdx.x % (unsigned)cnt);
  // wave-uniform operands of one epoch: through the scalar cache, fetched one epoch
  // ahead of their use so that the loop never waits on a scalar load
  const double* tn = tab + (size_t)(epoch0 + q) * L.stride;
  PowerRow nxt = fetch_row(L, o, tn);
  double nxt_flag = tn[L.off_misc + 2];
  for (int j = 0; j < cnt; ++j) {
    const PowerRow c = nxt;
    const double flag = nxt_flag;
    const int qc = q;
    ++q;
    if (q == q_hi) q = q_lo;
    tn = tab + (size_t)(epoch0 + q) * L.stride;   // (one harmless re-fetch on the last trip)
    nxt = fetch_row(L, o, tn);
    nxt_flag = tn[L.off_misc + 2];
    const bool same = j > 0 && qc > q_lo && flag != 0.0;
    if (!same) {
      const Epoch& E = epochs[epoch0 + qc];
      shape0 = power_shape_t<BAO>(E, s.lk0, s.k0);
      shape1 = power_shape_t<BAO>(E, s.lk1, s.k1);
    }
    double r0, r1;
    power_fast_pair<SSC>(c, tab + (size_t)(epoch0 + qc) * L.stride, o, v, shape0, shape1, w,
                         SSC ? delta_b[epoch0 + qc] : 0.0, r0, r1);
    double* ot = out + (size_t)qc * nk + s.i0;
    // Streamed once, never re-read by this launch: 16-byte write-through (sc1) stores
    // (plain stores leave ~0.5 GB of dirty lines for the end-of-kernel release to
    // write back; MI355X_MICROARCH.md rows "boundary" / "publish-large").
    if (s.vec) {
      store_wt16(ot, r0, r1);
    } else {
      __builtin_nontemporal_store(r0, ot);
      __builtin_nontemporal_store(r1, ot + 1);
    }
  }
}

// ---- large grids of one cosmology: k_power_prep + k_power_stream ------------------
// HBM likes the output written in address order by short-lived wavefronts (a kernel
// whose threads each walk all rows of a 2^20 x 64 grid reaches ~4.5 TB/s of stores, the
// same stores issued row-major by (k chunk, few rows) blocks ~6.5 TB/s).  So everything
// that depends on k alone is tabulated once by k_power_prep -- 16 B per k: the offset of
// ln k in its knot interval and the Eisenstein-Hu shape 2 pi^2 (k/H0)^(3+n) T^2 / k^3 --
// and k_power_stream, launched row-major over (k chunk, PER rows), re-reads that table
// from L2 (a k chunk always lands on the same XCD: gridDim.x is a multiple of 8) and
// does 3 cubics + 1 multiply-add per sample.
constexpr int kWaveIdxMask = 0xffff, kWaveSlow = 1 << 16, kWaveTwo = 1 << 17;

// grid roundup8(ceil(nk / 512)), block 256.  ktab[2 i] = ln k_i - x_idx, ktab[2 i + 1] = shape_i,
// negative when k_i lies in the upper one of the wavefront's two knot intervals;
// winfo[g] = lowest knot interval of k group g | kWaveTwo | kWaveSlow.
template <bool BAO>
__global__ __launch_bounds__(256) void k_power_prep(chomp_config cfg, TabLayout L,
                                                    const Epoch* __restrict__ epochs,
                                                    int e_shape, int w,
                                                    const double* __restrict__ k, size_t nk,
                                                    double* __restrict__ ktab,
                                                    int* __restrict__ winfo,
                                                    int* __restrict__ slow, int parity) {
  slow_list_begin(slow, parity);
  const int k_group = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
  const size_t ti = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const KLanes s = load_k_lanes(cfg, L.NK, k, nk, ti);
  WaveKnots v = classify_wave(cfg, L.NK, s, w);
  if ((threadIdx.x & 63) == 0) {
    winfo[k_group] = v.idxu | (v.two ? kWaveTwo : 0) | (v.fast ? 0 : kWaveSlow);
    if (!v.fast && (size_t)k_group * 128 < nk) slow_list_append(slow, parity, k_group);
  }
  if (!v.fast) return;
  const Epoch& E = epochs[e_shape];
  const double sh0 = power_shape_t<BAO>(E, s.lk0, s.k0), sh1 = power_shape_t<BAO>(E, s.lk1, s.k1);
  knot_offsets(cfg, L.NK, s, v);
  double4 kt;
  kt.x = v.d0; kt.y = v.s0 ? -sh0 : sh0;
  kt.z = v.d1; kt.w = v.s1 ? -sh1 : sh1;
  *reinterpret_cast<double4*>(ktab + 4 * ti) = kt;
}

// grid (roundup8(ceil(nk / 512)), ceil(n_epoch / PER)), block 256; blockIdx.x fastest =
// row-major over the output.  nk even, out 16-byte aligned; winfo covers every k group
// of the (padded) grid, groups past nk are marked slow.  n_epoch is a multiple of PER
// (the host picks PER accordingly).
template <int PER, bool SSC = false>
__global__ __launch_bounds__(256) void k_power_stream(TabLayout L, const double* __restrict__ tab,
                                                      int w, int epoch0,
                                                      const double* __restrict__ ktab,
                                                      const int* __restrict__ winfo, size_t nk,
                                                      double* __restrict__ out,
                                                      const double* __restrict__ delta_b) {
  const int k_group = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const int info = winfo[k_group];
  const size_t ti = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const double4 kt = *reinterpret_cast<const double4*>(ktab + 4 * ti);  // (padded: in bounds)
  if (info & kWaveSlow) return;
  const int idxu = info & kWaveIdxMask;
  const bool two = (info & kWaveTwo) != 0;
  const RowCols o = row_cols(L, w, idxu);
  const int q_lo = blockIdx.y * PER;
  // wave-uniform operands of the PER rows: all fetched through the scalar cache before
  // the first use
  PowerRow r[PER];
  double db[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    r[j] = fetch_row(L, o, tab + (size_t)(epoch0 + q_lo + j) * L.stride);
    db[j] = SSC ? delta_b[epoch0 + q_lo + j] : 0.0;
  }
  const WaveKnots v{idxu, true, two, kt.y < 0.0, kt.w < 0.0, kt.x, kt.z};
  const double shape0 = fabs(kt.y), shape1 = fabs(kt.w);
  double* ot = out + (size_t)q_lo * nk + 2 * ti;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    double r0, r1;
    power_fast_pair<SSC>(r[j], tab + (size_t)(epoch0 + q_lo + j) * L.stride, o, v, shape0, shape1,
                         w, db[j], r0, r1);
    // write-through: the output is never re-read by this launch, and the k table must
    // stay in L2 next to it
    store_wt16(ot, r0, r1);
    ot += nk;
  }
}

// The per-lane pass of the streaming shape, over the k groups k_power_prep listed: 1-D grid;
// every wavefront walks work items (listed k group, chunk of epochs).  The chunk length adapts
// to the length of the list: few listed groups -> short chunks over many wavefronts (the
// per-epoch coefficient loads of this path are a dependent chain), a fully listed grid -> one
// item per group.
template <bool BAO, bool SSC = false>
__global__ __launch_bounds__(256) void k_power_grid_lanes(
    chomp_config cfg, TabLayout L, const Epoch* __restrict__ epochs,
    const double* __restrict__ tab, int w, bool extrap, int epoch0, int n_epoch,
    const double* __restrict__ k, size_t nk, double* __restrict__ out,
    const int* __restrict__ slow, int parity, const double* __restrict__ delta_b) {
  const int count = slow[parity];
  if (count == 0) return;
  const int NK = L.NK;
  const long n_waves = (long)gridDim.x * 4;
  int chunks = (int)(n_waves / count);
  chunks = chunks < 1 ? 1 : (chunks > n_epoch ? n_epoch : chunks);
  const int epochs_per_item = (n_epoch + chunks - 1) / chunks;
  chunks = (n_epoch + epochs_per_item - 1) / epochs_per_item;
  const long n_items = (long)count * chunks;
  const int lane = threadIdx.x & 63;
  for (long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6); item < n_items; item += n_waves) {
    const int k_group = slow[2 + (int)(item / chunks)], c = (int)(item % chunks);
    const int q_lo = c * epochs_per_item;
    int q_hi = q_lo + epochs_per_item;
    if (q_hi > n_epoch) q_hi = n_epoch;
    const KLanes s = load_k_lanes(cfg, NK, k, nk, (size_t)k_group * 64 + lane);
    power_lanes_range<BAO, SSC>(cfg, L, epochs, tab, w, extrap, epoch0, q_lo, q_hi, s, nk, out,
                                delta_b);
  }
}

// sigma_r at arbitrary scales (SingleEpoch.sigma_r): grid n, block 256.
template <bool BAO>
__global__ __launch_bounds__(256) void k_sigma_r(chomp_config cfg,
                                                 const Epoch* __restrict__ epochs, int e,
                                                 const double* __restrict__ scale,
                                                 const double* __restrict__ snodes,
                                                 double* __restrict__ out) {
  __shared__ Epoch E;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  __syncthreads();
  const double s2 = sigma2_block<4, 1, BAO>(E, snodes + (size_t)E.cosmo_slot * kSigmaStride, scale[blockIdx.x], cfg,
                                    cfg.cosmo_precision, red);
  if (threadIdx.x == 0) out[blockIdx.x] = sqrt(s2);
}

// Halo.y (NFW) at (ln k, M) pairs.
__global__ void k_y_nfw(const Epoch* __restrict__ epochs, int e,
                        const SiCiTab* __restrict__ sici_g, const double* __restrict__ ln_k,
                        const double* __restrict__ mass, int n, double* __restrict__ out) {
  __shared__ Epoch E;
  __shared__ SiCiTab S;
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&S), reinterpret_cast<const double*>(sici_g),
               (int)(sizeof(SiCiTab) / sizeof(double)));
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = y_nfw(E, S, ln_k[i], log(mass[i]));
}

// Element-wise accessors of one epoch's tables (the public lookup methods of
// MassFunction / HOD / Halo: mass_function.py:243-346, hod.py:189-230,
// halo.py:441-463).
__global__ void k_eval(TabLayout L, const Epoch* __restrict__ epochs, int e,
                       const double* __restrict__ tab, int what,
                       const double* __restrict__ x, int n, double* __restrict__ out) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  const int NM = L.NM;
  double* nu_knots = sm;
  double* lnm_pp = nu_knots + NM;
  double* nu_pp = lnm_pp + 4 * (NM - 1);
  const double* t = tab + (size_t)e * L.stride;
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(nu_knots, t + L.off_nu, NM);
  copy_doubles(lnm_pp, t + L.off_lnm_pp, 4 * (NM - 1));
  copy_doubles(nu_pp, t + L.off_nu_pp, 4 * (NM - 1));
  __syncthreads();
  const double dlnm = (E.ln_mass_max - E.ln_mass_min) / (double)(NM - 1);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double v = x[i];
    double r = 0.0;
    switch (what) {
      case CHOMP_EV_NU_OF_MASS: r = spline_eval_uniform(E.ln_mass_min, dlnm, nu_pp, NM, log(v)); break;
      case CHOMP_EV_LN_MASS_OF_NU: r = spline_eval(nu_knots, lnm_pp, NM, v); break;
      case CHOMP_EV_F_NU: r = f_nu(E, v); break;
      case CHOMP_EV_BIAS_NU: r = bias_nu(E, v); break;
      case CHOMP_EV_HOD_FIRST: r = hod_first(E, v); break;
      case CHOMP_EV_HOD_SECOND: r = hod_second(E, v); break;
      case CHOMP_EV_HOD_CENTRAL: r = hod_central(E, v); break;
      case CHOMP_EV_HOD_SATELLITE: r = hod_satellite(E, v); break;
      case CHOMP_EV_VIRIAL_RADIUS: r = exp((E.ln_rv_const + log(v)) * (1.0 / 3.0)); break;
      case CHOMP_EV_CONCENTRATION: r = exp(E.ln_c_const + E.beta * log(v)); break;
      case CHOMP_EV_DELTA_K:
        r = E.with_bao ? delta_k_ln_t<true>(E, log(v), v) : delta_k_ln_t<false>(E, log(v), v);
        break;
      default: r = 0.0;
    }
    out[i] = r;
  }
}

}  // namespace chomp
