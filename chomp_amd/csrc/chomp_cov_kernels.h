// chomp_cov_kernels.h -- the super-sample covariance of w(theta) (gfx950):
// Covariance(corr, corr, nongaussian_cov=False, ssc_cov=True), covariance.py:144-151, 685-776,
// on KernelCovariance.kernel_ssc, kernel.py:961-972, 1113-1231.
//
//   k_ssc_prep      sigma^2 spline over ln chi, z_bar_NG and its chi / growth
//   k_ssc_table     raw_kernel_ssc: the 50 x 50 knot table (upper triangle, mirrored, levels)
//                   or the caller's points
//   k_ssc_bicubic   RectBivariateSpline(s=0) of the table as a piecewise bicubic
//   k_ssc_eval      kernel_ssc with the reference's clamp and zero rules
//   k_ssc_kb        covariance_ssc, inner integrals: one k_b Romberg per (pair, k_a knot)
//   k_ssc_outer     covariance_ssc, the k_a spline and the outer Romberg per pair
//
// Everything runs in one context: the halo copy's.  The windows and the MultiEpoch are set up
// there (Kernel._setup_on, as Correlation._prepare does for its own halo), so the table, its
// bicubic and the response dlnP/ddelta_b meet without a hand-over.
#pragma once

#include <hip/hip_runtime.h>

#include "chomp_proj_kernels.h"

namespace chomp {

// Device block of the kernel_ssc state: scalars | ln k theta knots | sigma^2 knots and spline |
// table | levels | bicubic | scratch of the bicubic build.
struct SscLayout {
  int N, NS, scal, kx, sx, sy, spp, tab, lev, bic, rowt, work, total;
};
inline SscLayout make_ssc_layout(int N, int NS) {
  SscLayout S;
  S.N = N;
  S.NS = NS;
  int o = 0;
  S.scal = o; o += 8;
  S.kx = o; o += N;
  S.sx = o; o += NS;
  S.sy = o; o += NS;
  S.spp = o; o += 4 * (NS - 1);
  S.tab = o; o += N * N;
  S.lev = o; o += N * N;
  S.bic = o; o += 16 * (N - 1) * (N - 1);
  S.rowt = o; o += 4 * (N - 1) * N;
  S.work = o; o += 4 * (N - 1) * (6 * N);
  S.total = (o + 7) & ~7;
  return S;
}
// scalars
constexpr int kSscZBar = 0, kSscChiPeak = 1, kSscDz = 2, kSscLnMin = 3, kSscLnMax = 4,
              kSscLimit = 5;

// Dynamic LDS of the covariance_ssc launches, in doubles.
inline int ssc_kb_lds_doubles(int NK_halo, int N) { return 12 * (NK_halo - 1) + 5 * N - 4; }
inline int ssc_outer_lds_doubles(int N) { return N + N + 4 * (N - 1) + 2 * N; }

// kernel.py:1224-1231 (_sigma2): the spline of sigma^2 in ln chi inside [chi_min, chi_max], 0
// outside.
struct Sigma2View {
  const double *x, *pp;
  int NS;
  double chi_min, chi_max;
  __device__ __forceinline__ double operator()(double chi) const {
    return (chi >= chi_min && chi <= chi_max) ? spline_eval(x, pp, NS, log(chi)) : 0.0;
  }
};

// kernel.py:1048-1056 (_kernel_NG_integrand) with a1 = b1 = window a, a2 = b2 = window b, in
// the reference's order of operations.
__device__ __forceinline__ double ssc_ng_integrand(const ProjLds& P, const BesselTab* B,
                                                   double chi, double kta, double ktb) {
  const double D = P.me.growth_factor(P.me.redshift(chi));
  const double wa = P.wa(chi), wb = P.wb(chi);
  return wa * wb * wa * wb * D * D * D * D / (chi * chi) * bessel_j<0>(kta * chi, *B) *
         bessel_j<0>(ktb * chi, *B);
}

// kernel.py:1208-1215 (_kernel_ssc_integrand) as raw_kernel_ssc calls it: the Romberg variable
// is x = ln chi, and it is what the integrand receives as chi -- every factor is evaluated at x.
// Where sigma^2(x) or a window is 0 the value is 0 (numpy multiplies the zero into finite
// numbers there; a J0 or growth of a negative x is never formed).
struct SscKernelIntegrand {
  const ProjLds* P;
  const Sigma2View* S;
  const BesselTab* B;
  double kta, ktb, norm;
  __device__ __forceinline__ double operator()(double x) const {
    const double s2 = (*S)(x);
    if (s2 == 0.0) return 0.0;
    const double wa = P->wa(x), wb = P->wb(x);
    if (wa == 0.0 || wb == 0.0) return 0.0;
    const double D = P->me.growth_factor(P->me.redshift(x));
    return norm * wa * wb * wa * wb * D * D * D * D * D * D * s2 / x *
           bessel_j<0>(kta * x, *B) * bessel_j<0>(ktb * x, *B);
  }
};

// grid 1, block 256: the sigma^2 spline (kernel.py:1208-1222) from the host's knots (ln chi,
// MultiEpoch.sigma_r(chi, 0)^2 from the device's sigma(R)), the ln k theta knots and z_bar_NG
// (kernel.py:961-972: the first argmax over linspace(z_min, z_max, N) of W^4 D^4 / chi^2, chi
// floored at window_precision), its chi and MultiEpoch.growth_factor (covariance.py:143).
__global__ __launch_bounds__(256) void k_ssc_prep(chomp_config cfg, ProjLayout L, SscLayout S,
                                                  const ProjDev* __restrict__ pdg,
                                                  const double* __restrict__ ptab,
                                                  double ln_kt_min, double ln_kt_max,
                                                  double j0_limit, double* __restrict__ st) {
  __shared__ double cand[256];
  __shared__ double work[2 * 256];
  const ProjDev& pd = *pdg;
  const MEView me = me_view(L, pd, ptab, 0);
  const WindowView wa{ptab + L.w_pp[0], L.NWp, pd.w_chi_min[0], pd.w_chi_max[0]};
  const WindowView wb{ptab + L.w_pp[1], L.NWp, pd.w_chi_min[1], pd.w_chi_max[1]};
  const int t = threadIdx.x;
  for (int i = t; i < S.N; i += blockDim.x) st[S.kx + i] = linspace_at(ln_kt_min, ln_kt_max, S.N, i);
  if (t < S.N) {
    const double z = linspace_at(pd.z_min, pd.z_max, S.N, t);
    double chi = me.comoving_distance(z);
    if (!(chi > cfg.window_precision)) chi = cfg.window_precision;
    const double D = me.growth_factor(me.redshift(chi));
    const double a = wa(chi), b = wb(chi);
    cand[t] = a * b * a * b * D * D * D * D / (chi * chi);
  }
  __syncthreads();
  if (t != 0) return;
  spline_build(st + S.sx, st + S.sy, S.NS, st + S.spp, work);
  // numpy.argmax: the first of equal maxima, and the first NaN if there is one
  int best = 0;
  for (int i = 1; i < S.N && !isnan(cand[best]); ++i)
    if (isnan(cand[i]) || cand[i] > cand[best]) best = i;
  const double zb = linspace_at(pd.z_min, pd.z_max, S.N, best);
  st[S.scal + kSscZBar] = zb;
  st[S.scal + kSscChiPeak] = me.comoving_distance(zb);
  st[S.scal + kSscDz] = me.growth_factor(zb);
  st[S.scal + kSscLnMin] = ln_kt_min;
  st[S.scal + kSscLnMax] = ln_kt_max;
  st[S.scal + kSscLimit] = j0_limit;
}

// grid n integrals, block 256.  ln_a == nullptr: the knot table of _initialize_ssc_spline
// (kernel.py:1132-1153), block b -> the b-th (i, j), i <= j, of the upper triangle, written to
// [i][j] and [j][i] with its Romberg level; otherwise raw_kernel_ssc(ln_a[b], ln_b[b]) into out.
__global__ __launch_bounds__(256) void k_ssc_table(chomp_config cfg, ProjLayout L, SscLayout S,
                                                   const ProjDev* __restrict__ pdg,
                                                   const double* __restrict__ ptab,
                                                   const BesselTab* __restrict__ bess_g,
                                                   double* __restrict__ st,
                                                   const double* __restrict__ ln_a,
                                                   const double* __restrict__ ln_b,
                                                   double* __restrict__ out) {
  extern __shared__ __align__(16) double sm[];
  __shared__ ProjDev pd;
  __shared__ BesselTab B;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&pd), reinterpret_cast<const double*>(pdg), kProjDoubles);
  copy_doubles(reinterpret_cast<double*>(&B), reinterpret_cast<const double*>(bess_g),
               (int)(sizeof(BesselTab) / sizeof(double)));
  __syncthreads();
  ProjLds P;
  double* sx = P.stage(L, pd, ptab, sm);
  double* spp = sx + S.NS;
  copy_doubles(sx, st + S.sx, S.NS);
  copy_doubles(spp, st + S.spp, 4 * (S.NS - 1));
  P.bess = &B;
  __syncthreads();
  const Sigma2View sig{sx, spp, S.NS, pd.chi_min, pd.chi_max};
  int i = 0, j = 0;
  double la, lb;
  if (ln_a) {
    la = ln_a[blockIdx.x];
    lb = ln_b[blockIdx.x];
  } else {
    int b = (int)blockIdx.x;                       // row i holds N - i entries
    while (b >= S.N - i) { b -= S.N - i; ++i; }
    j = i + b;
    la = st[S.kx + i];
    lb = st[S.kx + j];
  }
  // kernel.py:1165-1206
  const double kta = exp(la), ktb = exp(lb);
  const double lim = st[S.scal + kSscLimit];
  double chi_max = fmax(lim / kta, lim / ktb);
  double v = 0.0;
  int level = 0;
  bool zero = false;
  if (chi_max >= pd.chi_max) chi_max = pd.chi_max;
  else if (chi_max <= pd.chi_min) zero = true;
  if (!zero) {
    // the norm passes ln(k theta_a) where k theta_a belongs (kernel.py:1178-1183)
    const double inv = ssc_ng_integrand(P, &B, st[S.scal + kSscChiPeak], la, la);
    const double norm = (inv > 1e-16 || inv < -1e-16) ? 1.0 / inv : 1.0;
    SscKernelIntegrand f{&P, &sig, &B, kta, ktb, norm};
    const double r = romberg1<4>(f, log(pd.chi_min), log(chi_max), cfg.global_precision,
                                 cfg.kernel_precision, cfg.divmax, red, &level);
    v = r * (16.0 * kPi * kPi / 9.0) / norm;
  }
  if (threadIdx.x == 0) {
    if (ln_a) {
      out[blockIdx.x] = v;
    } else {
      st[S.tab + i * S.N + j] = v;
      st[S.tab + j * S.N + i] = v;
      st[S.lev + i * S.N + j] = (double)level;
      st[S.lev + j * S.N + i] = (double)level;
    }
  }
}

// The tensor-product not-a-knot bicubic of an N x N table over the knots x in both directions
// -- what FITPACK's regrid with s = 0 and kx = ky = 3 interpolates with (knots at x_0 x4, x_2 ..
// x_{N-3}, x_{N-1} x4 in both directions).  The 1D solver of chomp_math.h runs along b for every
// row, then along a for every (interval, power) of the row pieces:
//   S(a, b) = sum_{p,q} bic[((ia (N-1) + jb) 4 + p) 4 + q] (a - x_ia)^p (b - x_jb)^q.
// One block (blockDim.x >= N; all threads call).  rowt: 4 (N-1) N doubles, work: 4 (N-1) 6 N
// doubles (6 N per thread), bic: 16 (N-1)^2 doubles, all in global memory.  Shared by
// KernelCovariance.kernel_ssc (k_ssc_bicubic) and HaloTrispectrumOneHalo (k_tri1h_bicubic).
__device__ __forceinline__ void bicubic_build(int N, const double* x, const double* tab,
                                              double* rowt, double* work, double* bic) {
  const int M = N - 1;
  double* wk = work + (size_t)threadIdx.x * 6 * N;   // (4 M + 2 N doubles per thread)
  if ((int)threadIdx.x < N) {
    const int i = threadIdx.x;
    double* c = wk;
    spline_build(x, tab + (size_t)i * N, N, c, c + 4 * M);
    for (int q = 0; q < 4 * M; ++q) rowt[(size_t)q * N + i] = c[q];
  }
  __threadfence_block();
  __syncthreads();
  for (int q = threadIdx.x; q < 4 * M; q += blockDim.x) {
    double* wq = work + (size_t)q * 6 * N;
    double* c = wq;
    spline_build(x, rowt + (size_t)q * N, N, c, c + 4 * M);
    const int jb = q >> 2, mb = q & 3;
    for (int ia = 0; ia < M; ++ia)
      for (int ma = 0; ma < 4; ++ma)
        bic[(((size_t)ia * M + jb) * 4 + ma) * 4 + mb] = c[4 * ia + ma];
  }
}

// grid 1, block 256: the bicubic of the kernel_ssc table.
__global__ __launch_bounds__(256) void k_ssc_bicubic(SscLayout S, double* __restrict__ st) {
  bicubic_build(S.N, st + S.kx, st + S.tab, st + S.rowt, st + S.work, st + S.bic);
}

// A bicubic of bicubic_build: knots x[0..N-1] (uniform in intent, lo = x_0, hi = x_{N-1}), the
// interval search and the tensor-product polynomial, with no range rule of its own.
struct Bicubic {
  const double *x, *bic;
  int N;
  double lo, hi;
  __device__ __forceinline__ int interval(double v) const {
    const double inv_dx = (double)(N - 1) / (hi - lo);
    int i = (int)floor((v - lo) * inv_dx);
    i = i < 0 ? 0 : (i > N - 2 ? N - 2 : i);
    if (i > 0 && v < x[i]) --i;
    if (i < N - 2 && v >= x[i + 1]) ++i;
    return i;
  }
  __device__ __forceinline__ double poly(double a, double b) const {
    const int ia = interval(a), jb = interval(b);
    const double da = a - x[ia], db = b - x[jb];
    const double* c = bic + ((size_t)ia * (N - 1) + jb) * 16;
    double r[4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
      r[p] = fma(fma(fma(c[4 * p + 3], db, c[4 * p + 2]), db, c[4 * p + 1]), db, c[4 * p]);
    return fma(fma(fma(r[3], da, r[2]), da, r[1]), da, r[0]);
  }
};

// KernelCovariance.kernel_ssc at one point (kernel.py:1113-1130): ln k theta <= min is clamped
// to min; either above max gives 0.
struct SscSpline : Bicubic {
  __device__ __forceinline__ double operator()(double a, double b) const {
    if (a <= lo) a = lo;
    if (b <= lo) b = lo;
    if (!(a <= hi && b <= hi)) return 0.0;
    return poly(a, b);
  }
};
__device__ __forceinline__ SscSpline ssc_spline(const SscLayout& S, const double* st) {
  SscSpline K;
  K.x = st + S.kx;
  K.bic = st + S.bic;
  K.N = S.N;
  K.lo = st[S.scal + kSscLnMin];
  K.hi = st[S.scal + kSscLnMax];
  return K;
}

__global__ void k_ssc_eval(SscLayout S, const double* __restrict__ st,
                           const double* __restrict__ a, const double* __restrict__ b, int n,
                           double* __restrict__ out) {
  const SscSpline K = ssc_spline(S, st);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = K(a[i], b[i]);
}

// kernel_ssc(a, .) at one fixed first argument a, as a cubic spline in b staged in LDS: the
// bicubic's pieces of a's interval, summed over the powers of (a - x_ia).  The same clamp and zero
// rules as SscSpline; agrees with it to rounding (the two sums run in the other order).
// lds: 5 N - 4 doubles (knots, then 4 (N - 1) coefficients).  All threads call build(); a
// barrier must follow before use.
struct SscRow {
  const double *x, *c;
  int N;
  double lo, hi;
  bool zero;                       // a above the range (or NaN): every value is 0
  __device__ __forceinline__ void build(const SscSpline& K, double a, double* lds) {
    double* lx = lds;
    double* lc = lds + K.N;
    x = lx; c = lc; N = K.N; lo = K.lo; hi = K.hi;
    if (a <= lo) a = lo;
    zero = !(a <= hi);
    for (int i = threadIdx.x; i < N; i += blockDim.x) lx[i] = K.x[i];
    if (zero) return;
    const int ia = K.interval(a);
    const double da = a - K.x[ia];
    for (int q = threadIdx.x; q < 4 * (N - 1); q += blockDim.x) {
      const int jb = q >> 2, m = q & 3;
      const double* cc = K.bic + ((size_t)ia * (N - 1) + jb) * 16 + m;
      lc[q] = fma(fma(fma(cc[12], da, cc[8]), da, cc[4]), da, cc[0]);
    }
  }
  __device__ __forceinline__ double operator()(double b) const {
    if (zero) return 0.0;
    if (b <= lo) b = lo;
    if (!(b <= hi)) return 0.0;
    const double inv_dx = (double)(N - 1) / (hi - lo);
    int j = (int)floor((b - lo) * inv_dx);
    j = j < 0 ? 0 : (j > N - 2 ? N - 2 : j);
    if (j > 0 && b < x[j]) --j;
    if (j < N - 2 && b >= x[j + 1]) ++j;
    return pp_poly(c, j, b - x[j]);
  }
};

// covariance.py:765-776 (_kb_ssc_integrand): k_b^2 R(k_a) R(k_b) kernel_ssc(ln k_a theta_a,
// ln k_b theta_b), norm = 1, with R = dln_power_ddelta_b of the context's epoch -- the Stage E
// function itself (PowerEval, CHOMP_P_SSC_RESPONSE), exactly 0 outside [k_min, k_max].
template <bool BAO>
struct SscKbIntegrand {
  const PowerEval* P;
  const SscRow* K;
  double ra, theta_b;
  __device__ __forceinline__ double operator()(double ln_kb) const {
    const double kb = exp(ln_kb);
    const double rb = P->template eval_t<BAO>(kb);
    return kb * kb * 1.0 * ra * rb * (*K)(log(kb * theta_b));
  }
};

// grid (kernel_npoints, n pairs), block 256: the k_b integral at k_a knot x of pair y
// (covariance.py:723-763).  LDS: ssc_kb_lds_doubles.
template <bool BAO>
__global__ __launch_bounds__(256) void k_ssc_kb(chomp_config cfg, TabLayout HL, SscLayout S,
                                                const Epoch* __restrict__ epochs, int e,
                                                const double* __restrict__ htab,
                                                const double* __restrict__ st,
                                                const double* __restrict__ theta_a,
                                                const double* __restrict__ theta_b,
                                                double* __restrict__ knots,
                                                double* __restrict__ levels) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  __syncthreads();
  PowerEval P;
  P.stage(cfg, HL, &E, htab + (size_t)e * HL.stride, CHOMP_P_SSC_RESPONSE, sm);
  const int i = blockIdx.x, pair = blockIdx.y, NK = cfg.kernel_npoints;
  const double ln_k_min = log(cfg.k_min), ln_k_max = log(cfg.k_max);
  const double ka = exp(linspace_at(ln_k_min, ln_k_max, NK, i));
  SscRow K;
  K.build(ssc_spline(S, st), log(ka * theta_a[pair]), sm + 12 * (HL.NK - 1));
  __syncthreads();
  P.template finish_t<BAO>();
  SscKbIntegrand<BAO> f{&P, &K, P.template eval_t<BAO>(ka), theta_b[pair]};
  int level = 0;
  const double v = romberg1<4>(f, ln_k_min, ln_k_max, cfg.global_precision, cfg.corr_precision,
                               cfg.divmax, red, &level);
  if (threadIdx.x == 0) {
    knots[(size_t)pair * NK + i] = v;
    if (levels) levels[(size_t)pair * NK + i] = (double)level;
  }
}

// covariance.py:694-721: the not-a-knot spline of the k_a knots, norm = 1 / spline(0), the
// Romberg over ln k_a of k_a^2 spline norm, / (4 pi^2 norm area).
struct SscKaIntegrand {
  const double *x, *pp;
  int N;
  double norm;
  __device__ __forceinline__ double operator()(double ln_ka) const {
    const double ka = exp(ln_ka);
    return ka * ka * spline_eval(x, pp, N, ln_ka) * norm;
  }
};

// grid n pairs, block 256.  LDS: ssc_outer_lds_doubles(kernel_npoints) -- the knots x and y
// (N each), the spline pieces (4 (N - 1)) and spline_build's work (2 N).
__global__ __launch_bounds__(256) void k_ssc_outer(chomp_config cfg, double area,
                                                   const double* __restrict__ knots,
                                                   double* __restrict__ out) {
  extern __shared__ __align__(16) double sm[];
  __shared__ double red[romberg_scratch<4, 2>()];
  const int N = cfg.kernel_npoints, pair = blockIdx.x;
  double* x = sm;
  double* y = x + N;
  double* pp = y + N;
  double* work = pp + 4 * (N - 1);
  const double ln_k_min = log(cfg.k_min), ln_k_max = log(cfg.k_max);
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    x[i] = linspace_at(ln_k_min, ln_k_max, N, i);
    y[i] = knots[(size_t)pair * N + i];
  }
  __syncthreads();
  if (threadIdx.x == 0) spline_build(x, y, N, pp, work);
  __syncthreads();
  SscKaIntegrand f{x, pp, N, 1.0};
  const double norm = 1.0 / f(0.0);
  double v;
  if (!isfinite(norm)) {
    // every knot 0 (or spline(0) = 0): the reference's integrand is 0 * inf or inf everywhere,
    // its Romberg runs to divmax and the result is NaN
    v = NAN;
  } else {
    f.norm = norm;
    v = romberg1<4>(f, ln_k_min, ln_k_max, cfg.global_precision, cfg.corr_precision,
                    cfg.divmax, red) / (4.0 * kPi * kPi * norm * area);
  }
  if (threadIdx.x == 0) out[pair] = v;
}

}  // namespace chomp
