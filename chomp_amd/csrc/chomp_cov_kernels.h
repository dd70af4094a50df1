// chomp_cov_kernels.h -- the super-sample and one-halo trispectrum terms of the covariance of
// w(theta) (gfx950): Covariance(corr, corr, ssc_cov=True), covariance.py:144-151, 685-776, on
// KernelCovariance.kernel_ssc, kernel.py:961-972, 1113-1231; and Covariance(corr, corr,
// nongaussian_cov=True, input_halo_trispectrum=HaloTrispectrumOneHalo), covariance.py:593-683, on
// KernelCovariance.kernel_NG, kernel.py:996-1073, 1103-1111.
//
//   k_ssc_prep      sigma^2 spline over ln chi, z_bar_NG and its chi / growth
//   k_ssc_table     raw_kernel_ssc: the 50 x 50 knot table (upper triangle, mirrored, levels)
//                   or the caller's points
//   k_ssc_bicubic   RectBivariateSpline(s=0) of the table as a piecewise bicubic
//   k_ssc_eval      kernel_ssc with the reference's clamp and zero rules
//   k_ssc_kb        covariance_ssc, inner integrals: one k_b Romberg per (pair, k_a knot)
//   k_ssc_kb_cross  ... of a cross block: halo_a's response at k_a, halo_b's at k_b
//   k_ssc_outer     covariance_ssc / covariance_NG, the k_a spline and the outer Romberg per pair
//
//   k_ng_prep       the kernel_NG state from the kernel_ssc one (z_bar_NG, its chi and growth, the
//                   ln k theta knots)
//   k_ng_table      raw_kernel_NG: the knot table (upper triangle, mirrored, levels) or the
//                   caller's points
//   k_ng_bicubic    min(table) and the bicubic of log(table - 10 min)
//   k_ng_eval       kernel_NG with the reference's clamp and zero rules
//   k_ng_tri        the bicubic of an uploaded I_0^4 table (HaloTrispectrumOneHalo's)
//   k_ng_kb         covariance_NG, inner integrals: one k_b Romberg per (pair, k_a knot)
//
//   k_ssc_blocks_*  the super-sample term with the block of a CovarianceMulti as a grid dimension
//   k_ng_blocks_*   ... and the trispectrum term: prep (the scalars alone, cov_scalars_body),
//                   table, bicubic and kb; the outer integrals are k_ssc_blocks_outer's
//
// ... and the Gaussian covariance of C_l, CovarianceFourier, covariance.py:874-1083 (at the end):
//
//   k_covf_zbar     z_bar and the range of the four window pairs a1a2, b1b2, a1b2, b1a2
//   k_covf_knots    the four Limber tables over ln l: one Romberg over chi per (knot, pair)
//   k_covf_spline   the not-a-knot splines of their logarithms
//   k_covf_eval     _pl_X and covariance_G at the caller's multipoles
//
// k_ssc_prep, k_ssc_table and k_ng_table are templates over where the four windows come from
// (CovSrc / CovWindows): a matching block's two windows, each used twice, or the four windows in
// the two slots of a cross block (Covariance(corr_a, corr_b, cross_terms=True), kernel.py:893-972
// with a1 != b1 or a2 != b2; k_cov_cross_range gives that block's common range).  Everything
// behind the tables is shared.
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
  S.scal = o; o += 16;
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
// ... and the common range of the four windows (kernel.py:910-931), which the table kernels read
constexpr int kSscZMin = 8, kSscZMax = 9, kSscChiMin = 10, kSscChiMax = 11;

// Dynamic LDS of the covariance_ssc launches, in doubles.
inline int ssc_kb_lds_doubles(int NK_halo, int N) { return 12 * (NK_halo - 1) + 5 * N - 4; }
// ... with the two responses of a cross block
inline int ssc_kb_cross_lds_doubles(int NK_halo, int N) { return 24 * (NK_halo - 1) + 5 * N - 4; }
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

// Where the four windows a1, a2, b1, b2 of a KernelCovariance come from.  A matching block
// (Covariance(corr, corr)) has a1 = b1, a2 = b2: the two windows of one projection set-up (pd,
// ptab), each used twice.  A cross block (FOUR) takes a1, a2 and the MultiEpoch from slot 0 of the
// block's CrossLayout (pd, ptab) and b1, b2 from slot 1 (pd_b, ptab_b): kernel.py:918-931, the
// MultiEpoch is correlation a's throughout.
struct CovSrc {
  const ProjDev* pd;
  const double* ptab;
  const ProjDev* pd_b;
  const double* ptab_b;
};
template <bool FOUR>
struct CovWindows {
  ProjLds P;                       // MultiEpoch, a1, a2
  WindowView b1, b2;               // (FOUR only)
  // Carve `sm` and copy the tables in (all threads; barrier afterwards); pd, pd_b: copies of the
  // sources' scalars the caller holds in LDS.
  __device__ __forceinline__ double* stage(const ProjLayout& L, const CovSrc& src,
                                           const ProjDev& pd, const ProjDev& pd_b, double* sm) {
    double* end = P.stage(L, pd, src.ptab, sm);
    if constexpr (FOUR) {
      const int n = 4 * (L.NWp - 1);
      copy_doubles(end, src.ptab_b + L.w_pp[0], n);
      copy_doubles(end + n, src.ptab_b + L.w_pp[1], n);
      b1 = WindowView{end, L.NWp, pd_b.w_chi_min[0], pd_b.w_chi_max[0]};
      b2 = WindowView{end + n, L.NWp, pd_b.w_chi_min[1], pd_b.w_chi_max[1]};
      end += 2 * n;
    }
    return end;
  }
  // the four window values at chi, in the reference's order a1, a2, b1, b2
  __device__ __forceinline__ void at(double chi, double& a1, double& a2, double& b1v,
                                     double& b2v) const {
    a1 = P.wa(chi);
    a2 = P.wb(chi);
    if constexpr (FOUR) {
      b1v = b1(chi);
      b2v = b2(chi);
    } else {
      b1v = a1;
      b2v = a2;
    }
  }
  static __host__ __device__ int doubles(const ProjLayout& L) {
    return ProjLds::doubles(L) + (FOUR ? 8 * (L.NWp - 1) : 0);
  }
};
// Dynamic LDS of k_ssc_table / k_ng_table, in doubles.
inline int ssc_table_lds_doubles(const ProjLayout& L, int NS, bool four) {
  return (four ? CovWindows<true>::doubles(L) : CovWindows<false>::doubles(L)) + 5 * NS - 4;
}
inline int ng_table_lds_doubles(const ProjLayout& L, bool four) {
  return four ? CovWindows<true>::doubles(L) : CovWindows<false>::doubles(L);
}

// The host's plan of the super-sample launches -- what kernel_ssc_setup, chomp_kernel_ssc_raw,
// chomp_covariance_ssc, _ssc_cross and _ssc_blocks size and launch by.  Indexed by `four`: the two
// windows of a matching block, or the four of a cross block (and with them its two responses).
struct SscPlan {
  SscLayout S;
  int NK;                           // the k_b knots of a pair of angles (kernel_npoints)
  size_t sh_table[2];               // dynamic LDS of k_ssc_table / k_ssc_blocks_table
  size_t sh_kb[2];                  // ... of k_ssc_kb, of k_ssc_kb_cross / k_ssc_blocks_kb
  size_t sh_outer;                  // ... of k_ssc_outer / k_ssc_blocks_outer
  unsigned n_tab;                   // blocks of a table launch: the upper triangle of N x N
};
// (NK_halo: the knots of P(k); NS: the sigma^2 knots)
inline SscPlan ssc_plan(const chomp_config& cfg, int NK_halo, const ProjLayout& L, int NS) {
  SscPlan P;
  P.S = make_ssc_layout(L.NKT, NS);
  P.NK = cfg.kernel_npoints;
  for (int four = 0; four < 2; ++four)
    P.sh_table[four] = (size_t)ssc_table_lds_doubles(L, NS, four != 0) * sizeof(double);
  P.sh_kb[0] = (size_t)ssc_kb_lds_doubles(NK_halo, P.S.N) * sizeof(double);
  P.sh_kb[1] = (size_t)ssc_kb_cross_lds_doubles(NK_halo, P.S.N) * sizeof(double);
  P.sh_outer = (size_t)ssc_outer_lds_doubles(P.NK) * sizeof(double);
  P.n_tab = (unsigned)(P.S.N * (P.S.N + 1) / 2);
  return P;
}

// kernel.py:1103-1111 (_kernel_NG_integrand): a1 a2 b1 b2 D^4 / chi^2 J0 J0 in the reference's
// order of operations (norm = 1 multiplies exactly); with a1 = b1, a2 = b2 of a matching block
// that is wa wb wa wb.
template <bool FOUR>
__device__ __forceinline__ double ssc_ng_integrand(const CovWindows<FOUR>& W, const BesselTab* B,
                                                   double chi, double kta, double ktb,
                                                   double norm = 1.0) {
  const double D = W.P.me.growth_factor(W.P.me.redshift(chi));
  double a1, a2, b1, b2;
  W.at(chi, a1, a2, b1, b2);
  return norm * a1 * a2 * b1 * b2 * D * D * D * D / (chi * chi) * bessel_j<0>(kta * chi, *B) *
         bessel_j<0>(ktb * chi, *B);
}

// kernel.py:1197-1206 (_kernel_ssc_integrand) as raw_kernel_ssc calls it: the Romberg variable
// is x = ln chi, and it is what the integrand receives as chi -- every factor is evaluated at x.
// Where sigma^2(x) or a window is 0 the value is 0 (numpy multiplies the zero into finite
// numbers there; a J0 or growth of a negative x is never formed).
template <bool FOUR>
struct SscKernelIntegrand {
  const CovWindows<FOUR>* W;
  const Sigma2View* S;
  const BesselTab* B;
  double kta, ktb, norm;
  __device__ __forceinline__ double operator()(double x) const {
    const double s2 = (*S)(x);
    if (s2 == 0.0) return 0.0;
    double a1, a2, b1, b2;
    W->at(x, a1, a2, b1, b2);
    if (a1 == 0.0 || a2 == 0.0) return 0.0;
    if constexpr (FOUR)
      if (b1 == 0.0 || b2 == 0.0) return 0.0;
    const double D = W->P.me.growth_factor(W->P.me.redshift(x));
    return norm * a1 * a2 * b1 * b2 * D * D * D * D * D * D * s2 / x *
           bessel_j<0>(kta * x, *B) * bessel_j<0>(ktb * x, *B);
  }
};

// grid 1, block 256: the sigma^2 spline (kernel.py:1208-1222) from the host's knots (ln chi,
// MultiEpoch.sigma_r(chi, 0)^2 from the device's sigma(R)), the ln k theta knots and z_bar_NG
// (kernel.py:961-972: the first argmax over linspace(z_min, z_max, N) of W^4 D^4 / chi^2, chi
// floored at window_precision), its chi and MultiEpoch.growth_factor (covariance.py:143).
// FOUR: the four windows of a cross block and their common range -- z_min = max, z_max = min of the
// two sides', chi_min = max(window_precision, chi(z_min)), chi_max = chi(z_max) on slot 0's
// MultiEpoch (kernel.py:910-931).  The range goes into the scalars in both cases.
//
// cov_scalars_body is the part that reads no sigma^2 knot: the N ln k theta knots into kx and the
// scalars (kSsc*: z_bar_NG, its chi and growth, the ln k theta range, `limit`, the common range)
// into scal.  The trispectrum term's block axis runs it alone (k_ng_blocks_prep).  All threads
// call; thread 0 writes the scalars behind the body's one barrier.
template <bool FOUR>
__device__ __forceinline__ void cov_scalars_body(const chomp_config& cfg, const ProjLayout& L,
                                                 int N, const CovSrc& src, double ln_kt_min,
                                                 double ln_kt_max, double limit,
                                                 double* __restrict__ scal,
                                                 double* __restrict__ kx) {
  __shared__ double cand[256];
  const ProjDev& pd = *src.pd;
  const double* ptab = src.ptab;
  const MEView me = me_view(L, pd, ptab, 0);
  const WindowView wa{ptab + L.w_pp[0], L.NWp, pd.w_chi_min[0], pd.w_chi_max[0]};
  const WindowView wb{ptab + L.w_pp[1], L.NWp, pd.w_chi_min[1], pd.w_chi_max[1]};
  WindowView wc = wa, wd = wb;
  double z_min = pd.z_min, z_max = pd.z_max, chi_min = pd.chi_min, chi_max = pd.chi_max;
  if constexpr (FOUR) {
    const ProjDev& pb = *src.pd_b;
    wc = WindowView{src.ptab_b + L.w_pp[0], L.NWp, pb.w_chi_min[0], pb.w_chi_max[0]};
    wd = WindowView{src.ptab_b + L.w_pp[1], L.NWp, pb.w_chi_min[1], pb.w_chi_max[1]};
    z_min = pb.z_min > z_min ? pb.z_min : z_min;
    z_max = pb.z_max < z_max ? pb.z_max : z_max;
    const double c0 = me.comoving_distance(z_min);
    chi_min = cfg.window_precision > c0 ? cfg.window_precision : c0;
    chi_max = me.comoving_distance(z_max);
  }
  const int t = threadIdx.x;
  for (int i = t; i < N; i += blockDim.x) kx[i] = linspace_at(ln_kt_min, ln_kt_max, N, i);
  if (t < N) {
    const double z = linspace_at(z_min, z_max, N, t);
    double chi = me.comoving_distance(z);
    if (!(chi > cfg.window_precision)) chi = cfg.window_precision;
    const double D = me.growth_factor(me.redshift(chi));
    const double a = wa(chi), b = wb(chi);
    const double c = FOUR ? wc(chi) : a, d = FOUR ? wd(chi) : b;
    cand[t] = a * b * c * d * D * D * D * D / (chi * chi);
  }
  __syncthreads();
  if (t != 0) return;
  // numpy.argmax: the first of equal maxima, and the first NaN if there is one
  int best = 0;
  for (int i = 1; i < N && !isnan(cand[best]); ++i)
    if (isnan(cand[i]) || cand[i] > cand[best]) best = i;
  const double zb = linspace_at(z_min, z_max, N, best);
  scal[kSscZBar] = zb;
  scal[kSscChiPeak] = me.comoving_distance(zb);
  scal[kSscDz] = me.growth_factor(zb);
  scal[kSscLnMin] = ln_kt_min;
  scal[kSscLnMax] = ln_kt_max;
  scal[kSscLimit] = limit;
  scal[kSscZMin] = z_min;
  scal[kSscZMax] = z_max;
  scal[kSscChiMin] = chi_min;
  scal[kSscChiMax] = chi_max;
}
// (the body of k_ssc_prep and of k_ssc_blocks_prep: the scalars, and one thread builds the
//  sigma^2 spline from the knots already in the slab -- the scalars' barrier stands behind the
//  stores of k_ssc_blocks_prep)
template <bool FOUR>
__device__ __forceinline__ void ssc_prep_body(const chomp_config& cfg, const ProjLayout& L,
                                              const SscLayout& S, const CovSrc& src,
                                              double ln_kt_min, double ln_kt_max, double j0_limit,
                                              double* __restrict__ st) {
  __shared__ double work[2 * 256];
  cov_scalars_body<FOUR>(cfg, L, S.N, src, ln_kt_min, ln_kt_max, j0_limit, st + S.scal,
                         st + S.kx);
  if (threadIdx.x == 0) spline_build(st + S.sx, st + S.sy, S.NS, st + S.spp, work);
}
template <bool FOUR>
__global__ __launch_bounds__(256) void k_ssc_prep(chomp_config cfg, ProjLayout L, SscLayout S,
                                                  CovSrc src, double ln_kt_min, double ln_kt_max,
                                                  double j0_limit, double* __restrict__ st) {
  ssc_prep_body<FOUR>(cfg, L, S, src, ln_kt_min, ln_kt_max, j0_limit, st);
}

// grid 1, block 64: out[4] = z_min, z_max, chi_min, chi_max of a cross block's four windows, as
// k_ssc_prep<true> finds them -- what the host lays the sigma^2 knots over before that launch.
// (the body of k_cov_cross_range and of a cross block of k_ssc_blocks_range; one thread calls)
__device__ __forceinline__ void cov_cross_range_body(const chomp_config& cfg, const ProjLayout& L,
                                                     const CovSrc& src, double* __restrict__ out) {
  const ProjDev& pd = *src.pd;
  const ProjDev& pb = *src.pd_b;
  const MEView me = me_view(L, pd, src.ptab, 0);
  const double z_min = pb.z_min > pd.z_min ? pb.z_min : pd.z_min;
  const double z_max = pb.z_max < pd.z_max ? pb.z_max : pd.z_max;
  const double c0 = me.comoving_distance(z_min);
  out[0] = z_min;
  out[1] = z_max;
  out[2] = cfg.window_precision > c0 ? cfg.window_precision : c0;
  out[3] = me.comoving_distance(z_max);
}
__global__ void k_cov_cross_range(chomp_config cfg, ProjLayout L, CovSrc src,
                                  double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  cov_cross_range_body(cfg, L, src, out);
}

// grid n integrals, block 256.  ln_a == nullptr: the knot table of _initialize_ssc_spline
// (kernel.py:1132-1153), block b -> the b-th (i, j), i <= j, of the upper triangle, written to
// [i][j] and [j][i] with its Romberg level; otherwise raw_kernel_ssc(ln_a[b], ln_b[b]) into out.
// (the body of k_ssc_table and of k_ssc_blocks_table; workgroup blockIdx.x)
template <bool FOUR>
__device__ __forceinline__ void ssc_table_body(const chomp_config& cfg, const ProjLayout& L,
                                               const SscLayout& S, const CovSrc& src,
                                               const BesselTab* __restrict__ bess_g,
                                               double* __restrict__ st,
                                               const double* __restrict__ ln_a,
                                               const double* __restrict__ ln_b,
                                               double* __restrict__ out) {
  extern __shared__ __align__(16) double sm[];
  __shared__ ProjDev pd, pd_b;      // (pd_b: FOUR only)
  __shared__ BesselTab B;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&pd), reinterpret_cast<const double*>(src.pd), kProjDoubles);
  if constexpr (FOUR)
    copy_doubles(reinterpret_cast<double*>(&pd_b), reinterpret_cast<const double*>(src.pd_b),
                 kProjDoubles);
  copy_doubles(reinterpret_cast<double*>(&B), reinterpret_cast<const double*>(bess_g),
               (int)(sizeof(BesselTab) / sizeof(double)));
  __syncthreads();
  CovWindows<FOUR> P;
  double* sx = P.stage(L, src, pd, pd_b, sm);
  double* spp = sx + S.NS;
  copy_doubles(sx, st + S.sx, S.NS);
  copy_doubles(spp, st + S.spp, 4 * (S.NS - 1));
  P.P.bess = &B;
  __syncthreads();
  // the common range of the windows (k_ssc_prep; pd's own for a matching block)
  const double chi_lo = st[S.scal + kSscChiMin], chi_hi = st[S.scal + kSscChiMax];
  const Sigma2View sig{sx, spp, S.NS, chi_lo, chi_hi};
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
  if (chi_max >= chi_hi) chi_max = chi_hi;
  else if (chi_max <= chi_lo) zero = true;
  if (!zero) {
    // the norm passes ln(k theta_a) where k theta_a belongs (kernel.py:1178-1183)
    const double inv = ssc_ng_integrand(P, &B, st[S.scal + kSscChiPeak], la, la);
    const double norm = (inv > 1e-16 || inv < -1e-16) ? 1.0 / inv : 1.0;
    SscKernelIntegrand<FOUR> f{&P, &sig, &B, kta, ktb, norm};
    const double r = romberg1<4>(f, log(chi_lo), log(chi_max), cfg.global_precision,
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
template <bool FOUR>
__global__ __launch_bounds__(256) void k_ssc_table(chomp_config cfg, ProjLayout L, SscLayout S,
                                                   CovSrc src,
                                                   const BesselTab* __restrict__ bess_g,
                                                   double* __restrict__ st,
                                                   const double* __restrict__ ln_a,
                                                   const double* __restrict__ ln_b,
                                                   double* __restrict__ out) {
  ssc_table_body<FOUR>(cfg, L, S, src, bess_g, st, ln_a, ln_b, out);
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
// (the body of k_ssc_bicubic and of k_ssc_blocks_bicubic)
__device__ __forceinline__ void ssc_bicubic_body(const SscLayout& S, double* __restrict__ st) {
  bicubic_build(S.N, st + S.kx, st + S.tab, st + S.rowt, st + S.work, st + S.bic);
}
__global__ __launch_bounds__(256) void k_ssc_bicubic(SscLayout S, double* __restrict__ st) {
  ssc_bicubic_body(S, st);
}

// One cell of a bicubic of bicubic_build: sum_{p,q} c[4 p + q] da^p db^q, db innermost.
__device__ __forceinline__ double bicubic_cell(const double* c, double da, double db) {
  double r[4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
    r[p] = fma(fma(fma(c[4 * p + 3], db, c[4 * p + 2]), db, c[4 * p + 1]), db, c[4 * p]);
  return fma(fma(fma(r[3], da, r[2]), da, r[1]), da, r[0]);
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
    return bicubic_cell(bic + ((size_t)ia * (N - 1) + jb) * 16, da, db);
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
  // the clamp and zero rules on b: false where the value is 0
  __device__ __forceinline__ bool inside(double& b) const {
    if (zero) return false;
    if (b <= lo) b = lo;
    return b <= hi;
  }
  // the row's cubic at b in [lo, hi]
  __device__ __forceinline__ double at(double b) const {
    const double inv_dx = (double)(N - 1) / (hi - lo);
    int j = (int)floor((b - lo) * inv_dx);
    j = j < 0 ? 0 : (j > N - 2 ? N - 2 : j);
    if (j > 0 && b < x[j]) --j;
    if (j < N - 2 && b >= x[j + 1]) ++j;
    return pp_poly(c, j, b - x[j]);
  }
  __device__ __forceinline__ double operator()(double b) const {
    return inside(b) ? at(b) : 0.0;
  }
};

// covariance.py:765-776 (_kb_ssc_integrand): k_b^2 R(k_a) R(k_b) kernel_ssc(ln k_a theta_a,
// ln k_b theta_b), norm = 1, with R = dln_power_ddelta_b of the context's epoch -- the Stage E
// function itself (PowerEval, CHOMP_P_SSC_RESPONSE), exactly 0 outside [k_min, k_max].
// In a cross block R(k_a) is halo_a's (in ra) and P is halo_b's response (:771-772).
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
// (the body of k_ssc_kb and of a diagonal block of k_ssc_blocks_kb; epoch: the epoch record,
//  htab: its knot-table slab)
template <bool BAO>
__device__ __forceinline__ void ssc_kb_body(const chomp_config& cfg, const TabLayout& HL,
                                            const SscLayout& S, const Epoch* __restrict__ epoch,
                                            const double* __restrict__ htab,
                                            const double* __restrict__ st,
                                            const double* __restrict__ theta_a,
                                            const double* __restrict__ theta_b,
                                            double* __restrict__ knots,
                                            double* __restrict__ levels) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(epoch),
               kEpochDoubles);
  __syncthreads();
  PowerEval P;
  P.stage(cfg, HL, &E, htab, CHOMP_P_SSC_RESPONSE, sm);
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
template <bool BAO>
__global__ __launch_bounds__(256) void k_ssc_kb(chomp_config cfg, TabLayout HL, SscLayout S,
                                                const Epoch* __restrict__ epochs, int e,
                                                const double* __restrict__ htab,
                                                const double* __restrict__ st,
                                                const double* __restrict__ theta_a,
                                                const double* __restrict__ theta_b,
                                                double* __restrict__ knots,
                                                double* __restrict__ levels) {
  ssc_kb_body<BAO>(cfg, HL, S, epochs + e, htab + (size_t)e * HL.stride, st, theta_a, theta_b,
                   knots, levels);
}

// k_ssc_kb of a cross block: R(k_a) from slot 0's epoch (halo_a at z_bar_a) and R(k_b) from
// slot 1's (halo_b at z_bar_b), both CHOMP_P_SSC_RESPONSE, staged side by side in LDS as
// k_cov_cross_knots stages its two spectra.  LDS: ssc_kb_cross_lds_doubles.
// (the body of k_ssc_kb_cross and of a cross block of k_ssc_blocks_kb; per side the epoch record
//  as doubles and its knot-table slab)
template <bool BAO>
__device__ __forceinline__ void ssc_kb_cross_body(const chomp_config& cfg, const TabLayout& HL,
                                                  const SscLayout& S,
                                                  const double* __restrict__ ep_a,
                                                  const double* __restrict__ ep_b,
                                                  const double* __restrict__ htab_a,
                                                  const double* __restrict__ htab_b,
                                                  const double* __restrict__ st,
                                                  const double* __restrict__ theta_a,
                                                  const double* __restrict__ theta_b,
                                                  double* __restrict__ knots,
                                                  double* __restrict__ levels) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch Ea, Eb;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&Ea), ep_a, kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&Eb), ep_b, kEpochDoubles);
  __syncthreads();
  PowerEval Pa, Pb;
  Pa.stage(cfg, HL, &Ea, htab_a, CHOMP_P_SSC_RESPONSE, sm);
  Pb.stage(cfg, HL, &Eb, htab_b, CHOMP_P_SSC_RESPONSE, sm + 12 * (HL.NK - 1));
  const int i = blockIdx.x, pair = blockIdx.y, NK = cfg.kernel_npoints;
  const double ln_k_min = log(cfg.k_min), ln_k_max = log(cfg.k_max);
  const double ka = exp(linspace_at(ln_k_min, ln_k_max, NK, i));
  SscRow K;
  K.build(ssc_spline(S, st), log(ka * theta_a[pair]), sm + 24 * (HL.NK - 1));
  __syncthreads();
  Pa.template finish_t<BAO>();
  Pb.template finish_t<BAO>();
  SscKbIntegrand<BAO> f{&Pb, &K, Pa.template eval_t<BAO>(ka), theta_b[pair]};
  int level = 0;
  const double v = romberg1<4>(f, ln_k_min, ln_k_max, cfg.global_precision, cfg.corr_precision,
                               cfg.divmax, red, &level);
  if (threadIdx.x == 0) {
    knots[(size_t)pair * NK + i] = v;
    if (levels) levels[(size_t)pair * NK + i] = (double)level;
  }
}
template <bool BAO>
__global__ __launch_bounds__(256) void k_ssc_kb_cross(chomp_config cfg, TabLayout HL, SscLayout S,
                                                      CrossLayout C,
                                                      const double* __restrict__ ct,
                                                      const double* __restrict__ st,
                                                      const double* __restrict__ theta_a,
                                                      const double* __restrict__ theta_b,
                                                      double* __restrict__ knots,
                                                      double* __restrict__ levels) {
  ssc_kb_cross_body<BAO>(cfg, HL, S, ct + C.ep[0], ct + C.ep[1], ct + C.htab[0], ct + C.htab[1],
                         st, theta_a, theta_b, knots, levels);
}

// covariance.py:605-622, 694-721 (covariance_NG and covariance_ssc alike): the not-a-knot spline
// of the k_a knots, norm = 1 / spline(0), the
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
// (the body of k_ssc_outer and of k_ssc_blocks_outer; workgroup blockIdx.x)
__device__ __forceinline__ void ssc_outer_body(const chomp_config& cfg, double area,
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
__global__ __launch_bounds__(256) void k_ssc_outer(chomp_config cfg, double area,
                                                   const double* __restrict__ knots,
                                                   double* __restrict__ out) {
  ssc_outer_body(cfg, area, knots, out);
}

// ---------------------------------------------------------------------------------------------
// The block axis of the super-sample term (chomp_covariance_ssc_blocks: the super-sample values
// of every block of a CovarianceMulti(ssc_cov=True, cross_terms=True) in one call)
// ---------------------------------------------------------------------------------------------
// The blocks, their order and what they read are those of the Gaussian block axis
// (chomp_proj_kernels.h, "The block axis of the Gaussian covariance"): block (i, j), i <= j, in
// the row-major order of the upper triangle, reads projection set i, set j, epoch i and epoch j
// where they lie -- no snapshot, no CrossState.  A diagonal block runs the bodies of the matching
// path (FOUR = false, ssc_kb_body with epoch i), a cross block those of the four-window path: a1,
// a2 and the MultiEpoch from set i, b1, b2 from set j, the response of epoch i at k_a and of epoch
// j at k_b.  The same code, so the same bits; the branch is uniform in a workgroup.
//
// Every block owns one SscLayout slab.  The two template instances of the prep and table bodies
// differ in their dynamic LDS (the four-window one stages two more windows), so each runs as a
// launch of its own over a list of its blocks; the kernels behind the table take the block as a
// grid dimension.  The index block of a call, ints:
//   epoch[n_corr] | (i, j)[n_blocks] | the diagonal blocks [n_corr] | the cross blocks [n_blocks - n_corr].
//
// What the state of a term on the block axis holds whatever the term (this one and the
// trispectrum's below); a term adds its slab layout and the buffer of what its host sends.
struct TermBlocksState {
  DeviceBuffer<double> d;      // n_blocks slabs of the term's layout
  DeviceBuffer<double> d_kb;   // the k_b knots, then their levels: [n_blocks][n_pairs][kernel_npoints] each
  StagedBuffer<int> d_index;   // the index block
  size_t n_corr = 0;           // correlations of the last call (0: none yet)
  size_t n_pairs = 0;          // ... and its pairs of angles
};
struct SscBlocksState : TermBlocksState {
  DeviceBuffer<double> d_sigma;   // the blocks' sigma^2 knots (ln chi, then sigma^2) on their way into the slabs
  SscLayout S;
};
__device__ __forceinline__ CovSrc ssc_blocks_src(const ProjDev* pd, const double* ptab,
                                                 size_t pstride, int i, int j) {
  return CovSrc{pd + i, ptab + pstride * i, pd + j, ptab + pstride * j};
}

// grid ceil(n_blocks / 64), block 64, a thread per block: out[b] = z_min, z_max, chi_min, chi_max
// of the block's windows -- set i's own for a diagonal block (what chomp_kernel_info returns),
// k_cov_cross_range's for a cross block.
__global__ __launch_bounds__(64) void k_ssc_blocks_range(chomp_config cfg, ProjLayout L, int n_corr,
                                                         int n_blocks,
                                                         const ProjDev* __restrict__ pd,
                                                         const double* __restrict__ ptab,
                                                         size_t pstride,
                                                         const int* __restrict__ index,
                                                         double* __restrict__ out) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= n_blocks) return;
  const int i = index[n_corr + 2 * b], j = index[n_corr + 2 * b + 1];
  double* o = out + 4 * (size_t)b;
  if (i == j) {
    o[0] = pd[i].z_min;
    o[1] = pd[i].z_max;
    o[2] = pd[i].chi_min;
    o[3] = pd[i].chi_max;
    return;
  }
  cov_cross_range_body(cfg, L, ssc_blocks_src(pd, ptab, pstride, i, j), o);
}

// grid n listed blocks, block 256: the block's sigma^2 knots (ln_chi, sigma2: [n_blocks][NS]) into
// its slab, then k_ssc_prep.  (The body's barrier stands between these stores and the one thread
// that builds the spline from them.)
template <bool FOUR>
__global__ __launch_bounds__(256) void k_ssc_blocks_prep(
    chomp_config cfg, ProjLayout L, SscLayout S, int n_corr, const ProjDev* __restrict__ pd,
    const double* __restrict__ ptab, size_t pstride, const int* __restrict__ index,
    const int* __restrict__ list, double ln_kt_min, double ln_kt_max, double j0_limit,
    const double* __restrict__ ln_chi, const double* __restrict__ sigma2, double* slabs) {
  const int b = list[blockIdx.x];
  const int i = index[n_corr + 2 * b], j = index[n_corr + 2 * b + 1];
  double* st = slabs + (size_t)b * S.total;
  for (int q = threadIdx.x; q < S.NS; q += blockDim.x) {
    st[S.sx + q] = ln_chi[(size_t)b * S.NS + q];
    st[S.sy + q] = sigma2[(size_t)b * S.NS + q];
  }
  ssc_prep_body<FOUR>(cfg, L, S, ssc_blocks_src(pd, ptab, pstride, i, j), ln_kt_min, ln_kt_max,
                      j0_limit, st);
}

// grid (N (N + 1) / 2, n listed blocks), block 256: the knot table of block list[y].  LDS:
// ssc_table_lds_doubles of the instance.
template <bool FOUR>
__global__ __launch_bounds__(256) void k_ssc_blocks_table(
    chomp_config cfg, ProjLayout L, SscLayout S, int n_corr, const ProjDev* __restrict__ pd,
    const double* __restrict__ ptab, size_t pstride, const int* __restrict__ index,
    const int* __restrict__ list, const BesselTab* __restrict__ bess_g, double* slabs) {
  const int b = list[blockIdx.y];
  const int i = index[n_corr + 2 * b], j = index[n_corr + 2 * b + 1];
  ssc_table_body<FOUR>(cfg, L, S, ssc_blocks_src(pd, ptab, pstride, i, j), bess_g,
                       slabs + (size_t)b * S.total, nullptr, nullptr, nullptr);
}

// grid n_blocks, block 256: the bicubic of block x's table.
__global__ __launch_bounds__(256) void k_ssc_blocks_bicubic(SscLayout S, double* slabs) {
  ssc_bicubic_body(S, slabs + (size_t)blockIdx.x * S.total);
}

// grid (kernel_npoints, n_pairs, n_blocks), block 256: the k_b integral at k_a knot x of pair y of
// block z -- k_ssc_kb with epoch i for a diagonal block, k_ssc_kb_cross with epoch i's response at
// k_a and epoch j's at k_b for a cross block.  knots, levels: [n_blocks][n_pairs][kernel_npoints].
// LDS: ssc_kb_cross_lds_doubles (the larger of the two).
template <bool BAO>
__global__ __launch_bounds__(256) void k_ssc_blocks_kb(
    chomp_config cfg, TabLayout HL, SscLayout S, int n_corr, const Epoch* __restrict__ epochs,
    const double* __restrict__ htab, const int* __restrict__ index,
    const double* __restrict__ slabs, const double* __restrict__ theta_a,
    const double* __restrict__ theta_b, double* __restrict__ knots, double* __restrict__ levels) {
  const int b = blockIdx.z;
  const int i = index[n_corr + 2 * b], j = index[n_corr + 2 * b + 1];
  const int ea = index[i], eb = index[j];
  const double* st = slabs + (size_t)b * S.total;
  const size_t row = (size_t)b * gridDim.y * cfg.kernel_npoints;
  if (i == j) {
    ssc_kb_body<BAO>(cfg, HL, S, epochs + ea, htab + (size_t)ea * HL.stride, st, theta_a, theta_b,
                     knots + row, levels + row);
    return;
  }
  ssc_kb_cross_body<BAO>(cfg, HL, S, reinterpret_cast<const double*>(epochs + ea),
                         reinterpret_cast<const double*>(epochs + eb),
                         htab + (size_t)ea * HL.stride, htab + (size_t)eb * HL.stride, st, theta_a,
                         theta_b, knots + row, levels + row);
}

// grid (n_pairs, n_blocks), block 256: k_ssc_outer of pair x of block y; out [n_blocks][n_pairs].
__global__ __launch_bounds__(256) void k_ssc_blocks_outer(chomp_config cfg, double area,
                                                          const double* __restrict__ knots,
                                                          double* __restrict__ out) {
  const size_t b = blockIdx.y;
  ssc_outer_body(cfg, area, knots + b * gridDim.x * cfg.kernel_npoints, out + b * gridDim.x);
}

// ---------------------------------------------------------------------------------------------
// The one-halo trispectrum term: KernelCovariance.kernel_NG and Covariance.covariance_NG
// ---------------------------------------------------------------------------------------------
constexpr unsigned kStCovNgDivmax = CHOMP_ST_COV_NG_DIVMAX;

// Device block of the kernel_NG state: scalars | ln k theta knots | table | levels |
// log(table - 10 min) | its bicubic | scratch of the bicubic build.  It holds its own copy of
// what it takes from the kernel_ssc block, so a later kernel_ssc set-up leaves it valid.
struct NgLayout {
  int N, scal, kx, tab, lev, ltab, bic, rowt, work, total;
};
inline NgLayout make_ng_layout(int N) {
  NgLayout G;
  G.N = N;
  int o = 0;
  G.scal = o; o += 16;
  G.kx = o; o += N;
  G.tab = o; o += N * N;
  G.lev = o; o += N * N;
  G.ltab = o; o += N * N;
  G.bic = o; o += 16 * (N - 1) * (N - 1);
  G.rowt = o; o += 4 * (N - 1) * N;
  G.work = o; o += 4 * (N - 1) * (6 * N);
  G.total = (o + 7) & ~7;
  return G;
}
// scalars 0..5 and 8..11 as kSsc* (kSscLimit holds _j0_limit here), and min(table)
constexpr int kNgMin = 6;

// Device block of an uploaded I_0^4 table: ln k knots | table | bicubic | scratch.
struct NgTriLayout {
  int N, kx, tab, bic, rowt, work, total;
};
inline NgTriLayout make_ng_tri_layout(int N) {
  NgTriLayout T;
  T.N = N;
  int o = 0;
  T.kx = o; o += N;
  T.tab = o; o += N * N;
  T.bic = o; o += 16 * (N - 1) * (N - 1);
  T.rowt = o; o += 4 * (N - 1) * N;
  T.work = o; o += 4 * (N - 1) * (6 * N);
  T.total = (o + 7) & ~7;
  return T;
}
// Dynamic LDS of k_ng_kb, in doubles: the kernel_NG row (SscRow) and the trispectrum row.
inline int ng_kb_lds_doubles(int N, int NT) { return 5 * N - 4 + NT + 16 * (NT - 1); }

// The host's plan of the kernel_NG launches, as SscPlan is of the super-sample ones: what
// chomp_kernel_ng_setup, _ng_raw, _ng_eval and chomp_covariance_ng size and launch by.
struct NgPlan {
  NgLayout G;
  int NK;                           // the k_b knots of a pair of angles (kernel_npoints)
  size_t sh_table[2];               // dynamic LDS of k_ng_table: two windows, four
  size_t sh_outer;                  // ... of k_ssc_outer
  unsigned n_tab;                   // blocks of the table launch: the upper triangle of N x N
};
inline NgPlan ng_plan(const chomp_config& cfg, const ProjLayout& L) {
  NgPlan P;
  P.G = make_ng_layout(L.NKT);
  P.NK = cfg.kernel_npoints;
  for (int four = 0; four < 2; ++four)
    P.sh_table[four] = (size_t)ng_table_lds_doubles(L, four != 0) * sizeof(double);
  P.sh_outer = (size_t)ssc_outer_lds_doubles(P.NK) * sizeof(double);
  P.n_tab = (unsigned)(P.G.N * (P.G.N + 1) / 2);
  return P;
}

// grid 1, block 256: z_bar_NG, chi(z_bar_NG), D(z_bar_NG) and the ln k theta knots from the
// kernel_ssc block (k_ssc_prep has run), _j0_limit, and the status bit cleared.
__global__ __launch_bounds__(256) void k_ng_prep(SscLayout S, NgLayout G,
                                                 const double* __restrict__ st, double j0_limit,
                                                 double* __restrict__ ng,
                                                 unsigned* __restrict__ status) {
  const int t = threadIdx.x;
  for (int i = t; i < G.N; i += blockDim.x) ng[G.kx + i] = st[S.kx + i];
  if (t < 16)
    ng[G.scal + t] = t == kSscLimit ? j0_limit : (t < kSscLimit || t >= kSscZMin ? st[S.scal + t] : 0.0);
  if (t == 0 && status) atomicAnd(status, ~kStCovNgDivmax);
}

// kernel.py:1103-1111 (_kernel_NG_integrand) with the norm of raw_kernel_NG; the Romberg
// variable is chi itself.
template <bool FOUR>
struct NgKernelIntegrand {
  const CovWindows<FOUR>* P;
  const BesselTab* B;
  double kta, ktb, norm;
  __device__ __forceinline__ double operator()(double chi) const {
    return ssc_ng_integrand(*P, B, chi, kta, ktb, norm);
  }
};

// grid n integrals, block 256, LDS ng_table_lds_doubles.  ln_a == nullptr: the knot table of
// _initialize_NG_spline (kernel.py:1016-1030), block b -> the b-th (i, j), i <= j, of the upper
// triangle, written to [i][j] and [j][i] with its Romberg level; otherwise
// raw_kernel_NG(ln_a[b], ln_b[b]) into out.
// (the body of k_ng_table and of k_ng_blocks_table; workgroup blockIdx.x)
template <bool FOUR>
__device__ __forceinline__ void ng_table_body(const chomp_config& cfg, const ProjLayout& L,
                                              const NgLayout& G, const CovSrc& src,
                                              const BesselTab* __restrict__ bess_g,
                                              double* __restrict__ ng,
                                              const double* __restrict__ ln_a,
                                              const double* __restrict__ ln_b,
                                              double* __restrict__ out,
                                              unsigned* __restrict__ status) {
  extern __shared__ __align__(16) double sm[];
  __shared__ ProjDev pd, pd_b;      // (pd_b: FOUR only)
  __shared__ BesselTab B;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&pd), reinterpret_cast<const double*>(src.pd), kProjDoubles);
  if constexpr (FOUR)
    copy_doubles(reinterpret_cast<double*>(&pd_b), reinterpret_cast<const double*>(src.pd_b),
                 kProjDoubles);
  copy_doubles(reinterpret_cast<double*>(&B), reinterpret_cast<const double*>(bess_g),
               (int)(sizeof(BesselTab) / sizeof(double)));
  __syncthreads();
  CovWindows<FOUR> P;
  P.stage(L, src, pd, pd_b, sm);
  P.P.bess = &B;
  __syncthreads();
  // the common range of the windows (k_ssc_prep, through k_ng_prep; pd's own for a matching block)
  const double chi_lo = ng[G.scal + kSscChiMin], chi_hi = ng[G.scal + kSscChiMax];
  int i = 0, j = 0;
  double la, lb;
  if (ln_a) {
    la = ln_a[blockIdx.x];
    lb = ln_b[blockIdx.x];
  } else {
    int b = (int)blockIdx.x;                       // row i holds N - i entries
    while (b >= G.N - i) { b -= G.N - i; ++i; }
    j = i + b;
    la = ng[G.kx + i];
    lb = ng[G.kx + j];
  }
  // kernel.py:1044-1073
  const double kta = exp(la), ktb = exp(lb);
  const double lim = ng[G.scal + kSscLimit];
  double chi_max = fmax(lim / kta, lim / ktb);
  double v = 0.0;
  int level = 0;
  bool zero = false, converged = true;
  if (chi_max >= chi_hi) chi_max = chi_hi;
  else if (chi_max <= chi_lo) zero = true;
  if (!zero) {
    // the norm passes ln(k theta_a) where k theta_a belongs (kernel.py:1055-1056)
    const double inv = ssc_ng_integrand(P, &B, ng[G.scal + kSscChiPeak], la, la, 1.0);
    const double norm = (inv > 1e-16 || inv < -1e-16) ? 1.0 / inv : 1.0;
    const NgKernelIntegrand<FOUR> f{&P, &B, kta, ktb, norm};
    Scalar1<NgKernelIntegrand<FOUR>> w{f};
    const RombergOut<1> r = romberg_group<4, 1>(w, chi_lo, chi_max, cfg.global_precision,
                                                cfg.kernel_precision, cfg.divmax, red);
    v = r.value[0] / norm;
    level = r.level[0];
    converged = r.converged[0];
  }
  if (threadIdx.x == 0) {
    if (ln_a) {
      out[blockIdx.x] = v;
    } else {
      ng[G.tab + i * G.N + j] = v;
      ng[G.tab + j * G.N + i] = v;
      ng[G.lev + i * G.N + j] = (double)level;
      ng[G.lev + j * G.N + i] = (double)level;
    }
    if (!converged && status) atomicOr(status, kStCovNgDivmax);
  }
}
template <bool FOUR>
__global__ __launch_bounds__(256) void k_ng_table(chomp_config cfg, ProjLayout L, NgLayout G,
                                                  CovSrc src,
                                                  const BesselTab* __restrict__ bess_g,
                                                  double* __restrict__ ng,
                                                  const double* __restrict__ ln_a,
                                                  const double* __restrict__ ln_b,
                                                  double* __restrict__ out,
                                                  unsigned* __restrict__ status) {
  ng_table_body<FOUR>(cfg, L, G, src, bess_g, ng, ln_a, ln_b, out, status);
}

// grid 1, block 256: kernel.py:1026-1029 -- min(table) (numpy.min: a NaN entry gives NaN), then
// the bicubic of log(table - 10 min).  Nothing is guarded: with min >= 0 an entry equal to
// 10 min gives log(0) and the reference's spline is not finite either.
// (the body of k_ng_bicubic and of k_ng_blocks_bicubic)
__device__ __forceinline__ void ng_bicubic_body(const NgLayout& G, double* __restrict__ ng) {
  __shared__ double part[256];
  const int t = threadIdx.x, NN = G.N * G.N;
  double m = INFINITY;
  bool nan = false;
  for (int q = t; q < NN; q += blockDim.x) {
    const double v = ng[G.tab + q];
    nan = nan || isnan(v);
    m = v < m ? v : m;
  }
  part[t] = nan ? NAN : m;
  __syncthreads();
  if (t == 0) {
    for (int q = 0; q < (int)blockDim.x; ++q) {
      const double v = part[q];
      nan = nan || isnan(v);
      m = v < m ? v : m;
    }
    part[0] = nan ? NAN : m;
    ng[G.scal + kNgMin] = part[0];
  }
  __syncthreads();
  const double off = part[0] * 10.0;
  for (int q = t; q < NN; q += blockDim.x) ng[G.ltab + q] = log(ng[G.tab + q] - off);
  __threadfence_block();
  __syncthreads();
  bicubic_build(G.N, ng + G.kx, ng + G.ltab, ng + G.rowt, ng + G.work, ng + G.bic);
}
__global__ __launch_bounds__(256) void k_ng_bicubic(NgLayout G, double* __restrict__ ng) {
  ng_bicubic_body(G, ng);
}

// The bicubic of log(table - 10 min) with kernel_ssc's range rules (kernel.py:1003-1014 clamps
// with < where kernel_ssc has <=: the clamped value is the same), and 10 min.
struct NgSpline {
  SscSpline K;
  double off;
  // kernel_NG at one point
  __device__ __forceinline__ double operator()(double a, double b) const {
    if (a <= K.lo) a = K.lo;
    if (b <= K.lo) b = K.lo;
    if (!(a <= K.hi && b <= K.hi)) return 0.0;
    return exp(K.poly(a, b)) + off;
  }
};
__device__ __forceinline__ NgSpline ng_spline(const NgLayout& G, const double* ng) {
  NgSpline K;
  K.K.x = ng + G.kx;
  K.K.bic = ng + G.bic;
  K.K.N = G.N;
  K.K.lo = ng[G.scal + kSscLnMin];
  K.K.hi = ng[G.scal + kSscLnMax];
  K.off = ng[G.scal + kNgMin] * 10.0;
  return K;
}

__global__ void k_ng_eval(NgLayout G, const double* __restrict__ ng,
                          const double* __restrict__ a, const double* __restrict__ b, int n,
                          double* __restrict__ out) {
  const NgSpline K = ng_spline(G, ng);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = K(a[i], b[i]);
}

// grid 1, block 256: the ln k knots linspace(ln k_min, ln k_max, N) and the bicubic of the
// uploaded I_0^4 table -- the knots and the routine of k_tri1h_table / k_tri1h_bicubic, so the
// coefficients are those of the trispectrum object's own context.
__global__ __launch_bounds__(256) void k_ng_tri(NgTriLayout T, double k_min, double k_max,
                                                double* __restrict__ tri) {
  const double ln_k_min = log(k_min), ln_k_max = log(k_max);
  for (int i = threadIdx.x; i < T.N; i += blockDim.x)
    tri[T.kx + i] = linspace_at(ln_k_min, ln_k_max, T.N, i);
  __threadfence_block();
  __syncthreads();
  bicubic_build(T.N, tri + T.kx, tri + T.tab, tri + T.rowt, tri + T.work, tri + T.bic);
}

// trispectrum_parallelogram(k_a, .) of HaloTrispectrumOneHalo at one fixed k_a
// (halo_trispectrum.py:100-106): k < k_min is clamped to k_min, either k > k_max gives 0, and
// the spline clamps ln k into its knot range (k_tri1h_eval).  The 16 (N - 1) coefficients of
// k_a's row of cells are staged in LDS and the cell polynomial is Bicubic::poly's, so the value
// is k_tri1h_eval's at the same (ln k_a, ln k_b).  lds: N + 16 (N - 1) doubles.  All threads
// call build(); a barrier must follow before use.
struct TriRow {
  Bicubic B;                       // (x: the knots in LDS; bic: the row's cells in LDS)
  double k_min, k_max, da;
  bool zero;                       // k_a above k_max (or NaN): every value is 0
  __device__ __forceinline__ void build(const NgTriLayout& T, const double* tri, double k_min_,
                                        double k_max_, double ka, double* lds) {
    double* lx = lds;
    double* lc = lds + T.N;
    Bicubic K;
    K.x = tri + T.kx; K.bic = tri + T.bic; K.N = T.N;
    K.lo = K.x[0]; K.hi = K.x[T.N - 1];
    B = K; B.x = lx; B.bic = lc;
    k_min = k_min_; k_max = k_max_;
    if (ka < k_min) ka = k_min;
    zero = !(ka <= k_max);
    for (int i = threadIdx.x; i < T.N; i += blockDim.x) lx[i] = K.x[i];
    da = 0.0;
    if (zero) return;
    double u = log(ka);
    u = u < K.lo ? K.lo : (u > K.hi ? K.hi : u);
    const int ia = K.interval(u);
    da = u - K.x[ia];
    const double* src = K.bic + (size_t)ia * (T.N - 1) * 16;
    for (int q = threadIdx.x; q < 16 * (T.N - 1); q += blockDim.x) lc[q] = src[q];
  }
  __device__ __forceinline__ double operator()(double kb) const {
    if (kb < k_min) kb = k_min;
    if (zero || !(kb <= k_max)) return 0.0;
    double v = log(kb);
    v = v < B.lo ? B.lo : (v > B.hi ? B.hi : v);
    const int jb = B.interval(v);
    return bicubic_cell(B.bic + (size_t)jb * 16, da, v - B.x[jb]);
  }
};

// covariance.py:673-683 (_kb_integrand): k_b^2 T(k_a, k_b) kernel_NG(ln k_a theta_a,
// ln k_b theta_b), norm = 1.
struct NgKbIntegrand {
  const TriRow* T;
  const SscRow* K;
  double off, theta_b;
  __device__ __forceinline__ double operator()(double ln_kb) const {
    const double kb = exp(ln_kb);
    double b = log(kb * theta_b);
    const double kern = K->inside(b) ? exp(K->at(b)) + off : 0.0;
    return kb * kb * 1.0 * (*T)(kb) * kern;
  }
};

// grid (kernel_npoints, n pairs), block 256: the k_b integral at k_a knot x of pair y
// (covariance.py:624-671), / D(z_bar_NG)^4.  LDS: ng_kb_lds_doubles.
// (the body of k_ng_kb and of k_ng_blocks_kb; workgroup (blockIdx.x, blockIdx.y))
__device__ __forceinline__ void ng_kb_body(const chomp_config& cfg, const NgLayout& G,
                                           const NgTriLayout& T, const double* __restrict__ ng,
                                           const double* __restrict__ tri, double tri_k_min,
                                           double tri_k_max, const double* __restrict__ theta_a,
                                           const double* __restrict__ theta_b,
                                           double* __restrict__ knots,
                                           double* __restrict__ levels,
                                           unsigned* __restrict__ status) {
  extern __shared__ __align__(16) double sm[];
  __shared__ double red[romberg_scratch<4, 2>()];
  const int i = blockIdx.x, pair = blockIdx.y, NK = cfg.kernel_npoints;
  const double ln_k_min = log(cfg.k_min), ln_k_max = log(cfg.k_max);
  const double ka = exp(linspace_at(ln_k_min, ln_k_max, NK, i));
  const NgSpline S = ng_spline(G, ng);
  SscRow K;
  K.build(S.K, log(ka * theta_a[pair]), sm);
  TriRow R;
  R.build(T, tri, tri_k_min, tri_k_max, ka, sm + 5 * G.N - 4);
  __syncthreads();
  const NgKbIntegrand f{&R, &K, S.off, theta_b[pair]};
  Scalar1<NgKbIntegrand> w{f};
  const RombergOut<1> r = romberg_group<4, 1>(w, ln_k_min, ln_k_max, cfg.global_precision,
                                              cfg.corr_precision, cfg.divmax, red);
  if (threadIdx.x == 0) {
    const double D = ng[G.scal + kSscDz];
    knots[(size_t)pair * NK + i] = r.value[0] / (1.0 * D * D * D * D);
    if (levels) levels[(size_t)pair * NK + i] = (double)r.level[0];
    if (!r.converged[0] && status) atomicOr(status, kStCovNgDivmax);
  }
}
__global__ __launch_bounds__(256) void k_ng_kb(chomp_config cfg, NgLayout G, NgTriLayout T,
                                               const double* __restrict__ ng,
                                               const double* __restrict__ tri, double tri_k_min,
                                               double tri_k_max,
                                               const double* __restrict__ theta_a,
                                               const double* __restrict__ theta_b,
                                               double* __restrict__ knots,
                                               double* __restrict__ levels,
                                               unsigned* __restrict__ status) {
  ng_kb_body(cfg, G, T, ng, tri, tri_k_min, tri_k_max, theta_a, theta_b, knots, levels, status);
}

// ---------------------------------------------------------------------------------------------
// The block axis of the trispectrum term (chomp_covariance_ng_blocks: the one-halo trispectrum
// values of every block of a CovarianceMulti(nongaussian_cov=True, cross_terms=True) in one call)
// ---------------------------------------------------------------------------------------------
// The blocks, their order and the windows they read are those of the super-sample block axis
// above: block (i, j), i <= j, in the row-major order of the upper triangle, reads projection set
// i and set j where they lie (ssc_blocks_src) -- no snapshot, no CrossState.  The term reads no
// halo epoch: the one I_0^4 table of the call (k_ng_tri, once) serves every block, and an epoch
// only names the status word CHOMP_ST_COV_NG_DIVMAX of block (i, j) goes to, epoch[i]'s.  A
// diagonal block runs the bodies of the matching path (FOUR = false), a cross block those of the
// four-window path: the same code as k_ssc_prep + k_ng_prep, k_ng_table, k_ng_bicubic and k_ng_kb,
// so the same bits; every branch on the block is uniform in a workgroup.
//
// Every block owns one NgLayout slab.  Its scalars come from cov_scalars_body alone: no sigma^2
// knot is read, so the host sends none.  The two instances of the prep and table bodies differ in
// their dynamic LDS, so each runs as a launch of its own over a list of its blocks (the index
// block of the super-sample calls, with the lists).
struct NgBlocksState : TermBlocksState {
  DeviceBuffer<double> d_tri;  // the I_0^4 table of the last call and its bicubic (NgTriLayout)
  NgLayout G;
};

// grid n listed blocks, block 256: what k_ssc_prep and k_ng_prep leave in a kernel_NG block -- the
// scalars with _j0_limit, the ln k theta knots -- in block list[x]'s slab, and the status bit of
// epoch[i]'s word cleared (every i has its diagonal block; the tables are launched behind both
// prep launches).  status == nullptr: no status.
template <bool FOUR>
__global__ __launch_bounds__(256) void k_ng_blocks_prep(
    chomp_config cfg, ProjLayout L, NgLayout G, int n_corr, const ProjDev* __restrict__ pd,
    const double* __restrict__ ptab, size_t pstride, const int* __restrict__ index,
    const int* __restrict__ list, double ln_kt_min, double ln_kt_max, double j0_limit,
    double* slabs, unsigned* __restrict__ status) {
  const int b = list[blockIdx.x];
  const int i = index[n_corr + 2 * b], j = index[n_corr + 2 * b + 1];
  double* ng = slabs + (size_t)b * G.total;
  const int t = threadIdx.x;
  // (the scalars k_ng_prep leaves at 0, and those nothing reads)
  if (t == 6 || t == 7 || (t >= 12 && t < 16)) ng[G.scal + t] = 0.0;
  if (t == 0 && status) atomicAnd(status + index[i], ~kStCovNgDivmax);
  cov_scalars_body<FOUR>(cfg, L, G.N, ssc_blocks_src(pd, ptab, pstride, i, j), ln_kt_min,
                         ln_kt_max, j0_limit, ng + G.scal, ng + G.kx);
}

// grid (N (N + 1) / 2, n listed blocks), block 256: the knot table of block list[y].  LDS:
// ng_table_lds_doubles of the instance.
template <bool FOUR>
__global__ __launch_bounds__(256) void k_ng_blocks_table(
    chomp_config cfg, ProjLayout L, NgLayout G, int n_corr, const ProjDev* __restrict__ pd,
    const double* __restrict__ ptab, size_t pstride, const int* __restrict__ index,
    const int* __restrict__ list, const BesselTab* __restrict__ bess_g, double* slabs,
    unsigned* __restrict__ status) {
  const int b = list[blockIdx.y];
  const int i = index[n_corr + 2 * b], j = index[n_corr + 2 * b + 1];
  ng_table_body<FOUR>(cfg, L, G, ssc_blocks_src(pd, ptab, pstride, i, j), bess_g,
                      slabs + (size_t)b * G.total, nullptr, nullptr, nullptr,
                      status ? status + index[i] : nullptr);
}

// grid n_blocks, block 256: min(table) and the bicubic of log(table - 10 min) of block x.
__global__ __launch_bounds__(256) void k_ng_blocks_bicubic(NgLayout G, double* slabs) {
  ng_bicubic_body(G, slabs + (size_t)blockIdx.x * G.total);
}

// grid (kernel_npoints, n_pairs, n_blocks), block 256: the k_b integral at k_a knot x of pair y of
// block z, every block with the one I_0^4 slab `tri`.  knots, levels:
// [n_blocks][n_pairs][kernel_npoints].  LDS: ng_kb_lds_doubles.
__global__ __launch_bounds__(256) void k_ng_blocks_kb(
    chomp_config cfg, NgLayout G, NgTriLayout T, int n_corr, const int* __restrict__ index,
    const double* __restrict__ slabs, const double* __restrict__ tri, double tri_k_min,
    double tri_k_max, const double* __restrict__ theta_a, const double* __restrict__ theta_b,
    double* __restrict__ knots, double* __restrict__ levels, unsigned* __restrict__ status) {
  const int b = blockIdx.z;
  const int i = index[n_corr + 2 * b];
  const size_t row = (size_t)b * gridDim.y * cfg.kernel_npoints;
  ng_kb_body(cfg, G, T, slabs + (size_t)b * G.total, tri, tri_k_min, tri_k_max, theta_a, theta_b,
             knots + row, levels + row, status ? status + index[i] : nullptr);
}

// ---------------------------------------------------------------------------
// Gaussian covariance of C_l: CovarianceFourier (covariance.py:874-1083)
// ---------------------------------------------------------------------------
// Four Limber tables over ln l, one per window pair X = a1a2, b1b2, a1b2, b1a2, each from the
// P_mm of its own halo epoch (at that pair's z_bar).  The windows and the MultiEpoch are the two
// slots of a cross block staged with CHOMP_CROSS_WINDOWS (slot 0: a1, a2 and the MultiEpoch; slot
// 1: b1, b2); the epochs are the context's own.  Device block: per pair 8 scalars | ln l knots |
// per pair {table, its logarithm, the spline of that, Romberg levels, spline_build's work}.
constexpr int kCovfA1A2 = 0, kCovfB1B2 = 1, kCovfA1B2 = 2, kCovfB1A2 = 3;
// scalars of a pair
constexpr int kCovfZMin = 0, kCovfZMax = 1, kCovfZBar = 2, kCovfChiBar = 3, kCovfChiMin = 4,
              kCovfChiMax = 5, kCovfDBar = 6, kCovfNorm = 7;
struct FourierLayout {
  int N, scal, ln_l, tab[4], logt[4], pp[4], lev[4], work[4], total;
};
inline FourierLayout make_fourier_layout(int N) {
  FourierLayout F;
  F.N = N;
  int o = 0;
  F.scal = o; o += 4 * 8;
  F.ln_l = o; o += N;
  for (int t = 0; t < 4; ++t) {
    F.tab[t] = o; o += N;
    F.logt[t] = o; o += N;
    F.pp[t] = o; o += 4 * (N - 1);
    F.lev[t] = o; o += N;
    F.work[t] = o; o += 2 * N;
  }
  F.total = (o + 7) & ~7;
  return F;
}
struct FourierState {
  DeviceBuffer<double> d;  // the block of FourierLayout
  FourierLayout F;
  bool zbar = false;       // the scalars of the four pairs (chomp_covariance_fourier_zbar) valid
  bool ready = false;      // ... and the four tables with their splines (chomp_covariance_fourier_table)
  double ln_l_min = 0.0, ln_l_max = 0.0;
};
// Dynamic LDS of k_covf_knots, in doubles: one PowerEval staging, the MultiEpoch and the pair's two
// window splines.
inline int covf_lds_doubles(int NK_halo, const ProjLayout& L) {
  return 12 * (NK_halo - 1) + L.NC + 8 * (L.NC - 1) + 8 * (L.NWp - 1);
}

// The two windows of pair X in the two slots: (first of slot 0 or 1, second of slot 0 or 1).
__device__ __forceinline__ void covf_pair_windows(const ProjLayout& L, const CovSrc& src, int X,
                                                  const double** pp1, const double** pp2,
                                                  const ProjDev** pd1, const ProjDev** pd2) {
  const bool first_b = X == kCovfB1B2 || X == kCovfB1A2;
  const bool second_b = X == kCovfB1B2 || X == kCovfA1B2;
  *pd1 = first_b ? src.pd_b : src.pd;
  *pd2 = second_b ? src.pd_b : src.pd;
  *pp1 = (first_b ? src.ptab_b : src.ptab) + L.w_pp[0];
  *pp2 = (second_b ? src.ptab_b : src.ptab) + L.w_pp[1];
}

// grid 4 (pairs), block 256: _calculate_zbar (covariance.py:1067-1075) on the caller's z grid
// (CovarianceFourier._z_array, nz <= 256): the first argmax of w1 w2 / chi^2 D(z(chi))^2 at chi =
// comoving_distance(z) -- numpy.argmax: the first of equal maxima, and the first NaN if there is
// one -- and the pair's scalars: z_min = max, z_max = min of its two windows', z_bar, chi(z_bar),
// chi(z_min), chi(z_max), MultiEpoch.growth_factor(z_bar).
__global__ __launch_bounds__(256) void k_covf_zbar(ProjLayout L, FourierLayout F, CovSrc src,
                                                   const double* __restrict__ z, int nz,
                                                   double* __restrict__ ft) {
  __shared__ double cand[256];
  const int X = blockIdx.x, t = threadIdx.x;
  const double *pp1, *pp2;
  const ProjDev *pd1, *pd2;
  covf_pair_windows(L, src, X, &pp1, &pp2, &pd1, &pd2);
  const MEView me = me_view(L, *src.pd, src.ptab, 0);
  const WindowView w1{pp1, L.NWp, pd1->w_chi_min[0], pd1->w_chi_max[0]};
  const WindowView w2{pp2, L.NWp, pd2->w_chi_min[1], pd2->w_chi_max[1]};
  if (t < nz) {
    const double chi = me.comoving_distance(z[t]);
    const double D = me.growth_factor(me.redshift(chi));
    cand[t] = w1(chi) * w2(chi) / (chi * chi) * D * D;
  }
  __syncthreads();
  if (t != 0) return;
  int best = 0;
  for (int i = 1; i < nz && !isnan(cand[best]); ++i)
    if (isnan(cand[i]) || cand[i] > cand[best]) best = i;
  const double z_min = pd1->w_z_min[0] > pd2->w_z_min[1] ? pd1->w_z_min[0] : pd2->w_z_min[1];
  const double z_max = pd1->w_z_max[0] < pd2->w_z_max[1] ? pd1->w_z_max[0] : pd2->w_z_max[1];
  double* s = ft + F.scal + 8 * X;
  s[kCovfZMin] = z_min;
  s[kCovfZMax] = z_max;
  s[kCovfZBar] = z[best];
  s[kCovfChiBar] = me.comoving_distance(z[best]);
  s[kCovfChiMin] = me.comoving_distance(z_min);
  s[kCovfChiMax] = me.comoving_distance(z_max);
  s[kCovfDBar] = me.growth_factor(z[best]);
  s[kCovfNorm] = 0.0;
}

// covariance.py:1077-1083 (_pl_integrand) in the reference's order of operations.  The end-point
// guard is CovProjIntegrand's.
template <bool BAO>
struct CovFourierIntegrand {
  const PowerEval* P;
  const MEView* me;
  const WindowView *w1, *w2;
  double l, norm;
  __device__ __forceinline__ double operator()(double chi) const {
    const double D = me->growth_factor(me->redshift(chi));
    double k = l / chi;
    if (k > P->k_max && k <= P->k_max * (1.0 + 8.9e-16)) k = P->k_max;
    return norm * (*w1)(chi) * (*w2)(chi) * D * D / (chi * chi) * P->template eval_t<BAO>(k);
  }
};

// grid (N = corr_npoints, 4 pairs), block 256: knot x of table y of _initialize_pl
// (covariance.py:958-1044), the Romberg over [chi(z_min_X), chi(z_max_X)] of norm_X w1 w2 D^2 /
// chi^2 P_mm,X(l / chi) with epoch[X]'s spectrum, divided by D(z_bar_X)^2.  norm_X is formed here
// as the reference forms it (:987-1006): 1 / integrand at chi(z_bar_X) with l = chi (k = 1), the
// windows a1 and a2 whatever the pair, and the spectrum of epoch[X] -- but halo_a1a2's, epoch[0],
// for a1b2.  A norm integrand that is not positive and finite leaves the knot NaN (the host
// reports it).  LDS: covf_lds_doubles.
template <bool BAO>
__global__ __launch_bounds__(256) void k_covf_knots(chomp_config cfg, TabLayout HL, ProjLayout L,
                                                    FourierLayout F, CovSrc src,
                                                    const Epoch* __restrict__ epochs,
                                                    const double* __restrict__ htab, int which,
                                                    int e0, int e1, int e2, int e3,
                                                    double* __restrict__ ft) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ ProjDev pda;
  __shared__ double red[romberg_scratch<4, 2>()];
  const int i = blockIdx.x, X = blockIdx.y;
  const int e = X == 0 ? e0 : (X == 1 ? e1 : (X == 2 ? e2 : e3));
  const int en = X == kCovfA1B2 ? e0 : e;                // (:997-1001: halo_a1a2)
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[en]),
               kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&pda), reinterpret_cast<const double*>(src.pd),
               kProjDoubles);
  __syncthreads();
  PowerEval P;
  P.stage(cfg, HL, &E, htab + (size_t)en * HL.stride, which, sm);
  const int NC = L.NC, NW = L.NWp;
  double* chi_t = sm + 12 * (HL.NK - 1);                // [NC]
  double* pp_z = chi_t + NC;                            // [4 (NC - 1)]
  double* pp_g = pp_z + 4 * (NC - 1);
  double* wpp = pp_g + 4 * (NC - 1);                    // 2 x [4 (NW - 1)]
  const double *pp1, *pp2;
  const ProjDev *pd1, *pd2;
  covf_pair_windows(L, src, X, &pp1, &pp2, &pd1, &pd2);
  copy_doubles(chi_t, src.ptab + L.me_chi[0], NC);
  copy_doubles(pp_z, src.ptab + L.me_pp_z[0], 4 * (NC - 1));
  copy_doubles(pp_g, src.ptab + L.me_pp_g[0], 4 * (NC - 1));
  copy_doubles(wpp, pp1, 4 * (NW - 1));
  copy_doubles(wpp + 4 * (NW - 1), pp2, 4 * (NW - 1));
  const MEView me{nullptr, chi_t, nullptr, pp_z, pp_g, NC, pda.me_z_min[0], pda.me_z_max[0]};
  const WindowView w1{wpp, NW, pd1->w_chi_min[0], pd1->w_chi_max[0]};
  const WindowView w2{wpp + 4 * (NW - 1), NW, pd2->w_chi_min[1], pd2->w_chi_max[1]};
  __syncthreads();
  P.template finish_t<BAO>();
  const double* s = ft + F.scal + 8 * X;
  const double chi_bar = s[kCovfChiBar], D_bar = s[kCovfDBar];
  // the norm: a1 and a2 (read where they lie: one evaluation), l = exp(ln chi)
  const WindowView a1{src.ptab + L.w_pp[0], NW, pda.w_chi_min[0], pda.w_chi_max[0]};
  const WindowView a2{src.ptab + L.w_pp[1], NW, pda.w_chi_min[1], pda.w_chi_max[1]};
  CovFourierIntegrand<BAO> f{&P, &me, &a1, &a2, exp(log(chi_bar)), 1.0};
  const double norm_int = f(chi_bar);
  if (en != e) {                                         // (a1b2: now its own epoch's spectrum)
    __syncthreads();
    copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
                 kEpochDoubles);
    __syncthreads();
    P.stage(cfg, HL, &E, htab + (size_t)e * HL.stride, which, sm);
    __syncthreads();
    P.template finish_t<BAO>();
  }
  const bool ok = norm_int > 0.0 && norm_int < INFINITY;
  double v = NAN;
  int level = 0;
  if (ok) {
    f.w1 = &w1;
    f.w2 = &w2;
    f.l = exp(ft[F.ln_l + i]);
    f.norm = 1.0 / norm_int;
    v = romberg1<4>(f, s[kCovfChiMin], s[kCovfChiMax], cfg.global_precision, cfg.corr_precision,
                    cfg.divmax, red, &level) / (D_bar * D_bar);
  }
  if (threadIdx.x == 0) {
    ft[F.tab[X] + i] = v;
    ft[F.lev[X] + i] = (double)level;
    if (i == 0) ft[F.scal + 8 * X + kCovfNorm] = 1.0 / norm_int;
  }
}

// grid 4, block 64: the not-a-knot spline of ln(table blockIdx.x) over ln l (covariance.py:1048-1063).
__global__ void k_covf_spline(FourierLayout F, double* __restrict__ ft) {
  const int X = blockIdx.x;
  if (threadIdx.x != 0 || X >= 4) return;
  for (int i = 0; i < F.N; ++i) ft[F.logt[X] + i] = log(ft[F.tab[X] + i]);
  spline_build(ft + F.ln_l, ft + F.logt[X], F.N, ft + F.pp[X], ft + F.work[X]);
}

// Element-wise over n multipoles, x = ln l[n] then l[n]: out[X n + j] = _pl_X(l_j) =
// exp(spline_X(ln l)) / norm_X inside ln_l_min <= ln l <= ln_l_max and exactly 0 outside
// (covariance.py:934-956), and out[4 n + j] = covariance_G(l_j) = (pl_a1a2 pl_b1b2 + pl_a1b2
// pl_b1a2) / (2 l + 1) (:928-932).
__global__ __launch_bounds__(256) void k_covf_eval(FourierLayout F, const double* __restrict__ ft,
                                                   double ln_l_min, double ln_l_max,
                                                   const double* __restrict__ x, size_t n,
                                                   double* __restrict__ out) {
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += (size_t)gridDim.x * blockDim.x) {
    const double ln_l = x[j], l = x[n + j];
    const bool inside = ln_l >= ln_l_min && ln_l <= ln_l_max;
    double p[4];
#pragma unroll
    for (int X = 0; X < 4; ++X) {
      p[X] = inside ? exp(spline_eval(ft + F.ln_l, ft + F.pp[X], F.N, ln_l)) /
                          ft[F.scal + 8 * X + kCovfNorm]
                    : 0.0;
      out[(size_t)X * n + j] = p[X];
    }
    out[4 * n + j] = 1.0 / (2.0 * l + 1.0) * (p[0] * p[1] + p[2] * p[3]);
  }
}

}  // namespace chomp
