// chomp_proj_kernels.h -- HIP kernels of the projection side (gfx950):
//
//   k_halofit_sigma / k_halofit_finalize   HaloFit._initialize_sigma_spline (halo.py:1268-1319)
//   k_proj_chi          MultiEpoch chi(z) Romberg per grid point (cosmology.py:787-794),
//                       growth table (:813-814), dNdz.normalize (kernel.py:43-54)
//   k_proj_me_splines   chi(z), z(chi), D(z) splines (cosmology.py:795-817) and the
//                       windows' chi grids (kernel.py:289-306)
//   k_proj_window       raw_window_function per chi knot: galaxy (kernel.py:382-387),
//                       convergence with its inner Romberg (:443-484)
//   k_proj_window_splines  window splines (:308-313) + Kernel.__init__ scalars and
//                       _find_z_bar (:595-639)
//   k_proj_kernel_knots K(ln k theta) knots: Romberg over chi with J0 / J2 truncated at
//                       the 8th Bessel zero (:678-712, 812-839)
//   k_proj_kernel_spline  (:641-649)
//   k_kernel_eval / k_window_eval   Kernel.kernel (:714-729), window_function (:326-340)
//   k_wtheta            Correlation.correlation (correlation.py:242-275)
//   k_cell              CorrelationFourier.correlation (correlation.py:360-392)
//
// One integral per workgroup (1 or 4 wavefronts), all splines / Bessel Chebyshev
// tables / P(k) knot splines staged in LDS, __shfl_xor reductions.
#pragma once

#include <hip/hip_runtime.h>

#include "chomp_buffers.h"
#include "chomp_de_kernels.h"
#include "chomp_power_kernels.h"

namespace chomp {

struct DndzDev {
  int kind, pp_n;
  double z_min, z_max, p[4], norm;
  const double* pp;          // CHOMP_DNDZ_PPOLY: breaks[pp_n + 1], then coef[pp_n][pp_order + 1]
  int pp_order, pad;
};

// Scalars of one projection set-up (host fills the inputs, kernels fill the rest).
struct ProjDev {
  // SingleEpoch(0) background of the MultiEpoch (cosmology.py:761-783)
  double om0, ol0, or0, H0, growth_norm;
  double me_z_min[3], me_z_max[3];   // 0: the kernel's MultiEpoch, 1/2: windows' copies
  DndzDev dist[2];
  int wkind[2];
  double w_z_min[2], w_z_max[2], w_chi_min[2], w_chi_max[2], w_g_chi_min[2];
  double z_min, z_max, chi_min, chi_max, ln_kt_min, ln_kt_max, j_limit, z_bar, D_zbar;
  int order, pad;
};
static_assert(sizeof(ProjDev) % 8 == 0, "ProjDev granularity");
constexpr int kProjDoubles = (int)(sizeof(ProjDev) / sizeof(double));

struct ProjLayout {
  int NC, NWp, NKT;
  int me_z[3], me_chi[3], me_growth[3], me_pp_chi[3], me_pp_z[3], me_pp_g[3];
  int w_chi[2], w_wf[2], w_pp[2];
  int k_ln, k_arr, k_pp, k_lev;
  int total;
};

inline ProjLayout make_proj_layout(int NC, int NWp, int NKT) {
  ProjLayout L;
  L.NC = NC; L.NWp = NWp; L.NKT = NKT;
  int o = 0;
  for (int m = 0; m < 3; ++m) {
    L.me_z[m] = o; o += NC;
    L.me_chi[m] = o; o += NC;
    L.me_growth[m] = o; o += NC;
    L.me_pp_chi[m] = o; o += 4 * (NC - 1);
    L.me_pp_z[m] = o; o += 4 * (NC - 1);
    L.me_pp_g[m] = o; o += 4 * (NC - 1);
  }
  for (int w = 0; w < 2; ++w) {
    L.w_chi[w] = o; o += NWp;
    L.w_wf[w] = o; o += NWp;
    L.w_pp[w] = o; o += 4 * (NWp - 1);
  }
  L.k_ln = o; o += NKT;
  L.k_arr = o; o += NKT;
  L.k_pp = o; o += 4 * (NKT - 1);
  L.k_lev = o; o += NKT;
  L.total = (o + 7) & ~7;
  return L;
}

struct ProjState {
  bool ready = false;      // full kernel set-up done
  bool me_ready = false;   // MultiEpoch 0 tables valid
  bool de = false;         // the set-up's cosmology has w0-wa dark energy (its table: chomp_ctx::de_proj)
  ProjLayout L;
  ProjDev host;            // host copy of the scalars (refreshed by kernel_info)
  DeviceBuffer<ProjDev> d_pd;
  DeviceBuffer<ProjDev> d_pd_init;   // the block as the host prepared it (the device fills d_pd in)
  DeviceBuffer<double> d_tab;
  size_t pp_total = 0;     // doubles of tabulated redshift distributions behind the tables
  bool cov_ready = false;  // covariance table (chomp_covariance_table) valid
  DeviceBuffer<double> d_cov;
  bool ssc_prep = false;   // sigma^2 spline and z_bar_NG (chomp_kernel_ssc_setup) valid
  bool ssc_ready = false;  // ... and the kernel_ssc table with its bicubic
  int ssc_ns = 0;          // sigma^2 knots of that set-up
  DeviceBuffer<double> d_ssc;
  bool ssc_four = false;   // that state is of the four windows of a cross block (chomp_kernel_ssc_setup_cross)
  bool ng_four = false;    // ... and so is the kernel_NG state built from it
  bool ng_prep = false;    // kernel_NG scalars and knots (chomp_kernel_ng_setup) valid
  bool ng_ready = false;   // ... and the kernel_NG table with its log-offset bicubic
  DeviceBuffer<double> d_ng;
  DeviceBuffer<double> d_ng_tri;   // the I_0^4 table of the last chomp_covariance_ng and its bicubic
};

// The projection set-ups of chomp_kernel_setup_sets / chomp_kernel_setup_pairs, beside ProjState
// (which they never touch): n ProjDev blocks and n slabs of L.total doubles, set s at d_pd[s] and d_tab + s * L.total.
// The buffers are kept across calls and only grow.  The sets have their own arena of tabulated
// redshift distributions (d_pp: the distinct tables of the last call, placed by chomp_pp_plan.h;
// the blocks' dist[w].pp point into it and are rebuilt every call, so a moved arena is harmless)
// and their own pressure tables (de, with every set's table in d_de_slot, -1 for Lambda-CDM):
// the single set-up's tables (behind ProjState::d_tab, chomp_ctx::de_proj) are not touched.
struct ProjSets {
  size_t n = 0;            // sets of the last set-up of sets (0: none yet)
  ProjLayout L;
  ProjDev host;            // what the sets share, as the host prepared it (ln k theta range, order)
  DeviceBuffer<ProjDev> d_pd;
  StagedBuffer<ProjDev> d_pd_init;   // the blocks as the host prepared them (the device fills d_pd in)
  DeviceBuffer<double> d_tab;
  StagedBuffer<double> d_pp;
  DeTables de;
  StagedBuffer<int> d_de_slot;
};

// ---------------------------------------------------------------------------
// HaloFit
// ---------------------------------------------------------------------------
// grid NK, block 256: ln sigma^2(R_i), R_i = exp(linspace(ln 0.1, ln 10, NK)).
template <bool BAO>
__global__ __launch_bounds__(256) void k_halofit_sigma(chomp_config cfg, TabLayout L,
                                                       const Epoch* __restrict__ epochs,
                                                       int e, double* __restrict__ tab) {
  __shared__ Epoch E;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  __syncthreads();
  const int i = blockIdx.x;
  const double R = exp(linspace_at(log(0.1), log(10.0), L.NK, i));
  HalofitSigmaIntegrand<BAO> f{&E, R};
  const double s2 = romberg1<4>(f, log(cfg.k_min), log(cfg.k_max), cfg.global_precision,
                                cfg.halo_precision, cfg.divmax, red);
  if (threadIdx.x == 0) tab[(size_t)e * L.stride + L.off_hf_lns2 + i] = log(s2);
}

// First two derivatives at xq of the quintic interpolating spline through (x, y) -- what
// quintic_derivs (chomp_math.h) computes -- by one wavefront: the collocation rows are set up
// one per lane, the banded elimination runs its (row, column) updates of a pivot step in
// parallel lanes, the back substitution its five products.  Same row operations in the same
// order as the serial routine (only the 5-term sums of the back substitution are added in
// another order).  x, y: LDS or global; work: (n + 6) + 11 n + n doubles of LDS; n <= 64 rows
// per pass are handled by striding the lanes.  All 64 lanes call; barriers inside (the block
// is one wavefront).
__device__ __forceinline__ void quintic_derivs_wave(const double* x, const double* y, int n,
                                                    double xq, double* work, double* d1,
                                                    double* d2) {
  const int lane = threadIdx.x & 63;
  double* t = work;               // [n + 6]
  double* ab = t + (n + 6);       // [n][11] band storage, column j at j - i + 5
  double* c = ab + 11 * n;        // [n]
  for (int i = lane; i < 6; i += 64) { t[i] = x[0]; t[n + i] = x[n - 1]; }
  for (int i = lane; i < n - 6; i += 64) t[6 + i] = x[3 + i];
  for (int i = lane; i < 11 * n; i += 64) ab[i] = 0.0;
  __syncthreads();
  for (int i = lane; i < n; i += 64) {
    int m = 5;
    while (m < n - 1 && x[i] >= t[m + 1]) ++m;
    double N[6];
    bspline_basis(t, m, 5, x[i], N);
#pragma unroll
    for (int r = 0; r < 6; ++r) ab[11 * i + (m - 5 + r - i + 5)] = N[r];
    c[i] = y[i];
  }
  __syncthreads();
  // banded elimination without pivoting (the collocation matrix is totally positive):
  // lane = 6 (r - col - 1) + (j - col) updates element (r, j); lanes 30..34 the right-hand side
  for (int col = 0; col < n; ++col) {
    const int rr = lane < 30 ? lane / 6 : lane - 30, jj = lane < 30 ? lane % 6 : 0;
    const int r = col + 1 + rr, j = col + jj;
    const bool row_ok = lane < 35 && r < n;
    double f = 0.0;
    if (row_ok) {
      const double a = ab[11 * r + (col - r + 5)];
      f = a == 0.0 ? 0.0 : a / ab[11 * col + 5];
    }
    __syncthreads();               // (every lane has read its factor before (r, col) is cleared)
    if (row_ok && f != 0.0) {
      if (lane < 30) {
        if (j < n) ab[11 * r + (j - r + 5)] -= f * ab[11 * col + (j - col + 5)];
      } else {
        c[r] -= f * c[col];
      }
    }
    __syncthreads();
  }
  for (int i = n - 1; i >= 0; --i) {
    const int j = i + 1 + lane;
    double term = (lane < 5 && j < n) ? ab[11 * i + (j - i + 5)] * c[j] : 0.0;
    term += __shfl_xor(term, 1, 64);
    term += __shfl_xor(term, 2, 64);
    term += __shfl_xor(term, 4, 64);
    if (lane == 0) c[i] = (c[i] - term) / ab[11 * i + 5];
    __syncthreads();
  }
  if (lane == 0) {
    int m = 5;
    while (m < n - 1 && xq >= t[m + 1]) ++m;
    double c1[6], c2[5], N[6];
    for (int r = 1; r <= 5; ++r) {          // j = m-5+r = m-4 .. m
      const int j = m - 5 + r;
      c1[r] = 5.0 * (c[j] - c[j - 1]) / (t[j + 5] - t[j]);
    }
    for (int r = 2; r <= 5; ++r) {          // j = m-3 .. m
      const int j = m - 5 + r;
      c2[r - 1] = 4.0 * (c1[r] - c1[r - 1]) / (t[j + 4] - t[j]);
    }
    bspline_basis(t, m, 4, xq, N);
    double s1 = 0.0;
    for (int r = 0; r < 5; ++r) s1 += c1[r + 1] * N[r];
    bspline_basis(t, m, 3, xq, N);
    double s2 = 0.0;
    for (int r = 0; r < 4; ++r) s2 += c2[r + 1] * N[r];
    *d1 = s1;
    *d2 = s2;
  }
  __syncthreads();
}

// The inverse of the quintic spline's collocation matrix on HaloFit's ln R grid
// (linspace(ln 0.1, ln 10, n): halo.py:1270-1272 -- the grid, hence the matrix, depends on n
// alone), transposed: ainv_t[j * n + i] = (A^-1)[i][j].  Host, once per context (long double
// Gauss-Jordan with partial pivoting).  The B-spline coefficients of the sigma table are then
// c = A^-1 y: fifty multiply-adds per lane, where the banded elimination and back substitution
// of quintic_derivs_wave are ~150 dependent steps of one wavefront (30 of k_halofit_finalize's
// 39 us).
inline void halofit_collocation_inverse_host(int n, double* ainv_t) {
  std::vector<double> x(n), t(n + 6);
  for (int i = 0; i < n; ++i) x[i] = linspace_at(std::log(0.1), std::log(10.0), n, i);
  for (int i = 0; i < 6; ++i) { t[i] = x[0]; t[n + i] = x[n - 1]; }
  for (int i = 0; i < n - 6; ++i) t[6 + i] = x[3 + i];
  std::vector<long double> a((size_t)n * 2 * n, 0.0L);          // [A | I]
  int m = 5;
  for (int i = 0; i < n; ++i) {
    while (m < n - 1 && x[i] >= t[m + 1]) ++m;
    double N[6];
    bspline_basis(t.data(), m, 5, x[i], N);
    for (int r = 0; r < 6; ++r) a[(size_t)i * 2 * n + (m - 5 + r)] = N[r];
    a[(size_t)i * 2 * n + n + i] = 1.0L;
  }
  for (int col = 0; col < n; ++col) {
    int piv = col;
    for (int r = col + 1; r < n; ++r)
      if (fabsl(a[(size_t)r * 2 * n + col]) > fabsl(a[(size_t)piv * 2 * n + col])) piv = r;
    if (piv != col)
      for (int j = 0; j < 2 * n; ++j) std::swap(a[(size_t)col * 2 * n + j], a[(size_t)piv * 2 * n + j]);
    const long double d = a[(size_t)col * 2 * n + col];
    for (int j = 0; j < 2 * n; ++j) a[(size_t)col * 2 * n + j] /= d;
    for (int r = 0; r < n; ++r) {
      if (r == col) continue;
      const long double f = a[(size_t)r * 2 * n + col];
      if (f == 0.0L) continue;
      for (int j = 0; j < 2 * n; ++j) a[(size_t)r * 2 * n + j] -= f * a[(size_t)col * 2 * n + j];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) ainv_t[(size_t)j * n + i] = (double)a[(size_t)i * 2 * n + n + j];
}

// quintic_derivs_wave with the coefficients from the tabulated inverse (one wavefront; work:
// (n + 6) + n doubles of LDS; barriers inside).
__device__ __forceinline__ void quintic_derivs_inv(const double* x, const double* y, int n,
                                                   double xq, const double* __restrict__ ainv_t,
                                                   double* work, double* d1, double* d2) {
  const int lane = threadIdx.x & 63;
  double* t = work;               // [n + 6]
  double* c = t + (n + 6);        // [n]
  for (int i = lane; i < 6; i += 64) { t[i] = x[0]; t[n + i] = x[n - 1]; }
  for (int i = lane; i < n - 6; i += 64) t[6 + i] = x[3 + i];
  for (int i = lane; i < n; i += 64) {
    double acc = 0.0;
    for (int j = 0; j < n; ++j) acc = fma(ainv_t[(size_t)j * n + i], y[j], acc);
    c[i] = acc;
  }
  __syncthreads();
  if (lane == 0) {
    int m = 5;
    while (m < n - 1 && xq >= t[m + 1]) ++m;
    double c1[6], c2[5], N[6];
    for (int r = 1; r <= 5; ++r) {          // j = m-5+r = m-4 .. m
      const int j = m - 5 + r;
      c1[r] = 5.0 * (c[j] - c[j - 1]) / (t[j + 5] - t[j]);
    }
    for (int r = 2; r <= 5; ++r) {          // j = m-3 .. m
      const int j = m - 5 + r;
      c2[r - 1] = 4.0 * (c1[r] - c1[r - 1]) / (t[j + 4] - t[j]);
    }
    bspline_basis(t, m, 4, xq, N);
    double s1 = 0.0;
    for (int r = 0; r < 5; ++r) s1 += c1[r + 1] * N[r];
    bspline_basis(t, m, 3, xq, N);
    double s2 = 0.0;
    for (int r = 0; r < 4; ++r) s2 += c2[r + 1] * N[r];
    *d1 = s1;
    *d2 = s2;
  }
  __syncthreads();
}

// grid 1, block 64 (one wavefront, on LDS copies): k_sigma, n_eff, C and the Takahashi et al.
// coefficients (halo.py:1285-1317) of epoch `src` stored into epoch `dst`.  The cubic spline of
// ln R over ln sigma^2 by parallel cyclic reduction, the quintic one of ln sigma^2 over ln R
// by quintic_derivs_wave.  Dynamic LDS: 25 NK + 64 doubles.
__global__ __launch_bounds__(64) void k_halofit_finalize(TabLayout L, Epoch* __restrict__ epochs,
                                                         int dst, int src,
                                                         const double* __restrict__ tab, double f1,
                                                         double f2, double f3, double omega_l,
                                                         double w, const double* __restrict__ ainv_t) {
  extern __shared__ __align__(16) double work[];
  __shared__ double sh_d[2];
  const int n = L.NK;
  double* lns2 = work + 24 * n + 64;
  double* xr = work;             // reversed ln sigma^2 (increasing)
  double* yr = xr + n;           // reversed ln R
  double* lnR = yr + n;
  double* c = lnR + n;           // [4(n-1)]
  double* w2 = c + 4 * (n - 1);  // scratch: max(9 n, (n + 6) + 12 n)
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    lns2[i] = tab[(size_t)src * L.stride + L.off_hf_lns2 + i];
    lnR[i] = linspace_at(log(0.1), log(10.0), n, i);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    xr[i] = lns2[n - 1 - i];
    yr[i] = lnR[n - 1 - i];
  }
  __syncthreads();
  spline_build_pcr(xr, yr, n, c, w2, (int)threadIdx.x, 64, true);
  const double k_s = 1.0 / exp(spline_eval(xr, c, n, 0.0));            // halo.py:1285-1287
  if (ainv_t != nullptr)                                                        // :1289-1292
    quintic_derivs_inv(lnR, lns2, n, log(1.0 / k_s), ainv_t, w2, &sh_d[0], &sh_d[1]);
  else
    quintic_derivs_wave(lnR, lns2, n, log(1.0 / k_s), w2, &sh_d[0], &sh_d[1]);
  if (threadIdx.x != 0) return;
  const double ne = -sh_d[0] - 3.0, C = -sh_d[1];
  Epoch& E = epochs[dst];
  E.hf_f1 = f1; E.hf_f2 = f2; E.hf_f3 = f3;
  E.hf_k_s = k_s; E.hf_n_eff = ne; E.hf_C = C;
  E.hf_a_n = pow(10.0, 1.5222 + 2.8553 * ne + 2.3706 * ne * ne + 0.9903 * ne * ne * ne +
                           0.2250 * ne * ne * ne * ne + -0.6038 * C +
                           0.1749 * omega_l * (1.0 + w));
  E.hf_b_n = pow(10.0, -0.5642 + 0.5864 * ne + 0.5716 * ne * ne + -1.5474 * C +
                           0.2279 * omega_l * (1.0 + w));
  E.hf_c_n = pow(10.0, 0.3698 + 2.0404 * ne + 0.8161 * ne * ne + 0.5869 * C);
  E.hf_gamma_n = 0.1971 - 0.0843 * ne + 0.8460 * C;
  E.hf_alpha_n = fabs(6.0835 + 1.3373 * ne - 0.1959 * ne * ne + -5.5274 * C);
  E.hf_beta_n = 2.0379 - 0.7354 * ne + 0.3157 * ne * ne + 1.2490 * ne * ne * ne +
                0.3980 * ne * ne * ne * ne + -0.1682 * C;
  E.hf_mu_n = 0.0;
  E.hf_nu_n = pow(10.0, 5.2105 + 3.6902 * ne);
}

// ---------------------------------------------------------------------------
// Redshift distributions (kernel.py:26-179)
// ---------------------------------------------------------------------------
__device__ __forceinline__ double dndz_raw(const DndzDev& d, double z) {
  if (d.kind == CHOMP_DNDZ_MAGLIM)          // z^a exp(-(z/z0)^b), p = {a, z0, b}
    return pow(z, d.p[0]) * exp(-1.0 * pow(z / d.p[1], d.p[2]));
  if (d.kind == CHOMP_DNDZ_BOXCAR) return 1.0;   // the base class (kernel.py:56-65)
  if (d.kind == CHOMP_DNDZ_PPOLY) {              // dNdzInterpolation: the caller's spline
    const double* br = d.pp;
    int lo = 0, hi = d.pp_n - 1;                 // last piece with br[i] <= z (ends extrapolate)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (z >= br[mid]) lo = mid; else hi = mid - 1;
    }
    const double* cf = br + d.pp_n + 1 + (size_t)lo * (d.pp_order + 1);
    const double t = z - br[lo];
    double v = cf[d.pp_order];
    for (int m = d.pp_order - 1; m >= 0; --m) v = fma(v, t, cf[m]);
    return v;
  }
  const double t = z - d.p[0];              // Gaussian, p = {z0, sigma_z}
  return exp(-1.0 * t * t / (2.0 * d.p[1] * d.p[1]));
}
__device__ __forceinline__ double dndz_eval(const DndzDev& d, double z) {
  return (z <= d.z_max && z >= d.z_min) ? d.norm * dndz_raw(d, z) : 0.0;
}
struct DndzRaw {
  const DndzDev* d;
  __device__ __forceinline__ double operator()(double z) const { return dndz_raw(*d, z); }
};

// grid (NC, 4), block 64.  y < 3: chi and growth of MultiEpoch y at grid point x;
// y == 3, x < 2: normalisation of distribution x.  DE: E with the pressure spline `de`.
// (the body of k_proj_chi and k_proj_chi_sets, in its two parts: the normalising blocks, which
//  hold the body's only barrier and never look at E, and the grid points)
__device__ __forceinline__ void proj_chi_norm(const chomp_config& cfg, ProjDev* __restrict__ pd) {
  const int i = blockIdx.x;
  if (i >= 2) return;
  __shared__ DndzDev D;
  if (threadIdx.x == 0) D = pd->dist[i];
  __syncthreads();
  DndzRaw f{&D};
  const double norm = romberg1<1>(f, D.z_min, D.z_max, cfg.global_precision,
                                  cfg.dNdz_precision, cfg.divmax, nullptr);
  if (threadIdx.x == 0) pd->dist[i].norm = 1.0 / norm;
}
template <bool DE>
__device__ __forceinline__ void proj_chi_point(const chomp_config& cfg, const ProjLayout& L,
                                               ProjDev* __restrict__ pd, double* __restrict__ tab,
                                               const DeSpline& de) {
  const int i = blockIdx.x, m = blockIdx.y;
  const double z = linspace_at(pd->me_z_min[m], pd->me_z_max[m], L.NC, i);
  double chi;
  if constexpr (DE) {
    EIntegrandDE f{pd->om0, pd->ol0, pd->or0, pd->H0, de};
    chi = romberg1<1>(f, 0.0, z, cfg.global_precision, cfg.cosmo_precision, cfg.divmax, nullptr);
  } else {
    EIntegrand f{pd->om0, pd->ol0, pd->or0, pd->H0};
    chi = romberg1<1>(f, 0.0, z, cfg.global_precision, cfg.cosmo_precision, cfg.divmax, nullptr);
  }
  if (threadIdx.x == 0) {
    tab[L.me_z[m] + i] = z;
    tab[L.me_chi[m] + i] = chi;
    tab[L.me_growth[m] + i] = growth_approx(pd->om0, pd->ol0, 1.0 / (1.0 + z)) / pd->growth_norm;
  }
}
template <bool DE>
__device__ __forceinline__ void proj_chi_body(const chomp_config& cfg, const ProjLayout& L,
                                              ProjDev* __restrict__ pd, double* __restrict__ tab,
                                              const DeSpline& de) {
  if (blockIdx.y == 3) { proj_chi_norm(cfg, pd); return; }
  proj_chi_point<DE>(cfg, L, pd, tab, de);
}
template <bool DE>
__global__ __launch_bounds__(64) void k_proj_chi(chomp_config cfg, ProjLayout L,
                                                 ProjDev* __restrict__ pd,
                                                 double* __restrict__ tab, DeSpline de) {
  proj_chi_body<DE>(cfg, L, pd, tab, de);
}

// The set axis (chomp_kernel_setup_sets: one projection set-up per cosmology of a design or
// chain, Kernel.set_cosmology of kernel.py:657-676 as one batch).  Every kernel of the set-up
// takes its cosmology from its ProjDev block and its tables from one slab of ProjLayout::total
// doubles, and none of their grids uses blockIdx.z: the *_sets forms run the same bodies with
// set blockIdx.z's block pd[blockIdx.z] and its slab, `stride` doubles after the previous set's.
// A tabulated redshift distribution of a set is read where its block's dist[w].pp points: into
// the sets' own arena of tables (ProjSets::d_pp, laid out by chomp_pp_plan.h), never behind the
// single set-up's slab.  Dark energy: a batch with a w0-wa cosmology runs the <true> forms of the
// two kernels that evaluate E(z) (k_proj_chi_sets, k_proj_window_sets) with DeSets, the sets'
// pressure tables and a slot per set; a batch without one runs the <false> forms, which are the
// kernels of a Lambda-CDM batch and ignore it.  kProjSetsMax: the sets of one call -- 1024 slabs
// of the default layout (3752 doubles) are 29 MiB; a grid's z dimension would allow 65535.
constexpr int kProjSetsMax = CHOMP_KERNEL_SETS_MAX;   // 1024
static_assert(kProjSetsMax <= 65535, "the set axis is a grid's z dimension");

// The pressure tables of a batch of sets: table t at tab + t * stride (de_stride(n) doubles, n =
// cosmo_npoints), and per set its table, or -1 for a Lambda-CDM set -- which then runs the
// arithmetic it runs in a pure Lambda-CDM batch.  The choice is uniform over a block.
struct DeSets {
  const double* tab;
  const int* slot;
  int stride, n;
};

// grid (NC, 4, n_set), block 64.
template <bool DE>
__global__ __launch_bounds__(64) void k_proj_chi_sets(chomp_config cfg, ProjLayout L,
                                                      ProjDev* __restrict__ pd,
                                                      double* __restrict__ tab, size_t stride,
                                                      DeSets de) {
  ProjDev* p = pd + blockIdx.z;
  double* t = tab + stride * blockIdx.z;
  if constexpr (DE) {
    if (blockIdx.y == 3) { proj_chi_norm(cfg, p); return; }
    const int slot = de.slot[blockIdx.z];
    if (slot >= 0)            // (no barrier on either side)
      proj_chi_point<true>(cfg, L, p, t, de_spline(de.tab + (size_t)slot * de.stride, de.n));
    else
      proj_chi_point<false>(cfg, L, p, t, DeSpline{nullptr, nullptr, 0});
  } else {
    proj_chi_body<false>(cfg, L, p, t, DeSpline{nullptr, nullptr, 0});
  }
}

// MultiEpoch lookups with the reference's range rules (cosmology.py:873-953).
struct MEView {
  const double *z, *chi, *pp_chi, *pp_z, *pp_g;   // z uniform, chi increasing
  int NC;
  double z_min, z_max;
  __device__ __forceinline__ double dz() const { return (z_max - z_min) / (double)(NC - 1); }
  __device__ __forceinline__ double comoving_distance(double zz) const {
    return (zz <= z_max && zz >= z_min) ? spline_eval_uniform(z_min, dz(), pp_chi, NC, zz) : 0.0;
  }
  __device__ __forceinline__ double redshift(double c) const {
    return spline_eval(chi, pp_z, NC, c);
  }
  __device__ __forceinline__ double growth_factor(double zz) const {
    return (zz <= z_max && zz >= z_min) ? spline_eval_uniform(z_min, dz(), pp_g, NC, zz) : 1.0;
  }
};
__device__ __forceinline__ MEView me_view(const ProjLayout& L, const ProjDev& pd,
                                          const double* tab, int m) {
  return MEView{tab + L.me_z[m], tab + L.me_chi[m], tab + L.me_pp_chi[m], tab + L.me_pp_z[m],
                tab + L.me_pp_g[m], L.NC, pd.me_z_min[m], pd.me_z_max[m]};
}

// Not-a-knot build of one spline per wavefront, in LDS: the lanes copy the knots in, the
// wavefronts run the parallel cyclic reduction of chomp_mass_kernels.h in lockstep and copy
// their coefficients out.  Every thread of the block calls it (block barriers); `mine`:
// this wavefront has a system.  lds: 11 n doubles per wavefront.
__device__ __forceinline__ void spline_build_staged(const double* x, const double* y, int n,
                                                    double* c, double* lds, bool mine) {
  const int lane = threadIdx.x & 63;
  double* lx = lds;
  double* ly = lx + n;
  double* lw = ly + n;            // [9n]
  if (mine)
    for (int i = lane; i < n; i += 64) { lx[i] = x[i]; ly[i] = y[i]; }
  __syncthreads();
  spline_build_pcr(lx, ly, n, c, lw, lane, 64, mine);
  __threadfence_block();
  __syncthreads();
}

// grid 3, block 192.  Splines of MultiEpoch m; blocks 1/2 then lay out window
// (m-1)'s chi grid (kernel.py:298-304, 438-441).
// (the body of k_proj_me_splines and k_proj_me_splines_sets)
__device__ __forceinline__ void proj_me_splines_body(const chomp_config& cfg, const ProjLayout& L,
                                                     ProjDev* __restrict__ pd,
                                                     double* __restrict__ tab) {
  extern __shared__ __align__(16) double sm_me[];      // 3 x 11 NC doubles
  const int m = blockIdx.x, NC = L.NC;
  const int wave = threadIdx.x >> 6;
  const double* sx = tab + (wave == 1 ? L.me_chi[m] : L.me_z[m]);
  const double* sy = tab + (wave == 0 ? L.me_chi[m] : (wave == 1 ? L.me_z[m] : L.me_growth[m]));
  double* sc = tab + (wave == 0 ? L.me_pp_chi[m] : (wave == 1 ? L.me_pp_z[m] : L.me_pp_g[m]));
  spline_build_staged(sx, sy, NC, sc, sm_me + (size_t)wave * 11 * NC, true);
  if (m == 0) return;
  const int w = m - 1;
  __shared__ double lim[2];
  if (threadIdx.x == 0) {
    const MEView me = me_view(L, *pd, tab, m);
    const double wp = cfg.window_precision;
    double cmin = me.comoving_distance(pd->w_z_min[w]);
    if (cmin < wp) cmin = wp;
    const double cmax = me.comoving_distance(pd->w_z_max[w]);
    double g = me.comoving_distance(pd->dist[w].z_min);
    if (g < wp) g = wp;
    pd->w_chi_min[w] = cmin;
    pd->w_chi_max[w] = cmax;
    pd->w_g_chi_min[w] = g;
    lim[0] = cmin;
    lim[1] = cmax;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < L.NWp; i += blockDim.x)
    tab[L.w_chi[w] + i] = linspace_at(lim[0], lim[1], L.NWp, i);
}
__global__ __launch_bounds__(192) void k_proj_me_splines(chomp_config cfg, ProjLayout L,
                                                         ProjDev* __restrict__ pd,
                                                         double* __restrict__ tab) {
  proj_me_splines_body(cfg, L, pd, tab);
}
// ... with the set axis: grid (3, 1, n_set), block 192.
__global__ __launch_bounds__(192) void k_proj_me_splines_sets(chomp_config cfg, ProjLayout L,
                                                              ProjDev* __restrict__ pd,
                                                              double* __restrict__ tab,
                                                              size_t stride) {
  proj_me_splines_body(cfg, L, pd + blockIdx.z, tab + stride * blockIdx.z);
}

// E0(z) of the projection's cosmology: Lambda-CDM, or (DE) with the pressure spline.
template <bool DE>
__device__ __forceinline__ double proj_E0(const ProjDev& pd, const DeSpline& de, double z) {
  if constexpr (DE) return E0_de(pd.om0, pd.ol0, pd.or0, de, z);
  else return E0_of(pd.om0, pd.ol0, pd.or0, z);
}

// Lensing-efficiency integrand, kernel.py:479-484.
template <bool DE>
struct LensIntegrand {
  const double *chi_knots, *pp_z;
  int NC;
  const DndzDev* d;
  double om0, ol0, or0, H0, chi0;
  DeSpline de;
  __device__ __forceinline__ double operator()(double c) const {
    const double z = spline_eval(chi_knots, pp_z, NC, c);
    double E0;
    if constexpr (DE) E0 = E0_de(om0, ol0, or0, de, z);
    else E0 = E0_of(om0, ol0, or0, z);
    const double dzdchi = H0 * sqrt(E0);
    return dzdchi * dndz_eval(*d, z) * (c - chi0) / c;
  }
};

// grid (NWp, 2), block 64: raw window function of window y at its x-th chi knot.
// (the body of k_proj_window and k_proj_window_sets, in its two parts: the staging of the
//  MultiEpoch's chi knots and z(chi) spline in `sm` and of the distribution in LDS, with the
//  body's only barrier, and the value, which alone looks at E)
__device__ __forceinline__ const DndzDev* proj_window_stage(const ProjLayout& L,
                                                            const ProjDev* __restrict__ pd,
                                                            const double* __restrict__ tab,
                                                            double* sm) {
  __shared__ DndzDev D;
  const int w = blockIdx.y, m = w + 1, NC = L.NC;
  copy_doubles(sm, tab + L.me_chi[m], NC);
  copy_doubles(sm + NC, tab + L.me_pp_z[m], 4 * (NC - 1));
  if (threadIdx.x == 0) D = pd->dist[w];
  __syncthreads();
  return &D;
}
template <bool DE>
__device__ __forceinline__ void proj_window_value(const chomp_config& cfg, const ProjLayout& L,
                                                  const ProjDev* __restrict__ pd,
                                                  double* __restrict__ tab, const DeSpline& de,
                                                  const double* sm, const DndzDev& D) {
  const int i = blockIdx.x, w = blockIdx.y, NC = L.NC;
  const double* chi_knots = sm;
  const double* pp_z = sm + NC;
  const double chi = tab[L.w_chi[w] + i];
  const double z = spline_eval(chi_knots, pp_z, NC, chi);
  double val;
  if (pd->wkind[w] == CHOMP_WINDOW_GALAXY) {                       // kernel.py:382-387
    val = pd->H0 * sqrt(proj_E0<DE>(*pd, de, z)) * dndz_eval(D, z);
  } else if (pd->wkind[w] == CHOMP_WINDOW_FLAT_CONVERGENCE) {      // kernel.py:507-513
    val = 3.0 / 2.0 * pd->om0 * (pd->H0 * pd->H0 * 1907.71);
  } else if (pd->wkind[w] == CHOMP_WINDOW_CONVERGENCE_DELTA) {     // kernel.py:541-556
    const double a = 1.0 / (1.0 + pd->w_z_max[w]);                 // (the source plane's a)
    const double cmax = pd->w_chi_max[w];
    double g = chi > cmax ? 0.0 : (cmax - chi) / cmax;
    g *= pd->H0 * pd->H0 * chi;
    val = 3.0 / 2.0 * pd->om0 * g / a;
  } else {                                                         // kernel.py:443-477
    const double a = 1.0 / (1.0 + z);
    double bound = chi;
    if (bound < pd->w_g_chi_min[w]) bound = pd->w_g_chi_min[w];
    double g = 0.0;
    if (!(bound <= cfg.window_precision)) {
      LensIntegrand<DE> f{chi_knots, pp_z, NC, &D, pd->om0, pd->ol0, pd->or0, pd->H0, chi, de};
      g = romberg1<1>(f, bound, pd->w_chi_max[w], cfg.global_precision,
                      cfg.window_precision, cfg.divmax, nullptr);
    }
    g *= pd->H0 * pd->H0 * chi;
    val = 3.0 / 2.0 * pd->om0 * g / a;
  }
  if (threadIdx.x == 0) tab[L.w_wf[w] + i] = val;
}
template <bool DE>
__device__ __forceinline__ void proj_window_body(const chomp_config& cfg, const ProjLayout& L,
                                                 const ProjDev* __restrict__ pd,
                                                 double* __restrict__ tab, const DeSpline& de) {
  extern __shared__ __align__(16) double sm[];
  const DndzDev* D = proj_window_stage(L, pd, tab, sm);
  proj_window_value<DE>(cfg, L, pd, tab, de, sm, *D);
}
template <bool DE>
__global__ __launch_bounds__(64) void k_proj_window(chomp_config cfg, ProjLayout L,
                                                    const ProjDev* __restrict__ pd,
                                                    double* __restrict__ tab, DeSpline de) {
  proj_window_body<DE>(cfg, L, pd, tab, de);
}
// ... with the set axis: grid (NWp, 2, n_set), block 64.  DE: as k_proj_chi_sets.
template <bool DE>
__global__ __launch_bounds__(64) void k_proj_window_sets(chomp_config cfg, ProjLayout L,
                                                         const ProjDev* __restrict__ pd,
                                                         double* __restrict__ tab, size_t stride,
                                                         DeSets de) {
  const ProjDev* p = pd + blockIdx.z;
  double* t = tab + stride * blockIdx.z;
  if constexpr (DE) {
    extern __shared__ __align__(16) double sm[];
    const DndzDev* D = proj_window_stage(L, p, t, sm);
    const int slot = de.slot[blockIdx.z];
    if (slot >= 0)            // (no barrier on either side)
      proj_window_value<true>(cfg, L, p, t, de_spline(de.tab + (size_t)slot * de.stride, de.n), sm, *D);
    else
      proj_window_value<false>(cfg, L, p, t, DeSpline{nullptr, nullptr, 0}, sm, *D);
  } else {
    proj_window_body<false>(cfg, L, p, t, DeSpline{nullptr, nullptr, 0});
  }
}

// Window lookup with the range rule of kernel.py:326-340 (uniform chi knots).
struct WindowView {
  const double* pp;
  int N;
  double chi_min, chi_max;
  __device__ __forceinline__ double operator()(double c) const {
    if (!(c >= chi_min && c <= chi_max)) return 0.0;
    return spline_eval_uniform(chi_min, (chi_max - chi_min) / (double)(N - 1), pp, N, c);
  }
};

// grid 1, block 128: window splines, then Kernel.__init__ scalars + _find_z_bar.
// (the body of k_proj_window_splines and k_proj_window_splines_sets)
__device__ __forceinline__ void proj_window_splines_body(const chomp_config& cfg,
                                                         const ProjLayout& L,
                                                         ProjDev* __restrict__ pd,
                                                         double* __restrict__ tab) {
  extern __shared__ __align__(16) double sm_w[];       // 2 x 11 NWp doubles
  const int wave = threadIdx.x >> 6;
  spline_build_staged(tab + L.w_chi[wave], tab + L.w_wf[wave], L.NWp, tab + L.w_pp[wave],
                      sm_w + (size_t)wave * 11 * L.NWp, true);
  const MEView me = me_view(L, *pd, tab, 0);
  const WindowView wa{tab + L.w_pp[0], L.NWp, pd->w_chi_min[0], pd->w_chi_max[0]};
  const WindowView wb{tab + L.w_pp[1], L.NWp, pd->w_chi_min[1], pd->w_chi_max[1]};
  const double z_min = pd->w_z_min[0] > pd->w_z_min[1] ? pd->w_z_min[0] : pd->w_z_min[1];
  const double z_max = pd->w_z_max[0] < pd->w_z_max[1] ? pd->w_z_max[0] : pd->w_z_max[1];
  for (int i = threadIdx.x; i < L.NKT; i += blockDim.x)
    tab[L.k_ln + i] = linspace_at(pd->ln_kt_min, pd->ln_kt_max, L.NKT, i);
  // _find_z_bar (:635-639): argmax over linspace(z_min, z_max, NKT) of W_a W_b D^2 --
  // numpy.argmax: the first of equal maxima.  One candidate per thread, then thread 0 scans
  // the values in order.
  __shared__ double cand_v[128];
  for (int base = 0; base < L.NKT; base += 128) {        // (NKT <= 128 in any sensible set-up)
    const int i = base + (int)threadIdx.x;
    if (i < L.NKT && i < base + 128) {
      const double z = linspace_at(z_min, z_max, L.NKT, i);
      const double chi = me.comoving_distance(z);
      const double D = me.growth_factor(me.redshift(chi));
      cand_v[threadIdx.x] = wa(chi) * wb(chi) * D * D;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double best = base == 0 ? -INFINITY : pd->D_zbar;  // (D_zbar: scratch for the running maximum)
      double zb = base == 0 ? z_min : pd->z_bar;
      for (int q = 0; q < 128 && base + q < L.NKT; ++q)
        if (cand_v[q] > best) { best = cand_v[q]; zb = linspace_at(z_min, z_max, L.NKT, base + q); }
      pd->z_bar = zb;
      pd->D_zbar = best;
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  pd->z_min = z_min;                                               // kernel.py:595-598
  pd->z_max = z_max;
  const double c0 = me.comoving_distance(z_min);
  pd->chi_min = cfg.window_precision > c0 ? cfg.window_precision : c0;   // :610-612
  pd->chi_max = me.comoving_distance(z_max);
  pd->D_zbar = me.growth_factor(pd->z_bar);                        // correlation.py:94
}
__global__ __launch_bounds__(128) void k_proj_window_splines(chomp_config cfg, ProjLayout L,
                                                             ProjDev* __restrict__ pd,
                                                             double* __restrict__ tab) {
  proj_window_splines_body(cfg, L, pd, tab);
}
// ... with the set axis: grid (1, 1, n_set), block 128 -- the single-block kernel of a set-up,
// one block per set here.
__global__ __launch_bounds__(128) void k_proj_window_splines_sets(chomp_config cfg, ProjLayout L,
                                                                  ProjDev* __restrict__ pd,
                                                                  double* __restrict__ tab,
                                                                  size_t stride) {
  proj_window_splines_body(cfg, L, pd + blockIdx.z, tab + stride * blockIdx.z);
}

// LDS-resident view of everything a projection integrand needs.
struct ProjLds {
  MEView me;
  WindowView wa, wb;
  const BesselTab* bess;
  // Carve `sm` and copy the tables in (all threads; barrier afterwards).
  __device__ __forceinline__ double* stage(const ProjLayout& L, const ProjDev& pd,
                                           const double* tab, double* sm) {
    const int NC = L.NC, NW = L.NWp;
    double* chi = sm;                 // [NC]
    double* pp_z = chi + NC;          // [4(NC-1)]
    double* pp_g = pp_z + 4 * (NC - 1);
    double* pa = pp_g + 4 * (NC - 1); // [4(NW-1)]
    double* pb = pa + 4 * (NW - 1);
    copy_doubles(chi, tab + L.me_chi[0], NC);
    copy_doubles(pp_z, tab + L.me_pp_z[0], 4 * (NC - 1));
    copy_doubles(pp_g, tab + L.me_pp_g[0], 4 * (NC - 1));
    copy_doubles(pa, tab + L.w_pp[0], 4 * (NW - 1));
    copy_doubles(pb, tab + L.w_pp[1], 4 * (NW - 1));
    me = MEView{nullptr, chi, nullptr, pp_z, pp_g, NC, pd.me_z_min[0], pd.me_z_max[0]};
    wa = WindowView{pa, NW, pd.w_chi_min[0], pd.w_chi_max[0]};
    wb = WindowView{pb, NW, pd.w_chi_min[1], pd.w_chi_max[1]};
    return pb + 4 * (NW - 1);
  }
  static __host__ __device__ int doubles(const ProjLayout& L) {
    return L.NC + 8 * (L.NC - 1) + 8 * (L.NWp - 1);
  }
};

// kernel.py:707-712 (J0) / 833-839 (J2)
template <int ORDER>
struct KernelIntegrand {
  const ProjLds* P;
  double ktheta;
  __device__ __forceinline__ double operator()(double chi) const {
    const double D = P->me.growth_factor(P->me.redshift(chi));
    return P->wa(chi) * P->wb(chi) * D * D * bessel_j<ORDER>(ktheta * chi, *P->bess);
  }
};

// grid NKT, block 256: one kernel knot per block.
// (the body of k_proj_kernel_knots and k_proj_kernel_knots_sets)
__device__ __forceinline__ void proj_kernel_knots_body(const chomp_config& cfg, const ProjLayout& L,
                                                       const ProjDev* __restrict__ pdg,
                                                       double* __restrict__ tab,
                                                       const BesselTab* __restrict__ bess_g,
                                                       const double* __restrict__ ln_in,
                                                       double* __restrict__ out) {
  // ln_in == nullptr: the 50 knots of the spline table (Kernel._initialize_spline);
  // otherwise Kernel.raw_kernel at the caller's ln(k theta), results into `out`.
  extern __shared__ __align__(16) double sm[];
  __shared__ ProjDev pd;
  __shared__ BesselTab B;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&pd), reinterpret_cast<const double*>(pdg), kProjDoubles);
  copy_doubles(reinterpret_cast<double*>(&B), reinterpret_cast<const double*>(bess_g),
               (int)(sizeof(BesselTab) / sizeof(double)));
  __syncthreads();
  ProjLds P;
  P.stage(L, pd, tab, sm);
  P.bess = &B;
  __syncthreads();
  const int i = blockIdx.x;
  const double ktheta = exp(ln_in ? ln_in[i] : tab[L.k_ln + i]);
  double chi_max = pd.j_limit / ktheta;                            // kernel.py:689-691
  if (chi_max >= pd.chi_max) chi_max = pd.chi_max;
  int level = 0;
  double v;
  if (pd.order == 0) {
    KernelIntegrand<0> f{&P, ktheta};
    v = romberg1<4>(f, pd.chi_min, chi_max, cfg.global_precision, cfg.kernel_precision,
                    cfg.divmax, red, &level);
  } else {
    KernelIntegrand<2> f{&P, ktheta};
    v = romberg1<4>(f, pd.chi_min, chi_max, cfg.global_precision, cfg.kernel_precision,
                    cfg.divmax, red, &level);
  }
  if (threadIdx.x == 0) {
    if (out) {
      out[i] = v;
    } else {
      tab[L.k_arr + i] = v;
      tab[L.k_lev + i] = (double)level;
    }
  }
}
__global__ __launch_bounds__(256) void k_proj_kernel_knots(chomp_config cfg, ProjLayout L,
                                                           const ProjDev* __restrict__ pdg,
                                                           double* __restrict__ tab,
                                                           const BesselTab* __restrict__ bess_g,
                                                           const double* __restrict__ ln_in,
                                                           double* __restrict__ out) {
  proj_kernel_knots_body(cfg, L, pdg, tab, bess_g, ln_in, out);
}
// ... with the set axis: grid (NKT, 1, n_set), block 256; the knots of the spline tables only.
__global__ __launch_bounds__(256) void k_proj_kernel_knots_sets(chomp_config cfg, ProjLayout L,
                                                                const ProjDev* __restrict__ pdg,
                                                                double* __restrict__ tab,
                                                                const BesselTab* __restrict__ bess_g,
                                                                size_t stride) {
  proj_kernel_knots_body(cfg, L, pdg + blockIdx.z, tab + stride * blockIdx.z, bess_g, nullptr,
                         nullptr);
}

// (the body of k_proj_kernel_spline and k_proj_kernel_spline_sets)
__device__ __forceinline__ void proj_kernel_spline_body(const ProjLayout& L,
                                                        double* __restrict__ tab) {
  extern __shared__ __align__(16) double sm_k[];       // 11 NKT doubles
  spline_build_staged(tab + L.k_ln, tab + L.k_arr, L.NKT, tab + L.k_pp, sm_k, threadIdx.x < 64);
}
__global__ void k_proj_kernel_spline(ProjLayout L, double* __restrict__ tab) {
  proj_kernel_spline_body(L, tab);
}
// ... with the set axis: grid (1, 1, n_set), block 64.
__global__ void k_proj_kernel_spline_sets(ProjLayout L, double* __restrict__ tab, size_t stride) {
  proj_kernel_spline_body(L, tab + stride * blockIdx.z);
}

// Kernel.kernel(ln_ktheta), kernel.py:714-729 (uniform ln(k theta) knots).
struct KernelView {
  const double* pp;
  int N;
  double lo, hi;
  __device__ __forceinline__ double operator()(double x) const {
    const double dx = (hi - lo) / (double)(N - 1);
    const double inv_dx = (double)(N - 1) / (hi - lo);    // (both loop-invariant for a caller)
    if (x < lo) return pp_poly(pp, 0, 0.0);
    if (x <= hi) {
      int i = (int)floor((x - lo) * inv_dx);
      i = i < 0 ? 0 : (i > N - 2 ? N - 2 : i);
      return pp_poly(pp, i, x - (lo + dx * (double)i));
    }
    return 0.0;
  }
};

__global__ void k_kernel_eval(ProjLayout L, const ProjDev* __restrict__ pd,
                              const double* __restrict__ tab, const double* __restrict__ x,
                              int n, double* __restrict__ out) {
  const KernelView K{tab + L.k_pp, L.NKT, pd->ln_kt_min, pd->ln_kt_max};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = K(x[i]);
}

__global__ void k_me_eval(ProjLayout L, const ProjDev* __restrict__ pd,
                          const double* __restrict__ tab, int what,
                          const double* __restrict__ x, int n, double* __restrict__ out) {
  const MEView me = me_view(L, *pd, tab, 0);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double v = x[i];
    out[i] = what == CHOMP_ME_CHI_OF_Z ? me.comoving_distance(v)
             : what == CHOMP_ME_Z_OF_CHI ? me.redshift(v) : me.growth_factor(v);
  }
}

__global__ void k_window_eval(ProjLayout L, const ProjDev* __restrict__ pd,
                              const double* __restrict__ tab, int w,
                              const double* __restrict__ x, int n, double* __restrict__ out) {
  const WindowView W{tab + L.w_pp[w], L.NWp, pd->w_chi_min[w], pd->w_chi_max[w]};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = W(x[i]);
}

// correlation.py:270-275
template <bool HF, bool BAO = false>   // HF: a HaloFit spectrum; BAO: wiggle transfer function
struct WthetaIntegrand {
  const PowerEval* P;
  const KernelView* K;
  double theta, inv_D2, ln_theta;
  __device__ __forceinline__ double operator()(double ln_k) const {
    const double k = exp(ln_k);
    return k * k / (2.0 * kPi) * P->template at_ln<HF, BAO>(ln_k, k) * inv_D2 * (*K)(ln_k + ln_theta);
  }
};

// Every theta integrates over the same ln k range, so all of them visit the same Romberg
// nodes and the theta-independent factor k^2/(2 pi) P(k)/D_z^2 of the integrand is
// tabulated once per call on the level-LT grid (level-major, as the sigma(R) and halo node
// tables): per node a theta block then only evaluates the kernel spline.
// grid ceil((2^LT + 1) / (256 kWthNodesPerThread)), block 256.
constexpr int kWthetaTabLevel = 20;     // 2^20 + 1 doubles = 8 MiB: the default divmax
constexpr int kWthNodesPerThread = 8;
// (the body of k_wtheta_nodes and k_wtheta_nodes_epochs; bx: the block's index along the nodes)
template <bool HF, bool BAO>
__device__ __forceinline__ void wth_nodes_body(const chomp_config& cfg, const TabLayout& HL,
                                               const Epoch* __restrict__ epochs, int e,
                                               const double* __restrict__ htab, int which,
                                               double k_min, double k_max, double D_z, int LT,
                                               double* __restrict__ nodes, unsigned bx) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  PowerEval P;
  P.stage(cfg, HL, &E, htab + (size_t)e * HL.stride, which, sm);
  __syncthreads();
  P.template finish_t<BAO>();
  const double a = log(k_min), b = log(k_max), intrange = b - a;
  // (kWthNodesPerThread nodes per thread: a block stages 5 KB of spline tables before its first
  //  node -- at one node per thread, 4097 blocks of it, that staging was most of the 33 us)
#pragma unroll 2
  for (int r = 0; r < kWthNodesPerThread; ++r) {
    const long idx = ((long)bx * kWthNodesPerThread + r) * blockDim.x + threadIdx.x;
    if (idx > (1L << LT)) return;
    double x;
    if (idx < 2) {
      x = idx == 0 ? a : b;
    } else {                                   // the node arithmetic of chomp_romberg.h
      const unsigned m = (unsigned)(idx - 1);
      const int lev = 32 - __builtin_clz(m);
      const long j = (long)m - (1L << (lev - 1));
      const double h = ldexp(intrange, 1 - lev);
      x = (a + 0.5 * h) + h * (double)j;
    }
    const double k = exp(x);
    nodes[idx] = k * k / (2.0 * kPi) * P.template at_ln<HF, BAO>(x, k) * (1.0 / (D_z * D_z));
  }
}
template <bool HF, bool BAO>
__global__ __launch_bounds__(256) void k_wtheta_nodes(chomp_config cfg, TabLayout HL,
                                                      const Epoch* __restrict__ epochs, int e,
                                                      const double* __restrict__ htab, int which,
                                                      double k_min, double k_max, double D_z,
                                                      int LT, double* __restrict__ nodes) {
  wth_nodes_body<HF, BAO>(cfg, HL, epochs, e, htab, which, k_min, k_max, D_z, LT, nodes, blockIdx.x);
}
// ... with an epoch axis (chomp_wtheta_epochs): grid (as k_wtheta_nodes, E), block 256; row
// blockIdx.y tabulates epoch e0 + blockIdx.y into its own table, `stride` doubles after the
// previous one.  Every block stages its own epoch exactly as k_wtheta_nodes does.
template <bool HF, bool BAO>
__global__ __launch_bounds__(256) void k_wtheta_nodes_epochs(chomp_config cfg, TabLayout HL,
                                                             const Epoch* __restrict__ epochs, int e0,
                                                             const double* __restrict__ htab, int which,
                                                             double k_min, double k_max, double D_z,
                                                             int LT, double* __restrict__ nodes,
                                                             size_t stride) {
  wth_nodes_body<HF, BAO>(cfg, HL, epochs, e0 + (int)blockIdx.y, htab, which, k_min, k_max, D_z, LT,
                          nodes + stride * blockIdx.y, blockIdx.x);
}
// ... with an epoch axis whose rows have their own growth factor (chomp_wtheta_sets: row
// blockIdx.y is the epoch of one cosmology, D_z[blockIdx.y] the growth at its z_bar).
template <bool HF, bool BAO>
__global__ __launch_bounds__(256) void k_wtheta_nodes_sets(chomp_config cfg, TabLayout HL,
                                                           const Epoch* __restrict__ epochs, int e0,
                                                           const double* __restrict__ htab, int which,
                                                           double k_min, double k_max,
                                                           const double* __restrict__ D_z, int LT,
                                                           double* __restrict__ nodes, size_t stride) {
  wth_nodes_body<HF, BAO>(cfg, HL, epochs, e0 + (int)blockIdx.y, htab, which, k_min, k_max,
                          D_z[blockIdx.y], LT, nodes + stride * blockIdx.y, blockIdx.x);
}

// correlation.py:270-275 from the node table (levels <= LT), directly beyond
template <bool HF, bool BAO>
struct WthetaTabIntegrand {
  const double* nodes;
  int LT;
  WthetaIntegrand<HF, BAO> direct;
  __device__ __forceinline__ void operator()(double ln_k, double (&out)[1], int lev,
                                             long j) const {
    if (lev <= LT) {
      const long idx = lev == 0 ? j : 1 + (1L << (lev - 1)) + j;
      out[0] = nodes[idx] * (*direct.K)(ln_k + direct.ln_theta);
    } else {
      out[0] = direct(ln_k);
    }
  }
};

// grid n_theta, block 64 * kWthetaNW: one theta per workgroup.  The integrals of large
// theta run to 2^18..2^20 nodes (the kernel oscillates in ln k theta) and set the launch's
// duration, hence the wide group.
constexpr int kWthetaNW = 16;
// (the body of k_wtheta and k_wtheta_epochs: theta[0] into out[0])
template <bool HF, bool BAO>
__device__ __forceinline__ void wth_direct_body(const chomp_config& cfg, const TabLayout& HL,
                                                const ProjLayout& L, const Epoch* __restrict__ epochs,
                                                int e, const double* __restrict__ htab, int which,
                                                const ProjDev* __restrict__ pd,
                                                const double* __restrict__ ptab, double k_min,
                                                double k_max, double D_z,
                                                const double* __restrict__ theta,
                                                double* __restrict__ out,
                                                const double* __restrict__ nodes, int LT) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ double red[romberg_scratch<kWthetaNW, 2>()];
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  PowerEval P;
  P.stage(cfg, HL, &E, htab + (size_t)e * HL.stride, which, sm);
  double* kpp = sm + 12 * (HL.NK - 1);
  copy_doubles(kpp, ptab + L.k_pp, 4 * (L.NKT - 1));
  __syncthreads();
  P.template finish_t<BAO>();
  const KernelView K{kpp, L.NKT, pd->ln_kt_min, pd->ln_kt_max};
  const double th = theta[0];
  WthetaTabIntegrand<HF, BAO> f{nodes, LT, {&P, &K, th, 1.0 / (D_z * D_z), log(th)}};
  const RombergOut<1> r = romberg_group<kWthetaNW, 1>(f, log(k_min), log(k_max),
                                                      cfg.global_precision, cfg.corr_precision,
                                                      cfg.divmax, red);
  if (threadIdx.x == 0) out[0] = r.value[0];
}
template <bool HF, bool BAO>
__global__ __launch_bounds__(64 * kWthetaNW) void k_wtheta(chomp_config cfg, TabLayout HL, ProjLayout L,
                                                const Epoch* __restrict__ epochs, int e,
                                                const double* __restrict__ htab, int which,
                                                const ProjDev* __restrict__ pd,
                                                const double* __restrict__ ptab, double k_min,
                                                double k_max, double D_z,
                                                const double* __restrict__ theta,
                                                double* __restrict__ out,
                                                const double* __restrict__ nodes, int LT) {
  wth_direct_body<HF, BAO>(cfg, HL, L, epochs, e, htab, which, pd, ptab, k_min, k_max, D_z,
                           theta + blockIdx.x, out + blockIdx.x, nodes, LT);
}
// ... with an epoch axis: grid (n_theta, E), block 64 * kWthetaNW; row blockIdx.y integrates
// epoch e0 + blockIdx.y from its own node table into out[blockIdx.y * n_theta + blockIdx.x].
template <bool HF, bool BAO>
__global__ __launch_bounds__(64 * kWthetaNW) void k_wtheta_epochs(
    chomp_config cfg, TabLayout HL, ProjLayout L, const Epoch* __restrict__ epochs, int e0,
    const double* __restrict__ htab, int which, const ProjDev* __restrict__ pd,
    const double* __restrict__ ptab, double k_min, double k_max, double D_z,
    const double* __restrict__ theta, double* __restrict__ out, const double* __restrict__ nodes,
    int LT, size_t stride) {
  wth_direct_body<HF, BAO>(cfg, HL, L, epochs, e0 + (int)blockIdx.y, htab, which, pd, ptab, k_min,
                           k_max, D_z, theta + blockIdx.x,
                           out + (size_t)blockIdx.y * gridDim.x + blockIdx.x,
                           nodes + stride * blockIdx.y, LT);
}
// ... with an epoch axis whose rows have their own projection set (chomp_wtheta_sets): row
// blockIdx.y integrates epoch e0 + blockIdx.y against pd[blockIdx.y] and its slab of tables,
// `pstride` doubles after the previous set's, with growth D_z[blockIdx.y].
template <bool HF, bool BAO>
__global__ __launch_bounds__(64 * kWthetaNW) void k_wtheta_sets(
    chomp_config cfg, TabLayout HL, ProjLayout L, const Epoch* __restrict__ epochs, int e0,
    const double* __restrict__ htab, int which, const ProjDev* __restrict__ pd,
    const double* __restrict__ ptab, size_t pstride, double k_min, double k_max,
    const double* __restrict__ D_z, const double* __restrict__ theta, double* __restrict__ out,
    const double* __restrict__ nodes, int LT, size_t stride) {
  wth_direct_body<HF, BAO>(cfg, HL, L, epochs, e0 + (int)blockIdx.y, htab, which, pd + blockIdx.y,
                           ptab + pstride * blockIdx.y, k_min, k_max, D_z[blockIdx.y],
                           theta + blockIdx.x, out + (size_t)blockIdx.y * gridDim.x + blockIdx.x,
                           nodes + stride * blockIdx.y, LT);
}

// ---------------------------------------------------------------------------
// w(theta) without visiting the nodes.  The kernel K(ln k + ln theta) is a 50-knot cubic
// spline -- a piecewise cubic -- and the rest of the integrand is the theta-independent node
// table g_j of k_wtheta_nodes.  Over the nodes that fall into one piece of the spline the
// level sum is therefore sum_j g_j (c0 + c1 d_j + c2 d_j^2 + c3 d_j^3), d_j = x_j + ln theta -
// X_i: a combination of the MOMENTS sum g_j u_j^q (q = 0..3) of the node table over an index
// range, and those come from prefix sums that do not depend on theta.  A Romberg level of
// 2^19 nodes then costs a theta one prefix lookup per spline knot (50) instead of 2^19 spline
// evaluations -- the same sum up to rounding, SciPy's rows and stopping test unchanged.
//
// Conditioning: a moment about a far origin would be recombined with large cancellation
// ((x - X)^3 from powers of x ~ 6), so the ln k range is cut into segments about as wide as a
// spline piece (never narrower: a piece then meets at most two of them), each with its own
// origin, and the prefix sums restart at every segment.  Recombination shifts a segment's
// moments by |delta| <= two piece widths.  Segment membership is integer arithmetic on the node
// index (wth_seg_of / WthSeg::start), so that both kernels agree on it exactly.
// Measured agreement with the node-by-node kernel: tests/test_gpu_projection.py.
// ---------------------------------------------------------------------------
constexpr int kWthItems = 8;                 // nodes per thread and tile of k_wtheta_moments

// Node j of a level (x_j = a + (b - a)(j + 1/2) / n, n = 2^(lev - 1)) belongs to the segment its
// abscissa falls into, m = floor((2 j + 1) nseg / 2^lev): 0 <= x_j - O_m < the segment width.
__device__ __forceinline__ int wth_seg_of(long j, int nseg, int lev) {
  return (int)(((2 * j + 1) * nseg) >> lev);
}
// ... and the first node of segment m, the same statement solved for j (m = nseg: n):
// ceil((m 2^lev - nseg) / (2 nseg)), by a floating-point quotient made exact by three integer
// corrections (a 64-bit integer division costs a wavefront a few hundred instructions).
struct WthSeg {
  int nseg;
  double inv_q, a, seg_w;
  __device__ __forceinline__ WthSeg(int nseg_, double a_, double b_)
      : nseg(nseg_), inv_q(0.5 / (double)nseg_), a(a_), seg_w((b_ - a_) / (double)nseg_) {}
  __device__ __forceinline__ long start(int m, int lev) const {
    const long p = ((long)m << lev) - nseg, q = 2L * nseg;
    if (p <= 0) return 0;
    long c = (long)((double)p * inv_q) - 1;                // <= floor(p / q), short by 2 at most
    c += (c * q < p) ? 1 : 0;
    c += (c * q < p) ? 1 : 0;
    c += (c * q < p) ? 1 : 0;
    return c;
  }
  __device__ __forceinline__ double origin(int m) const { return a + seg_w * (double)m; }
};

// grid (nseg, LT, kWthParts), block 256: inclusive prefix sums of g_j u_j^q, q = 0..3, u_j = x_j
// - O_m, over the nodes of segment m of level blockIdx.y + 1 -- KEPT only where k_wtheta_fast
// cannot cheaply rebuild them: at every kWthItems-th node (rec: the record of node j with
// (j + 1) % kWthItems == 0 lives at index (2^(lev-1) + j + 1) / kWthItems, a heap over the levels;
// a look-up adds the <= kWthItems - 1 nodes behind the record itself) and at the last node of the
// segment (segtot[(lev nseg + m)]).  Four moments for every node were 32 MiB of writes per call
// (0.18 of the HBM rate for a scan); these are 4 MiB.  A long segment (deep levels) is cut into
// up to kWthParts parts, one block each: a part first sums the moments of the parts before it (a
// plain strided reduction of nodes already in L2) for its carry, then scans its own tiles of
// 256 * kWthItems nodes.  No block waits for another.
constexpr int kWthParts = 8;
__host__ __device__ inline size_t wth_rec_count(int LT) { return ((size_t)1 << LT) / kWthItems + 2; }

// The epoch axis (chomp_wtheta_epochs: one w(theta) per HOD of a design or chain).  The epochs of
// a call share everything but the node table g_j, so a chunk of E epochs keeps E copies of the
// single-epoch scratch -- node table, moment records, segment totals, in that order -- one after
// another in the context's w(theta) work buffer at a fixed stride (wth_epoch_stride: 12 MiB at
// the default divmax = 20), and the *_epochs kernels address epoch i at i * stride.  A call
// works its epochs off in chunks of kWthEpochChunk = 16, which bounds the buffer at 192 MiB
// however many epochs are asked for, while a chunk still fills the device (16 x 513 node blocks,
// 16 x n_theta Romberg blocks).  CHOMP_TUNE_WTHETA_EPOCH_CHUNK overrides the chunk (at most
// kWthEpochChunkMax, the 3 GiB mark).  Per (theta, epoch) the arithmetic is the single-epoch
// kernels': both sets of __global__s call the same bodies.
constexpr int kWthEpochChunk = 16;
constexpr int kWthEpochChunkMax = 256;
// The doubles of one epoch's scratch (fast: with the records and totals of the moment route);
// even, so that every epoch's records stay 16-byte aligned.
inline size_t wth_epoch_stride(int LT, int nseg, bool fast) {
  const size_t n_nodes = ((size_t)1 << LT) + 1;
  const size_t n = n_nodes + 1 + (fast ? 4 * wth_rec_count(LT) + 4 * (size_t)(LT + 1) * (size_t)nseg + 2 : 0);
  return (n + 1) & ~(size_t)1;
}

// The host's plan of the w(theta) scratch and launches -- what chomp_wtheta, chomp_wtheta_epochs,
// chomp_wtheta_sets and (its node-table part) chomp_xi3d_epochs size, place and launch by.  One
// epoch's scratch is wth_epoch_stride doubles: the node table, then from rec_at the moment
// records and from tot_at the segments' totals; a chunk keeps one such scratch per epoch.
struct WthPlan {
  int LT, nseg;                     // levels within the node table; segments of the moment route
  bool fast;                        // the moment route (k_wtheta_moments + k_wtheta_fast)
  size_t n_nodes, stride, rec_at, tot_at;
  size_t sh_nodes, sh;              // dynamic LDS of k_wtheta_nodes, of k_wtheta
  unsigned gnodes;                  // blocks of k_wtheta_nodes
};

// (the scratch of given LT, nseg and route; NK, NKT: the knots of P(k) and of the kernel spline)
inline WthPlan wth_plan_of(int LT, int nseg, bool fast, int NK = 1, int NKT = 1) {
  WthPlan P;
  P.LT = LT; P.nseg = nseg; P.fast = fast;
  P.n_nodes = ((size_t)1 << LT) + 1;
  P.stride = wth_epoch_stride(LT, nseg, fast);
  P.rec_at = P.n_nodes + (P.n_nodes & 1);   // 16-byte aligned records
  P.tot_at = P.rec_at + 4 * wth_rec_count(LT);
  P.sh_nodes = (size_t)(12 * (NK - 1)) * sizeof(double);
  P.sh = (size_t)(12 * (NK - 1) + 4 * (NKT - 1)) * sizeof(double);
  P.gnodes = (unsigned)((P.n_nodes + 256 * kWthNodesPerThread - 1) / (256 * kWthNodesPerThread));
  return P;
}

// The plan of a call: every level within the node table by the moment route (segments about as
// wide as -- never narrower than -- a piece of the kernel spline) unless `direct`
// (CHOMP_TUNE_WTHETA_DIRECT), a divmax beyond the table or a long kernel spline rule it out.
inline WthPlan wth_plan(int divmax, int NK, const ProjLayout& L, double ln_kt_min, double ln_kt_max,
                        double k_min, double k_max, long long direct) {
  const double dxK = (ln_kt_max - ln_kt_min) / (double)(L.NKT - 1);
  int nseg = dxK > 0.0 ? (int)std::floor((std::log(k_max) - std::log(k_min)) / dxK) : 1;
  nseg = nseg < 1 ? 1 : (nseg > 65535 ? 65535 : nseg);
  const bool fast = direct <= 0 && divmax <= kWthetaTabLevel && L.NKT <= 63;
  return wth_plan_of(divmax < kWthetaTabLevel ? divmax : kWthetaTabLevel, nseg, fast, NK, L.NKT);
}

// (the body of k_wtheta_moments and k_wtheta_moments_epochs; part: the block's part of its segment)
__device__ __forceinline__ void wth_moments_body(const double* __restrict__ nodes, int LT, int nseg,
                                                 double a, double b, double* __restrict__ rec,
                                                 double* __restrict__ segtot, unsigned part) {
  __shared__ double wtot[2][4][4];
  __shared__ double ctot[4][4];
  const int m = blockIdx.x, lev = blockIdx.y + 1, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long n = 1L << (lev - 1);
  const WthSeg G(nseg, a, b);
  const long j0 = G.start(m, lev), j1 = G.start(m + 1, lev);
  constexpr long kTile = 256L * kWthItems;
  const long len = j1 - j0;
  long parts = (len + kTile - 1) / kTile;
  parts = parts > kWthParts ? kWthParts : parts;
  if ((long)part >= parts) return;                          // (block-uniform; also len == 0)
  const long plen = (len + parts - 1) / parts;
  const long p0 = j0 + plen * part;
  const long p1 = p0 + plen < j1 ? p0 + plen : j1;
  const double h = (b - a) / (double)n, lox = a + 0.5 * h;
  const double O = G.origin(m);
  const long base = 1 + n;                                  // level-major index of j = 0
  static_assert((kWthItems & (kWthItems - 1)) == 0, "records at a power-of-two spacing");
  double carry[4] = {0.0, 0.0, 0.0, 0.0};
  if (p0 > j0) {                                            // (block-uniform)
    double r[4] = {0.0, 0.0, 0.0, 0.0};
    for (long jj = j0 + t; jj < p0; jj += 256 * 8) {       // (eight loads in flight)
      double g[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const long j = jj + 256L * i;
        g[i] = j < p0 ? nodes[base + j] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const double u = (lox + h * (double)(jj + 256L * i)) - O;
        r[0] += g[i]; r[1] += g[i] * u; r[2] += g[i] * (u * u); r[3] += g[i] * (u * u * u);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double x = wave_sum(r[q]);
      if (lane == 0) ctot[w][q] = x;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) carry[q] = (ctot[0][q] + ctot[1][q]) + (ctot[2][q] + ctot[3][q]);
  }
  int buf = 0;
  for (long tile = p0; tile < p1; tile += kTile, buf ^= 1) {
    const long c0 = tile + (long)t * kWthItems;
    double v[kWthItems][4];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < kWthItems; ++i) {
      const long j = c0 + i;
      if (j < p1) {
        const double g = nodes[base + j], u = (lox + h * (double)j) - O;
        s[0] += g; s[1] += g * u; s[2] += g * (u * u); s[3] += g * (u * u * u);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) v[i][q] = s[q];
    }
    double inc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) inc[q] = s[q];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double y = __shfl_up(inc[q], off, 64);
        if (lane >= off) inc[q] += y;
      }
    }
    if (lane == 63) {
#pragma unroll
      for (int q = 0; q < 4; ++q) wtot[buf][w][q] = inc[q];
    }
    __syncthreads();
    double pre[4], next[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double before = 0.0, all = 0.0;
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        const double x = wtot[buf][ww][q];
        if (ww < w) before += x;
        all += x;
      }
      pre[q] = carry[q] + before + (inc[q] - s[q]);
      next[q] = carry[q] + all;
    }
    // of this thread's kWthItems consecutive nodes exactly one closes a record; the segment's
    // last node also leaves the segment's total
    const int i_rec = (int)((kWthItems - ((c0 + 1) & (kWthItems - 1))) & (kWthItems - 1));
#pragma unroll
    for (int i = 0; i < kWthItems; ++i) {
      const long j = c0 + i;
      if (j < p1 && (i == i_rec || j == j1 - 1)) {
        const double2 lo2 = make_double2(pre[0] + v[i][0], pre[1] + v[i][1]);
        const double2 hi2 = make_double2(pre[2] + v[i][2], pre[3] + v[i][3]);
        if (i == i_rec) {
          double2* o = reinterpret_cast<double2*>(rec + 4 * ((n + j + 1) / kWthItems));
          o[0] = lo2; o[1] = hi2;
        }
        if (j == j1 - 1) {
          double2* o = reinterpret_cast<double2*>(segtot + 4 * ((size_t)lev * nseg + m));
          o[0] = lo2; o[1] = hi2;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) carry[q] = next[q];
  }
}
__global__ __launch_bounds__(256) void k_wtheta_moments(const double* __restrict__ nodes, int LT,
                                                        int nseg, double a, double b,
                                                        double* __restrict__ rec,
                                                        double* __restrict__ segtot) {
  wth_moments_body(nodes, LT, nseg, a, b, rec, segtot, blockIdx.z);
}
// ... with an epoch axis: grid (nseg, LT, kWthParts * E), block 256; blockIdx.z = part +
// kWthParts * epoch, every epoch's node table, records and segment totals `stride` doubles after
// the previous epoch's.
__global__ __launch_bounds__(256) void k_wtheta_moments_epochs(const double* __restrict__ nodes,
                                                               int LT, int nseg, double a, double b,
                                                               double* __restrict__ rec,
                                                               double* __restrict__ segtot,
                                                               size_t stride) {
  const size_t off = stride * (blockIdx.z / kWthParts);
  wth_moments_body(nodes + off, LT, nseg, a, b, rec + off, segtot + off, blockIdx.z % kWthParts);
}

// Moments of the whole of segment m (0 for an empty one).
__device__ __forceinline__ void wth_seg_total(const double* __restrict__ segtot, int m,
                                              const WthSeg& G, int lev, double (&T)[4]) {
  const long g0 = G.start(m, lev), g1 = G.start(m + 1, lev);
  if (g1 > g0) {
    const double2* p = reinterpret_cast<const double2*>(segtot + 4 * ((size_t)lev * G.nseg + m));
    const double2 x = p[0], y = p[1];
    T[0] = x.x; T[1] = x.y; T[2] = y.x; T[3] = y.y;
  } else {
    T[0] = T[1] = T[2] = T[3] = 0.0;
  }
}
// sum over a range of c0 + c1 d + c2 d^2 + c3 d^3, d = u + dl, from the range's moments in u.
__device__ __forceinline__ double wth_combine(const double (&D)[4], double dl, double c0, double c1,
                                              double c2, double c3) {
  const double p1 = D[1] + dl * D[0];
  const double p2 = D[2] + dl * (2.0 * D[1] + dl * D[0]);
  const double p3 = D[3] + dl * (3.0 * D[2] + dl * (3.0 * D[1] + dl * D[0]));
  return c0 * D[0] + c1 * p1 + c2 * p2 + c3 * p3;
}

// grid n_theta, block 256: one theta per workgroup, one Romberg level per wavefront and round
// (four levels a round); lane i <= NP holds knot i of the kernel spline: the first node at or
// beyond it and the prefix moments just below.  Levels <= LT only (the host keeps the
// node-by-node kernel for a divmax beyond the table).  Needs NKT <= 63.
// (the body of k_wtheta_fast and k_wtheta_fast_epochs: theta[0] into out[0])
__device__ __forceinline__ void wth_fast_body(const chomp_config& cfg, const ProjLayout& L,
                                              const ProjDev* __restrict__ pd,
                                              const double* __restrict__ ptab, double k_min,
                                              double k_max, const double* __restrict__ theta,
                                              double* __restrict__ out,
                                              const double* __restrict__ nodes,
                                              const double* __restrict__ rec,
                                              const double* __restrict__ segtot, int LT, int nseg) {
  __shared__ double level_sum[2][4];
  __shared__ double ctab[(kWthetaTabLevel + 1) * 32];   // the rows' weights (RombergRows2::ctab)
  romberg_weights_to_lds(ctab, LT);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double a = log(k_min), b = log(k_max);
  const double lo = pd->ln_kt_min, hi = pd->ln_kt_max;
  const int NP = L.NKT - 1;                              // spline pieces
  const double dxK = (hi - lo) / (double)NP;
  const double s = log(theta[0]);
  const double* pp = ptab + L.k_pp;
  const int piece = lane < NP ? lane : NP - 1;
  const double c0 = pp[4 * piece], c1 = pp[4 * piece + 1], c2 = pp[4 * piece + 2],
               c3 = pp[4 * piece + 3];
  const double k_lo = pp[0];                             // K below its range (kernel.py:723-725)
  const double X = lo + dxK * (double)lane;              // knot i (= hi for lane NP, up to rounding)
  const KernelView K{pp, L.NKT, lo, hi};
  RombergRows2 R;
  R.ctab = ctab;
  R.start(b - a, cfg.global_precision, cfg.corr_precision,
          0.5 * (nodes[0] * K(a + s) + nodes[1] * K(b + s)), 0.0, true, false);
  const WthSeg G(nseg, a, b);
  for (int g = 0; 4 * g < LT && !R.all_done(); ++g) {
    const int lv = 4 * g + 1 + wave;
    double contrib = 0.0;
    if (lv <= LT) {                                      // (wave-uniform)
      const long n = 1L << (lv - 1);
      const double h = (b - a) / (double)n, lox = a + 0.5 * h, inv_h = (double)n / (b - a);
      const long base = 1 + n;
      // B: the first node of this lane's region (piece i, or beyond the range for lane NP)
      long B = 0;
      if (lane < NP) {
        const double q = ceil((X - s - lox) * inv_h);
        B = q <= 0.0 ? 0 : (q >= (double)n ? n : (long)q);
      } else if (lane == NP) {                           // x + s == hi still inside (kernel.py:728)
        const double q = floor((hi - s - lox) * inv_h) + 1.0;
        B = q <= 0.0 ? 0 : (q >= (double)n ? n : (long)q);
      }
      // prefix moments just below B -- the record at or before node B - 1 and the nodes behind
      // it, or the nodes from the segment's start -- and the total of that segment (every load
      // issued before anything waits for it; for B = 0 valid addresses whose values are not used)
      const bool has = lane <= NP && B >= 1;
      const int mB = has ? wth_seg_of(B - 1, nseg, lv) : 0;
      const long jl = has ? B - 1 : 0;                   // the last node of the prefix
      const long js = has ? G.start(mB, lv) : 0;         // ... the first node of its segment
      const long jb = ((jl + 1) / kWthItems) * kWthItems;     // nodes < jb are in the record
      const bool from_rec = jb > js;
      const long i0 = from_rec ? jb : js;                // the nodes i0 .. jl are added here
      const double2* pR = reinterpret_cast<const double2*>(rec + 4 * (from_rec ? (n + jb) / kWthItems : 0));
      const double2* pT = reinterpret_cast<const double2*>(segtot + 4 * ((size_t)lv * nseg + mB));
      const double2 R01 = pR[0], R23 = pR[1], T01 = pT[0], T23 = pT[1];
      double gtail[kWthItems - 1];
#pragma unroll
      for (int i = 0; i < kWthItems - 1; ++i) {
        const long jn = i0 + i;
        gtail[i] = nodes[base + (jn <= jl ? jn : jl)];
      }
      double P[4] = {from_rec ? R01.x : 0.0, from_rec ? R01.y : 0.0, from_rec ? R23.x : 0.0,
                     from_rec ? R23.y : 0.0};
      {
        const double O = G.origin(mB);
#pragma unroll
        for (int i = 0; i < kWthItems - 1; ++i) {
          const long jn = i0 + i;
          const double g = jn <= jl ? gtail[i] : 0.0;
          const double u = (lox + h * (double)jn) - O;
          P[0] += g; P[1] += g * u; P[2] += g * (u * u); P[3] += g * (u * u * u);
        }
      }
      if (!has) { P[0] = P[1] = P[2] = P[3] = 0.0; }
      const long B0 = __shfl((long long)B, 0, 64);
      const int m0 = __shfl(mB, 0, 64);
      double below = 0.0;                                // plain sum of g over the segments < m0
      if (B0 >= 1) {
        for (int m = lane; m < m0; m += 64) {
          double T[4];
          wth_seg_total(segtot, m, G, lv, T);
          below += T[0];
        }
      }
      // the next knot's
      const long Bn = __shfl_down((long long)B, 1, 64);
      const int mn = __shfl_down(mB, 1, 64);
      double Pn[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) Pn[q] = __shfl_down(P[q], 1, 64);
      if (lane < NP && Bn > B) {
        if (mn == mB && B >= 1) {
          const double D[4] = {Pn[0] - P[0], Pn[1] - P[1], Pn[2] - P[2], Pn[3] - P[3]};
          contrib = wth_combine(D, G.origin(mB) + s - X, c0, c1, c2, c3);
        } else {
          // the rest of segment mB, whole segments between, the head of segment mn
          if (B >= 1) {
            const double D[4] = {T01.x - P[0], T01.y - P[1], T23.x - P[2], T23.y - P[3]};
            contrib = wth_combine(D, G.origin(mB) + s - X, c0, c1, c2, c3);
          }
          for (int m = B >= 1 ? mB + 1 : 0; m < mn; ++m) {
            double T[4];
            wth_seg_total(segtot, m, G, lv, T);
            contrib += wth_combine(T, G.origin(m) + s - X, c0, c1, c2, c3);
          }
          contrib += wth_combine(Pn, G.origin(mn) + s - X, c0, c1, c2, c3);
        }
      }
      // nodes below the kernel's range: K(lo) times the plain sum of g over [0, B_0)
      if (lane == 0) below += P[0];
      contrib += k_lo * below;
    }
    const double S = wave_sum(contrib);
    if (lane == 0) level_sum[g & 1][wave] = S;
    __syncthreads();
    for (int q = 0; q < 4 && 4 * g + 1 + q <= LT && !R.all_done(); ++q)
      R.advance(4 * g + 1 + q, level_sum[g & 1][q], 0.0);
  }
  if (threadIdx.x == 0) out[0] = R.value[0];
}
__global__ __launch_bounds__(256) void k_wtheta_fast(chomp_config cfg, ProjLayout L,
                                                     const ProjDev* __restrict__ pd,
                                                     const double* __restrict__ ptab, double k_min,
                                                     double k_max, const double* __restrict__ theta,
                                                     double* __restrict__ out,
                                                     const double* __restrict__ nodes,
                                                     const double* __restrict__ rec,
                                                     const double* __restrict__ segtot, int LT,
                                                     int nseg) {
  wth_fast_body(cfg, L, pd, ptab, k_min, k_max, theta + blockIdx.x, out + blockIdx.x, nodes, rec,
                segtot, LT, nseg);
}
// ... with an epoch axis: grid (n_theta, E), block 256: one Romberg per (theta, epoch), epoch
// blockIdx.y from its own tables (`stride` doubles apart) into out[blockIdx.y * n_theta +
// blockIdx.x]; epochs stop at their own levels.  theta is the fast grid axis, so the blocks that
// are resident together mostly share an epoch and its records in L2.
__global__ __launch_bounds__(256) void k_wtheta_fast_epochs(
    chomp_config cfg, ProjLayout L, const ProjDev* __restrict__ pd, const double* __restrict__ ptab,
    double k_min, double k_max, const double* __restrict__ theta, double* __restrict__ out,
    const double* __restrict__ nodes, const double* __restrict__ rec,
    const double* __restrict__ segtot, int LT, int nseg, size_t stride) {
  const size_t off = stride * blockIdx.y;
  wth_fast_body(cfg, L, pd, ptab, k_min, k_max, theta + blockIdx.x,
                out + (size_t)blockIdx.y * gridDim.x + blockIdx.x, nodes + off, rec + off,
                segtot + off, LT, nseg);
}
// ... with an epoch axis whose rows have their own projection set (chomp_wtheta_sets): row
// blockIdx.y reads the kernel spline of set blockIdx.y (pd[blockIdx.y], its slab `pstride`
// doubles after the previous one).  The sets share the ln(k theta) range, so nseg is one number.
__global__ __launch_bounds__(256) void k_wtheta_fast_sets(
    chomp_config cfg, ProjLayout L, const ProjDev* __restrict__ pd, const double* __restrict__ ptab,
    size_t pstride, double k_min, double k_max, const double* __restrict__ theta,
    double* __restrict__ out, const double* __restrict__ nodes, const double* __restrict__ rec,
    const double* __restrict__ segtot, int LT, int nseg, size_t stride) {
  const size_t off = stride * blockIdx.y;
  wth_fast_body(cfg, L, pd + blockIdx.y, ptab + pstride * blockIdx.y, k_min, k_max,
                theta + blockIdx.x, out + (size_t)blockIdx.y * gridDim.x + blockIdx.x, nodes + off,
                rec + off, segtot + off, LT, nseg);
}

// ---------------------------------------------------------------------------
// Precision sweep of w(theta) (BASELINE.json configs[4]): the same
// integral with parts of the arithmetic in fp32.
//   CHOMP_PREC_F32_EVAL    integrand evaluated in fp32 from the fp64 tables, fp64 sums
//   CHOMP_PREC_F32_TABLES  spline coefficients rounded to fp32, fp64 evaluation and sums
//   CHOMP_PREC_F32_ALL     fp32 tables, fp32 evaluation, fp32 sums and extrapolation
// The fp64 mode (k_wtheta) is the product path; these exist to measure what each
// narrowing costs against the reference's numbers.
// ---------------------------------------------------------------------------
namespace f32 {

// fp32 restatement of PowerEval + KernelView (same branches, halo.py:314-320, 649-672,
// 1339-1360; kernel.py:714-729); tables are read as stored and narrowed on the fly.
struct Eval {
  const PowerEval* P;
  const KernelView* K;
  float theta, inv_D2;
  float eh_s, eh_omh, eh_alpha, eh_theta, amp2, ns, ln_H0;
  float k_s, beta_n, alpha_n, a_n, b_n, c_n, gamma_n, mu_n, nu_n, f1, f2, f3;

  __device__ __forceinline__ void init(const PowerEval* P_, const KernelView* K_, double th,
                                       double invD2) {
    P = P_; K = K_; theta = (float)th; inv_D2 = (float)invD2;
    const Epoch& E = *P->E;
    eh_s = (float)E.eh_s; eh_omh = (float)E.eh_omh; eh_alpha = (float)E.eh_alpha;
    eh_theta = (float)E.eh_theta; amp2 = (float)(E.amp * E.sigma_norm * E.sigma_norm);
    ns = (float)E.ns; ln_H0 = (float)E.ln_H0;
    k_s = (float)E.hf_k_s; beta_n = (float)E.hf_beta_n; alpha_n = (float)E.hf_alpha_n;
    a_n = (float)E.hf_a_n; b_n = (float)E.hf_b_n; c_n = (float)E.hf_c_n;
    gamma_n = (float)E.hf_gamma_n; mu_n = (float)E.hf_mu_n; nu_n = (float)E.hf_nu_n;
    f1 = (float)E.hf_f1; f2 = (float)E.hf_f2; f3 = (float)E.hf_f3;
  }
  __device__ __forceinline__ float poly(const double* c, int i, float d) const {
    const double* q = c + 4 * i;
    return fmaf(fmaf(fmaf((float)q[3], d, (float)q[2]), d, (float)q[1]), d, (float)q[0]);
  }
  __device__ __forceinline__ float spline(float x0, float dx, const double* c, int n,
                                          float xv) const {
    int i = (int)floorf((xv - x0) / dx);
    i = i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
    return poly(c, i, xv - (x0 + dx * (float)i));
  }
  __device__ __forceinline__ float delta_k(float lk, float k) const {
    const float t = 1.0f + 0.43f * k * eh_s;
    const float t2 = t * t;
    const float G = eh_omh * (eh_alpha + (1.0f - eh_alpha) / (t2 * t2));
    const float q = k * eh_theta / G;
    const float L0 = logf(2.0f * 2.7182818f + 1.8f * q);
    const float C0 = 14.2f + 731.0f / (1.0f + 62.5f * q);
    const float T = L0 / (L0 + C0 * q * q);
    return amp2 * expf((3.0f + ns) * (lk - ln_H0)) * T * T;
  }
  __device__ __forceinline__ float halofit(float lk, float k) const {
    const float dk = delta_k(lk, k);
    const float y = k / k_s;
    const float d2q = dk * (powf(1.0f + dk, beta_n) / (1.0f + alpha_n * dk) *
                            expf(-(y / 4.0f + y * y / 8.0f)));
    const float d2h = (a_n * powf(y, 3.0f * f1) /
                       (1.0f + b_n * powf(y, f2) + powf(c_n * f3 * y, 3.0f - gamma_n))) /
                      (1.0f + mu_n / y + nu_n / (y * y));
    return 2.0f * 9.8696044f / (k * k * k) * (d2q + d2h);
  }
  __device__ __forceinline__ float power(float lk, float k) const {
    const float x0 = (float)P->x0, dx = (float)P->dx;
    const float k_min = (float)P->k_min, k_max = (float)P->k_max;
    const float plin = 2.0f * 9.8696044f * delta_k(lk, k) / (k * k * k);
    if (P->w == CHOMP_P_LIN) return plin;
    const bool in = k >= k_min && k <= k_max;
    if (P->halofit) {
      const float pmm = halofit(lk, k);
      if (P->w == CHOMP_P_MM) return pmm;
      float ha = 0.0f, hb = 0.0f, pp = 0.0f;
      if (in) {
        ha = spline(x0, dx, P->ca, P->NK, lk);
        hb = spline(x0, dx, P->cb, P->NK, lk);
        pp = spline(x0, dx, P->cp, P->NK, lk);
      }
      return pmm * ha * hb + pp;
    }
    if (k < k_min) return plin * (float)P->c_lo;
    if (in) {
      return plin * spline(x0, dx, P->ca, P->NK, lk) * spline(x0, dx, P->cb, P->NK, lk) +
             spline(x0, dx, P->cp, P->NK, lk);
    }
    return 0.0f;
  }
  __device__ __forceinline__ float kernel(float x) const {
    const float lo = (float)K->lo, hi = (float)K->hi;
    const float dx = (hi - lo) / (float)(K->N - 1);
    if (x < lo) return poly(K->pp, 0, 0.0f);
    if (x <= hi) return spline(lo, dx, K->pp, K->N, x);
    return 0.0f;
  }
  // correlation.py:270-275
  __device__ __forceinline__ float operator()(float ln_k) const {
    const float k = expf(ln_k);
    return k * k / (2.0f * 3.14159265f) * power(ln_k, k) * inv_D2 * kernel(logf(k * theta));
  }
};

struct EvalAsDouble {          // fp32 integrand under the fp64 Romberg driver
  const Eval* f;
  __device__ __forceinline__ double operator()(double ln_k) const {
    return (double)(*f)((float)ln_k);
  }
};

// scipy.integrate.romberg in single precision, one integral per 256-thread block
// (plain level-by-level version: this path is for the accuracy sweep, not for speed).
// red: 8 floats of LDS.
template <class F>
__device__ float romberg_block(const F& f, float a, float b, float tol, float rtol, int divmax,
                               float* red) {
  const float len = b - a;
  float ordsum = 0.5f * (f(a) + f(b));
  float prev[24], cur[24];
  prev[0] = len * ordsum;
  float result = prev[0];
  int n = 1;
  for (int i = 1; i <= divmax; ++i) {
    const float h = len / (float)n;
    float part = 0.0f;
    for (int j = threadIdx.x; j < n; j += blockDim.x) part += f(a + 0.5f * h + h * (float)j);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    float tot = 0.0f;
    for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) tot += red[wv];
    ordsum += tot;
    n *= 2;
    cur[0] = len * ordsum / (float)n;
    float p4 = 1.0f;
    for (int m = 1; m <= i; ++m) {
      p4 *= 4.0f;
      cur[m] = (p4 * cur[m - 1] - prev[m - 1]) / (p4 - 1.0f);
    }
    result = cur[i];
    const float err = fabsf(result - prev[i - 1]);
    for (int m = 0; m <= i; ++m) prev[m] = cur[m];
    if (err < tol || err < rtol * fabsf(result)) break;
  }
  return result;
}

}  // namespace f32

// grid n_theta, block 256: k_wtheta with a narrowed precision mode (MODE = CHOMP_PREC_*).
template <int MODE>
__global__ __launch_bounds__(256) void k_wtheta_mixed(chomp_config cfg, TabLayout HL, ProjLayout L,
                                                      const Epoch* __restrict__ epochs, int e,
                                                      const double* __restrict__ htab, int which,
                                                      const ProjDev* __restrict__ pd,
                                                      const double* __restrict__ ptab,
                                                      double k_min, double k_max, double D_z,
                                                      const double* __restrict__ theta,
                                                      double* __restrict__ out) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  PowerEval P;
  P.stage(cfg, HL, &E, htab + (size_t)e * HL.stride, which, sm);
  double* kpp = sm + 12 * (HL.NK - 1);
  copy_doubles(kpp, ptab + L.k_pp, 4 * (L.NKT - 1));
  __syncthreads();
  if (MODE == CHOMP_PREC_F32_TABLES || MODE == CHOMP_PREC_F32_ALL) {
    const int n_tab = 12 * (HL.NK - 1) + 4 * (L.NKT - 1);
    for (int i = threadIdx.x; i < n_tab; i += blockDim.x) sm[i] = (double)(float)sm[i];
    __syncthreads();
  }
  P.finish();
  const KernelView K{kpp, L.NKT, pd->ln_kt_min, pd->ln_kt_max};
  double v;
  if (MODE == CHOMP_PREC_F32_TABLES) {
    if (P.halofit) {
      WthetaIntegrand<true> f{&P, &K, theta[blockIdx.x], 1.0 / (D_z * D_z), log(theta[blockIdx.x])};
      v = romberg1<4>(f, log(k_min), log(k_max), cfg.global_precision, cfg.corr_precision,
                      cfg.divmax, red);
    } else {
      WthetaIntegrand<false> f{&P, &K, theta[blockIdx.x], 1.0 / (D_z * D_z), log(theta[blockIdx.x])};
      v = romberg1<4>(f, log(k_min), log(k_max), cfg.global_precision, cfg.corr_precision,
                      cfg.divmax, red);
    }
  } else {
    f32::Eval f;
    f.init(&P, &K, theta[blockIdx.x], 1.0 / (D_z * D_z));
    if (MODE == CHOMP_PREC_F32_EVAL) {
      f32::EvalAsDouble g{&f};
      v = romberg1<4>(g, log(k_min), log(k_max), cfg.global_precision, cfg.corr_precision,
                      cfg.divmax, red);
    } else {
      v = (double)f32::romberg_block(f, (float)log(k_min), (float)log(k_max),
                                     (float)cfg.global_precision, (float)cfg.corr_precision,
                                     cfg.divmax, reinterpret_cast<float*>(red));
    }
  }
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// correlation.py:496-501 (Correlation3d._correlation_integrand)
template <bool BAO>
struct Xi3dIntegrand {
  const PowerEval* P;
  const BesselTab* B;
  double r;
  __device__ __forceinline__ double operator()(double ln_k) const {
    const double k = exp(ln_k);
    const double p = P->halofit ? P->template at_ln<true, BAO>(ln_k, k)
                                : P->template at_ln<false, BAO>(ln_k, k);
    return k * k / (2.0 * kPi) * p * bessel_j<0>(k * r, *B);
  }
};

// grid n_r, block 256: one separation per workgroup.
template <bool BAO>
__global__ __launch_bounds__(256) void k_xi3d(chomp_config cfg, TabLayout HL,
                                              const Epoch* __restrict__ epochs, int e,
                                              const double* __restrict__ htab, int which,
                                              const BesselTab* __restrict__ bess_g,
                                              double k_min, double k_max,
                                              const double* __restrict__ r,
                                              double* __restrict__ out) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ BesselTab B;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&B), reinterpret_cast<const double*>(bess_g),
               (int)(sizeof(BesselTab) / sizeof(double)));
  PowerEval P;
  P.stage(cfg, HL, &E, htab + (size_t)e * HL.stride, which, sm);
  __syncthreads();
  P.template finish_t<BAO>();
  Xi3dIntegrand<BAO> f{&P, &B, r[blockIdx.x]};
  const double v = romberg1<4>(f, log(k_min), log(k_max), cfg.global_precision,
                               cfg.corr_precision, cfg.divmax, red);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// The epoch axis (chomp_xi3d_epochs: one xi(r) per HOD or cosmology of a design or chain).  Every
// separation integrates over the same ln k range, so the r-independent factor k^2/(2 pi) P(k) of
// the integrand is the node table of k_wtheta_nodes_epochs with D_z = 1.0 (its last factor is
// then 1.0 / (1.0 * 1.0) = 1.0 and the product by it exact): one table per epoch at a fixed
// stride in the context's w(theta) work buffer, the epochs worked off in chunks of
// kWthEpochChunk.  Per node a block then only reads the table and evaluates J0(k r) -- no
// PowerEval, no epoch record, no knot splines.  Every level lies within the table (the entry point
// refuses divmax > kWthetaTabLevel).
struct Xi3dTabIntegrand {
  const double* nodes;
  const BesselTab* B;
  double r;
  // ln_k: romberg_group's node (the node arithmetic wth_nodes_body tabulated with)
  __device__ __forceinline__ void operator()(double ln_k, double (&out)[1], int lev, long j) const {
    const long idx = lev == 0 ? j : 1 + (1L << (lev - 1)) + j;
    const double k = exp(ln_k);
    out[0] = nodes[idx] * bessel_j<0>(k * r, *B);
  }
};

// grid (n_r, E), block 256: block (i, y) integrates separation r[i] of the epoch whose table is
// row y of `nodes` into out[y * n_r + i] -- the sums of k_xi3d in its order (romberg_group<4, 1>
// on 256 threads), so bit for bit its value.  The separation is the fast grid axis: the blocks
// that read one table run together.  102 VGPRs, no scratch, 2 KB of LDS (tools/kernel_regs.py;
// k_xi3d: 153): four waves per SIMD, four blocks per CU, which the second bound keeps.
__global__ __launch_bounds__(256, 4) void k_xi3d_epochs(double tol, double rtol, int divmax,
                                                     const BesselTab* __restrict__ bess_g,
                                                     double k_min, double k_max,
                                                     const double* __restrict__ r,
                                                     double* __restrict__ out,
                                                     const double* __restrict__ nodes,
                                                     size_t stride) {
  __shared__ BesselTab B;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&B), reinterpret_cast<const double*>(bess_g),
               (int)(sizeof(BesselTab) / sizeof(double)));
  __syncthreads();
  Xi3dTabIntegrand f{nodes + stride * blockIdx.y, &B, r[blockIdx.x]};
  const RombergOut<1> v = romberg_group<4, 1>(f, log(k_min), log(k_max), tol, rtol, divmax, red);
  if (threadIdx.x == 0) out[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = v.value[0];
}

// Not-a-knot cubic spline through (xk, yk) evaluated at x: one block; c: 4 (nk - 1)
// doubles, w: 2 nk doubles of scratch.
__global__ void k_spline_eval(const double* __restrict__ xk, const double* __restrict__ yk, int nk,
                              double* __restrict__ c, double* __restrict__ w,
                              const double* __restrict__ x, int n, int deriv,
                              double* __restrict__ out) {
  if (threadIdx.x == 0) spline_build(xk, yk, nk, c, w);
  __threadfence_block();
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    if (deriv == 0) {
      out[i] = spline_eval(xk, c, nk, x[i]);
    } else {                       // derivative of the piece that holds x
      int lo = 0, hi = nk - 2;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (x[i] >= xk[mid]) lo = mid; else hi = mid - 1;
      }
      const double* q = c + 4 * lo;
      const double d = x[i] - xk[lo];
      out[i] = fma(fma(3.0 * q[3], d, 2.0 * q[2]), d, q[1]);
    }
  }
}

// correlation.py:387-392
template <bool BAO>
struct CellIntegrand {
  const PowerEval* P;
  const ProjLds* G;
  double ell, inv_D2;
  __device__ __forceinline__ double operator()(double chi) const {
    const double D = G->me.growth_factor(G->me.redshift(chi));
    return P->template eval_t<BAO>(ell / chi) * inv_D2 * G->wa(chi) * G->wb(chi) * D * D / (chi * chi);
  }
};

// Every multipole integrates over the same chi range, so all of them visit the same Romberg
// nodes and everything in the integrand that depends on chi alone -- both windows, the growth
// factor (two spline look-ups each), 1 / chi^2, 1 / D_z^2 -- is tabulated once per call on
// the level-LT grid (level-major, as w(theta)'s k-only factor): F_j, ln chi_j and chi_j.  A
// multipole then only evaluates P(l / chi_j) per node, with ln k = ln l - ln chi_j for free.
// grid ceil((2^LT + 1) / 256), block 256; dynamic LDS ProjLds::doubles(L).
constexpr int kCellTabLevel = 16;       // 3 x (2^16 + 1) doubles = 1.5 MiB (the C_l integrals of
                                        // configs[3] / [4] stop at levels 7..15, a few at 14, 15)
// (the body of k_cell_nodes and k_cell_nodes_sets)
__device__ __forceinline__ void cell_nodes_body(const ProjLayout& L, const ProjDev* __restrict__ pdg,
                                                const double* __restrict__ ptab, double D_z, int LT,
                                                double* __restrict__ nodes) {
  extern __shared__ __align__(16) double sm[];
  __shared__ ProjDev pd;
  copy_doubles(reinterpret_cast<double*>(&pd), reinterpret_cast<const double*>(pdg), kProjDoubles);
  __syncthreads();
  ProjLds G;
  G.stage(L, pd, ptab, sm);
  G.bess = nullptr;
  __syncthreads();
  const long N = (1L << LT) + 1;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N) return;
  const double a = pd.chi_min, b = pd.chi_max, intrange = b - a;
  double chi;
  if (idx < 2) {
    chi = idx == 0 ? a : b;
  } else {                                   // the node arithmetic of chomp_romberg.h
    const unsigned m = (unsigned)(idx - 1);
    const int lev = 32 - __builtin_clz(m);
    const long j = (long)m - (1L << (lev - 1));
    const double h = ldexp(intrange, 1 - lev);
    chi = (a + 0.5 * h) + h * (double)j;
  }
  const double D = G.me.growth_factor(G.me.redshift(chi));
  nodes[idx] = (1.0 / (D_z * D_z)) * G.wa(chi) * G.wb(chi) * D * D / (chi * chi);
  nodes[N + idx] = log(chi);
  nodes[2 * N + idx] = chi;
}
__global__ __launch_bounds__(256) void k_cell_nodes(ProjLayout L, const ProjDev* __restrict__ pdg,
                                                    const double* __restrict__ ptab, double D_z,
                                                    int LT, double* __restrict__ nodes,
                                                    int* __restrict__ deep, int n_lists,
                                                    size_t list_stride) {
  // k_cell's lists, one per epoch of the call (chomp_cell: one): count, head
  if (blockIdx.x == 0)
    for (int q = threadIdx.x; q < 2 * n_lists; q += blockDim.x)
      deep[(q >> 1) * list_stride + (q & 1)] = 0;
  cell_nodes_body(L, pdg, ptab, D_z, LT, nodes);
}
// ... with a set axis (chomp_cell_sets, "The set axis of C_l" below): grid (as k_cell_nodes, E);
// row blockIdx.y tabulates set pd[blockIdx.y] and its slab of projection tables, `pstride` doubles
// after the previous set's, with growth D_z[blockIdx.y] into its own node table, `stride` doubles
// after the previous row's, and empties its own list (deep: the first row's).
__global__ __launch_bounds__(256) void k_cell_nodes_sets(ProjLayout L, const ProjDev* __restrict__ pd,
                                                         const double* __restrict__ ptab,
                                                         size_t pstride, const double* __restrict__ D_z,
                                                         int LT, double* __restrict__ nodes,
                                                         int* __restrict__ deep, size_t stride) {
  if (blockIdx.x == 0 && threadIdx.x < 2) deep[2 * stride * blockIdx.y + threadIdx.x] = 0;
  cell_nodes_body(L, pd + blockIdx.y, ptab + pstride * blockIdx.y, D_z[blockIdx.y], LT,
                  nodes + stride * blockIdx.y);
}

// P(k) of the spectrum a C_l call integrates, on a uniform grid of kPTabN intervals in ln k
// over [ln k_min, ln k_max] (one evaluation of PowerEval::at_ln per point, once per call):
// inside that range a multipole's node then reads P(l / chi) off a 6-point Lagrange stencil
// (~1e-16 relative at this spacing: the spectrum is smooth in ln k) instead of evaluating
// three knot splines and the linear spectrum -- or the HaloFit formula -- per node.  Outside
// the range: zero where the spectrum is identically zero, else evaluated directly (the rescaled
// linear spectrum / the extrapolations, halo.py:300-320).  No-wiggle spectra only.
// grid ceil((kPTabN + 1) / 256), block 256; dynamic LDS 12 (NK - 1) doubles.
constexpr int kPTabN = 8192;
// (the body of k_cell_ptab and k_cell_ptab_epochs; bx: the block's index along the table)
template <bool HF, bool BAO>
__device__ __forceinline__ void cell_ptab_body(const chomp_config& cfg, const TabLayout& HL,
                                               const Epoch* __restrict__ epochs, int e,
                                               const double* __restrict__ htab, int which,
                                               double* __restrict__ ptab_out, unsigned bx) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  PowerEval P;
  P.stage(cfg, HL, &E, htab + (size_t)e * HL.stride, which, sm);
  __syncthreads();
  P.template finish_t<BAO>();
  const int i = bx * blockDim.x + threadIdx.x;
  if (i > kPTabN) return;
  const double x0 = log(cfg.k_min), x1 = log(cfg.k_max);
  double x = x0 + (x1 - x0) * ((double)i / (double)kPTabN);
  double k = exp(x);
  // (the end points exactly: exp(log(k_max)) may round past k_max, where the spectrum is 0)
  if (i == 0) { k = cfg.k_min; x = x0; }
  if (i == kPTabN) { k = cfg.k_max; x = x1; }
  ptab_out[i] = P.template at_ln<HF, BAO>(x, k);
}
template <bool HF, bool BAO>
__global__ __launch_bounds__(256) void k_cell_ptab(chomp_config cfg, TabLayout HL,
                                                   const Epoch* __restrict__ epochs, int e,
                                                   const double* __restrict__ htab, int which,
                                                   double* __restrict__ ptab_out) {
  cell_ptab_body<HF, BAO>(cfg, HL, epochs, e, htab, which, ptab_out, blockIdx.x);
}

// The epoch axis (chomp_cell_epochs: one C_l per HOD of a design or chain).  The chi-only node
// table of k_cell_nodes does not depend on the epoch and is built once per call; what an epoch
// owns -- its spectrum table, the Romberg states of its multipoles and its deep list -- follows
// the node table in the context's C_l work buffer, one slab per epoch of the chunk at a fixed
// stride (cell_epoch_stride):
//   3 (2^LT + 1) doubles   F_j, ln chi_j, chi_j                       (shared)
//   then per epoch:  kPTabN + 1 doubles       P(k) of k_cell_ptab
//                    n kRombergDump doubles   state[kRombergDump * multipole]
//                    2 + n ints               deep list: count, head, multipoles
// and the *_epochs kernels address the slab of epoch i at i * stride from the first one's table,
// states and list.  A list holds multipoles of its own epoch only: a block of k_cell_deep_epochs
// then stages one spectrum table for its lifetime, as k_cell_deep does.  A call works its epochs
// off in chunks of kWthEpochChunk (CHOMP_TUNE_WTHETA_EPOCH_CHUNK: the knob of both batched
// projections); a slab is 64 KiB + 276 n bytes, so the buffer stays small whatever the chunk.
// k_cell_nodes empties the lists of the first chunk, k_cell_ptab_epochs those of a later one (the
// slabs are reused in stream order).  Per (multipole, epoch) the arithmetic is the single-epoch
// kernels': both sets of __global__s call the same bodies.
inline size_t cell_epoch_stride(size_t n) {
  return (size_t)kPTabN + 1 + n * kRombergDump + (n + 3) / 2 + 1;
}
// grid (as k_cell_ptab, E), block 256: row blockIdx.y stages epoch e0 + blockIdx.y and writes that
// epoch's table.  deep (the first epoch's list; null: k_cell_nodes has emptied them): the row
// empties its list.
template <bool HF, bool BAO>
__global__ __launch_bounds__(256) void k_cell_ptab_epochs(chomp_config cfg, TabLayout HL,
                                                          const Epoch* __restrict__ epochs, int e0,
                                                          const double* __restrict__ htab, int which,
                                                          double* __restrict__ ptab_out,
                                                          int* __restrict__ deep, size_t stride) {
  if (deep != nullptr && blockIdx.x == 0 && threadIdx.x < 2)
    deep[2 * stride * blockIdx.y + threadIdx.x] = 0;
  cell_ptab_body<HF, BAO>(cfg, HL, epochs, e0 + (int)blockIdx.y, htab, which,
                          ptab_out + stride * blockIdx.y, blockIdx.x);
}

// correlation.py:387-392 from the node table (levels <= LT), directly beyond
// DIRECT = false: the caller never asks for a level beyond the node table (k_cell below its
// hand-over level): the node-by-node route -- windows, growth, ~100 registers -- is not compiled.
template <bool HF, bool BAO, bool DIRECT = true>
struct CellTabIntegrand {
  const PowerEval* P;
  const double* nodes;
  long N;
  int LT;
  double ell, ln_ell;
  const double* ptab;      // k_cell_ptab (nullptr: evaluate the spectrum at every node)
  double px0, pdx, pinv_dx;
  CellIntegrand<BAO> direct;
  // The spectrum at ln k = lk from the table, as straight-line code: inside [ln k_min, ln k_max]
  // the 6-point stencil, shifted at the two ends so that it never leaves the table (P drops to
  // zero beyond k_max: a stencil must not straddle that); outside the range the value where it
  // is identically zero (halo.py:300-320 without extrapolation above k_max; :649-672 for the
  // HaloFit cross spectra on both sides).  *ok = false: neither -- the caller evaluates
  // PowerEval::at_ln.  ptab must not be null.
  __device__ __forceinline__ double from_table(double lk, bool* ok) const {
    const double u = (lk - px0) * pinv_dx;
    const bool in = u >= 0.0 && u <= (double)kPTabN;
    const bool zero_out = HF ? P->w != CHOMP_P_MM
                             : (u > 0.0 && !P->extrap && P->w != CHOMP_P_LIN);
    int i = (int)u;
    i = (in && i > 2) ? (i < kPTabN - 3 ? i : kPTabN - 3) : 2;
    const double t = u - (double)i;
    const double* q = ptab + i - 2;
    const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4], q5 = q[5];
    const double a = t + 2.0, b = t + 1.0, d = t - 1.0, e = t - 2.0, f = t - 3.0;
    const double ab = a * b, ef = e * f, cd = t * d;
    const double v = q0 * (b * cd * ef) * (-1.0 / 120.0) + q1 * (a * cd * ef) * (1.0 / 24.0) +
                     q2 * (ab * d * ef) * (-1.0 / 12.0) + q3 * (ab * t * ef) * (1.0 / 12.0) +
                     q4 * (ab * cd * f) * (-1.0 / 24.0) + q5 * (ab * cd * e) * (1.0 / 120.0);
    *ok = in || zero_out;
    // (at the table's last point the weights are 0 .. 0 1 only up to the rounding of
    //  q5 * 120 * (1 / 120): the spectrum at k_max is the last entry itself)
    return in ? (u == (double)kPTabN ? q5 : v) : 0.0;
  }
  __device__ __forceinline__ void operator()(double chi, double (&out)[1], int lev, long j) const {
    if (lev <= LT) {
      const long idx = lev == 0 ? j : 1 + (1L << (lev - 1)) + j;
      const double lk = ln_ell - nodes[N + idx];
      bool ok = false;
      double p = 0.0;
      if (ptab != nullptr) p = from_table(lk, &ok);
      if (!ok) p = P->template at_ln<HF, BAO>(lk, ell / nodes[2 * N + idx]);
      out[0] = p * nodes[idx];
    } else if constexpr (DIRECT) {
      out[0] = direct(chi);
    } else {
      out[0] = 0.0;
    }
  }
  // The same value for a node of the table that from_table answers, as straight-line code
  // (detail::fast_f); false otherwise.
  __device__ __forceinline__ bool fast(double, double (&out)[1], int lev, long j) const {
    if (ptab == nullptr || lev > LT || lev == 0) return false;     // (uniform over the batch)
    const long idx = 1 + (1L << (lev - 1)) + j;
    const double g = nodes[idx], lk = ln_ell - nodes[N + idx];
    bool ok;
    out[0] = from_table(lk, &ok) * g;
    return ok;
  }
};

// grid n_ell, block 256: one multipole per workgroup, up to Romberg level `split` (= divmax: the
// whole integral).  A multipole not converged there is listed for k_cell_deep with its Romberg
// state: deep[0] counts them, deep[2 + i] names them, state[kRombergDump * multipole].
// (Most multipoles of configs[3] / [4] stop at levels 7..9, a few dozen of the highest run to
//  14, 15: in one 256-thread block those walk 64..128 nodes per thread, each two dependent
//  reads of tables another kernel wrote -- a microsecond a piece on a CU whose L2 has not seen
//  them -- and set the launch's duration: 65 us measured against 9 us for a level-8 block.)
constexpr int kCellSplitLevel = 11;
// (the body of k_cell and k_cell_epochs: multipole il of ell into out[il])
template <bool HF, bool BAO, bool DIRECT>
__device__ __forceinline__ void cell_body(const chomp_config& cfg, const TabLayout& HL,
                                          const ProjLayout& L, const Epoch* __restrict__ epochs, int e,
                                          const double* __restrict__ htab, int which,
                                          const ProjDev* __restrict__ pdg,
                                          const double* __restrict__ ptab, double D_z,
                                          const double* __restrict__ ell, double* __restrict__ out,
                                          const double* __restrict__ nodes, int LT,
                                          const double* __restrict__ pk_tab, int split,
                                          int* __restrict__ deep, double* __restrict__ state,
                                          unsigned il) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ ProjDev pd;
  __shared__ double red[romberg_scratch<4, 2>()];
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&pd), reinterpret_cast<const double*>(pdg), kProjDoubles);
  __syncthreads();
  PowerEval P;
  P.stage(cfg, HL, &E, htab + (size_t)e * HL.stride, which, sm);
  ProjLds G;
  G.stage(L, pd, ptab, sm + 12 * (HL.NK - 1));
  G.bess = nullptr;
  __syncthreads();
  P.template finish_t<BAO>();
  const double l = ell[il];
  const double px0 = log(cfg.k_min), pdx = (log(cfg.k_max) - px0) / (double)kPTabN;
  CellTabIntegrand<HF, BAO, DIRECT> f{&P, nodes, (1L << LT) + 1, LT, l, log(l), pk_tab, px0, pdx,
                                      1.0 / pdx, {&P, &G, l, 1.0 / (D_z * D_z)}};
  const bool hand_over = split < cfg.divmax;
  const RombergOut<1> r = romberg_group<4, 1, CellTabIntegrand<HF, BAO, DIRECT>, 4>(
      f, pd.chi_min, pd.chi_max, cfg.global_precision, cfg.corr_precision, split, red,
      hand_over ? state + (size_t)il * kRombergDump : nullptr);
  if (threadIdx.x == 0) {
    out[il] = r.value[0];
    if (hand_over && !r.converged[0]) deep[2 + atomicAdd(&deep[0], 1)] = (int)il;
  }
}
template <bool HF, bool BAO, bool DIRECT>
// (three blocks per CU for the lean instance: 168 registers, one fewer than it would take)
__global__ __launch_bounds__(256, DIRECT ? 2 : 3) void k_cell(chomp_config cfg, TabLayout HL, ProjLayout L,
                                              const Epoch* __restrict__ epochs, int e,
                                              const double* __restrict__ htab, int which,
                                              const ProjDev* __restrict__ pdg,
                                              const double* __restrict__ ptab, double D_z,
                                              const double* __restrict__ ell,
                                              double* __restrict__ out,
                                              const double* __restrict__ nodes, int LT,
                                              const double* __restrict__ pk_tab, int split,
                                              int* __restrict__ deep, double* __restrict__ state) {
  cell_body<HF, BAO, DIRECT>(cfg, HL, L, epochs, e, htab, which, pdg, ptab, D_z, ell, out, nodes, LT,
                             pk_tab, split, deep, state, blockIdx.x);
}
// ... with an epoch axis (chomp_cell_epochs): grid (n_ell, E), block 256; row blockIdx.y integrates
// epoch e0 + blockIdx.y from its own spectrum table into out[blockIdx.y * n_ell + blockIdx.x], with
// its own states and list (pk_tab, deep, state: the first epoch's, `stride` doubles to the next).
template <bool HF, bool BAO, bool DIRECT>
__global__ __launch_bounds__(256, DIRECT ? 2 : 3) void k_cell_epochs(
    chomp_config cfg, TabLayout HL, ProjLayout L, const Epoch* __restrict__ epochs, int e0,
    const double* __restrict__ htab, int which, const ProjDev* __restrict__ pdg,
    const double* __restrict__ ptab, double D_z, const double* __restrict__ ell,
    double* __restrict__ out, const double* __restrict__ nodes, int LT,
    const double* __restrict__ pk_tab, int split, int* __restrict__ deep,
    double* __restrict__ state, size_t stride) {
  const size_t off = stride * blockIdx.y;
  cell_body<HF, BAO, DIRECT>(cfg, HL, L, epochs, e0 + (int)blockIdx.y, htab, which, pdg, ptab, D_z, ell,
                             out + (size_t)blockIdx.y * gridDim.x, nodes, LT, pk_tab + off, split,
                             deep + 2 * off, state + off, blockIdx.x);
}

// The set axis of C_l (chomp_cell_sets: one C_l per kernel -- window pair, MultiEpoch range,
// cosmology -- of a tomographic analysis or a chain over photo-z parameters).  Row y of a chunk
// integrates epoch e0 + y against projection set y of the last set-up of sets with growth D_z[y]:
// the chi range, the windows and the growth factor are the set's own, so the chi-only node table
// is the row's own too.  The work buffer holds one slab per row of the chunk at a fixed stride,
//   3 (2^LT + 1) doubles   F_j, ln chi_j, chi_j of set y   (k_cell_nodes_sets)
//   then the slab of the epoch axis above (cell_epoch_stride: P(k), states, deep list)
// and the *_sets kernels address row y's node table, spectrum table, states and list at y * stride
// from the first row's.  k_cell_ptab_epochs serves unchanged (the spectrum table depends on the
// epoch, not on the set).  A row is 1.5 MiB more than a row of the epoch axis: 34 MiB per chunk of
// 16 at 2048 multipoles, about 0.5 GiB at the chunk maximum of 256.  Per (multipole, row) the
// arithmetic is chomp_cell's after chomp_kernel_setup of the set's inputs: the same bodies.
inline size_t cell_set_stride(size_t n, int LT) {
  return 3 * (((size_t)1 << LT) + 1) + cell_epoch_stride(n);
}

// The host's plan of the C_l work buffer and launches -- what chomp_cell, chomp_cell_epochs and
// chomp_cell_sets size, place and launch by.  The first row's spectrum table, Romberg states and
// deep list (the hand-over of k_cell to k_cell_deep) sit at pk_at, state_at and deep_at in all
// three forms; they differ in what a further row of a chunk adds (`stride`):
//   single   the node table, then one slab            (doubles(1))
//   epochs   one node table, then a slab per epoch    (stride = cell_epoch_stride)
//   sets     a node table and a slab per row          (stride = cell_set_stride)
constexpr int kDeepLds = 160 * 1024 - 4096;   // dynamic LDS k_cell_deep is opted in to
struct CellPlan {
  size_t sh_nodes, sh, shd;         // dynamic LDS of k_cell_nodes, of k_cell / k_cell4, of k_cell_deep
  int deep_lds;                     // what k_cell_deep is opted in to (kDeepLds)
  bool deep_fits;                   // ... holds shd
  int LT, split;                    // levels within the node table; levels beyond `split` by k_cell_deep
  bool four;                        // k_cell4 (four multipoles to a block), not k_cell
  size_t n_nodes, stride, pk_at, state_at, deep_at;
  unsigned gnodes, gdeep;           // blocks of k_cell_nodes, of k_cell_deep
  bool per_row_nodes;
  // the doubles of the work buffer for a chunk of `rows`
  size_t doubles(size_t rows) const { return (per_row_nodes ? 0 : 3 * n_nodes) + stride * rows; }
};

// n: multipoles; one_kernel: CHOMP_TUNE_CELL_ONE_KERNEL (every level in k_cell); per_row_nodes:
// the sets form
inline CellPlan cell_plan(int divmax, int NK, const ProjLayout& L, size_t n, long long one_kernel,
                          bool per_row_nodes) {
  CellPlan P;
  P.sh_nodes = (size_t)ProjLds::doubles(L) * sizeof(double);
  P.sh = (size_t)(12 * (NK - 1)) * sizeof(double) + P.sh_nodes;
  P.shd = P.sh + (size_t)(kPTabN + 1) * sizeof(double);
  P.deep_lds = kDeepLds;
  P.deep_fits = P.shd <= (size_t)kDeepLds;
  P.LT = divmax < kCellTabLevel ? divmax : kCellTabLevel;
  P.split = (one_kernel > 0 || divmax <= kCellSplitLevel) ? divmax : kCellSplitLevel;
  P.four = P.split <= P.LT && P.split >= 6 && n >= 16;
  P.n_nodes = ((size_t)1 << P.LT) + 1;
  P.per_row_nodes = per_row_nodes;
  P.stride = per_row_nodes ? cell_set_stride(n, P.LT) : cell_epoch_stride(n);
  P.pk_at = 3 * P.n_nodes;
  P.state_at = P.pk_at + (size_t)kPTabN + 1;
  P.deep_at = P.state_at + n * kRombergDump;
  P.gnodes = (unsigned)((P.n_nodes + 255) / 256);
  P.gdeep = (unsigned)(n < 512 ? n : 512);
  return P;
}
// grid (n_ell, E), block 256: k_cell_epochs with row blockIdx.y's own set, tables, growth and nodes.
template <bool HF, bool BAO, bool DIRECT>
__global__ __launch_bounds__(256, DIRECT ? 2 : 3) void k_cell_sets(
    chomp_config cfg, TabLayout HL, ProjLayout L, const Epoch* __restrict__ epochs, int e0,
    const double* __restrict__ htab, int which, const ProjDev* __restrict__ pd,
    const double* __restrict__ ptab, size_t pstride, const double* __restrict__ D_z,
    const double* __restrict__ ell, double* __restrict__ out, const double* __restrict__ nodes,
    int LT, const double* __restrict__ pk_tab, int split, int* __restrict__ deep,
    double* __restrict__ state, size_t stride) {
  const size_t off = stride * blockIdx.y;
  cell_body<HF, BAO, DIRECT>(cfg, HL, L, epochs, e0 + (int)blockIdx.y, htab, which, pd + blockIdx.y,
                             ptab + pstride * blockIdx.y, D_z[blockIdx.y], ell,
                             out + (size_t)blockIdx.y * gridDim.x, nodes + off, LT, pk_tab + off,
                             split, deep + 2 * off, state + off, blockIdx.x);
}

// k_cell4: the same integrals, FOUR multipoles to a block -- one per wavefront up to level
// kCell4Level (romberg_wave6: a multipole that stops at level 7..8, the rule, costs two to four
// nodes per lane and no block barrier), then the block's multipoles that go on are walked by all
// four wavefronts together up to `split` (RombergResume from the rows the wavefront left), and
// what has not converged there is listed for k_cell_deep exactly as k_cell lists it.  The block's
// staging (epoch record, spectrum splines, projection tables) is shared by its four multipoles,
// and the 2048 multipoles of configs[3] / [4] are 512 blocks: resident at once, where k_cell's
// 2048 blocks took three rounds.  Wavefront w of block b takes multipole b + gridDim.x w (the
// deep ones are the highest l: one to a block).  grid ceil(n_ell / 4), block 256; the lean
// instance only (split <= LT, split >= 6).
constexpr int kCell4Level = 8;     // (7: 27.6, 8: 24.3, 9: 25.2, 10: 28.7 us per configs[3] launch)
// (the body of k_cell4 and k_cell4_epochs; bx: the block's index along the multipoles)
template <bool HF, bool BAO>
__device__ __forceinline__ void cell4_body(const chomp_config& cfg, const TabLayout& HL,
                                           const ProjLayout& L, const Epoch* __restrict__ epochs, int e,
                                           const double* __restrict__ htab, int which,
                                           const ProjDev* __restrict__ pdg,
                                           const double* __restrict__ ptab, double D_z,
                                           const double* __restrict__ ell, int n_ell,
                                           double* __restrict__ out,
                                           const double* __restrict__ nodes, int LT,
                                           const double* __restrict__ pk_tab, int split,
                                           int* __restrict__ deep, double* __restrict__ state,
                                           unsigned bx) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ ProjDev pd;
  __shared__ double red[romberg_scratch<4, 2>()];
  __shared__ double co_dump[4][kRombergDump];
  __shared__ double co_val[4];
  __shared__ int co_need[4], co_conv[4];
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&pd), reinterpret_cast<const double*>(pdg), kProjDoubles);
  __syncthreads();
  PowerEval P;
  P.stage(cfg, HL, &E, htab + (size_t)e * HL.stride, which, sm);
  ProjLds G;
  G.stage(L, pd, ptab, sm + 12 * (HL.NK - 1));
  G.bess = nullptr;
  __syncthreads();
  P.template finish_t<BAO>();
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int il = (int)bx + (int)gridDim.x * wave;
  const bool have = il < n_ell;
  const double px0 = log(cfg.k_min), pdx = (log(cfg.k_max) - px0) / (double)kPTabN;
  const double a = pd.chi_min, b = pd.chi_max;
  const bool hand_over = split < cfg.divmax;
  const int top = split < kCell4Level ? split : kCell4Level;      // (the wavefronts' own levels)
  RombergOut<1> r;
  r.value[0] = 0.0; r.level[0] = 0; r.converged[0] = true;
  if (have) {
    const double l = ell[il];
    CellTabIntegrand<HF, BAO, false> f{&P, nodes, (1L << LT) + 1, LT, l, log(l), pk_tab, px0, pdx,
                                       1.0 / pdx, {&P, &G, l, 1.0 / (D_z * D_z)}};
    double fb[1];
    f(b, fb, 0, 1L);                             // (the upper end point: node 1 of level 0)
    r = romberg_wave6<1>(f, a, b, fb, cfg.global_precision, cfg.corr_precision, top, co_dump[wave]);
  }
  if (lane == 0) {
    co_need[wave] = (have && !r.converged[0] && split > top) ? 1 : 0;
    co_val[wave] = r.value[0];
    co_conv[wave] = r.converged[0] ? 1 : 0;
  }
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    if (!co_need[w]) continue;                   // (block-uniform)
    const int ilw = (int)bx + (int)gridDim.x * w;
    const double l = ell[ilw];
    CellTabIntegrand<HF, BAO, false> f{&P, nodes, (1L << LT) + 1, LT, l, log(l), pk_tab, px0, pdx,
                                       1.0 / pdx, {&P, &G, l, 1.0 / (D_z * D_z)}};
    RombergResume R;
    R.load(co_dump[w], top, b - a, cfg.global_precision, cfg.corr_precision);
    int flip = 0;
    for (int i = top + 1; i <= split && !R.done; ++i) {
      const double c_il = CHOMP_ROMBERG_C[i][lane & 31];
      const long numtosum = 1L << (i - 1);
      const double h = ldexp(b - a, 1 - i);                    // ((b - a) / numtosum)
      const double lox = a + 0.5 * h;
      double part = 0.0;
      for (long j = threadIdx.x; j < numtosum; j += 256) {
        double v[1];
        f(lox + h * (double)j, v, i, j);
        part += v[0];
      }
      const double S = group_sum<4>(part, red, flip);
      R.advance(i, S, c_il);
    }
    __syncthreads();                             // (red: the last sum has been read)
    if (threadIdx.x < 64) {                      // (every wavefront holds the same rows)
      if (!R.done && hand_over) {
        double* st = state + (size_t)ilw * kRombergDump;
        if (lane < 32) st[lane] = R.Tl;
        if (lane == 0) { st[32] = R.ordsum; st[33] = R.prev; }
      }
      if (lane == 0) { co_val[w] = R.value; co_conv[w] = R.done ? 1 : 0; }
    }
  }
  __syncthreads();
  if (have && lane == 0) {
    out[il] = co_val[wave];
    if (hand_over && !co_conv[wave]) {
      // (a multipole that never entered the cooperative walk -- split <= kCell4Level -- hands
      //  on the rows its wavefront left)
      if (split <= top) {
        double* st = state + (size_t)il * kRombergDump;
        for (int q = 0; q < kRombergDump; ++q) st[q] = co_dump[wave][q];
      }
      deep[2 + atomicAdd(&deep[0], 1)] = il;
    }
  }
}
template <bool HF, bool BAO>
__global__ __launch_bounds__(256, 3) void k_cell4(chomp_config cfg, TabLayout HL, ProjLayout L,
                                              const Epoch* __restrict__ epochs, int e,
                                              const double* __restrict__ htab, int which,
                                              const ProjDev* __restrict__ pdg,
                                              const double* __restrict__ ptab, double D_z,
                                              const double* __restrict__ ell, int n_ell,
                                              double* __restrict__ out,
                                              const double* __restrict__ nodes, int LT,
                                              const double* __restrict__ pk_tab, int split,
                                              int* __restrict__ deep, double* __restrict__ state) {
  cell4_body<HF, BAO>(cfg, HL, L, epochs, e, htab, which, pdg, ptab, D_z, ell, n_ell, out, nodes, LT,
                      pk_tab, split, deep, state, blockIdx.x);
}
// ... with an epoch axis: grid (ceil(n_ell / 4), E), block 256; row blockIdx.y as in k_cell_epochs
// (wavefront w of block (b, y) keeps multipole b + gridDim.x w of epoch e0 + y).
template <bool HF, bool BAO>
__global__ __launch_bounds__(256, 3) void k_cell4_epochs(
    chomp_config cfg, TabLayout HL, ProjLayout L, const Epoch* __restrict__ epochs, int e0,
    const double* __restrict__ htab, int which, const ProjDev* __restrict__ pdg,
    const double* __restrict__ ptab, double D_z, const double* __restrict__ ell, int n_ell,
    double* __restrict__ out, const double* __restrict__ nodes, int LT,
    const double* __restrict__ pk_tab, int split, int* __restrict__ deep,
    double* __restrict__ state, size_t stride) {
  const size_t off = stride * blockIdx.y;
  cell4_body<HF, BAO>(cfg, HL, L, epochs, e0 + (int)blockIdx.y, htab, which, pdg, ptab, D_z, ell, n_ell,
                      out + (size_t)blockIdx.y * n_ell, nodes, LT, pk_tab + off, split, deep + 2 * off,
                      state + off, blockIdx.x);
}
// ... with a set axis: grid (ceil(n_ell / 4), E), block 256; row blockIdx.y as in k_cell_sets.
template <bool HF, bool BAO>
__global__ __launch_bounds__(256, 3) void k_cell4_sets(
    chomp_config cfg, TabLayout HL, ProjLayout L, const Epoch* __restrict__ epochs, int e0,
    const double* __restrict__ htab, int which, const ProjDev* __restrict__ pd,
    const double* __restrict__ ptab, size_t pstride, const double* __restrict__ D_z,
    const double* __restrict__ ell, int n_ell, double* __restrict__ out,
    const double* __restrict__ nodes, int LT, const double* __restrict__ pk_tab, int split,
    int* __restrict__ deep, double* __restrict__ state, size_t stride) {
  const size_t off = stride * blockIdx.y;
  cell4_body<HF, BAO>(cfg, HL, L, epochs, e0 + (int)blockIdx.y, htab, which, pd + blockIdx.y,
                      ptab + pstride * blockIdx.y, D_z[blockIdx.y], ell, n_ell,
                      out + (size_t)blockIdx.y * n_ell, nodes + off, LT, pk_tab + off, split,
                      deep + 2 * off, state + off, blockIdx.x);
}

// One node by the general route (inlined: a call would put a stack -- scratch memory -- behind
// every launch of the kernel, used or not).
template <bool HF, bool BAO>
__device__ __forceinline__ double cell_node_general(const CellTabIntegrand<HF, BAO>& f, double chi,
                                                    int lev, long j) {
  double v[1];
  f(chi, v, lev, j);
  return v[0];
}

// grid <= n_ell (blocks draw multipoles from the list until it is empty), block 512: the
// levels beyond `split` of the multipoles k_cell listed.  The spectrum table (64 KiB) is staged
// in LDS -- the second of a node's two dependent reads then costs an LDS access -- and a level's
// nodes are spread over eight wavefronts, four to a thread in flight.
// dynamic LDS: 12 (NK - 1) + ProjLds::doubles(L) + kPTabN + 1 doubles.
constexpr int kCellDeepThreads = 512;
// (the body of k_cell_deep and k_cell_deep_epochs; bx: the block's index among its list's blocks)
template <bool HF, bool BAO>
__device__ __forceinline__ void cell_deep_body(
    const chomp_config& cfg, const TabLayout& HL, const ProjLayout& L,
    const Epoch* __restrict__ epochs, int e, const double* __restrict__ htab, int which,
    const ProjDev* __restrict__ pdg, const double* __restrict__ ptab, double D_z,
    const double* __restrict__ ell, double* __restrict__ out, const double* __restrict__ nodes, int LT,
    const double* __restrict__ pk_tab, int split, int* __restrict__ deep,
    const double* __restrict__ state, unsigned bx) {
  constexpr int NW = kCellDeepThreads / 64, NT = kCellDeepThreads, U = 4;
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ ProjDev pd;
  __shared__ double red[2 * NW];
  __shared__ int item_sh;
  const int count = deep[0];
  if ((int)bx >= count) return;                         // (block-uniform)
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&pd), reinterpret_cast<const double*>(pdg), kProjDoubles);
  __syncthreads();
  PowerEval P;
  P.stage(cfg, HL, &E, htab + (size_t)e * HL.stride, which, sm);
  ProjLds G;
  double* pk_lds = G.stage(L, pd, ptab, sm + 12 * (HL.NK - 1));
  G.bess = nullptr;
  if (pk_tab != nullptr) copy_doubles(pk_lds, pk_tab, kPTabN + 1);
  __syncthreads();
  P.template finish_t<BAO>();
  const double px0 = log(cfg.k_min), pdx = (log(cfg.k_max) - px0) / (double)kPTabN;
  const double a = pd.chi_min, b = pd.chi_max;
  int flip = 0;
  for (;;) {
    __syncthreads();                                     // (the previous item's item_sh is read)
    if (threadIdx.x == 0) item_sh = atomicAdd(&deep[1], 1);
    __syncthreads();
    if (item_sh >= count) return;                        // (block-uniform)
    const int il = deep[2 + item_sh];
    const double l = ell[il];
    const CellTabIntegrand<HF, BAO> f{&P, nodes, (1L << LT) + 1, LT, l, log(l),
                                      pk_tab != nullptr ? pk_lds : nullptr, px0, pdx, 1.0 / pdx,
                                      {&P, &G, l, 1.0 / (D_z * D_z)}};
    RombergResume R;
    R.load(state + (size_t)il * kRombergDump, split, b - a, cfg.global_precision,
           cfg.corr_precision);
    for (int lv = split + 1; lv <= cfg.divmax && !R.done; ++lv) {
      const double c_il = CHOMP_ROMBERG_C[lv][threadIdx.x & 31];   // (in flight behind the nodes)
      const long numtosum = 1L << (lv - 1);
      const double h = ldexp(b - a, 1 - lv), lox = a + 0.5 * h;   // ((b - a) / numtosum)
      double part = 0.0;
      long j = threadIdx.x;
      for (; j + (U - 1) * (long)NT < numtosum; j += U * (long)NT) {
        double v[U][1];
        bool ok = true;
#pragma unroll
        for (int u = 0; u < U; ++u)
          ok = f.fast(lox + h * (double)(j + u * (long)NT), v[u], lv, j + u * (long)NT) && ok;
        if (!ok) {
          for (int u = 0; u < U; ++u)
            v[u][0] = cell_node_general<HF, BAO>(f, lox + h * (double)(j + u * (long)NT), lv,
                                                 j + u * (long)NT);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) part += v[u][0];
      }
      for (; j < numtosum; j += NT) {
        double v[1];
        if (!f.fast(lox + h * (double)j, v, lv, j))
          v[0] = cell_node_general<HF, BAO>(f, lox + h * (double)j, lv, j);
        part += v[0];
      }
      R.advance(lv, group_sum<NW>(part, red, flip), c_il);
    }
    if (threadIdx.x == 0) out[il] = R.value;
  }
}
template <bool HF, bool BAO>
__global__ __launch_bounds__(kCellDeepThreads) void k_cell_deep(
    chomp_config cfg, TabLayout HL, ProjLayout L, const Epoch* __restrict__ epochs, int e,
    const double* __restrict__ htab, int which, const ProjDev* __restrict__ pdg,
    const double* __restrict__ ptab, double D_z, const double* __restrict__ ell,
    double* __restrict__ out, const double* __restrict__ nodes, int LT,
    const double* __restrict__ pk_tab, int split, int* __restrict__ deep,
    const double* __restrict__ state) {
  cell_deep_body<HF, BAO>(cfg, HL, L, epochs, e, htab, which, pdg, ptab, D_z, ell, out, nodes, LT,
                          pk_tab, split, deep, state, blockIdx.x);
}
// ... with an epoch axis: grid (min(n_ell, 512), E), block 512; the blocks of row blockIdx.y draw
// from the list of epoch e0 + blockIdx.y alone, so what a block stages -- the epoch's splines, the
// projection tables, the epoch's spectrum table -- holds for every item it draws; a block beyond
// its list's count leaves at once.
template <bool HF, bool BAO>
__global__ __launch_bounds__(kCellDeepThreads) void k_cell_deep_epochs(
    chomp_config cfg, TabLayout HL, ProjLayout L, const Epoch* __restrict__ epochs, int e0,
    const double* __restrict__ htab, int which, const ProjDev* __restrict__ pdg,
    const double* __restrict__ ptab, double D_z, const double* __restrict__ ell, int n_ell,
    double* __restrict__ out, const double* __restrict__ nodes, int LT,
    const double* __restrict__ pk_tab, int split, int* __restrict__ deep,
    const double* __restrict__ state, size_t stride) {
  const size_t off = stride * blockIdx.y;
  cell_deep_body<HF, BAO>(cfg, HL, L, epochs, e0 + (int)blockIdx.y, htab, which, pdg, ptab, D_z, ell,
                          out + (size_t)blockIdx.y * n_ell, nodes, LT, pk_tab + off, split,
                          deep + 2 * off, state + off, blockIdx.x);
}
// ... with a set axis: grid (min(n_ell, 512), E), block 512; the blocks of row blockIdx.y draw
// from that row's list alone and stage its set's projection tables beside its epoch's splines and
// spectrum table (the levels beyond the node table evaluate windows and growth from them).
template <bool HF, bool BAO>
__global__ __launch_bounds__(kCellDeepThreads) void k_cell_deep_sets(
    chomp_config cfg, TabLayout HL, ProjLayout L, const Epoch* __restrict__ epochs, int e0,
    const double* __restrict__ htab, int which, const ProjDev* __restrict__ pd,
    const double* __restrict__ ptab, size_t pstride, const double* __restrict__ D_z,
    const double* __restrict__ ell, int n_ell, double* __restrict__ out,
    const double* __restrict__ nodes, int LT, const double* __restrict__ pk_tab, int split,
    int* __restrict__ deep, const double* __restrict__ state, size_t stride) {
  const size_t off = stride * blockIdx.y;
  cell_deep_body<HF, BAO>(cfg, HL, L, epochs, e0 + (int)blockIdx.y, htab, which, pd + blockIdx.y,
                          ptab + pstride * blockIdx.y, D_z[blockIdx.y], ell,
                          out + (size_t)blockIdx.y * n_ell, nodes + off, LT, pk_tab + off, split,
                          deep + 2 * off, state + off, blockIdx.x);
}

// ---------------------------------------------------------------------------
// Gaussian covariance of w(theta): Covariance(corr, corr), covariance.py:361-543
// ---------------------------------------------------------------------------
// Table layout of the covariance state: ln K knots | projected spectrum | its spline |
// scalars {ln_K_min, ln_K_max, D_z, chi_peak}.
struct CovLayout {
  int N, ln_K, proj, pp, lev, scal, work, total;
};
inline CovLayout make_cov_layout(int N) {
  CovLayout C;
  C.N = N;
  int o = 0;
  C.ln_K = o; o += N;
  C.proj = o; o += N;
  C.pp = o; o += 4 * (N - 1);
  C.lev = o; o += N;
  C.scal = o; o += 8;
  C.work = o; o += 2 * N;
  C.total = (o + 7) & ~7;
  return C;
}

// covariance.py:545-552 with kernel.py:1066-1071 (_halo_a_integrand)
template <bool BAO>
struct CovProjIntegrand {
  const PowerEval* P;
  const ProjLds* G;
  double K, norm;
  __device__ __forceinline__ double operator()(double chi) const {
    const double D = G->me.growth_factor(G->me.redshift(chi));
    // Where the lower limit is chi = K / k_max (the large-K knots), the end point's wavenumber
    // K / (K / k_max) is k_max or the double above it, by the luck of two roundings -- and halo
    // spectra are zero above k_max (halo.py:649-672): half an end-point value more or less in
    // every trapezoid sum, four Romberg levels and 1e-6 of the knot.  The reference's own knots
    // (G12) all sit on the k_max side; a wavenumber within 2^-50 above k_max is k_max here.
    double k = K / chi;
    if (k > P->k_max && k <= P->k_max * (1.0 + 8.9e-16)) k = P->k_max;
    return norm * P->template eval_t<BAO>(k) * (G->wa(chi) * G->wb(chi) * D * D / (chi * chi));
  }
};

// grid N (= kernel_npoints), block 256: one ln K knot of Covariance._halo_a_spline per
// workgroup (covariance.py:455-543, the matching_corrs branch).
// (the body of k_cov_proj_knots and of a diagonal block of k_cov_blocks_knots: the sources are
//  the epoch record `ep` with its knot-table slab `htab`, the ProjDev block `pdg` with its
//  projection slab `ptab`; the destination the slab `ctab` of layout C)
template <bool BAO>
__device__ __forceinline__ void cov_proj_knots_body(const chomp_config& cfg, const TabLayout& HL,
                                                    const ProjLayout& L, const CovLayout& C,
                                                    const Epoch* __restrict__ ep,
                                                    const double* __restrict__ htab, int which,
                                                    const ProjDev* __restrict__ pdg,
                                                    const double* __restrict__ ptab,
                                                    double D_z, double* __restrict__ ctab) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ ProjDev pd;
  __shared__ double red[romberg_scratch<4, 2>()];
  __shared__ double chi_peak_s;
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(ep),
               kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&pd), reinterpret_cast<const double*>(pdg), kProjDoubles);
  __syncthreads();
  PowerEval P;
  P.stage(cfg, HL, &E, htab, which, sm);
  ProjLds G;
  G.stage(L, pd, ptab, sm + 12 * (HL.NK - 1));
  G.bess = nullptr;
  if (threadIdx.x == 0)                                  // :466: a growth factor used as z
    chi_peak_s = me_view(L, pd, ptab, 0).comoving_distance(D_z);
  __syncthreads();
  P.template finish_t<BAO>();
  const int i = blockIdx.x;
  // pd.chi_min / chi_max are Covariance._chi_min_a / _chi_max_a (:132-141 = kernel.py:610-612)
  const double ln_K_min = log(cfg.k_min * pd.chi_min), ln_K_max = log(cfg.k_max * pd.chi_max);
  const double ln_K = linspace_at(ln_K_min, ln_K_max, C.N, i);
  const double K = exp(ln_K);
  double chi_min = K / cfg.k_max, chi_max = K / cfg.k_min;
  if (chi_min < pd.chi_min) chi_min = pd.chi_min;
  if (chi_max > pd.chi_max) chi_max = pd.chi_max;
  CovProjIntegrand<BAO> f{&P, &G, K, 1.0};
  const double norm_int = f(chi_peak_s);
  f.norm = norm_int > 0.0 ? 1.0 / norm_int : 1.0;
  int level = 0;
  const double v = romberg1<4>(f, chi_min, chi_max, cfg.global_precision, cfg.corr_precision,
                               cfg.divmax, red, &level);
  if (threadIdx.x == 0) {
    ctab[C.ln_K + i] = ln_K;
    ctab[C.proj + i] = v / f.norm;
    ctab[C.lev + i] = (double)level;
    if (i == 0) {
      ctab[C.scal + 0] = ln_K_min;
      ctab[C.scal + 1] = ln_K_max;
      ctab[C.scal + 2] = D_z;
      ctab[C.scal + 3] = chi_peak_s;
    }
  }
}
template <bool BAO>
__global__ __launch_bounds__(256) void k_cov_proj_knots(chomp_config cfg, TabLayout HL,
                                                        ProjLayout L, CovLayout C,
                                                        const Epoch* __restrict__ epochs, int e,
                                                        const double* __restrict__ htab, int which,
                                                        const ProjDev* __restrict__ pdg,
                                                        const double* __restrict__ ptab,
                                                        double D_z, double* __restrict__ ctab) {
  cov_proj_knots_body<BAO>(cfg, HL, L, C, epochs + e, htab + (size_t)e * HL.stride, which, pdg,
                           ptab, D_z, ctab);
}

// (the body of k_cov_spline and of a diagonal block of k_cov_blocks_spline; one thread)
__device__ __forceinline__ void cov_spline_body(const CovLayout& C, double* __restrict__ ctab) {
  spline_build(ctab + C.ln_K, ctab + C.proj, C.N, ctab + C.pp, ctab + C.work);
}
__global__ void k_cov_spline(CovLayout C, double* __restrict__ ctab) {
  if (threadIdx.x == 0 && blockIdx.x == 0) cov_spline_body(C, ctab);
}

// covariance.py:397-453 (_covariance_G_integrand, matching_corrs: the second two-point
// term repeats the first)
struct CovGIntegrand {
  const double *xk, *pp;
  int N;
  const BesselTab* B;
  double theta_a, theta_b, inv_D2, poiss_a, poiss_b, norm;
  __device__ __forceinline__ double operator()(double ln_K) const {
    const double K = exp(ln_K);
    const double s = spline_eval(xk, pp, N, log(K));
    const double Pa = s * inv_D2, Pb = s * inv_D2;
    const double t1 = Pa * Pb + Pa * poiss_b + Pb * poiss_a;
    return K * K * norm * (t1 + t1) * bessel_j<0>(K * theta_a, *B) * bessel_j<0>(K * theta_b, *B);
  }
};

// grid n pairs, block 256: Covariance.covariance_G(theta_a, theta_b) (covariance.py:361-395).
// (the body of k_cov_gaussian and of a diagonal block of k_cov_blocks_gaussian: pair blockIdx.x
//  of theta_a / theta_b from the tables of the slab `ctab` into out[blockIdx.x])
__device__ __forceinline__ void cov_gaussian_body(const chomp_config& cfg, const CovLayout& C,
                                                  const double* __restrict__ ctab,
                                                  const BesselTab* __restrict__ bess_g,
                                                  double j0_limit, double area,
                                                  double poiss_a, double poiss_b,
                                                  const double* __restrict__ theta_a,
                                                  const double* __restrict__ theta_b,
                                                  double* __restrict__ out,
                                                  double* __restrict__ levels) {
  extern __shared__ __align__(16) double sm[];
  __shared__ BesselTab B;
  __shared__ double red[romberg_scratch<4, 2>()];
  double* xk = sm;
  double* pp = sm + C.N;
  copy_doubles(xk, ctab + C.ln_K, C.N);
  copy_doubles(pp, ctab + C.pp, 4 * (C.N - 1));
  copy_doubles(reinterpret_cast<double*>(&B), reinterpret_cast<const double*>(bess_g),
               (int)(sizeof(BesselTab) / sizeof(double)));
  __syncthreads();
  const double ln_K_min = ctab[C.scal + 0], ln_K_hi = ctab[C.scal + 1], D_z = ctab[C.scal + 2];
  const double ta = theta_a[blockIdx.x], tb = theta_b[blockIdx.x];
  double ln_K_max = log(fmax(j0_limit / ta, j0_limit / tb));
  double v = 0.0;
  int level = 0;
  if (ln_K_max > ln_K_hi) ln_K_max = ln_K_hi;
  if (ln_K_max > ln_K_min) {
    CovGIntegrand f{xk, pp, C.N, &B, 0.0, 0.0, 1.0 / (D_z * D_z), poiss_a, poiss_b, 1.0};
    const double norm = 1.0 / f(0.0);                    // :390
    f.theta_a = ta;
    f.theta_b = tb;
    f.norm = norm;
    v = romberg1<4>(f, ln_K_min, ln_K_max, cfg.global_precision, cfg.corr_precision,
                    cfg.divmax, red, &level) / (norm * 2.0 * kPi * area);
  }
  if (threadIdx.x == 0) {
    out[blockIdx.x] = v;
    if (levels) levels[blockIdx.x] = (double)level;
  }
}
__global__ __launch_bounds__(256) void k_cov_gaussian(chomp_config cfg, CovLayout C,
                                                      const double* __restrict__ ctab,
                                                      const BesselTab* __restrict__ bess_g,
                                                      double j0_limit, double area,
                                                      double poiss_a, double poiss_b,
                                                      const double* __restrict__ theta_a,
                                                      const double* __restrict__ theta_b,
                                                      double* __restrict__ out,
                                                      double* __restrict__ levels) {
  cov_gaussian_body(cfg, C, ctab, bess_g, j0_limit, area, poiss_a, poiss_b, theta_a, theta_b, out,
                    levels);
}

// ---------------------------------------------------------------------------
// Gaussian cross-covariance of two w(theta): Covariance(corr_a, corr_b), the matching_corrs ==
// False branch (covariance.py:422-453, 495-541)
// ---------------------------------------------------------------------------
// A cross block needs two projection set-ups (four windows) and two P(k) epochs at once, and a
// context holds one of each: the block's context keeps a snapshot ("slot") of each side --
// slot 0 correlation a, slot 1 correlation b -- taken from whichever context holds that side
// (chomp_covariance_cross_stage): the epoch record, the epoch's knot tables, the projection
// scalars and the projection tables.  Behind the slots: ln K knots | the four projected spectra
// a, b, ab, ba | their splines | their Romberg levels | scalars {ln_K_min, ln_K_max, D_a, D_b,
// chi_peak_a, chi_peak_b} | spline_build's work, per table.
constexpr int kCrossA = 0, kCrossB = 1, kCrossAB = 2, kCrossBA = 3;
struct CrossLayout {
  int N, ep[2], htab[2], pd[2], ptab[2];
  int ln_K, proj[4], pp[4], lev[4], scal, work[4], total;
};
inline CrossLayout make_cross_layout(int N, int h_stride, int p_total) {
  CrossLayout C;
  C.N = N;
  int o = 0;
  for (int s = 0; s < 2; ++s) {
    C.ep[s] = o; o += kEpochDoubles;
    C.htab[s] = o; o += h_stride;
    C.pd[s] = o; o += kProjDoubles;
    C.ptab[s] = o; o += p_total;
    o = (o + 1) & ~1;
  }
  C.ln_K = o; o += N;
  for (int t = 0; t < 4; ++t) {
    C.proj[t] = o; o += N;
    C.pp[t] = o; o += 4 * (N - 1);
    C.lev[t] = o; o += N;
    C.work[t] = o; o += 2 * N;
  }
  C.scal = o; o += 8;
  C.total = (o + 7) & ~7;
  return C;
}
struct CrossState {
  DeviceBuffer<double> d;  // the block of CrossLayout
  CrossLayout C;
  bool staged[2] = {false, false};   // slot holds a snapshot (chomp_covariance_cross_stage)
  int which[2] = {0, 0};   // ... of this spectrum
  bool response[2] = {false, false};   // ... whose knot tables hold the super-sample response
  double z_min[2] = {0, 0}, z_max[2] = {0, 0};   // ... and this redshift range of its two windows
  bool ready = false;      // the four tables and their splines (chomp_covariance_table_cross) valid
};
// Dynamic LDS of k_cov_cross_knots, in doubles: two PowerEval stagings, the MultiEpoch of
// ProjLds and four window splines.
inline int cov_cross_lds_doubles(int NK_halo, const ProjLayout& L) {
  return 24 * (NK_halo - 1) + L.NC + 8 * (L.NC - 1) + 16 * (L.NWp - 1);
}

// covariance.py:545-591 with kernel.py:1075-1101: the integrand of table T.  a and b take their
// own spectrum, ab and ba the geometric mean of the two; the windows are (a1, a2), (b1, b2),
// (a1, b2), (a2, b1); the growth factor and z(chi) are those of correlation a's MultiEpoch
// (Covariance.kernel.cosmo) throughout.  The end-point guard is CovProjIntegrand's.
template <bool BAO>
struct CovCrossIntegrand {
  const PowerEval *Pa, *Pb;
  const MEView* me;
  const WindowView* w;             // a1, a2, b1, b2
  int T;
  double K, norm;
  __device__ __forceinline__ double operator()(double chi) const {
    const double D = me->growth_factor(me->redshift(chi));
    double k = K / chi;
    if (k > Pa->k_max && k <= Pa->k_max * (1.0 + 8.9e-16)) k = Pa->k_max;
    double power, ww;
    if (T == kCrossA) {
      power = Pa->template eval_t<BAO>(k);
      ww = w[0](chi) * w[1](chi);
    } else if (T == kCrossB) {
      power = Pb->template eval_t<BAO>(k);
      ww = w[2](chi) * w[3](chi);
    } else {
      power = sqrt(Pa->template eval_t<BAO>(k) * Pb->template eval_t<BAO>(k));
      ww = T == kCrossAB ? w[0](chi) * w[3](chi) : w[1](chi) * w[2](chi);
    }
    return norm * power * (ww * D * D / (chi * chi));
  }
};

// grid (N = kernel_npoints, 4 tables), block 256: knot x of table y of
// Covariance._initialize_halo_splines (covariance.py:455-531).  LDS: cov_cross_lds_doubles.
// (the body of k_cov_cross_knots and of a cross block of k_cov_blocks_knots: per side the epoch
//  record, its knot-table slab, the ProjDev block and its projection slab; the destination is
//  the table part of the slab `ct` of layout C -- the body reads none of C's source offsets)
template <bool BAO>
__device__ __forceinline__ void cov_cross_knots_body(
    const chomp_config& cfg, const TabLayout& HL, const ProjLayout& L, const CrossLayout& C,
    const double* __restrict__ epa, const double* __restrict__ epb,
    const double* __restrict__ hta, const double* __restrict__ htb,
    const double* __restrict__ pdga, const double* __restrict__ pdgb,
    const double* __restrict__ pta, const double* __restrict__ ptb, int which_a, int which_b,
    double D_a, double D_b, double* __restrict__ ct) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch Ea, Eb;
  __shared__ ProjDev pda, pdb;
  __shared__ double red[romberg_scratch<4, 2>()];
  __shared__ double sc[4];         // chi_peak_a, chi_peak_b, chi_min_b, chi_max_b
  copy_doubles(reinterpret_cast<double*>(&Ea), epa, kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&Eb), epb, kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&pda), pdga, kProjDoubles);
  copy_doubles(reinterpret_cast<double*>(&pdb), pdgb, kProjDoubles);
  __syncthreads();
  PowerEval Pa, Pb;
  Pa.stage(cfg, HL, &Ea, hta, which_a, sm);
  Pb.stage(cfg, HL, &Eb, htb, which_b, sm + 12 * (HL.NK - 1));
  const int NC = L.NC, NW = L.NWp;
  double* chi_t = sm + 24 * (HL.NK - 1);                // [NC]
  double* pp_z = chi_t + NC;                            // [4 (NC - 1)]
  double* pp_g = pp_z + 4 * (NC - 1);
  double* wpp = pp_g + 4 * (NC - 1);                    // 4 x [4 (NW - 1)]
  copy_doubles(chi_t, pta + L.me_chi[0], NC);
  copy_doubles(pp_z, pta + L.me_pp_z[0], 4 * (NC - 1));
  copy_doubles(pp_g, pta + L.me_pp_g[0], 4 * (NC - 1));
  for (int q = 0; q < 4; ++q)
    copy_doubles(wpp + q * 4 * (NW - 1), (q < 2 ? pta : ptb) + L.w_pp[q & 1], 4 * (NW - 1));
  const MEView me{nullptr, chi_t, nullptr, pp_z, pp_g, NC, pda.me_z_min[0], pda.me_z_max[0]};
  WindowView w[4];
  for (int q = 0; q < 4; ++q) {
    const ProjDev& pd = q < 2 ? pda : pdb;
    w[q] = WindowView{wpp + q * 4 * (NW - 1), NW, pd.w_chi_min[q & 1], pd.w_chi_max[q & 1]};
  }
  if (threadIdx.x == 0) {
    const MEView g = me_view(L, pda, pta, 0);
    sc[0] = g.comoving_distance(D_a);                    // :470-471: growth factors used as z
    sc[1] = g.comoving_distance(D_b);
    // :129-140: b's redshift range on a's MultiEpoch
    const double c0 = g.comoving_distance(pdb.z_min);
    sc[2] = cfg.window_precision > c0 ? cfg.window_precision : c0;
    sc[3] = g.comoving_distance(pdb.z_max);
  }
  __syncthreads();
  Pa.template finish_t<BAO>();
  Pb.template finish_t<BAO>();
  const int i = blockIdx.x, T = blockIdx.y;
  const double chi_min_a = pda.chi_min, chi_max_a = pda.chi_max;
  const double chi_min_b = sc[2], chi_max_b = sc[3];
  const double ln_K_min = log(fmin(cfg.k_min * chi_min_a, cfg.k_min * chi_min_b));   // :162-167
  const double ln_K_max = log(fmax(cfg.k_max * chi_max_a, cfg.k_max * chi_max_b));
  const double ln_K = linspace_at(ln_K_min, ln_K_max, C.N, i);
  const double K = exp(ln_K);
  double chi_min = K / cfg.k_max, chi_max = K / cfg.k_min;
  if (T != kCrossA) {
    if (chi_min < chi_min_b) chi_min = chi_min_b;
    if (chi_max > chi_max_b) chi_max = chi_max_b;
  }
  if (T != kCrossB) {                                    // (ab, ba: b's limits, then a's, :512-515)
    if (chi_min < chi_min_a) chi_min = chi_min_a;
    if (chi_max > chi_max_a) chi_max = chi_max_a;
  }
  CovCrossIntegrand<BAO> f{&Pa, &Pb, &me, w, kCrossA, K, 1.0};
  const double peak_a = f(sc[0]);
  f.T = kCrossB;
  const double peak_b = f(sc[1]);
  const double norm_int = T == kCrossA ? peak_a : (T == kCrossB ? peak_b : sqrt(peak_a * peak_b));
  f.T = T;
  f.norm = norm_int > 0.0 ? 1.0 / norm_int : 1.0;
  int level = 0;
  const double v = romberg1<4>(f, chi_min, chi_max, cfg.global_precision, cfg.corr_precision,
                               cfg.divmax, red, &level);
  if (threadIdx.x == 0) {
    if (T == 0) ct[C.ln_K + i] = ln_K;
    ct[C.proj[T] + i] = v / f.norm;
    ct[C.lev[T] + i] = (double)level;
    if (i == 0 && T == 0) {
      ct[C.scal + 0] = ln_K_min;
      ct[C.scal + 1] = ln_K_max;
      ct[C.scal + 2] = D_a;
      ct[C.scal + 3] = D_b;
      ct[C.scal + 4] = sc[0];
      ct[C.scal + 5] = sc[1];
    }
  }
}
template <bool BAO>
__global__ __launch_bounds__(256) void k_cov_cross_knots(chomp_config cfg, TabLayout HL,
                                                         ProjLayout L, CrossLayout C, int which_a,
                                                         int which_b, double D_a, double D_b,
                                                         double* __restrict__ ct) {
  cov_cross_knots_body<BAO>(cfg, HL, L, C, ct + C.ep[0], ct + C.ep[1], ct + C.htab[0],
                            ct + C.htab[1], ct + C.pd[0], ct + C.pd[1], ct + C.ptab[0],
                            ct + C.ptab[1], which_a, which_b, D_a, D_b, ct);
}

// grid 4, block 64: the not-a-knot spline of table blockIdx.x (covariance.py:533-541).
// (the body of k_cov_cross_spline and of a cross block of k_cov_blocks_spline; one thread)
__device__ __forceinline__ void cov_cross_spline_body(const CrossLayout& C,
                                                      double* __restrict__ ct, int T) {
  spline_build(ct + C.ln_K, ct + C.proj[T], C.N, ct + C.pp[T], ct + C.work[T]);
}
__global__ void k_cov_cross_spline(CrossLayout C, double* __restrict__ ct) {
  const int T = blockIdx.x;
  if (threadIdx.x == 0 && T < 4) cov_cross_spline_body(C, ct, T);
}

// covariance.py:422-453 (_covariance_G_integrand, matching_corrs == False): two two-point terms
// from the four projected spectra; poiss[p] = proj_power_poisson(window_pair = p).
struct CovCrossGIntegrand {
  const double *xk, *pp;           // pp: the four splines, 4 (N - 1) doubles each
  int N;
  const BesselTab* B;
  double theta_a, theta_b, inv_Da, inv_Db, poiss[4], norm;
  __device__ __forceinline__ double operator()(double ln_K) const {
    const double K = exp(ln_K);
    const double x = log(K);
    const int M = 4 * (N - 1);
    const double Pa = spline_eval(xk, pp, N, x) * (inv_Da * inv_Da);
    const double Pb = spline_eval(xk, pp + M, N, x) * (inv_Db * inv_Db);
    const double Pab = spline_eval(xk, pp + 2 * M, N, x) * (inv_Da * inv_Db);
    const double Pba = spline_eval(xk, pp + 3 * M, N, x) * (inv_Da * inv_Db);
    const double t1 = Pa * Pb + Pa * poiss[2] + Pb * poiss[0];
    const double t2 = Pab * Pba + Pab * poiss[1] + Pba * poiss[3];
    return K * K * norm * (t1 + t2) * bessel_j<0>(K * theta_a, *B) * bessel_j<0>(K * theta_b, *B);
  }
};

// grid n pairs, block 256: Covariance.covariance_G(theta_a, theta_b) of a cross block
// (covariance.py:361-390).  LDS: N + 16 (N - 1) doubles.
// (the body of k_cov_cross_gaussian and of a cross block of k_cov_blocks_gaussian)
__device__ __forceinline__ void cov_cross_gaussian_body(const chomp_config& cfg,
                                                        const CrossLayout& C,
                                                        const double* __restrict__ ct,
                                                        const BesselTab* __restrict__ bess_g,
                                                        double j0_limit, double area,
                                                        double poiss0, double poiss1,
                                                        double poiss2, double poiss3,
                                                        const double* __restrict__ theta_a,
                                                        const double* __restrict__ theta_b,
                                                        double* __restrict__ out,
                                                        double* __restrict__ levels) {
  extern __shared__ __align__(16) double sm[];
  __shared__ BesselTab B;
  __shared__ double red[romberg_scratch<4, 2>()];
  const int M = 4 * (C.N - 1);
  double* xk = sm;
  double* pp = sm + C.N;
  copy_doubles(xk, ct + C.ln_K, C.N);
  for (int t = 0; t < 4; ++t) copy_doubles(pp + t * M, ct + C.pp[t], M);
  copy_doubles(reinterpret_cast<double*>(&B), reinterpret_cast<const double*>(bess_g),
               (int)(sizeof(BesselTab) / sizeof(double)));
  __syncthreads();
  const double ln_K_min = ct[C.scal + 0], ln_K_hi = ct[C.scal + 1];
  const double D_a = ct[C.scal + 2], D_b = ct[C.scal + 3];
  const double ta = theta_a[blockIdx.x], tb = theta_b[blockIdx.x];
  double ln_K_max = log(fmax(j0_limit / ta, j0_limit / tb));
  double v = 0.0;
  int level = 0;
  if (ln_K_max > ln_K_hi) ln_K_max = ln_K_hi;
  if (ln_K_max > ln_K_min) {
    CovCrossGIntegrand f{xk, pp, C.N, &B, 0.0, 0.0, 1.0 / D_a, 1.0 / D_b,
                         {poiss0, poiss1, poiss2, poiss3}, 1.0};
    const double norm = 1.0 / f(0.0);                    // :383
    f.theta_a = ta;
    f.theta_b = tb;
    f.norm = norm;
    v = romberg1<4>(f, ln_K_min, ln_K_max, cfg.global_precision, cfg.corr_precision,
                    cfg.divmax, red, &level) / (norm * 2.0 * kPi * area);
  }
  if (threadIdx.x == 0) {
    out[blockIdx.x] = v;
    if (levels) levels[blockIdx.x] = (double)level;
  }
}
__global__ __launch_bounds__(256) void k_cov_cross_gaussian(chomp_config cfg, CrossLayout C,
                                                            const double* __restrict__ ct,
                                                            const BesselTab* __restrict__ bess_g,
                                                            double j0_limit, double area,
                                                            double poiss0, double poiss1,
                                                            double poiss2, double poiss3,
                                                            const double* __restrict__ theta_a,
                                                            const double* __restrict__ theta_b,
                                                            double* __restrict__ out,
                                                            double* __restrict__ levels) {
  cov_cross_gaussian_body(cfg, C, ct, bess_g, j0_limit, area, poiss0, poiss1, poiss2, poiss3,
                          theta_a, theta_b, out, levels);
}

// ---------------------------------------------------------------------------
// The block axis of the Gaussian covariance (chomp_covariance_blocks: every block of a
// CovarianceMulti, covariance.py:796-871, in one call)
// ---------------------------------------------------------------------------
// n correlations give n (n + 1) / 2 blocks (i, j), i <= j, in the row-major order of the upper
// triangle -- the order of CovarianceMulti.covariance_list.  With one projection set per
// correlation on the set axis (chomp_kernel_setup_pairs) and one P(k) epoch per correlation in the
// context, block (i, j) reads set i, set j, epoch i and epoch j where they lie: no snapshot.  The
// kernels below run the bodies of the single-block kernels above, a diagonal block (i == j) those
// of the matching path and a cross block those of the cross path -- the same code, so the same
// bits -- with the block as a grid dimension; the branch is uniform in a workgroup.
//
// Every block owns one slab of BlocksLayout's doubles: the table part of CrossLayout (ln K knots
// | per table the projected spectrum, its spline, its Romberg levels and spline_build's work |
// 8 scalars).  A diagonal block uses table 0 alone and holds the scalars of CovLayout
// {ln_K_min, ln_K_max, D_z, chi_peak}, a cross block those of CrossLayout {ln_K_min, ln_K_max,
// D_a, D_b, chi_peak_a, chi_peak_b}; scalars 6 and 7 are D_a and D_b as k_cov_blocks_prep found
// them (the knots kernel takes them from there, and rewrites neither).
// The index block of a call, ints: epoch[n_corr] | (i, j)[n_blocks].
inline CrossLayout make_blocks_layout(int N) {
  CrossLayout C = make_cross_layout(N, 0, 0);
  const int base = C.ln_K;         // (no snapshots in front of the tables)
  for (int s = 0; s < 2; ++s) C.ep[s] = C.htab[s] = C.pd[s] = C.ptab[s] = -1;
  C.ln_K -= base;
  for (int t = 0; t < 4; ++t) {
    C.proj[t] -= base; C.pp[t] -= base; C.lev[t] -= base; C.work[t] -= base;
  }
  C.scal -= base;
  C.total = (C.scal + 8 + 7) & ~7;
  return C;
}
constexpr int kBlocksScalDa = 6, kBlocksScalDb = 7;
// The state of chomp_covariance_blocks, beside ProjState and CrossState (which it never touches).
// The buffers are kept across calls and only grow.
struct BlocksState {
  DeviceBuffer<double> d;  // n_blocks slabs of C.total doubles
  StagedBuffer<int> d_index;   // the index block
  CrossLayout C;
  size_t n_corr = 0;       // correlations of the last call (0: none yet)
};
// Table 0 of a block's slab as the matching path's layout.
__host__ __device__ inline CovLayout blocks_cov_layout(const CrossLayout& C) {
  CovLayout D;
  D.N = C.N; D.ln_K = C.ln_K; D.proj = C.proj[0]; D.pp = C.pp[0]; D.lev = C.lev[0];
  D.scal = C.scal; D.work = C.work[0]; D.total = C.total;
  return D;
}

// grid ceil(n_blocks / 64), block 64, a thread per block: the growth factors of block (i, j) --
// D_a = D(z_bar_i) of set i (Correlation._growth_at_z_bar, correlation.py:94), D_b the growth
// factor of set i's MultiEpoch 0 at set j's z_bar with MultiEpoch's range rule
// (covariance.py:468-469: Covariance.kernel.cosmo is correlation a's) -- and the other scalars
// cleared, so that a slab never shows what an earlier call left.
__global__ __launch_bounds__(64) void k_cov_blocks_prep(ProjLayout L, CrossLayout C, int n_corr,
                                                        int n_blocks,
                                                        const ProjDev* __restrict__ pd,
                                                        const double* __restrict__ ptab,
                                                        size_t pstride,
                                                        const int* __restrict__ index,
                                                        double* __restrict__ slabs) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= n_blocks) return;
  const int i = index[n_corr + 2 * b], j = index[n_corr + 2 * b + 1];
  double* sc = slabs + (size_t)b * C.total + C.scal;
  const double D_a = pd[i].D_zbar;
  const double D_b =
      i == j ? D_a : me_view(L, pd[i], ptab + pstride * i, 0).growth_factor(pd[j].z_bar);
  for (int q = 0; q < 6; ++q) sc[q] = 0.0;
  sc[kBlocksScalDa] = D_a;
  sc[kBlocksScalDb] = D_b;
}

// grid (N = kernel_npoints, 4 tables, n_blocks), block 256: k_cov_cross_knots for a cross block
// -- side a (epoch i, set i), side b (epoch j, set j) --, k_cov_proj_knots in the y == 0
// workgroups of a diagonal block.  LDS: cov_cross_lds_doubles (the larger of the two).
template <bool BAO>
__global__ __launch_bounds__(256) void k_cov_blocks_knots(
    chomp_config cfg, TabLayout HL, ProjLayout L, CrossLayout C, int n_corr,
    const Epoch* __restrict__ epochs, const double* __restrict__ htab, int which,
    const ProjDev* __restrict__ pd, const double* __restrict__ ptab, size_t pstride,
    const int* __restrict__ index, double* __restrict__ slabs) {
  const int b = blockIdx.z;
  const int i = index[n_corr + 2 * b], j = index[n_corr + 2 * b + 1];
  double* ct = slabs + (size_t)b * C.total;
  const double D_a = ct[C.scal + kBlocksScalDa], D_b = ct[C.scal + kBlocksScalDb];
  const int ea = index[i], eb = index[j];
  if (i == j) {
    if (blockIdx.y != 0) return;
    cov_proj_knots_body<BAO>(cfg, HL, L, blocks_cov_layout(C), epochs + ea,
                             htab + (size_t)ea * HL.stride, which, pd + i, ptab + pstride * i, D_a,
                             ct);
    return;
  }
  cov_cross_knots_body<BAO>(
      cfg, HL, L, C, reinterpret_cast<const double*>(epochs + ea),
      reinterpret_cast<const double*>(epochs + eb), htab + (size_t)ea * HL.stride,
      htab + (size_t)eb * HL.stride, reinterpret_cast<const double*>(pd + i),
      reinterpret_cast<const double*>(pd + j), ptab + pstride * i, ptab + pstride * j, which,
      which, D_a, D_b, ct);
}

// grid (4, n_blocks), block 64: the serial spline_build of table x of block y, as k_cov_spline /
// k_cov_cross_spline run it (a diagonal block has table 0 alone).
__global__ void k_cov_blocks_spline(CrossLayout C, int n_corr, const int* __restrict__ index,
                                    double* __restrict__ slabs) {
  const int T = blockIdx.x, b = blockIdx.y;
  if (threadIdx.x != 0 || T >= 4) return;
  double* ct = slabs + (size_t)b * C.total;
  if (index[n_corr + 2 * b] == index[n_corr + 2 * b + 1]) {
    if (T == 0) cov_spline_body(blocks_cov_layout(C), ct);
    return;
  }
  cov_cross_spline_body(C, ct, T);
}

// grid (n_pairs, n_blocks), block 256: covariance_G of pair x of block y -- k_cov_cross_gaussian
// for a cross block, k_cov_gaussian (with proj_power_poisson(0) and (2)) for a diagonal one.
// poisson [n_blocks][4]; out [n_blocks][n_pairs].  LDS: N + 16 (N - 1) doubles.
__global__ __launch_bounds__(256) void k_cov_blocks_gaussian(
    chomp_config cfg, CrossLayout C, int n_corr, const int* __restrict__ index,
    const double* __restrict__ slabs, const BesselTab* __restrict__ bess_g, double j0_limit,
    double area, const double* __restrict__ poisson, const double* __restrict__ theta_a,
    const double* __restrict__ theta_b, double* __restrict__ out) {
  const int b = blockIdx.y;
  const double* ct = slabs + (size_t)b * C.total;
  const double* p = poisson + 4 * (size_t)b;
  double* o = out + (size_t)b * gridDim.x;
  if (index[n_corr + 2 * b] == index[n_corr + 2 * b + 1]) {
    cov_gaussian_body(cfg, blocks_cov_layout(C), ct, bess_g, j0_limit, area, p[0], p[2], theta_a,
                      theta_b, o, nullptr);
    return;
  }
  cov_cross_gaussian_body(cfg, C, ct, bess_g, j0_limit, area, p[0], p[1], p[2], p[3], theta_a,
                          theta_b, o, nullptr);
}

}  // namespace chomp
