// TEST-ONLY harness: the third device counterpart of tests/hostcheck.  One HIP translation unit
// that compiles the product's header chain (chomp_cov_kernels.h down to chomp_math.h) FOR THE
// DEVICE, with the product's compiler flags, and drives the projection and covariance layers
// piece by piece: the moment route of w(theta) (k_wtheta_moments, k_wtheta_fast and their epoch
// forms, on a node table, a kernel piecewise cubic and segment counts handed in), k_kernel_eval,
// the bicubic tables (k_ssc_bicubic / k_ssc_eval / SscRow, k_ng_bicubic / k_ng_eval) and
// HaloFit's quintic derivatives in both device forms.  It launches the product's own
// __global__ kernels with the product's launch shapes and buffer sizes; the two thin kernels
// below exist only where the product has no kernel of its own around a device function.  It
// includes the headers themselves, never copies of their functions.  Never loaded by the
// chomp_amd package, not in _lib.UNITS, no part of the C ABI.  Built and loaded by
// tests/devcheck_build.py.
//
// Every entry point allocates its buffers, launches, synchronises, returns the HIP error code
// (0: success; -1: an argument outside what the buffers were sized for) and frees its buffers,
// unless it is a plain getter.  The w(theta) work buffer is filled with NaN bytes before the
// moment kernel runs, as the product's is never cleared: a value k_wtheta_fast uses but
// k_wtheta_moments never wrote poisons the result.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../chomp_amd/csrc/chomp_cov_kernels.h"

namespace {

// ---------------------------------------------------------------------------------------
// host plumbing (as devphys.hip)
// ---------------------------------------------------------------------------------------
struct Dev {
  double* p = nullptr;
  hipError_t err = hipSuccess;
  size_t n;
  Dev(size_t n_, const double* host) : n(n_ ? n_ : 1) {
    err = hipMalloc((void**)&p, n * sizeof(double));
    if (err == hipSuccess && host != nullptr && n_ > 0)
      err = hipMemcpy(p, host, n_ * sizeof(double), hipMemcpyHostToDevice);
    else if (err == hipSuccess)
      err = hipMemset(p, 0, n * sizeof(double));
  }
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t back(double* host, size_t count) const {
    return hipMemcpy(host, p, count * sizeof(double), hipMemcpyDeviceToHost);
  }
  hipError_t put(size_t at, const double* host, size_t count) {
    if (at + count > n) return hipErrorInvalidValue;
    return hipMemcpy(p + at, host, count * sizeof(double), hipMemcpyHostToDevice);
  }
  hipError_t nan_fill() { return hipMemset(p, 0xFF, n * sizeof(double)); }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
};
#define DJ_TRY(expr)                            \
  do {                                          \
    const hipError_t e_ = (expr);               \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)
#define DJ_SYNC()                               \
  do {                                          \
    DJ_TRY(hipGetLastError());                  \
    DJ_TRY(hipDeviceSynchronize());             \
  } while (0)

// (chomp_capi.hip's)
dim3 grid_1d(size_t n) { return dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)); }

constexpr int kProjNC = 4, kProjNWp = 4;          // the layout's other tables: unused, small

// The projection tables with only what the kernels under test read: k_pp and the two range
// scalars.
struct KernelTab {
  chomp::ProjLayout L;
  std::vector<double> tab;
  chomp::ProjDev pd;
  KernelTab(int NKT, const double* k_pp, double lo, double hi)
      : L(chomp::make_proj_layout(kProjNC, kProjNWp, NKT)), tab((size_t)L.total, 0.0) {
    std::memset(&pd, 0, sizeof(pd));
    pd.ln_kt_min = lo;
    pd.ln_kt_max = hi;
    for (int i = 0; i < 4 * (NKT - 1); ++i) tab[(size_t)L.k_pp + i] = k_pp[i];
  }
};

// log(k_min), log(k_max) and log(theta_i) as the device's log gives them (wth_fast_body forms
// its range and shift with it)
__global__ void k_logs(double k_min, double k_max, const double* theta, int n, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { out[0] = log(k_min); out[1] = log(k_max); }
  if (i < n) out[2 + i] = log(theta[i]);
}

// The product's plan of the moment route's scratch, and the doubles of the work buffer by it:
// chomp_wtheta (E = 0) keeps one epoch's scratch, chomp_wtheta_epochs (E >= 1) one per epoch.
chomp::WthPlan wth_plan(int LT, int nseg) { return chomp::wth_plan_of(LT, nseg, true); }
size_t wth_total(const chomp::WthPlan& Z, int E) { return Z.stride * (size_t)(E > 0 ? E : 1); }

bool wth_args_ok(int LT, int nseg, int E) {
  return LT >= 1 && LT <= chomp::kWthetaTabLevel && nseg >= 1 && nseg <= 65535 && E >= 0 &&
         E <= chomp::kWthEpochChunkMax;
}

// NaN bytes everywhere, then every epoch's node table; the moment kernel of the form asked for.
int wth_moments(Dev& d_w, const chomp::WthPlan& Z, const double* nodes, int LT, int nseg, double k_min,
                double k_max, int E) {
  DJ_TRY(d_w.nan_fill());
  for (int e = 0; e < (E > 0 ? E : 1); ++e)
    DJ_TRY(d_w.put(Z.stride * (size_t)e, nodes + Z.n_nodes * (size_t)e, Z.n_nodes));
  double* rec = d_w.p + Z.rec_at;
  double* segtot = d_w.p + Z.tot_at;
  if (E == 0)
    chomp::k_wtheta_moments<<<dim3((unsigned)nseg, (unsigned)LT, chomp::kWthParts), dim3(256)>>>(
        d_w.p, LT, nseg, std::log(k_min), std::log(k_max), rec, segtot);
  else
    chomp::k_wtheta_moments_epochs<<<dim3((unsigned)nseg, (unsigned)LT, chomp::kWthParts * E),
                                     dim3(256)>>>(d_w.p, LT, nseg, std::log(k_min),
                                                  std::log(k_max), rec, segtot, Z.stride);
  DJ_SYNC();
  return 0;
}

// ---------------------------------------------------------------------------------------
// test-only kernels: the product has none around these device functions
// ---------------------------------------------------------------------------------------
// grid nq, block 64 (one wavefront): the two derivatives at xq[blockIdx.x] by
// quintic_derivs_wave (ainv_t == nullptr; LDS (n + 6) + 11 n + n doubles) or quintic_derivs_inv
// (LDS (n + 6) + n doubles); out[q], out[nq + q]
__global__ __launch_bounds__(64) void k_quintic(const double* x, const double* y, int n,
                                                const double* xq, const double* ainv_t,
                                                double* out) {
  extern __shared__ __align__(16) double work[];
  __shared__ double sh_d[2];
  const int q = blockIdx.x, nq = gridDim.x;
  if (ainv_t != nullptr)
    chomp::quintic_derivs_inv(x, y, n, xq[q], ainv_t, work, &sh_d[0], &sh_d[1]);
  else
    chomp::quintic_derivs_wave(x, y, n, xq[q], work, &sh_d[0], &sh_d[1]);
  if (threadIdx.x == 0) { out[q] = sh_d[0]; out[nq + q] = sh_d[1]; }
}

// grid n_rows, block 256: the SscRow of a[blockIdx.x] (LDS 5 N - 4 doubles) at every b;
// out[row * n + i]
__global__ __launch_bounds__(256) void k_ssc_row(chomp::SscLayout S, const double* st,
                                                 const double* a, const double* b, int n,
                                                 double* out) {
  extern __shared__ __align__(16) double lds[];
  const chomp::SscSpline K = chomp::ssc_spline(S, st);
  chomp::SscRow R;
  R.build(K, a[blockIdx.x], lds);
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) out[(size_t)blockIdx.x * n + i] = R(b[i]);
}

}  // namespace

// ---------------------------------------------------------------------------------------
// C entry points
// ---------------------------------------------------------------------------------------
extern "C" {

int dj_wth_items() { return chomp::kWthItems; }
int dj_wth_parts() { return chomp::kWthParts; }
// the doubles of the w(theta) work buffer, and where the records and the segment totals of the
// first epoch start in it (E = 0: the single-epoch call); out: total, rec, segtot, stride
int dj_wth_sizes(int LT, int nseg, int E, double* out) {
  if (!wth_args_ok(LT, nseg, E)) return -1;
  const chomp::WthPlan Z = wth_plan(LT, nseg);
  out[0] = (double)wth_total(Z, E); out[1] = (double)Z.rec_at; out[2] = (double)Z.tot_at;
  out[3] = E > 0 ? (double)Z.stride : 0.0;
  return 0;
}

// nodes: E (or 1) node tables of 2^LT + 1 doubles, level-major; work_out: the whole work buffer
// after k_wtheta_moments (E = 0) or k_wtheta_moments_epochs
int dj_moments(const double* nodes, int LT, int nseg, double k_min, double k_max, int E,
               double* work_out) {
  if (!wth_args_ok(LT, nseg, E)) return -1;
  const chomp::WthPlan Z = wth_plan(LT, nseg);
  Dev d_w(wth_total(Z, E), nullptr);
  DJ_TRY(d_w.err);
  if (const int rc = wth_moments(d_w, Z, nodes, LT, nseg, k_min, k_max, E)) return rc;
  DJ_TRY(d_w.back(work_out, wth_total(Z, E)));
  return 0;
}

// The moment route whole: the tables of level LT, then k_wtheta_fast once per entry of lt_run
// (each <= LT: the levels beyond it are not visited) on those tables, out[r * n_theta + i]; or,
// E >= 1, k_wtheta_fast_epochs once at LT (n_run = 1, lt_run[0] = LT), out[e * n_theta + i].
// k_pp: 4 (NKT - 1) coefficients; logs_out: 2 + n_theta doubles (k_logs); work_out: the work
// buffer afterwards, or nullptr.
int dj_wtheta(const double* nodes, int LT, int nseg, double k_min, double k_max, int E, int NKT,
              const double* k_pp, double ln_kt_min, double ln_kt_max, const double* theta,
              int n_theta, const int* lt_run, int n_run, double global_precision,
              double corr_precision, double* out, double* logs_out, double* work_out) {
  if (!wth_args_ok(LT, nseg, E) || NKT < 2 || NKT > 63 || n_theta < 1 || n_run < 1) return -1;
  if (E > 0 && (n_run != 1 || lt_run[0] != LT)) return -1;
  for (int r = 0; r < n_run; ++r)
    if (lt_run[r] < 1 || lt_run[r] > LT) return -1;
  const chomp::WthPlan Z = wth_plan(LT, nseg);
  const KernelTab T(NKT, k_pp, ln_kt_min, ln_kt_max);
  const size_t n_out = (size_t)n_theta * (size_t)(E > 0 ? E : n_run);
  Dev d_w(wth_total(Z, E), nullptr), d_tab(T.tab.size(), T.tab.data()),
      d_pd(chomp::kProjDoubles, reinterpret_cast<const double*>(&T.pd)), d_th(n_theta, theta),
      d_o(n_out, nullptr), d_l((size_t)2 + n_theta, nullptr);
  DJ_TRY(d_w.err); DJ_TRY(d_tab.err); DJ_TRY(d_pd.err); DJ_TRY(d_th.err); DJ_TRY(d_o.err);
  DJ_TRY(d_l.err);
  DJ_TRY(d_o.nan_fill());
  if (const int rc = wth_moments(d_w, Z, nodes, LT, nseg, k_min, k_max, E)) return rc;
  chomp_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.global_precision = global_precision;
  cfg.corr_precision = corr_precision;
  cfg.divmax = LT;
  const chomp::ProjDev* pd = reinterpret_cast<const chomp::ProjDev*>(d_pd.p);
  const double* rec = d_w.p + Z.rec_at;
  const double* segtot = d_w.p + Z.tot_at;
  if (E == 0) {
    for (int r = 0; r < n_run; ++r)
      chomp::k_wtheta_fast<<<dim3((unsigned)n_theta), dim3(256)>>>(
          cfg, T.L, pd, d_tab.p, k_min, k_max, d_th.p, d_o.p + (size_t)r * n_theta, d_w.p, rec,
          segtot, lt_run[r], nseg);
  } else {
    chomp::k_wtheta_fast_epochs<<<dim3((unsigned)n_theta, (unsigned)E), dim3(256)>>>(
        cfg, T.L, pd, d_tab.p, k_min, k_max, d_th.p, d_o.p, d_w.p, rec, segtot, LT, nseg, Z.stride);
  }
  DJ_SYNC();
  k_logs<<<(n_theta + 255) / 256, 256>>>(k_min, k_max, d_th.p, n_theta, d_l.p);
  DJ_SYNC();
  DJ_TRY(d_o.back(out, n_out));
  DJ_TRY(d_l.back(logs_out, (size_t)2 + n_theta));
  if (work_out != nullptr) DJ_TRY(d_w.back(work_out, wth_total(Z, E)));
  return 0;
}

// k_kernel_eval on a piecewise cubic handed in
int dj_kernel_eval(int NKT, const double* k_pp, double ln_kt_min, double ln_kt_max,
                   const double* x, int n, double* out) {
  if (NKT < 2 || n < 1) return -1;
  const KernelTab T(NKT, k_pp, ln_kt_min, ln_kt_max);
  Dev d_tab(T.tab.size(), T.tab.data()),
      d_pd(chomp::kProjDoubles, reinterpret_cast<const double*>(&T.pd)), d_x(n, x), d_o(n, nullptr);
  DJ_TRY(d_tab.err); DJ_TRY(d_pd.err); DJ_TRY(d_x.err); DJ_TRY(d_o.err);
  chomp::k_kernel_eval<<<grid_1d(n), dim3(256)>>>(
      T.L, reinterpret_cast<const chomp::ProjDev*>(d_pd.p), d_tab.p, d_x.p, n, d_o.p);
  DJ_SYNC();
  DJ_TRY(d_o.back(out, n));
  return 0;
}

// k_ssc_bicubic of the N x N table over the knots kx with the range scalars lo, hi;
// bic_out: 16 (N - 1)^2; k_ssc_eval at the n pairs (a, b) into eval_out; the SscRow of every
// ra[r] (n_row of them) at every rb[i] (n_rb) into row_out[r * n_rb + i]
int dj_ssc(int N, const double* kx, const double* tab, double lo, double hi, const double* a,
           const double* b, int n, const double* ra, int n_row, const double* rb, int n_rb,
           double* bic_out, double* eval_out, double* row_out) {
  if (N < 4 || N > 256 || n < 1 || n_row < 1 || n_rb < 1) return -1;
  const chomp::SscLayout S = chomp::make_ssc_layout(N, 2);
  std::vector<double> st((size_t)S.total, 0.0);
  st[S.scal + chomp::kSscLnMin] = lo;
  st[S.scal + chomp::kSscLnMax] = hi;
  for (int i = 0; i < N; ++i) st[S.kx + i] = kx[i];
  for (int i = 0; i < N * N; ++i) st[S.tab + i] = tab[i];
  Dev d_st(st.size(), st.data()), d_a(n, a), d_b(n, b), d_o(n, nullptr), d_ra(n_row, ra),
      d_rb(n_rb, rb), d_ro((size_t)n_row * n_rb, nullptr);
  DJ_TRY(d_st.err); DJ_TRY(d_a.err); DJ_TRY(d_b.err); DJ_TRY(d_o.err); DJ_TRY(d_ra.err);
  DJ_TRY(d_rb.err); DJ_TRY(d_ro.err);
  chomp::k_ssc_bicubic<<<dim3(1), dim3(256)>>>(S, d_st.p);
  DJ_SYNC();
  chomp::k_ssc_eval<<<grid_1d(n), dim3(256)>>>(S, d_st.p, d_a.p, d_b.p, n, d_o.p);
  k_ssc_row<<<dim3((unsigned)n_row), dim3(256), (size_t)(5 * N - 4) * sizeof(double)>>>(
      S, d_st.p, d_ra.p, d_rb.p, n_rb, d_ro.p);
  DJ_SYNC();
  DJ_TRY(hipMemcpy(bic_out, d_st.p + S.bic, (size_t)16 * (N - 1) * (N - 1) * sizeof(double),
                   hipMemcpyDeviceToHost));
  DJ_TRY(d_o.back(eval_out, n));
  DJ_TRY(d_ro.back(row_out, (size_t)n_row * n_rb));
  return 0;
}

// k_ng_bicubic of the table (min, log(table - 10 min), its bicubic) and k_ng_eval at the n
// pairs; min_out: 1 double; bic_out: 16 (N - 1)^2
int dj_ng(int N, const double* kx, const double* tab, double lo, double hi, const double* a,
          const double* b, int n, double* min_out, double* bic_out, double* eval_out) {
  if (N < 4 || N > 256 || n < 1) return -1;
  const chomp::NgLayout G = chomp::make_ng_layout(N);
  std::vector<double> ng((size_t)G.total, 0.0);
  ng[G.scal + chomp::kSscLnMin] = lo;
  ng[G.scal + chomp::kSscLnMax] = hi;
  for (int i = 0; i < N; ++i) ng[G.kx + i] = kx[i];
  for (int i = 0; i < N * N; ++i) ng[G.tab + i] = tab[i];
  Dev d_ng(ng.size(), ng.data()), d_a(n, a), d_b(n, b), d_o(n, nullptr);
  DJ_TRY(d_ng.err); DJ_TRY(d_a.err); DJ_TRY(d_b.err); DJ_TRY(d_o.err);
  chomp::k_ng_bicubic<<<dim3(1), dim3(256)>>>(G, d_ng.p);
  DJ_SYNC();
  chomp::k_ng_eval<<<grid_1d(n), dim3(256)>>>(G, d_ng.p, d_a.p, d_b.p, n, d_o.p);
  DJ_SYNC();
  DJ_TRY(hipMemcpy(min_out, d_ng.p + G.scal + chomp::kNgMin, sizeof(double),
                   hipMemcpyDeviceToHost));
  DJ_TRY(hipMemcpy(bic_out, d_ng.p + G.bic, (size_t)16 * (N - 1) * (N - 1) * sizeof(double),
                   hipMemcpyDeviceToHost));
  DJ_TRY(d_o.back(eval_out, n));
  return 0;
}

// HaloFit's ln R grid, linspace(ln 0.1, ln 10, n), as halofit_collocation_inverse_host and
// k_halofit_finalize form it
void dj_quintic_grid(int n, double* x) {
  for (int i = 0; i < n; ++i) x[i] = chomp::linspace_at(std::log(0.1), std::log(10.0), n, i);
}

// y on that grid (6 <= n <= 128: at 6 the spline has no interior knot); out: d1 and d2 at the nq points by quintic_derivs_wave
// (out[q], out[nq + q]), then by quintic_derivs_inv with halofit_collocation_inverse_host(n)
// (out[2 nq + q], out[3 nq + q])
int dj_quintic(const double* y, int n, const double* xq, int nq, double* out) {
  if (n < 6 || n > 128 || nq < 1) return -1;
  std::vector<double> x(n), ainv((size_t)n * n);
  dj_quintic_grid(n, x.data());
  chomp::halofit_collocation_inverse_host(n, ainv.data());
  Dev d_x(n, x.data()), d_y(n, y), d_q(nq, xq), d_ai(ainv.size(), ainv.data()),
      d_o((size_t)4 * nq, nullptr);
  DJ_TRY(d_x.err); DJ_TRY(d_y.err); DJ_TRY(d_q.err); DJ_TRY(d_ai.err); DJ_TRY(d_o.err);
  k_quintic<<<dim3((unsigned)nq), dim3(64), (size_t)((n + 6) + 11 * n + n) * sizeof(double)>>>(
      d_x.p, d_y.p, n, d_q.p, nullptr, d_o.p);
  k_quintic<<<dim3((unsigned)nq), dim3(64), (size_t)((n + 6) + n) * sizeof(double)>>>(
      d_x.p, d_y.p, n, d_q.p, d_ai.p, d_o.p + (size_t)2 * nq);
  DJ_SYNC();
  DJ_TRY(d_o.back(out, (size_t)4 * nq));
  return 0;
}

}  // extern "C"
