// TEST-ONLY harness: the second device counterpart of tests/hostcheck.  One HIP translation unit
// that compiles the product's header chain (chomp_cov_kernels.h down to chomp_math.h) FOR THE
// DEVICE, with the product's compiler flags, and drives the halo-model physics of chomp_math.h
// (epoch background, transfer functions and power, mass function, HOD moments and their node
// forms, the NFW transform in its three forms, the exclusion window, linspace_at, E0_de on a
// pressure spline) directly -- one small kernel per item, host arrays in and out.  It includes
// the headers themselves, never copies of their functions.  Never loaded by the chomp_amd
// package, not in _lib.UNITS, no part of the C ABI.  Built and loaded by tests/devcheck_build.py.
//
// Every entry point returns the HIP error code (0: success) unless it is a plain getter.
// Kernels index only inside the buffers the entry point allocated; outputs are laid out
// out[field * n + i].
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "../../chomp_amd/csrc/chomp_cov_kernels.h"
#include "epoch_fill.h"

using chomp::Epoch;
using chomp::SiCiTab;

namespace {

// ---------------------------------------------------------------------------------------
// host plumbing (as devcheck.hip)
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
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
};
#define DP_TRY(expr)                            \
  do {                                          \
    const hipError_t e_ = (expr);               \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)
#define DP_SYNC()                               \
  do {                                          \
    DP_TRY(hipGetLastError());                  \
    DP_TRY(hipDeviceSynchronize());             \
  } while (0)

using devcheck::kEpochD;
using devcheck::kEpochIn;

SiCiTab* g_sici = nullptr;
int tables_init() {
  if (g_sici) return 0;
  static SiCiTab hs;
  static chomp::BesselTab h0, h2;
  chomp::fill_tables(&hs, &h0, &h2);
  SiCiTab* d = nullptr;
  DP_TRY(hipMalloc((void**)&d, sizeof(SiCiTab)));
  DP_TRY(hipMemcpy(d, &hs, sizeof(SiCiTab), hipMemcpyHostToDevice));
  g_sici = d;
  return 0;
}

constexpr int kEB = 256;
inline int eblocks(int n) { return (n + kEB - 1) / kEB; }

// ---------------------------------------------------------------------------------------
// the Epoch, filled on the device by the product's own functions from the raw inputs
// ---------------------------------------------------------------------------------------
// (the inputs and the filling: epoch_fill.h, shared with devpower.hip)
__global__ void k_epoch(const double* in, Epoch* out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Epoch e;
  devcheck::fill_epoch(in, e);
  *out = e;
}

// E0_of, growth_approx (a = 1 / (1 + z)) and scale_of_mass beside the record
__global__ void k_scalars(const Epoch* ep, const double* z, const double* mass, int n,
                          double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Epoch& e = *ep;
  out[i] = chomp::E0_of(e.om0, e.ol0, e.or0, z[i]);
  out[n + i] = chomp::growth_approx(e.om0, e.ol0, 1.0 / (1.0 + z[i]));
  out[2 * n + i] = chomp::scale_of_mass(e, mass[i]);
}

// ---------------------------------------------------------------------------------------
// transfer functions and power: 12 fields
// ---------------------------------------------------------------------------------------
constexpr int kPowerFields = 12;
template <bool BAO>
__global__ void k_power(const Epoch* ep, const double* k, int n, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Epoch& e = *ep;
  const double kk = k[i], lk = log(kk);
  const double amp = e.amp * e.sigma_norm * e.sigma_norm;
  out[i] = chomp::eh_transfer(e, kk);
  out[n + i] = BAO ? chomp::eh_bao_transfer(e, kk) : 0.0;
  out[2 * n + i] = chomp::transfer_function(e, kk);
  out[3 * n + i] = chomp::transfer_t<BAO>(e, kk);
  out[4 * n + i] = chomp::linear_power(e, kk);
  out[5 * n + i] = chomp::linear_power_t<BAO>(e, kk);
  out[6 * n + i] = chomp::delta_k_ln(e, lk, kk);
  out[7 * n + i] = chomp::delta_k_ln_t<BAO>(e, lk, kk);
  out[8 * n + i] = amp * chomp::power_shape(e, chomp::fast_log(kk), kk);
  out[9 * n + i] = amp * chomp::power_shape_t<BAO>(e, chomp::fast_log(kk), kk);
  out[10 * n + i] = lk;                       // the device's ln k (what delta_k_ln received)
  out[11 * n + i] = chomp::fast_log(kk);
}
// SigmaIntegrandT and HalofitSigmaIntegrand at scale R over ln k; out[0] = the two limits of
// sigma_limits, then 2 fields
template <bool BAO>
__global__ void k_sigma(const Epoch* ep, double R, const double* lnk, int n, double* lim,
                        double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) chomp::sigma_limits(*ep, R, &lim[0], &lim[1]);
  if (i >= n) return;
  const chomp::SigmaIntegrandT<BAO> f{ep, R};
  const chomp::HalofitSigmaIntegrand<BAO> g{ep, R};
  out[i] = f(lnk[i]);
  out[n + i] = g(lnk[i]);
}

// ---------------------------------------------------------------------------------------
// mass function: f_nu, bias_nu, and mf_node with and without the bias; 5 fields
// ---------------------------------------------------------------------------------------
constexpr int kMfFields = 5;
__global__ void k_mf(const Epoch* ep, const double* nu, const double* ln_nu, int n, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Epoch& e = *ep;
  out[i] = chomp::f_nu(e, nu[i]);
  out[n + i] = chomp::bias_nu(e, nu[i]);
  double nf = 0.0, b = 0.0, nf2 = 0.0, b2 = -7.0;
  chomp::mf_node(e, nu[i], ln_nu[i], true, &nf, &b);
  chomp::mf_node(e, nu[i], ln_nu[i], false, &nf2, &b2);
  out[2 * n + i] = nf;
  out[3 * n + i] = b;
  out[4 * n + i] = nf2;
}

// ---------------------------------------------------------------------------------------
// HOD: the node gets (mass, ln_mass) as halo_node_fields forms them (mass = exp(ln_mass) in
// namespace chomp); the evaluators get that mass.  16 fields.
// ---------------------------------------------------------------------------------------
constexpr int kHodFields = 16;
__global__ void k_hod(const Epoch* ep, const double* ln_mass, int n, double* out) {
  using chomp::kHodMandelbaum;
  using chomp::hod_central; using chomp::hod_satellite; using chomp::hod_first;
  using chomp::hod_second; using chomp::hod_node; using chomp::zheng_node;
  using chomp::mandelbaum_central; using chomp::mandelbaum_satellite; using chomp::zheng_central;
  using chomp::zheng_satellite; using chomp::zheng_first; using chomp::zheng_second;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Epoch& e = *ep;
  const double lnm = ln_mass[i];
  const double mass = chomp::exp(lnm);
  out[i] = mass;
  out[n + i] = log10(mass);                           // the device library's
  out[2 * n + i] = lnm * 0.43429448190325182765;      // the node route
  out[3 * n + i] = hod_central(e, mass);
  out[4 * n + i] = hod_satellite(e, mass);
  out[5 * n + i] = hod_first(e, mass);
  out[6 * n + i] = hod_second(e, mass);
  double n1 = 0.0, n2 = 0.0;
  const int st = hod_node(e, mass, lnm, &n1, &n2);
  out[7 * n + i] = n1;
  out[8 * n + i] = n2;
  out[9 * n + i] = (double)st;
  if (e.hod_model == kHodMandelbaum) {
    out[10 * n + i] = mandelbaum_central(e, mass);
    out[11 * n + i] = mandelbaum_satellite(e, mass);
    out[12 * n + i] = 0.0;
    out[13 * n + i] = 0.0;
  } else {
    out[10 * n + i] = zheng_central(e, mass);
    out[11 * n + i] = zheng_satellite(e, mass);
    out[12 * n + i] = zheng_first(e, mass);
    out[13 * n + i] = zheng_second(e, mass);
    zheng_node(e, mass, lnm, &n1, &n2);
  }
  out[14 * n + i] = n1;                               // zheng_node called by itself
  out[15 * n + i] = n2;
}

// ---------------------------------------------------------------------------------------
// NFW transform: y_nfw, and the two core forms fed the node-table fields computed as
// halo_node_fields computes them (returned, so that the reference can use the same doubles).
// 13 fields.
// ---------------------------------------------------------------------------------------
constexpr int kNfwFields = 13;
__global__ void k_nfw(const Epoch* ep, const SiCiTab* T, const double* ln_k, const double* ln_mass,
                      int n, double* out) {
  using chomp::KnotK; using chomp::y_nfw; using chomp::y_nfw_core; using chomp::y_nfw_core_tab;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Epoch& E = *ep;
  const double lnm = ln_mass[i];
  const double ln_c = E.ln_c_const + E.beta * lnm;
  const double ln_rv = (E.ln_rv_const + lnm) * (1.0 / 3.0);
  const double con = chomp::exp(ln_c);
  const double cp = 1.0 + con;
  const double ln_cp = log(cp);
  const double ln_rs = ln_rv - ln_c;
  const double inv_mass_k = 1.0 / (ln_cp - con / cp);
  const double rs = chomp::exp(ln_rs);
  const double inv_cprs = 1.0 / (cp * rs);
  const KnotK kk(ln_k[i]);
  double z1 = 0.0, z2 = 0.0;
  out[i] = y_nfw(E, *T, ln_k[i], lnm);
  out[n + i] = y_nfw_core(*T, kk.ln_k, ln_rs, con, ln_cp, inv_mass_k, &z1);
  out[2 * n + i] = y_nfw_core_tab(*T, kk.ln_k, kk.k, kk.inv_k, ln_rs, con, ln_cp, inv_mass_k, rs,
                                  inv_cprs, &z2);
  out[3 * n + i] = z1;
  out[4 * n + i] = z2;
  out[5 * n + i] = ln_rs;
  out[6 * n + i] = con;
  out[7 * n + i] = ln_cp;
  out[8 * n + i] = inv_mass_k;
  out[9 * n + i] = rs;
  out[10 * n + i] = inv_cprs;
  out[11 * n + i] = kk.k;
  out[12 * n + i] = kk.inv_k;
}

__global__ void k_exclusion(const SiCiTab* T, const double* kR, int n, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = chomp::exclusion_window(*T, kR[i]);
}

// ---------------------------------------------------------------------------------------
// linspace_at inlined in a kernel compiled with contraction on, its result used in a
// following multiply-add (a contraction of linspace_at's own product and sum would show in
// out; the use is returned beside it)
// ---------------------------------------------------------------------------------------
__global__ void k_linspace(const double* a, const double* b, const double* nn, const double* ii,
                           int n, double s, double t, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = chomp::linspace_at(a[i], b[i], (int)nn[i], (int)ii[i]);
  out[i] = v;
  out[n + i] = v * s + t;
}

// ---------------------------------------------------------------------------------------
// E0_de on the pressure spline of a w0-wa cosmology: thread 0 builds the not-a-knot spline of
// (ln a_i, P_i) with the serial spline_build, as the table k_de_spline leaves it, then every
// thread evaluates.  One block.  pp: 4 (n - 1) coefficients (returned); work: 2 n; out[i] =
// E0_de(z_i), out[m + i] = DeSpline::factor(1 / (1 + z_i)).
// ---------------------------------------------------------------------------------------
constexpr int kDeMaxKnots = 256;
__global__ void k_e0_de(const Epoch* ep, const double* ln_a, const double* P, int n,
                        const double* z, int m, double* pp, double* work, double* out) {
  if (blockIdx.x != 0) return;
  if (threadIdx.x == 0) chomp::spline_build(ln_a, P, n, pp, work);
  __syncthreads();
  const Epoch& e = *ep;
  const chomp::DeSpline de{ln_a, pp, n};
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    out[i] = chomp::E0_de(e.om0, e.ol0, e.or0, de, z[i]);
    out[m + i] = de.factor(1.0 / (1.0 + z[i]));
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------
// C entry points
// ---------------------------------------------------------------------------------------
#define DP_EPOCH_FIELDS(X)                                                                        \
  X(om0) X(ob0) X(ol0) X(or0) X(tcmb) X(h) X(sigma8) X(ns) X(z) X(H0) X(delta_H) X(growth_norm)   \
  X(growth) X(sigma_norm) X(E0z) X(omega_m_z) X(omega_l_z) X(delta_c) X(delta_v) X(rho_bar)      \
  X(eh_theta) X(eh_s) X(eh_alpha) X(eh_omh) X(amp) X(ln_H0) X(k_min) X(k_max) X(ln_k_min)        \
  X(ln_k_max) X(gtab_xlo) X(gtab_dx) X(gtab_inv_dx) X(flat) X(open) X(closed) X(mf_kind) X(stq)  \
  X(st_a) X(mf_delta_v) X(m_star) X(f_norm) X(bias_norm) X(t_alpha) X(t_beta) X(t_gamma)         \
  X(t_phi) X(t_eta) X(tb_A) X(tb_a) X(tb_C) X(tb_dca) X(c0) X(beta) X(prof_delta_v)              \
  X(ln_rv_const) X(ln_c_const) X(hod_log_M_min) X(hod_sigma) X(hod_log_M_0) X(hod_log_M_1p)      \
  X(hod_alpha) X(hod_M0) X(hod_M1p) X(hod_model) X(hod_w) X(hod_M_min) X(ln_st_a) X(ln_t_beta)   \
  X(with_bao) X(bao_hs) X(bao_q_scale) X(bao_ksilk_h) X(bao_alpha_b) X(bao_beta_b)               \
  X(bao_alpha_c) X(bao_beta_c) X(bao_beta_node) X(bao_s) X(bao_ObO) X(bao_OcO)

extern "C" {

int dp_sizeof_epoch() { return (int)sizeof(Epoch); }
int dp_epoch_inputs() { return kEpochIn; }
int dp_power_fields() { return kPowerFields; }
int dp_mf_fields() { return kMfFields; }
int dp_hod_fields() { return kHodFields; }
int dp_nfw_fields() { return kNfwFields; }
// the names of the Epoch fields the tests read, comma-separated, in the order of
// dp_epoch_offsets
const char* dp_epoch_field_names() {
#define X(f) #f ","
  return DP_EPOCH_FIELDS(X);
#undef X
}
// per field: byte offset, and 1 where it is an int (0: a double)
void dp_epoch_offsets(int* out) {
  int j = 0;
#define X(f)                                                      \
  out[j++] = (int)offsetof(Epoch, f);                             \
  out[j++] = sizeof(((Epoch*)nullptr)->f) == sizeof(int) ? 1 : 0;
  DP_EPOCH_FIELDS(X)
#undef X
}

// fill an Epoch on the device from `in` (kEpochIn doubles) and copy it back whole
int dp_epoch(const double* in, void* epoch_out) {
  Dev d_in(kEpochIn, in), d_e(kEpochD, nullptr);
  DP_TRY(d_in.err); DP_TRY(d_e.err);
  k_epoch<<<1, 64>>>(d_in.p, reinterpret_cast<Epoch*>(d_e.p));
  DP_SYNC();
  DP_TRY(hipMemcpy(epoch_out, d_e.p, sizeof(Epoch), hipMemcpyDeviceToHost));
  return 0;
}

int dp_scalars(const void* epoch, const double* z, const double* mass, int n, double* out) {
  Dev d_e(kEpochD, (const double*)epoch), d_z(n, z), d_m(n, mass), d_o((size_t)3 * n, nullptr);
  DP_TRY(d_e.err); DP_TRY(d_z.err); DP_TRY(d_m.err); DP_TRY(d_o.err);
  k_scalars<<<eblocks(n), kEB>>>(reinterpret_cast<const Epoch*>(d_e.p), d_z.p, d_m.p, n, d_o.p);
  DP_SYNC();
  DP_TRY(d_o.back(out, (size_t)3 * n));
  return 0;
}

int dp_power(const void* epoch, const double* k, int n, double* out) {
  Dev d_e(kEpochD, (const double*)epoch), d_k(n, k), d_o((size_t)kPowerFields * n, nullptr);
  DP_TRY(d_e.err); DP_TRY(d_k.err); DP_TRY(d_o.err);
  const Epoch* ep = reinterpret_cast<const Epoch*>(d_e.p);
  if (((const Epoch*)epoch)->with_bao) k_power<true><<<eblocks(n), kEB>>>(ep, d_k.p, n, d_o.p);
  else k_power<false><<<eblocks(n), kEB>>>(ep, d_k.p, n, d_o.p);
  DP_SYNC();
  DP_TRY(d_o.back(out, (size_t)kPowerFields * n));
  return 0;
}

int dp_sigma(const void* epoch, double R, const double* lnk, int n, double* lim, double* out) {
  Dev d_e(kEpochD, (const double*)epoch), d_k(n, lnk), d_l(2, nullptr), d_o((size_t)2 * n, nullptr);
  DP_TRY(d_e.err); DP_TRY(d_k.err); DP_TRY(d_l.err); DP_TRY(d_o.err);
  const Epoch* ep = reinterpret_cast<const Epoch*>(d_e.p);
  const int nb = eblocks(n > 0 ? n : 1);
  if (((const Epoch*)epoch)->with_bao) k_sigma<true><<<nb, kEB>>>(ep, R, d_k.p, n, d_l.p, d_o.p);
  else k_sigma<false><<<nb, kEB>>>(ep, R, d_k.p, n, d_l.p, d_o.p);
  DP_SYNC();
  DP_TRY(d_l.back(lim, 2));
  if (n > 0) DP_TRY(d_o.back(out, (size_t)2 * n));
  return 0;
}

int dp_mf(const void* epoch, const double* nu, const double* ln_nu, int n, double* out) {
  Dev d_e(kEpochD, (const double*)epoch), d_n(n, nu), d_l(n, ln_nu),
      d_o((size_t)kMfFields * n, nullptr);
  DP_TRY(d_e.err); DP_TRY(d_n.err); DP_TRY(d_l.err); DP_TRY(d_o.err);
  k_mf<<<eblocks(n), kEB>>>(reinterpret_cast<const Epoch*>(d_e.p), d_n.p, d_l.p, n, d_o.p);
  DP_SYNC();
  DP_TRY(d_o.back(out, (size_t)kMfFields * n));
  return 0;
}

int dp_hod(const void* epoch, const double* ln_mass, int n, double* out) {
  Dev d_e(kEpochD, (const double*)epoch), d_m(n, ln_mass), d_o((size_t)kHodFields * n, nullptr);
  DP_TRY(d_e.err); DP_TRY(d_m.err); DP_TRY(d_o.err);
  k_hod<<<eblocks(n), kEB>>>(reinterpret_cast<const Epoch*>(d_e.p), d_m.p, n, d_o.p);
  DP_SYNC();
  DP_TRY(d_o.back(out, (size_t)kHodFields * n));
  return 0;
}

int dp_nfw(const void* epoch, const double* ln_k, const double* ln_mass, int n, double* out) {
  if (const int rc = tables_init()) return rc;
  Dev d_e(kEpochD, (const double*)epoch), d_k(n, ln_k), d_m(n, ln_mass),
      d_o((size_t)kNfwFields * n, nullptr);
  DP_TRY(d_e.err); DP_TRY(d_k.err); DP_TRY(d_m.err); DP_TRY(d_o.err);
  k_nfw<<<eblocks(n), kEB>>>(reinterpret_cast<const Epoch*>(d_e.p), g_sici, d_k.p, d_m.p, n,
                             d_o.p);
  DP_SYNC();
  DP_TRY(d_o.back(out, (size_t)kNfwFields * n));
  return 0;
}

int dp_exclusion(const double* kR, int n, double* out) {
  if (const int rc = tables_init()) return rc;
  Dev d_k(n, kR), d_o(n, nullptr);
  DP_TRY(d_k.err); DP_TRY(d_o.err);
  k_exclusion<<<eblocks(n), kEB>>>(g_sici, d_k.p, n, d_o.p);
  DP_SYNC();
  DP_TRY(d_o.back(out, n));
  return 0;
}

// ln_a, P: the n knots of a pressure table (4 <= n <= kDeMaxKnots, ln_a increasing); z: m
// redshifts; pp_out: 4 (n - 1) doubles; out: 2 m doubles
int dp_e0_de(const void* epoch, const double* ln_a, const double* P, int n, const double* z,
             int m, double* pp_out, double* out) {
  if (n < 4 || n > kDeMaxKnots || m < 1) return -1;
  for (int i = 1; i < n; ++i)
    if (!(ln_a[i] > ln_a[i - 1])) return -1;
  Dev d_e(kEpochD, (const double*)epoch), d_x(n, ln_a), d_y(n, P), d_z(m, z),
      d_pp((size_t)4 * (n - 1), nullptr), d_w((size_t)2 * n, nullptr), d_o((size_t)2 * m, nullptr);
  DP_TRY(d_e.err); DP_TRY(d_x.err); DP_TRY(d_y.err); DP_TRY(d_z.err); DP_TRY(d_pp.err);
  DP_TRY(d_w.err); DP_TRY(d_o.err);
  k_e0_de<<<1, kEB>>>(reinterpret_cast<const Epoch*>(d_e.p), d_x.p, d_y.p, n, d_z.p, m, d_pp.p,
                      d_w.p, d_o.p);
  DP_SYNC();
  DP_TRY(d_pp.back(pp_out, (size_t)4 * (n - 1)));
  DP_TRY(d_o.back(out, (size_t)2 * m));
  return 0;
}

// a, b, nn, ii: per point (nn, ii integers held in doubles, 0 <= ii < nn, nn >= 2)
int dp_linspace(const double* a, const double* b, const double* nn, const double* ii, int n,
                double s, double t, double* out) {
  for (int i = 0; i < n; ++i)
    if (!(nn[i] >= 2.0 && ii[i] >= 0.0 && ii[i] < nn[i])) return -1;
  Dev d_a(n, a), d_b(n, b), d_n(n, nn), d_i(n, ii), d_o((size_t)2 * n, nullptr);
  DP_TRY(d_a.err); DP_TRY(d_b.err); DP_TRY(d_n.err); DP_TRY(d_i.err); DP_TRY(d_o.err);
  k_linspace<<<eblocks(n), kEB>>>(d_a.p, d_b.p, d_n.p, d_i.p, n, s, t, d_o.p);
  DP_SYNC();
  DP_TRY(d_o.back(out, (size_t)2 * n));
  return 0;
}

}  // extern "C"
