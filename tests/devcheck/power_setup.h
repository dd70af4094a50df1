// TEST-ONLY: the host plumbing and the spectrum-side set-up shared by the harnesses that launch
// kernels on epochs and knot tables handed in (devpower.hip, devcell.hip): an owning device buffer,
// the error macros, and the Epoch records and table blocks filled on the device through
// epoch_fill.h.  Includes the product's headers themselves; no part of the package.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "../../chomp_amd/csrc/chomp_cov_kernels.h"
#include "epoch_fill.h"

namespace devcheck {

template <class T>
struct DevT {
  T* p = nullptr;
  hipError_t err = hipSuccess;
  size_t n;
  DevT(size_t n_, const T* host) : n(n_ ? n_ : 1) {
    err = hipMalloc((void**)&p, n * sizeof(T));
    if (err == hipSuccess && host != nullptr && n_ > 0)
      err = hipMemcpy(p, host, n_ * sizeof(T), hipMemcpyHostToDevice);
    else if (err == hipSuccess)
      err = hipMemset(p, 0, n * sizeof(T));
  }
  ~DevT() { if (p) (void)hipFree(p); }
  hipError_t back(T* host, size_t count) const {
    if (count > n) return hipErrorInvalidValue;
    return hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost);
  }
  hipError_t nan_fill() { return hipMemset(p, 0xFF, n * sizeof(T)); }
  DevT(const DevT&) = delete;
  DevT& operator=(const DevT&) = delete;
};
using Dev = DevT<double>;
using DevI = DevT<int>;
#define DW_TRY(expr)                            \
  do {                                          \
    const hipError_t e_ = (expr);               \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)
#define DW_SYNC()                               \
  do {                                          \
    DW_TRY(hipGetLastError());                  \
    DW_TRY(hipDeviceSynchronize());             \
  } while (0)

constexpr int kHf = 12;
constexpr int kIn = kEpochIn + kHf;
constexpr int kNM = 4;                      // the layout's mass tables: unused, small
constexpr int kMaxEpochs = 8, kMinNK = 8, kMaxNK = 64;

// grid n, block 64: epoch e from its inputs, and misc[1] of its table block
__global__ void k_fill(const double* in, int n, chomp::TabLayout L, chomp::Epoch* ep, double* tab) {
  const int e = blockIdx.x;
  if (threadIdx.x != 0 || e >= n) return;
  chomp::Epoch E;
  fill_epoch(in + (size_t)e * kIn, E);
  const double* h = in + (size_t)e * kIn + kEpochIn;
  E.hf_k_s = h[0]; E.hf_a_n = h[1]; E.hf_b_n = h[2]; E.hf_c_n = h[3]; E.hf_alpha_n = h[4];
  E.hf_beta_n = h[5]; E.hf_gamma_n = h[6]; E.hf_mu_n = h[7]; E.hf_nu_n = h[8];
  E.hf_f1 = h[9]; E.hf_f2 = h[10]; E.hf_f3 = h[11];
  ep[e] = E;
  tab[(size_t)e * L.stride + L.off_misc + 1] = E.amp * E.sigma_norm * E.sigma_norm;
}

inline bool setup_ok(int n_epoch, int NK, double k_min, double k_max) {
  return n_epoch >= 1 && n_epoch <= kMaxEpochs && NK >= kMinNK && NK <= kMaxNK && k_min > 0.0 &&
         k_max > k_min;
}

// The epochs and table blocks on the device.  (Construct only after setup_ok.)
struct Setup {
  chomp_config cfg;
  chomp::TabLayout L;
  int n;
  Dev d_in, d_ep, d_tab, d_db;
  Setup(int n_epoch, const double* ein, const double* tab, int NK, double k_min, double k_max,
        const double* delta_b)
      : L(chomp::make_layout(kNM, NK)), n(n_epoch), d_in((size_t)n_epoch * kIn, ein),
        d_ep((size_t)n_epoch * kEpochD, nullptr),
        d_tab((size_t)n_epoch * chomp::make_layout(kNM, NK).stride, tab), d_db(n_epoch, delta_b) {
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.k_min = k_min;
    cfg.k_max = k_max;
  }
  const chomp::Epoch* ep() const { return reinterpret_cast<const chomp::Epoch*>(d_ep.p); }
  size_t lds() const { return (size_t)(12 * (L.NK - 1)) * sizeof(double); }   // (PowerEval::stage)
  int init() {
    DW_TRY(d_in.err); DW_TRY(d_ep.err); DW_TRY(d_tab.err); DW_TRY(d_db.err);
    DW_TRY(d_ep.nan_fill());
    k_fill<<<dim3((unsigned)n), dim3(64)>>>(d_in.p, n, L, reinterpret_cast<chomp::Epoch*>(d_ep.p),
                                            d_tab.p);
    DW_SYNC();
    return 0;
  }
};

}  // namespace devcheck
