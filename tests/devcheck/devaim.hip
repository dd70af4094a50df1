// TEST-ONLY harness: the AIM of the mass-limit search as compiled for the device, with the
// product's compiler flags -- the coarse ln S(R) table of k_sigma_nodes<false, 1> (launched here
// as the library launches it) against the same integrals at the reference's tolerance, and
// plan_side's inverse interpolation against its two-round search on that table.  It includes the
// product's header itself, never copies of its functions.  Never loaded by the chomp_amd package,
// not in _lib.UNITS, no part of the C ABI.  Built and loaded by tests/test_gpu_devaim.py through
// tests/devcheck_build.py.
//
// Every entry point allocates its buffers, launches, synchronises, returns the HIP error code
// (0: success; -1: an argument outside what the buffers were sized for) and frees its buffers.
// Output buffers are filled with NaN bytes before the launch.
//
//   cosmo  8 doubles: om0 ob0 ol0 or0 tcmb h sigma8 ns
//   lim    4 doubles: k_min k_max cosmo_precision global_precision
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "../../chomp_amd/csrc/chomp_mass_kernels.h"

using chomp::Epoch;
using chomp::kSGrid;
using chomp::kSigmaStride;

namespace {

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
#define DA_TRY(expr)                            \
  do {                                          \
    const hipError_t e_ = (expr);               \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)
#define DA_SYNC()                               \
  do {                                          \
    DA_TRY(hipGetLastError());                  \
    DA_TRY(hipDeviceSynchronize());             \
  } while (0)

constexpr int kMaxZ = 8;
constexpr int kPlanOut = 13;   // da_plan: doubles per (epoch, side)

chomp_config make_config(const double* lim, int divmax) {
  chomp_config cfg{};
  cfg.k_min = lim[0]; cfg.k_max = lim[1];
  cfg.mass_min = -1.0; cfg.mass_max = -1.0;
  cfg.cosmo_precision = lim[2]; cfg.global_precision = lim[3];
  cfg.divmax = divmax;
  return cfg;
}
bool limits_ok(const double* lim, int divmax) {
  return lim[0] > 0.0 && lim[1] > lim[0] && lim[2] > 0.0 && lim[3] > 0.0 && divmax >= 1 &&
         divmax <= chomp::kMaxDivmax;
}

// The product's k_sigma_nodes<false, 1> for n_epoch epochs of ONE cosmology, as chomp_epochs_set
// launches it (without the chi rows): snodes (zeroed: the arrival counter), epochs, status.
int run_sigma_nodes(const chomp_config& cfg, const double* cosmo, const double* z, int n_epoch,
                    Dev& snodes, DevT<Epoch>& epochs) {
  std::vector<chomp_cosmo> c(n_epoch);
  for (int e = 0; e < n_epoch; ++e) {
    c[e] = chomp_cosmo{};
    c[e].omega_m0 = cosmo[0]; c[e].omega_b0 = cosmo[1]; c[e].omega_l0 = cosmo[2];
    c[e].omega_r0 = cosmo[3]; c[e].cmb_temp = cosmo[4]; c[e].h = cosmo[5];
    c[e].sigma_8 = cosmo[6]; c[e].n_scalar = cosmo[7];
    c[e].w0 = -1.0; c[e].wa = 0.0;
  }
  std::vector<int> zero(n_epoch, 0);
  DevT<chomp_cosmo> d_cosmo(n_epoch, c.data());
  Dev d_z(n_epoch, z);
  DevT<int> d_first(1, zero.data()), d_slots(n_epoch, zero.data());
  DevT<unsigned> d_status(n_epoch, nullptr);
  DA_TRY(d_cosmo.err); DA_TRY(d_z.err); DA_TRY(d_first.err); DA_TRY(d_slots.err);
  DA_TRY(d_status.err);
  constexpr int gx = chomp::sigma_node_blocks<1>() + chomp::sigma_lns_blocks<1>() +
                     chomp::sigma_gtab_blocks<1>();
  const unsigned gy = (unsigned)(1 + chomp::sigma_epoch_rows(n_epoch));
  hipLaunchKernelGGL((chomp::k_sigma_nodes<false, 1>), dim3(gx, gy), dim3(256), 0, 0, cfg,
                     d_cosmo.p, d_z.p, d_first.p, d_slots.p, 1, n_epoch, epochs.p, snodes.p,
                     d_status.p, (double*)nullptr);
  DA_SYNC();
  return 0;
}

// grid kSGrid, block 256: the ln S integral of table point blockIdx.x by romberg1<4> on the direct
// integrand -- out[i] at (tol, rtol_ref, divmax), the reference's tolerance; out[kSGrid + i] at
// (tol, 1e-5, min(divmax, 10)), the adaptive rule the one-pass table replaces; out[2 kSGrid + i]
// = ln R_i.
__global__ __launch_bounds__(256) void k_ref_lns(chomp_config cfg, const double* cosmo,
                                                 double* out) {
  __shared__ Epoch E;
  __shared__ double red[chomp::romberg_scratch<4, 1>()];
  if (threadIdx.x == 0) {
    E.om0 = cosmo[0]; E.ob0 = cosmo[1]; E.ol0 = cosmo[2]; E.or0 = cosmo[3];
    E.tcmb = cosmo[4]; E.h = cosmo[5]; E.sigma8 = cosmo[6]; E.ns = cosmo[7];
    E.z = 0.0;
    chomp::epoch_shape_only(E, cfg.k_min, cfg.k_max, 0);
  }
  __syncthreads();
  const int i = blockIdx.x;
  const double x = chomp::make_sgrid(cfg.k_min, cfg.k_max).ln_r(i);
  const double R = exp(x);
  double lo, hi;
  chomp::sigma_limits(E, R, &lo, &hi);
  chomp::SigmaIntegrandT<false> f{&E, R};
  const double ref = chomp::romberg1<4>(f, lo, hi, cfg.global_precision, cfg.cosmo_precision,
                                        cfg.divmax, red);
  __syncthreads();
  const double ada = chomp::romberg1<4>(f, lo, hi, cfg.global_precision, 1e-5,
                                        cfg.divmax < 10 ? cfg.divmax : 10, red);
  if (threadIdx.x == 0) {
    out[i] = log(ref);
    out[kSGrid + i] = log(ada);
    out[2 * kSGrid + i] = x;
  }
}

// grid 2 n_epoch, block 64 or 256: block 2 e + side plans that side of epoch e twice, by inverse
// interpolation and by the two-round search, on the record and table k_epoch_probe would read.
// out: ok dir j at_edge searched nu_start of the first, the same six of the second, then the
// number of threads whose first plan differs from thread 0's.
__global__ __launch_bounds__(256) void k_plan(const Epoch* epochs, const double* snodes,
                                              const double* cand, double* out) {
  __shared__ Epoch E;
  __shared__ double lns[kSGrid];
  __shared__ int sh_j, differ, ref[3];
  const int e = (int)blockIdx.x >> 1, side = (int)blockIdx.x & 1;
  chomp::copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
                      chomp::kEpochDoubles);
  __syncthreads();
  const double* snode = snodes + (size_t)E.cosmo_slot * kSigmaStride;
  chomp::copy_doubles(lns, snode + chomp::kSigmaOffLnS, kSGrid);
  if (threadIdx.x == 0) {
    E.sigma_norm = E.sigma8 * E.growth / sqrt(E.amp * snode[chomp::kSigmaOffI8]);
    differ = 0;
  }
  __syncthreads();
  const chomp::SidePlan a = chomp::plan_side<true>(E, lns, side, cand, &sh_j);
  __syncthreads();
  const chomp::SidePlan b = chomp::plan_side<false>(E, lns, side, cand, &sh_j);
  if (threadIdx.x == 0) { ref[0] = a.ok; ref[1] = a.dir; ref[2] = a.j; }
  __syncthreads();
  if ((int)a.ok != ref[0] || a.dir != ref[1] || a.j != ref[2]) atomicAdd(&differ, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = out + (size_t)blockIdx.x * kPlanOut;
    o[0] = a.ok; o[1] = a.dir; o[2] = a.j; o[3] = a.at_edge; o[4] = a.searched; o[5] = a.nu_start;
    o[6] = b.ok; o[7] = b.dir; o[8] = b.j; o[9] = b.at_edge; o[10] = b.searched; o[11] = b.nu_start;
    o[12] = differ;
  }
}

}  // namespace

extern "C" {

int da_sgrid() { return kSGrid; }
int da_plan_out() { return kPlanOut; }

// out [4 kSGrid]: the product's one-pass table, the reference-tolerance integrals, the adaptive
// rule's, ln R.
int da_lns(const double* cosmo, const double* lim, int divmax, double* out) {
  if (!limits_ok(lim, divmax)) return -1;
  const chomp_config cfg = make_config(lim, divmax);
  const double z0 = 0.0;
  Dev snodes(kSigmaStride, nullptr), d_cosmo(8, cosmo), d_out(3 * kSGrid, nullptr);
  DevT<Epoch> epochs(1, nullptr);
  DA_TRY(snodes.err); DA_TRY(d_cosmo.err); DA_TRY(d_out.err); DA_TRY(epochs.err);
  DA_TRY(d_out.nan_fill());
  const int rc = run_sigma_nodes(cfg, cosmo, &z0, 1, snodes, epochs);
  if (rc) return rc;
  hipLaunchKernelGGL(k_ref_lns, dim3(kSGrid), dim3(256), 0, 0, cfg, d_cosmo.p, d_out.p);
  DA_SYNC();
  DA_TRY(hipMemcpy(out, snodes.p + chomp::kSigmaOffLnS, kSGrid * sizeof(double),
                   hipMemcpyDeviceToHost));
  DA_TRY(d_out.back(out + kSGrid, 3 * kSGrid));
  return 0;
}

// out [nz][2][da_plan_out()]: k_plan's record of every (epoch, side); threads: 64 or 256.
int da_plan(const double* cosmo, const double* lim, int divmax, const double* z, int nz,
            int threads, double* out) {
  if (!limits_ok(lim, divmax) || nz < 1 || nz > kMaxZ || (threads != 64 && threads != 256))
    return -1;
  const chomp_config cfg = make_config(lim, divmax);
  // the candidate masses of the 5 % walk, as chomp_ctx_create tabulates them
  std::vector<double> cand(4 * chomp::kSearchJ);
  const double start[4] = {1.0e9, 1.0e9, 1.0e16, 1.0e16};
  const bool mul[4] = {false, true, true, false};
  for (int t = 0; t < 4; ++t) {
    double m = start[t];
    for (int j = 0; j < chomp::kSearchJ; ++j) {
      cand[t * chomp::kSearchJ + j] = m;
      m = mul[t] ? m * 1.05 : m / 1.05;
    }
  }
  Dev snodes(kSigmaStride, nullptr), d_cand(cand.size(), cand.data());
  Dev d_out((size_t)nz * 2 * kPlanOut, nullptr);
  DevT<Epoch> epochs(nz, nullptr);
  DA_TRY(snodes.err); DA_TRY(d_cand.err); DA_TRY(d_out.err); DA_TRY(epochs.err);
  DA_TRY(d_out.nan_fill());
  const int rc = run_sigma_nodes(cfg, cosmo, z, nz, snodes, epochs);
  if (rc) return rc;
  hipLaunchKernelGGL(k_plan, dim3(2 * nz), dim3(threads), 0, 0, epochs.p, snodes.p, d_cand.p,
                     d_out.p);
  DA_SYNC();
  DA_TRY(d_out.back(out, (size_t)nz * 2 * kPlanOut));
  return 0;
}

}  // extern "C"
