// TEST-ONLY harness: the one-wavefront not-a-knot build, spline_build_pcr_wave, beside the block
// builder it stands in for, spline_build_pcr, on the same knots in the shapes the product calls
// them in (thin kernels: the product has none around them).  It includes the product's header,
// never a copy of its functions.  Never loaded by the chomp_amd package, not in _lib.UNITS, no
// part of the C ABI.  Built and loaded through tests/devcheck_build.py by tests/test_gpu_devspline.py.
//
// The entry point allocates its buffers, fills the outputs with NaN bytes (what a kernel never
// wrote stays recognisable), launches, synchronises, returns the HIP error code (0: success; -1:
// an argument outside what the buffers were sized for) and frees its buffers.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../chomp_amd/csrc/chomp_mass_kernels.h"

namespace {

constexpr int kMaxSys = 2, kBlock = 256;

struct Dev {
  double* p = nullptr;
  hipError_t err = hipSuccess;
  size_t n;
  Dev(size_t n_, const double* host) : n(n_) {
    err = hipMalloc((void**)&p, n * sizeof(double));
    if (err == hipSuccess)
      err = host ? hipMemcpy(p, host, n * sizeof(double), hipMemcpyHostToDevice)
                 : hipMemset(p, 0xFF, n * sizeof(double));
  }
  ~Dev() { if (p) (void)hipFree(p); }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
};
#define DS_TRY(expr)                            \
  do {                                          \
    const hipError_t e_ = (expr);               \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)

// LDS: per system s, x [n], y [n], work [9 n] at sm + 11 n s
__device__ __forceinline__ void stage(double* sm, const double* x, const double* y, int n, int n_sys) {
  for (int i = threadIdx.x; i < n_sys * n; i += blockDim.x) {
    const int s = i / n, r = i - s * n;
    sm[(size_t)11 * n * s + r] = x[i];
    sm[(size_t)11 * n * s + n + r] = y[i];
  }
  __syncthreads();
}

// block 256: system s on the threads [s tps, (s + 1) tps), rows strided by tps; tps 64 is the
// knot families' shape (one wavefront each), tps 128 the mass tables'
__global__ __launch_bounds__(kBlock) void k_block(const double* x, const double* y, int n, int n_sys,
                                                  int tps, double* c) {
  extern __shared__ __align__(16) double sm[];
  stage(sm, x, y, n, n_sys);
  const int s = (int)threadIdx.x / tps, tid = (int)threadIdx.x % tps;
  const bool active = s < n_sys;
  double* my = sm + (size_t)11 * n * (active ? s : 0);
  chomp::spline_build_pcr(my, my + n, n, c + (size_t)(active ? s : 0) * 4 * (n - 1), my + 2 * n, tid,
                          tps, active);
}

// block 256: system s by wavefront s alone; the other wavefronts go straight to the end
__global__ __launch_bounds__(kBlock) void k_wave(const double* x, const double* y, int n, int n_sys,
                                                 double* c) {
  extern __shared__ __align__(16) double sm[];
  stage(sm, x, y, n, n_sys);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave >= n_sys) return;
  double* my = sm + (size_t)11 * n * wave;
  chomp::spline_build_pcr_wave(my, my + n, n, c + (size_t)wave * 4 * (n - 1), my + 2 * n, lane);
}

}  // namespace

extern "C" {

int ds_wave_max() { return chomp::kSplineWaveMax; }

// n_sys systems of n knots, x[s n + i], y[s n + i]: c_block[s 4 (n - 1) + 4 i + p] by
// spline_build_pcr (tps 64 or 128), c_wave[...] by spline_build_pcr_wave.
int ds_build(const double* x, const double* y, int n, int n_sys, int tps, double* c_block,
             double* c_wave) {
  if (n < 4 || n > chomp::kSplineWaveMax || n_sys < 1 || n_sys > kMaxSys || (tps != 64 && tps != 128))
    return -1;
  const size_t nk = (size_t)n_sys * n, nc = (size_t)n_sys * 4 * (n - 1);
  Dev d_x(nk, x), d_y(nk, y), d_b(nc, nullptr), d_w(nc, nullptr);
  DS_TRY(d_x.err); DS_TRY(d_y.err); DS_TRY(d_b.err); DS_TRY(d_w.err);
  const size_t lds = (size_t)n_sys * 11 * n * sizeof(double);
  k_block<<<dim3(1), dim3(kBlock), lds>>>(d_x.p, d_y.p, n, n_sys, tps, d_b.p);
  k_wave<<<dim3(1), dim3(kBlock), lds>>>(d_x.p, d_y.p, n, n_sys, d_w.p);
  DS_TRY(hipGetLastError());
  DS_TRY(hipDeviceSynchronize());
  DS_TRY(hipMemcpy(c_block, d_b.p, nc * sizeof(double), hipMemcpyDeviceToHost));
  DS_TRY(hipMemcpy(c_wave, d_w.p, nc * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
