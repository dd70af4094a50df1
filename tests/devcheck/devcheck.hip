// TEST-ONLY harness: the device counterpart of tests/hostcheck/hostcheck.cpp.  One HIP
// translation unit that compiles chomp_math.h and chomp_romberg.h FOR THE DEVICE, with the
// product's compiler flags, and drives the fp64 primitives, the wavefront / workgroup
// reductions and the Romberg / Gauss-Legendre quadratures directly -- one small kernel per
// primitive, host arrays in and out.  It is never loaded by the chomp_amd package, is not in
// _lib.UNITS and is no part of the C ABI.  Built and loaded by tests/devcheck_build.py.
//
// Every entry point returns the HIP error code (0: success).  Kernels index only inside the
// buffers the entry point allocated and use the launch shapes the headers document
// (blockDim.x == 64 NW, romberg_scratch<NW, NF>() doubles of LDS).
#include <hip/hip_runtime.h>

#include "../../chomp_amd/csrc/chomp_math.h"
#include "../../chomp_amd/csrc/chomp_romberg.h"

using chomp::BesselTab;
using chomp::SiCiTab;
using chomp::kRombergDump;

namespace {

// ---------------------------------------------------------------------------------------
// host plumbing
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
#define DC_TRY(expr)                            \
  do {                                          \
    const hipError_t e_ = (expr);               \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)
// after a launch: launch errors, then everything the kernel did
#define DC_SYNC()                               \
  do {                                          \
    DC_TRY(hipGetLastError());                  \
    DC_TRY(hipDeviceSynchronize());             \
  } while (0)

struct Tables {
  SiCiTab* sici = nullptr;
  BesselTab* j0 = nullptr;
  BesselTab* j2 = nullptr;
  double* gl16 = nullptr;
  bool ready = false;
};
Tables g_tab;
// the tables as the product uploads them: fill_tables on the host, one copy to the device
int tables_init() {
  if (g_tab.ready) return 0;
  static SiCiTab hs;
  static BesselTab h0, h2;
  chomp::fill_tables(&hs, &h0, &h2);
  DC_TRY(hipMalloc((void**)&g_tab.sici, sizeof(SiCiTab)));
  DC_TRY(hipMalloc((void**)&g_tab.j0, sizeof(BesselTab)));
  DC_TRY(hipMalloc((void**)&g_tab.j2, sizeof(BesselTab)));
  DC_TRY(hipMalloc((void**)&g_tab.gl16, 32 * sizeof(double)));
  DC_TRY(hipMemcpy(g_tab.sici, &hs, sizeof(SiCiTab), hipMemcpyHostToDevice));
  DC_TRY(hipMemcpy(g_tab.j0, &h0, sizeof(BesselTab), hipMemcpyHostToDevice));
  DC_TRY(hipMemcpy(g_tab.j2, &h2, sizeof(BesselTab), hipMemcpyHostToDevice));
  DC_TRY(hipMemcpy(g_tab.gl16, CHOMP_GL16, 32 * sizeof(double), hipMemcpyHostToDevice));
  g_tab.ready = true;
  return 0;
}

constexpr int kEB = 256;                       // block of the element-wise kernels
inline int eblocks(int n) { return (n + kEB - 1) / kEB; }

// ---------------------------------------------------------------------------------------
// element-wise primitives: one thread per element
// ---------------------------------------------------------------------------------------
__global__ void k_exp(const double* x, int n, double* mine, double* lib) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  mine[i] = chomp::exp(x[i]);
  lib[i] = ::exp(x[i]);
}
__global__ void k_fast_log(const double* x, int n, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = chomp::fast_log(x[i]);
}
// fast_sincos, fast_sincos_pm, sin x - x cos x from fast_sincos, and tophat_numer_pm in both call
// forms: with its default argument, and with sincos_lead() fetched outside a loop over the
// elements (the product's form: a grid-stride loop here)
__global__ void k_sincos(const double* x, int n, double* s, double* c, double* spm, double* cpm,
                         double* th_ref, double* th_default, double* th_lead) {
  const chomp::SinCosLead lead = chomp::sincos_lead();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double ss, cc;
    chomp::fast_sincos(x[i], &ss, &cc);
    s[i] = ss;
    c[i] = cc;
    th_ref[i] = fma(-x[i], cc, ss);
    chomp::fast_sincos_pm(x[i], &ss, &cc);
    spm[i] = ss;
    cpm[i] = cc;
    th_default[i] = chomp::tophat_numer_pm(x[i]);
    th_lead[i] = chomp::tophat_numer_pm(x[i], lead);
  }
}
__global__ void k_sici(const double* x, const double* ln_x, int n, const SiCiTab* T, double* si,
                       double* ci, double* si_ln, double* ci_ln) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  chomp::sici(x[i], *T, &si[i], &ci[i]);
  double s = 0.0, c = 1.0;
  if (x[i] >= 4.0) chomp::fast_sincos(x[i], &s, &c);
  chomp::sici_sc_ln(x[i], ln_x[i], s, c, *T, &si_ln[i], &ci_ln[i]);
}
template <int ORDER>
__global__ void k_bessel(const double* x, int n, const BesselTab* T, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = chomp::bessel_j<ORDER>(x[i], *T);
}
// fma_k(a, b, C) beside fma(a, b, C) for kFmaK compile-time constants C; out[k * n + i]
constexpr int kFmaK = 6;
#define DC_FMA_CONSTANTS(X)                                                                    \
  X(0, 1.0) X(1, -1.0 / 3.0) X(2, 2.75573137070700676789e-06) X(3, -1.0e300) X(4, 3.0e-310)   \
  X(5, -2.2250738585072014e-308)
__global__ void k_fma_k(const double* a, const double* b, int n, double* out_k, double* out_f) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double av = a[i], bv = b[i];
#define X(k, C)                                             \
  out_k[(size_t)(k) * n + i] = chomp::fma_k(av, bv, (C));   \
  out_f[(size_t)(k) * n + i] = fma(av, bv, (C));
  DC_FMA_CONSTANTS(X)
#undef X
}
// the not-a-knot spline: coefficients by spline_build on the device (one thread, as the kernels
// that build a spline serially do), evaluated by another launch
__global__ void k_spline_build(const double* x, const double* y, int n, double* c, double* work) {
  if (blockIdx.x == 0 && threadIdx.x == 0) chomp::spline_build(x, y, n, c, work);
}
__global__ void k_spline_eval(const double* x, const double* c, int n, const double* xe, int ne,
                              double* out, int uniform) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ne) return;
  out[i] = uniform ? chomp::spline_eval_uniform(x[0], (x[n - 1] - x[0]) / (n - 1), c, n, xe[i])
                   : chomp::spline_eval(x, c, n, xe[i]);
}

// ---------------------------------------------------------------------------------------
// reductions: 64 doubles per wavefront in, one double per lane out
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_wave_sum(const double* in, double* out, int mode) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  const double v = in[i];
  double r;
  if (mode == 0) r = chomp::wave_sum(v);
  else if (mode == 1) r = chomp::wave_sum32(v);
  else r = chomp::wave_sum16(v);
  out[i] = r;
}
// group_sum<NW> twice in a row (the second call uses the other half of `red`)
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_group_sum(const double* in1, const double* in2,
                                                       double* out1, double* out2) {
  extern __shared__ double lds[];
  const size_t i = (size_t)blockIdx.x * (64 * NW) + threadIdx.x;
  int flip = 0;
  out1[i] = chomp::group_sum<NW>(in1[i], lds, flip);
  out2[i] = chomp::group_sum<NW>(in2[i], lds, flip);
}

// ---------------------------------------------------------------------------------------
// quadrature: a fixed menu of integrands, each written once.  tests/test_gpu_romberg.py restates
// them in NumPy, operation for operation: no FMA contraction here, so that the two evaluate the
// same arithmetic and what the tests compare is the quadrature.
// ---------------------------------------------------------------------------------------
struct Menu {
  int id;
  __device__ double operator()(double x) const {
#pragma clang fp contract(off)
    switch (id) {
      case 0: return x * x * x - 2.0 * x + 1.0;
      case 1: return chomp::exp(x);
      case 2: return ::sin(10.0 * x);
      case 3: return 1.0 + ::sin(40.0 * x);
      case 4: return chomp::exp(-200.0 * ((x - 0.37) * (x - 0.37)));
      case 5: return ::sqrt(x);
      case 6: return x < 0.3 ? 1.0 : 0.25;
      case 7: return 1.0 / (1e-4 + (x - 0.5) * (x - 0.5));
      case 8: {
        const double d = 1.0 + chomp::exp(2.0 * x);
        return chomp::exp(1.5 * x) / (d * d);
      }
      case 9: return ::cos(x);
      case 10: return 0.0;
      // polynomials for gauss_panels
      case 11: {                                  // sum_{k=0}^{31} x^k / (k + 1), Horner
        double p = 1.0 / 32.0;
        for (int k = 30; k >= 0; --k) p = p * x + 1.0 / (double)(k + 1);
        return p;
      }
      case 12: {                                  // x^31 by squarings
        const double x2 = x * x, x4 = x2 * x2, x8 = x4 * x4, x16 = x8 * x8;
        return (((x16 * x8) * x4) * x2) * x;
      }
      case 13: return (x * x) * (x * x) * x + 3.0 * (x * x) + 0.5;   // x^5 + 3 x^2 + 1/2
      default: return 0.0;
    }
  }
};
// NF integrands that share their nodes
template <int NF>
struct MenuN {
  int id0, id1;
  __device__ void operator()(double x, double (&out)[NF]) const {
    out[0] = Menu{id0}(x);
    if constexpr (NF > 1) out[1] = Menu{id1}(x);
  }
};
// an integrand that offers fast() and refuses some nodes (what it leaves in `out` then must not
// reach the sum: NaN)
struct FastMenu {
  int id;
  __device__ bool fast(double x, double (&out)[1], int, long j) const {
    if (j % 7 == 3 || j % 64 == 10) {
      out[0] = __longlong_as_double(0x7ff8000000000000LL);
      return false;
    }
    out[0] = Menu{id}(x);
    return true;
  }
  __device__ void operator()(double x, double (&out)[1], int, long) const { out[0] = Menu{id}(x); }
};
// the (x, out, level, j) signature: j, level and 1 where x is the node (level, j) of [a, b]
// (1e9 where it is not) -- every value and every sum of them an exact integer in a double
struct IndexF {
  double a, b;
  __device__ void operator()(double x, double (&out)[3], int level, long j) const {
    out[0] = (double)j;
    out[1] = (double)level;
    double want;
    if (level == 0) {
      want = j == 0 ? a : b;
    } else {
      const double h = ldexp(b - a, 1 - level);
      want = (a + 0.5 * h) + h * (double)j;
    }
    out[2] = x == want ? 1.0 : 1.0e9;
  }
};

// One case: kCase doubles in, kOut doubles out.
//   in:  a, b, tol, rtol, divmax, id0, id1, use_loose, loose.rtol, lo1, hi1, lo2, hi2, d
//   out: value0, value1, level0, level1, converged0, converged1 (-1: not reported),
//        1 where a thread of the group disagrees with thread 0 in a value or level, resume steps
constexpr int kCase = 16, kOut = 8;
struct QCase {
  double a, b, tol, rtol;
  int divmax, id0, id1, d;
  bool use_loose;
  chomp::RombergLoose loose;
};
__device__ QCase load_case(const double* c) {
  QCase q;
  q.a = c[0]; q.b = c[1]; q.tol = c[2]; q.rtol = c[3];
  q.divmax = (int)c[4]; q.id0 = (int)c[5]; q.id1 = (int)c[6];
  q.use_loose = c[7] != 0.0;
  q.loose = chomp::RombergLoose{c[8], c[9], c[10], c[11], c[12]};
  q.d = (int)c[13];
  return q;
}
template <int NF>
__device__ void store_case(double* o, const double (&value)[NF], const int (&level)[NF],
                           const int (&conv)[NF], int steps) {
  __shared__ double v0[2];
  __shared__ int l0[2];
  __shared__ int bad;
  if (threadIdx.x == 0) {
    bad = 0;
    for (int q = 0; q < NF; ++q) { v0[q] = value[q]; l0[q] = level[q]; }
  }
  __syncthreads();
  for (int q = 0; q < NF; ++q)
    if (__double_as_longlong(value[q]) != __double_as_longlong(v0[q]) || level[q] != l0[q]) bad = 1;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 0; q < 6; ++q) o[q] = 0.0;
    for (int q = 0; q < NF; ++q) {
      o[q] = value[q];
      o[2 + q] = (double)level[q];
      o[4 + q] = (double)conv[q];
    }
    o[6] = (double)bad;
    o[7] = (double)steps;
  }
}

enum Kind { kGroup, kGroupU4, kGroupFast4, kWave6, kRomberg1 };
template <int KIND, int NW, int NF>
__global__ __launch_bounds__(64 * NW) void k_quad(const double* cases, double* out) {
  extern __shared__ double lds[];
  const QCase c = load_case(cases + (size_t)blockIdx.x * kCase);
  const chomp::RombergLoose* loose = c.use_loose ? &c.loose : nullptr;
  const MenuN<NF> f{c.id0, c.id1};
  double value[NF];
  int level[NF], conv[NF];
  if constexpr (KIND == kRomberg1) {
    static_assert(NF == 1, "romberg1 takes one integrand");
    const Menu m{c.id0};
    int lev = -1;
    value[0] = chomp::romberg1<NW>(m, c.a, c.b, c.tol, c.rtol, c.divmax, lds, &lev);
    level[0] = lev;
    conv[0] = -1;
  } else {
    chomp::RombergOut<NF> r;
    if constexpr (KIND == kGroup) {
      r = chomp::romberg_group<NW, NF>(f, c.a, c.b, c.tol, c.rtol, c.divmax, lds, nullptr, loose);
    } else if constexpr (KIND == kGroupU4) {
      r = chomp::romberg_group<NW, NF, MenuN<NF>, 4>(f, c.a, c.b, c.tol, c.rtol, c.divmax, lds);
    } else if constexpr (KIND == kGroupFast4) {
      static_assert(NF == 1, "FastMenu is one integrand");
      const FastMenu g{c.id0};
      r = chomp::romberg_group<NW, 1, FastMenu, 4>(g, c.a, c.b, c.tol, c.rtol, c.divmax, lds);
    } else {
      static_assert(NW == 1, "romberg_wave6 is one wavefront");
      double fb[NF];
      f(c.b, fb);
      r = chomp::romberg_wave6<NF>(f, c.a, c.b, fb, c.tol, c.rtol, c.divmax, nullptr, loose);
    }
    for (int q = 0; q < NF; ++q) {
      value[q] = r.value[q];
      level[q] = r.level[q];
      conv[q] = r.converged[q] ? 1 : 0;
    }
  }
  store_case<NF>(out + (size_t)blockIdx.x * kOut, value, level, conv, 0);
}
template <int KIND, int NW, int NF>
int run_quad(const double* cases, int ncases, double* out) {
  if (ncases <= 0) return 0;
  Dev dc((size_t)ncases * kCase, cases), dout((size_t)ncases * kOut, nullptr);
  DC_TRY(dc.err);
  DC_TRY(dout.err);
  const size_t lds = (size_t)chomp::romberg_scratch<NW, NF>() * sizeof(double);
  hipLaunchKernelGGL((k_quad<KIND, NW, NF>), dim3(ncases), dim3(64 * NW), lds, 0, dc.p, dout.p);
  DC_SYNC();
  DC_TRY(dout.back(out, (size_t)ncases * kOut));
  return 0;
}

// The hand-over: the integral stopped by divmax = d with its state dumped (STAGE 0:
// romberg_group<4, 1>, STAGE 1: romberg_wave6<1>, every wavefront the same integral), then
// carried on by RombergResume with group_sum<4> level sums to the final divmax.
template <int STAGE>
__global__ __launch_bounds__(256) void k_resume(const double* cases, double* out) {
  constexpr int NW = 4, NT = 64 * NW;
  extern __shared__ double lds[];
  __shared__ double dump[kRombergDump];
  const QCase c = load_case(cases + (size_t)blockIdx.x * kCase);
  const MenuN<1> f{c.id0, c.id0};
  chomp::RombergOut<1> r;
  if constexpr (STAGE == 0) {
    r = chomp::romberg_group<NW, 1>(f, c.a, c.b, c.tol, c.rtol, c.d, lds, dump);
  } else {
    double fb[1];
    f(c.b, fb);
    r = chomp::romberg_wave6<1>(f, c.a, c.b, fb, c.tol, c.rtol, c.d,
                                threadIdx.x < 64 ? dump : nullptr);
  }
  __syncthreads();
  double value[1] = {r.value[0]};
  int level[1] = {r.level[0]}, conv[1] = {r.converged[0] ? 1 : 0};
  int steps = 0;
  if (!r.converged[0]) {                                    // (block-uniform)
    chomp::RombergResume R;
    R.load(dump, c.d, c.b - c.a, c.tol, c.rtol);
    int flip = 0;
    for (int lv = c.d + 1; lv <= c.divmax && !R.done; ++lv) {
      const double c_il = CHOMP_ROMBERG_C[lv][threadIdx.x & 31];
      const long numtosum = 1L << (lv - 1);
      const double h = ldexp(c.b - c.a, 1 - lv), lox = c.a + 0.5 * h;
      double part = 0.0;
      for (long j = threadIdx.x; j < numtosum; j += NT) {
        double v[1];
        f(lox + h * (double)j, v);
        part += v[0];
      }
      R.advance(lv, chomp::group_sum<NW>(part, lds, flip), c_il);
      ++steps;
    }
    value[0] = R.value;
    level[0] = R.level;
    conv[0] = R.done ? 1 : 0;
  }
  store_case<1>(out + (size_t)blockIdx.x * kOut, value, level, conv, steps);
}

// Node indexing: IndexF run to divmax (tol = rtol = 0 never stops a row), the state dumped:
// per case 3 * kRombergDump doubles (T_0 .. T_31, the node sum, the last row) + level, converged
constexpr int kIndexOut = 3 * kRombergDump + 2;
template <int WAVE6, int NW>
__global__ __launch_bounds__(64 * NW) void k_index(const double* cases, double* out) {
  extern __shared__ double lds[];
  const QCase c = load_case(cases + (size_t)blockIdx.x * kCase);
  const IndexF f{c.a, c.b};
  double* o = out + (size_t)blockIdx.x * kIndexOut;
  chomp::RombergOut<3> r;
  if constexpr (WAVE6) {
    const double fb[3] = {1.0, 0.0, 1.0};                   // node (level 0, j = 1)
    r = chomp::romberg_wave6<3>(f, c.a, c.b, fb, 0.0, 0.0, c.divmax, o);
  } else {
    r = chomp::romberg_group<NW, 3>(f, c.a, c.b, 0.0, 0.0, c.divmax, lds, o);
  }
  if (threadIdx.x == 0) {
    o[3 * kRombergDump] = (double)r.level[0];
    o[3 * kRombergDump + 1] = (r.converged[0] || r.converged[1] || r.converged[2]) ? 1.0 : 0.0;
  }
}
template <int WAVE6, int NW>
int run_index(const double* cases, int ncases, double* out) {
  if (ncases <= 0) return 0;
  Dev dc((size_t)ncases * kCase, cases), dout((size_t)ncases * kIndexOut, nullptr);
  DC_TRY(dc.err);
  DC_TRY(dout.err);
  const size_t lds = (size_t)chomp::romberg_scratch<NW, 3>() * sizeof(double);
  hipLaunchKernelGGL((k_index<WAVE6, NW>), dim3(ncases), dim3(64 * NW), lds, 0, dc.p, dout.p);
  DC_SYNC();
  DC_TRY(dout.back(out, (size_t)ncases * kIndexOut));
  return 0;
}

// gauss_panels<NW>: case = a, b, npanel (the divmax slot), id0; one double out
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_gauss(const double* cases, const double* xw,
                                                   double* out) {
  extern __shared__ double lds[];
  const QCase c = load_case(cases + (size_t)blockIdx.x * kCase);
  const Menu m{c.id0};
  int flip = 0;
  const double v = chomp::gauss_panels<NW>(m, c.a, c.b, c.divmax, xw, lds, flip);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}
template <int NW>
int run_gauss(const double* cases, int ncases, double* out) {
  if (ncases <= 0) return 0;
  if (int e = tables_init()) return e;
  Dev dc((size_t)ncases * kCase, cases), dout((size_t)ncases, nullptr);
  DC_TRY(dc.err);
  DC_TRY(dout.err);
  hipLaunchKernelGGL((k_gauss<NW>), dim3(ncases), dim3(64 * NW), 2 * NW * sizeof(double), 0, dc.p,
                     g_tab.gl16, dout.p);
  DC_SYNC();
  DC_TRY(dout.back(out, (size_t)ncases));
  return 0;
}

template <int NW>
int run_group_sum(const double* in1, const double* in2, int ngroups, double* out1, double* out2) {
  const size_t n = (size_t)ngroups * 64 * NW;
  Dev a(n, in1), b(n, in2), o1(n, nullptr), o2(n, nullptr);
  DC_TRY(a.err); DC_TRY(b.err); DC_TRY(o1.err); DC_TRY(o2.err);
  hipLaunchKernelGGL((k_group_sum<NW>), dim3(ngroups), dim3(64 * NW), 2 * NW * sizeof(double), 0,
                     a.p, b.p, o1.p, o2.p);
  DC_SYNC();
  DC_TRY(o1.back(out1, n));
  DC_TRY(o2.back(out2, n));
  return 0;
}

}  // namespace

extern "C" {

int dc_case_stride() { return kCase; }
int dc_out_stride() { return kOut; }
int dc_index_out_stride() { return kIndexOut; }
int dc_fma_k_count() { return kFmaK; }
void dc_fma_k_constants(double* c) {
#define X(k, C) c[k] = (C);
  DC_FMA_CONSTANTS(X)
#undef X
}
// the 16 abscissae and 16 weights gauss_panels is given
void dc_gl16(double* xw) {
  for (int i = 0; i < 32; ++i) xw[i] = CHOMP_GL16[i];
}

int dc_exp(const double* x, int n, double* mine, double* lib) {
  if (n <= 0) return 0;
  Dev dx(n, x), dm(n, nullptr), dl(n, nullptr);
  DC_TRY(dx.err); DC_TRY(dm.err); DC_TRY(dl.err);
  hipLaunchKernelGGL(k_exp, dim3(eblocks(n)), dim3(kEB), 0, 0, dx.p, n, dm.p, dl.p);
  DC_SYNC();
  DC_TRY(dm.back(mine, n));
  DC_TRY(dl.back(lib, n));
  return 0;
}
int dc_fast_log(const double* x, int n, double* out) {
  if (n <= 0) return 0;
  Dev dx(n, x), dout(n, nullptr);
  DC_TRY(dx.err); DC_TRY(dout.err);
  hipLaunchKernelGGL(k_fast_log, dim3(eblocks(n)), dim3(kEB), 0, 0, dx.p, n, dout.p);
  DC_SYNC();
  DC_TRY(dout.back(out, n));
  return 0;
}
// out: 7 rows of n -- sin, cos, fast_sincos_pm's pair, sin x - x cos x from fast_sincos,
// tophat_numer_pm(x), tophat_numer_pm(x, lead)
int dc_sincos(const double* x, int n, double* out) {
  if (n <= 0) return 0;
  Dev dx(n, x), dout((size_t)7 * n, nullptr);
  DC_TRY(dx.err); DC_TRY(dout.err);
  double* o = dout.p;
  // (a third of the blocks one thread per element would take: the loop runs about three times)
  const int blocks = (eblocks(n) + 2) / 3;
  hipLaunchKernelGGL(k_sincos, dim3(blocks), dim3(kEB), 0, 0, dx.p, n, o, o + n, o + 2 * (size_t)n,
                     o + 3 * (size_t)n, o + 4 * (size_t)n, o + 5 * (size_t)n, o + 6 * (size_t)n);
  DC_SYNC();
  DC_TRY(dout.back(out, (size_t)7 * n));
  return 0;
}
// out: 4 rows of n -- sici's Si, Ci, sici_sc_ln's Si, Ci (ln_x: the caller's ln x)
int dc_sici(const double* x, const double* ln_x, int n, double* out) {
  if (n <= 0) return 0;
  if (int e = tables_init()) return e;
  Dev dx(n, x), dl(n, ln_x), dout((size_t)4 * n, nullptr);
  DC_TRY(dx.err); DC_TRY(dl.err); DC_TRY(dout.err);
  double* o = dout.p;
  hipLaunchKernelGGL(k_sici, dim3(eblocks(n)), dim3(kEB), 0, 0, dx.p, dl.p, n, g_tab.sici, o, o + n,
                     o + 2 * (size_t)n, o + 3 * (size_t)n);
  DC_SYNC();
  DC_TRY(dout.back(out, (size_t)4 * n));
  return 0;
}
int dc_bessel(int order, const double* x, int n, double* out) {
  if (n <= 0) return 0;
  if (order != 0 && order != 2) return (int)hipErrorInvalidValue;
  if (int e = tables_init()) return e;
  Dev dx(n, x), dout(n, nullptr);
  DC_TRY(dx.err); DC_TRY(dout.err);
  if (order == 0)
    hipLaunchKernelGGL(k_bessel<0>, dim3(eblocks(n)), dim3(kEB), 0, 0, dx.p, n, g_tab.j0, dout.p);
  else
    hipLaunchKernelGGL(k_bessel<2>, dim3(eblocks(n)), dim3(kEB), 0, 0, dx.p, n, g_tab.j2, dout.p);
  DC_SYNC();
  DC_TRY(dout.back(out, n));
  return 0;
}
// out_k, out_f: dc_fma_k_count() rows of n
int dc_fma_k(const double* a, const double* b, int n, double* out_k, double* out_f) {
  if (n <= 0) return 0;
  Dev da(n, a), db(n, b), dk((size_t)kFmaK * n, nullptr), df((size_t)kFmaK * n, nullptr);
  DC_TRY(da.err); DC_TRY(db.err); DC_TRY(dk.err); DC_TRY(df.err);
  hipLaunchKernelGGL(k_fma_k, dim3(eblocks(n)), dim3(kEB), 0, 0, da.p, db.p, n, dk.p, df.p);
  DC_SYNC();
  DC_TRY(dk.back(out_k, (size_t)kFmaK * n));
  DC_TRY(df.back(out_f, (size_t)kFmaK * n));
  return 0;
}
int dc_spline(const double* x, const double* y, int n, const double* xe, int ne, double* out,
              int uniform) {
  if (n < 4 || ne <= 0) return (int)hipErrorInvalidValue;
  Dev dx(n, x), dy(n, y), dcf((size_t)4 * (n - 1), nullptr), dw((size_t)2 * n, nullptr),
      de(ne, xe), dout(ne, nullptr);
  DC_TRY(dx.err); DC_TRY(dy.err); DC_TRY(dcf.err); DC_TRY(dw.err); DC_TRY(de.err); DC_TRY(dout.err);
  hipLaunchKernelGGL(k_spline_build, dim3(1), dim3(64), 0, 0, dx.p, dy.p, n, dcf.p, dw.p);
  hipLaunchKernelGGL(k_spline_eval, dim3(eblocks(ne)), dim3(kEB), 0, 0, dx.p, dcf.p, n, de.p, ne,
                     dout.p, uniform);
  DC_SYNC();
  DC_TRY(dout.back(out, ne));
  return 0;
}

// mode 0: wave_sum, 1: wave_sum32, 2: wave_sum16; in / out: 64 * nwaves doubles
int dc_wave_sum(int mode, const double* in, int nwaves, double* out) {
  if (nwaves <= 0) return 0;
  if (mode < 0 || mode > 2) return (int)hipErrorInvalidValue;
  const size_t n = (size_t)nwaves * 64;
  Dev di(n, in), dout(n, nullptr);
  DC_TRY(di.err); DC_TRY(dout.err);
  hipLaunchKernelGGL(k_wave_sum, dim3(nwaves), dim3(64), 0, 0, di.p, dout.p, mode);
  DC_SYNC();
  DC_TRY(dout.back(out, n));
  return 0;
}
// group_sum<nw> of in1, then of in2; 64 * nw * ngroups doubles each
int dc_group_sum(int nw, const double* in1, const double* in2, int ngroups, double* out1,
                 double* out2) {
  if (ngroups <= 0) return 0;
  switch (nw) {
    case 2: return run_group_sum<2>(in1, in2, ngroups, out1, out2);
    case 4: return run_group_sum<4>(in1, in2, ngroups, out1, out2);
    case 8: return run_group_sum<8>(in1, in2, ngroups, out1, out2);
    case 16: return run_group_sum<16>(in1, in2, ngroups, out1, out2);
    default: return (int)hipErrorInvalidValue;
  }
}

// shape: 0..4 romberg_group<1|2|4|8|16, 1>; 5, 6 romberg_group<1|4, 2>; 7 romberg_group<4, 1, F, 4>;
// 8 the same with an integrand that offers fast(); 9, 10 romberg_wave6<1|2>; 11, 12 romberg1<1|4>
int dc_quad(int shape, const double* cases, int ncases, double* out) {
  switch (shape) {
    case 0: return run_quad<kGroup, 1, 1>(cases, ncases, out);
    case 1: return run_quad<kGroup, 2, 1>(cases, ncases, out);
    case 2: return run_quad<kGroup, 4, 1>(cases, ncases, out);
    case 3: return run_quad<kGroup, 8, 1>(cases, ncases, out);
    case 4: return run_quad<kGroup, 16, 1>(cases, ncases, out);
    case 5: return run_quad<kGroup, 1, 2>(cases, ncases, out);
    case 6: return run_quad<kGroup, 4, 2>(cases, ncases, out);
    case 7: return run_quad<kGroupU4, 4, 1>(cases, ncases, out);
    case 8: return run_quad<kGroupFast4, 4, 1>(cases, ncases, out);
    case 9: return run_quad<kWave6, 1, 1>(cases, ncases, out);
    case 10: return run_quad<kWave6, 1, 2>(cases, ncases, out);
    case 11: return run_quad<kRomberg1, 1, 1>(cases, ncases, out);
    case 12: return run_quad<kRomberg1, 4, 1>(cases, ncases, out);
    default: return (int)hipErrorInvalidValue;
  }
}
// stage 0: romberg_group<4, 1> to divmax d, stage 1: romberg_wave6<1>; then RombergResume
int dc_resume(int stage, const double* cases, int ncases, double* out) {
  if (ncases <= 0) return 0;
  if (stage != 0 && stage != 1) return (int)hipErrorInvalidValue;
  Dev dc((size_t)ncases * kCase, cases), dout((size_t)ncases * kOut, nullptr);
  DC_TRY(dc.err);
  DC_TRY(dout.err);
  const size_t lds = (size_t)chomp::romberg_scratch<4, 1>() * sizeof(double);
  if (stage == 0) hipLaunchKernelGGL(k_resume<0>, dim3(ncases), dim3(256), lds, 0, dc.p, dout.p);
  else hipLaunchKernelGGL(k_resume<1>, dim3(ncases), dim3(256), lds, 0, dc.p, dout.p);
  DC_SYNC();
  DC_TRY(dout.back(out, (size_t)ncases * kOut));
  return 0;
}
// shape 0..4: romberg_group<1|2|4|8|16, 3>, 5: romberg_wave6<3>
int dc_index(int shape, const double* cases, int ncases, double* out) {
  switch (shape) {
    case 0: return run_index<0, 1>(cases, ncases, out);
    case 1: return run_index<0, 2>(cases, ncases, out);
    case 2: return run_index<0, 4>(cases, ncases, out);
    case 3: return run_index<0, 8>(cases, ncases, out);
    case 4: return run_index<0, 16>(cases, ncases, out);
    case 5: return run_index<1, 1>(cases, ncases, out);
    default: return (int)hipErrorInvalidValue;
  }
}
int dc_gauss(int nw, const double* cases, int ncases, double* out) {
  if (nw == 1) return run_gauss<1>(cases, ncases, out);
  if (nw == 4) return run_gauss<4>(cases, ncases, out);
  return (int)hipErrorInvalidValue;
}

}  // extern "C"
