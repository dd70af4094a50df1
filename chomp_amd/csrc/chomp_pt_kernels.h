// chomp_pt_kernels.h -- perturbation_spectra.PerturbationTheory (perturbation_spectra.py:36-345)
// and the second-order bias of mass_function.MassFunctionSecondOrder (mass_function.py:365-434).
//
//   k_pt        the tree-level forms (F2, F3 kernels, bispectrum, trispectrum) for N
//               configurations over an epoch range: one configuration per lane, grid-stride
//               loop, the epoch record staged once per block as Stage E does
//   k_mass_b2   per epoch: the not-a-knot sigma(nu) spline and bias_2_norm = -int f b2 dnu
//   k_eval_b2   bias_2_nu / sigma(nu) lookups of one epoch
//
// The forms keep the reference's order of operations, its thresholds and its branches; every
// function body switches floating-point contraction off, so no multiply-add is fused where numpy
// rounds twice.  P_lin is linear_power_t, the function every CHOMP_P_LIN launch of Stage E calls.
#pragma once

#include "chomp_power_kernels.h"

namespace chomp {

// Forms (include/chomp_mi355x.h CHOMP_PT_*) and the doubles of one configuration.
enum {
  PT_FS2 = 0, PT_FS2_LEN = 1, PT_FS2_KDIFF = 2, PT_FS3 = 3, PT_FS3_PARALLELOGRAM = 4, PT_F3 = 5,
  PT_FS3_BCGS = 6, PT_BISPECTRUM = 7, PT_BISPECTRUM_LEN = 8, PT_TRISPECTRUM = 9,
  PT_TRISPECTRUM_PARALLELOGRAM = 10
};
constexpr int kPtForms = 11;
__host__ __device__ constexpr int pt_arity(int form) {
  return form == PT_FS2 ? 6
       : (form == PT_FS3 || form == PT_F3 || form == PT_FS3_BCGS || form == PT_BISPECTRUM) ? 9
       : form == PT_BISPECTRUM_LEN ? 6
       : form == PT_TRISPECTRUM ? 12
       : 3;
}
__host__ __device__ constexpr bool pt_needs_power(int form) {
  return form == PT_BISPECTRUM || form == PT_BISPECTRUM_LEN || form == PT_TRISPECTRUM ||
         form == PT_TRISPECTRUM_PARALLELOGRAM;
}

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 v3(const double* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a) { return V3{-a.x, -a.y, -a.z}; }
// numpy.dot / numpy.vdot of two 3-vectors: the products summed from the first
__device__ __forceinline__ double dot3(V3 a, V3 b) {
#pragma clang fp contract(off)
  double s = a.x * b.x;
  s = s + a.y * b.y;
  return s + a.z * b.z;
}

// alpha_BCGS, gamma_BCGS (perturbation_spectra.py:36-56): 0 on exact zeros
__device__ __forceinline__ double pt_alpha(V3 k1, V3 k2) {
#pragma clang fp contract(off)
  const double k1sq = dot3(k1, k1);
  if (k1sq == 0.0) return 0.0;
  return dot3(k1 + k2, k1) / k1sq;
}
__device__ __forceinline__ double pt_gamma(V3 k1, V3 k2) {
#pragma clang fp contract(off)
  const double k1a = dot3(k1, k1), k2a = dot3(k2, k2);
  if (k1a * k2a == 0.0) return 0.0;
  const double d = dot3(k1, k2);
  return 1.0 - (d * d) / (k1a * k2a);
}

// Fs2 (perturbation_spectra.py:89-105): 5/7 when |k1| or |k2| < 1e-8
__device__ __forceinline__ double pt_fs2(V3 k1, V3 k2) {
#pragma clang fp contract(off)
  const double d = dot3(k1, k2);
  const double k1a = sqrt(dot3(k1, k1));
  const double k2a = sqrt(dot3(k2, k2));
  if (k1a < 1.e-8 || k2a < 1.e-8) return 5. / 7.;
  const double rat = d / (k1a * k2a);
  return (5. / 7. + (rat / 2.) * (k1a / k2a + k2a / k1a)) + ((2. / 7.) * rat) * rat;
}

// Fs2_len (:107-123): a numpy.where -- both branches are evaluated, only the values matter
__device__ __forceinline__ double pt_fs2_len(double k1, double k2, double z) {
#pragma clang fp contract(off)
  const double other = (5. / 7. + (z / 2.) * (k1 / k2 + k2 / k1)) + ((2. / 7.) * z) * z;
  return (k1 < 1.e-8 || k2 < 1.e-8) ? 5.0 / 7.0 : other;
}

// Fs2_kdiff (:125-132): z divides by x, the squared length, as shipped
__device__ __forceinline__ double pt_fs2_kdiff(double k1, double k2, double mu) {
#pragma clang fp contract(off)
  const double x = (k1 * k1 + k2 * k2) - ((2. * k1) * k2) * mu;
  const double z = (k1 * mu - k2) / x;
  const double xrt = sqrt(x);
  return pt_fs2_len(xrt, k2, z);
}

// Fs3 (:147-180): c1, c3 guarded on squared lengths < 1e-8; c4 unguarded
__device__ __forceinline__ double pt_fs3(V3 k1, V3 k2, V3 k3) {
#pragma clang fp contract(off)
  const V3 k12 = k1 + k2, k23 = k2 + k3, k123 = k1 + k2 + k3;
  const double k1a = dot3(k1, k1);
  const double k2a = dot3(k2, k2);
  const double k3a = dot3(k3, k3);
  const double k12a = dot3(k12, k12);
  const double k23a = dot3(k23, k23);
  const double k123a = dot3(k123, k123);
  const double b1 = ((1. / 21.) * dot3(k1, k2)) * k12a + ((1. / 14.) * k2a) * dot3(k1, k12);
  const double b2 = (7. * k3a) * dot3(k12, k123) + dot3(k3, k12) * k123a;
  const double b3 = ((1. / 21.) * dot3(k2, k3)) * k23a + ((1. / 14.) * k3a) * dot3(k2, k23);
  const double b4 = dot3(k2, k3) * k23a + (5. * k3a) * dot3(k2, k23);
  double c1, c3;
  if (k12a < 1.0e-8) c1 = 0.0;
  else c1 = 1. / ((((3. * k1a) * k2a) * k3a) * k12a);
  if (k23a < 1.0e-8) c3 = 0.0;
  else c3 = (dot3(k1, k23) * k123a) / ((((3. * k1a) * k2a) * k3a) * k23a);
  const double c4 = dot3(k1, k123) / (((18. * k1a) * k2a) * k3a);
  return ((c1 * b1) * b2 + c3 * b3) + c4 * b4;
}

// Fs3_parallelogram (:182-199): Fs3(k1, -k1, k2) from lengths and the cosine
__device__ __forceinline__ double pt_fs3_par(double k1, double k2, double mu) {
#pragma clang fp contract(off)
  const double x = k2 / k1;
  const double y = x * mu - 1.0;
  const double z = (1.0 + x * x) - (2.0 * x) * mu;
  const double term1 = (((1. / 21.) * x) * y) * ((mu / 3.) + ((0.5 * x) * y) / z);
  const double term2 = (-(mu / 18.)) * (mu * z + (5 * x) * y);
  return term1 + term2;
}

// F3 (:201-223), BCGS eq. 73 with nu2 = 34/21, nu3 = 682/189, lambda3 = 9/10
__device__ __forceinline__ double pt_f3(V3 k1, V3 k2, V3 k3) {
#pragma clang fp contract(off)
  const double nu2 = 34. / 21.;
  const double nu3 = 682. / 189.;
  const double lambda3 = 9. / 10.;
  const V3 k12 = k1 + k2;
  const double g312 = pt_gamma(k3, k12);
  const double g12 = pt_gamma(k1, k2);
  const double R11 = ((0.5 * pt_alpha(k3, k12) + 0.5 * pt_alpha(k12, k3)) - (1. / 3.) * g312) *
                     pt_alpha(k1, k2);
  const double R12 = ((-1.5 * pt_alpha(k12, k3) - (4. / 3.) * pt_alpha(k3, k12)) + 2.5 * g312) * g12;
  const double R2 = (0.75 * ((pt_alpha(k3, k12) + pt_alpha(k12, k3)) - 3. * g312)) * g12;
  const double R3 = ((3. / 8.) * g312) * g12;
  const double R4 = ((2. / 3.) * g312) * pt_alpha(k1, k2) -
                    ((1. / 3.) * pt_alpha(k3, k12) + 0.5 * g312) * g12;
  return (((R11 + R12) + nu2 * R2) + nu3 * R3) + lambda3 * R4;
}

// Fs3_BCGS (:225-229) with the default F3
__device__ __forceinline__ double pt_fs3_bcgs(V3 k1, V3 k2, V3 k3) {
#pragma clang fp contract(off)
  return (((((pt_f3(k1, k2, k3) + pt_f3(k3, k1, k2)) + pt_f3(k2, k3, k1)) + pt_f3(k2, k1, k3)) +
           pt_f3(k3, k2, k1)) + pt_f3(k1, k3, k2)) / 6.;
}

template <bool BAO>
__device__ __forceinline__ double pt_plin(const Epoch& E, double k) {
  return linear_power_t<BAO>(E, k);
}
template <bool BAO>
__device__ __forceinline__ double pt_plin_vec(const Epoch& E, V3 k) {
  return linear_power_t<BAO>(E, sqrt(dot3(k, k)));
}

// bispectrum (:231-249)
template <bool BAO>
__device__ __forceinline__ double pt_bispectrum(const Epoch& E, V3 k1, V3 k2, V3 k3) {
#pragma clang fp contract(off)
  const double p1 = pt_plin_vec<BAO>(E, k1);
  const double p2 = pt_plin_vec<BAO>(E, k2);
  const double p3 = pt_plin_vec<BAO>(E, k3);
  return 2. * (((pt_fs2(k1, k2) * p1) * p2 + (pt_fs2(k1, k3) * p1) * p3) +
               (pt_fs2(k2, k3) * p2) * p3);
}

// bispectrum_len (:251-259)
template <bool BAO>
__device__ __forceinline__ double pt_bispectrum_len(const Epoch& E, const double* a) {
#pragma clang fp contract(off)
  const double k1 = a[0], k2 = a[1], k3 = a[2];
  const double p1 = pt_plin<BAO>(E, k1);
  const double p2 = pt_plin<BAO>(E, k2);
  const double p3 = pt_plin<BAO>(E, k3);
  return 2. * (((pt_fs2_len(k1, k2, a[3]) * p1) * p2 + (pt_fs2_len(k1, k3, a[4]) * p1) * p3) +
               (pt_fs2_len(k2, k3, a[5]) * p2) * p3);
}

// One term Fs2(a, -b) Fs2(a, c) pX pY pZ of the trispectrum's b1 sum
__device__ __forceinline__ double pt_t1(V3 a, V3 b, V3 c, double px, double py, double pz) {
#pragma clang fp contract(off)
  return (((pt_fs2(a, -b) * pt_fs2(a, c)) * px) * py) * pz;
}

// trispectrum (:261-310): NaN zeroed for p12 and p34 only; k1 + k2 = 0 gives P_lin = 1e-16
template <bool BAO>
__device__ __forceinline__ double pt_trispectrum(const Epoch& E, V3 k1, V3 k2, V3 k3, V3 k4) {
#pragma clang fp contract(off)
  const double p1 = pt_plin_vec<BAO>(E, k1);
  const double p2 = pt_plin_vec<BAO>(E, k2);
  const double p3 = pt_plin_vec<BAO>(E, k3);
  const double p4 = pt_plin_vec<BAO>(E, k4);
  double p12 = pt_plin_vec<BAO>(E, k1 + k2);
  const double p13 = pt_plin_vec<BAO>(E, k1 + k3);
  const double p14 = pt_plin_vec<BAO>(E, k1 + k4);
  const double p23 = pt_plin_vec<BAO>(E, k2 + k3);
  const double p24 = pt_plin_vec<BAO>(E, k2 + k4);
  double p34 = pt_plin_vec<BAO>(E, k3 + k4);
  if (isnan(p12)) p12 = 0.0;
  if (isnan(p34)) p34 = 0.0;
  double b1 = pt_t1(k1 + k2, k1, k3, p1, p12, p3);
  b1 = b1 + pt_t1(k2 + k3, k2, k1, p2, p23, p1);
  b1 = b1 + pt_t1(k3 + k1, k3, k2, p3, p13, p2);
  b1 = b1 + pt_t1(k1 + k2, k1, k4, p1, p12, p4);
  b1 = b1 + pt_t1(k2 + k4, k2, k1, p2, p24, p1);
  b1 = b1 + pt_t1(k4 + k1, k4, k2, p4, p14, p2);
  b1 = b1 + pt_t1(k1 + k3, k1, k4, p1, p13, p4);
  b1 = b1 + pt_t1(k3 + k4, k3, k1, p3, p34, p1);
  b1 = b1 + pt_t1(k4 + k1, k4, k3, p4, p14, p3);
  b1 = b1 + pt_t1(k2 + k3, k2, k4, p2, p23, p4);
  b1 = b1 + pt_t1(k3 + k4, k3, k2, p3, p34, p2);
  b1 = b1 + pt_t1(k4 + k2, k4, k3, p4, p24, p3);
  double b2 = ((pt_fs3(k1, k2, k3) * p1) * p2) * p3;
  b2 = b2 + ((pt_fs3(k1, k2, k4) * p1) * p2) * p4;
  b2 = b2 + ((pt_fs3(k1, k3, k4) * p1) * p3) * p4;
  b2 = b2 + ((pt_fs3(k2, k3, k4) * p2) * p3) * p4;
  return 4. * b1 + 6. * b2;
}

// trispectrum_parallelogram (:312-345)
template <bool BAO>
__device__ __forceinline__ double pt_trispectrum_par(const Epoch& E, double k1, double k2, double mu) {
#pragma clang fp contract(off)
  const double x = k2 / k1;
  const double z = (1 + x * x) - (2 * x) * mu;
  const double p1 = pt_plin<BAO>(E, k1);
  const double p2 = pt_plin<BAO>(E, k2);
  const double p12 = pt_plin<BAO>(E, k1 * sqrt(z));
  const double F21 = pt_fs2_kdiff(k1, k2, mu);
  const double F22 = pt_fs2_kdiff(k2, k1, mu);
  const double a1 = ((12. * pt_fs3_par(k1, k2, mu)) * (p1 * p1)) * p2;
  const double a2 = ((8. * (F21 * F21)) * p12) * (p2 * p2);
  const double a3 = ((((16. * F21) * F22) * p1) * p2) * p12;
  const double b1 = ((12. * pt_fs3_par(k2, k1, mu)) * (p2 * p2)) * p1;
  const double b2 = ((8. * (F22 * F22)) * p12) * (p1 * p1);
  return (((a1 + b1) + a2) + b2) + 2. * a3;
}

template <bool BAO, int FORM>
__device__ __forceinline__ double pt_form(const Epoch& E, const double* a) {
  if constexpr (FORM == PT_FS2) return pt_fs2(v3(a), v3(a + 3));
  else if constexpr (FORM == PT_FS2_LEN) return pt_fs2_len(a[0], a[1], a[2]);
  else if constexpr (FORM == PT_FS2_KDIFF) return pt_fs2_kdiff(a[0], a[1], a[2]);
  else if constexpr (FORM == PT_FS3) return pt_fs3(v3(a), v3(a + 3), v3(a + 6));
  else if constexpr (FORM == PT_FS3_PARALLELOGRAM) return pt_fs3_par(a[0], a[1], a[2]);
  else if constexpr (FORM == PT_F3) return pt_f3(v3(a), v3(a + 3), v3(a + 6));
  else if constexpr (FORM == PT_FS3_BCGS) return pt_fs3_bcgs(v3(a), v3(a + 3), v3(a + 6));
  else if constexpr (FORM == PT_BISPECTRUM) return pt_bispectrum<BAO>(E, v3(a), v3(a + 3), v3(a + 6));
  else if constexpr (FORM == PT_BISPECTRUM_LEN) return pt_bispectrum_len<BAO>(E, a);
  else if constexpr (FORM == PT_TRISPECTRUM)
    return pt_trispectrum<BAO>(E, v3(a), v3(a + 3), v3(a + 6), v3(a + 9));
  else return pt_trispectrum_par<BAO>(E, a[0], a[1], a[2]);
}

// ---------------------------------------------------------------------------
// k_pt: out[(e - epoch0) n + i] = FORM(args[i]; epoch e).  grid (gx, n_epoch), block 256.
// A lane owns one configuration per step of the grid-stride loop and reads its arity's doubles
// (contiguous across the wavefront: 48-96 B per lane, whole cache lines); the epoch record is
// staged in LDS once per block, and only by the forms with a P_lin in them.
// ---------------------------------------------------------------------------
constexpr int kPtThreads = 256;
template <bool BAO, int FORM>
__global__ __launch_bounds__(kPtThreads) void k_pt(const Epoch* __restrict__ epochs, int epoch0,
                                                   const double* __restrict__ args, size_t n,
                                                   double* __restrict__ out) {
  constexpr int NA = pt_arity(FORM);
  __shared__ Epoch E;
  if constexpr (pt_needs_power(FORM)) {
    copy_doubles(reinterpret_cast<double*>(&E),
                 reinterpret_cast<const double*>(&epochs[epoch0 + (int)blockIdx.y]), kEpochDoubles);
    __syncthreads();
  }
  double* o = out + (size_t)blockIdx.y * n;
  const size_t step = (size_t)gridDim.x * kPtThreads;
  for (size_t i = (size_t)blockIdx.x * kPtThreads + threadIdx.x; i < n; i += step) {
    double a[NA];
    const double* p = args + i * NA;
#pragma unroll
    for (int j = 0; j < NA; ++j) a[j] = p[j];
    o[i] = pt_form<BAO, FORM>(E, a);
  }
}

// ---------------------------------------------------------------------------
// MassFunctionSecondOrder (mass_function.py:365-434).  Per epoch, beside the table block: the
// sigma(M) knots (k_nu_table<.., true> writes them from the integrals that give nu), the pp
// coefficients of sigma(nu) over the nu knots, then bias_2_norm, its Romberg level and a
// converged flag.
// ---------------------------------------------------------------------------
struct B2Layout {
  int NM, off_sigma, off_pp, off_sc, stride;
};
inline B2Layout make_b2_layout(int NM) {
  B2Layout B;
  B.NM = NM;
  B.off_sigma = 0;
  B.off_pp = NM;
  B.off_sc = NM + 4 * (NM - 1);
  B.stride = (B.off_sc + 4 + 7) & ~7;
  return B;
}

// bias_2_nu (mass_function.py:423-429), sigma from the sigma(nu) spline
__device__ __forceinline__ double bias_2_nu(const Epoch& E, double b2norm, double sigma, double nu) {
#pragma clang fp contract(off)
  const double nu_prime = nu * E.st_a;
  return b2norm + (((8.0 / 21.0) * (bias_nu(E, nu) - 1.0) + (nu - 3.0) / (sigma * sigma)) +
                   (2.0 * E.stq / ((E.delta_c * E.delta_c) * (1.0 + pow(nu_prime, E.stq)))) *
                       ((2.0 * E.stq + 2 * nu_prime) - 1.0));
}

struct FnuBias2Lin {   // mass_function.py:408-414: f(nu) b2(nu) with bias_2_norm = 0
  const Epoch* e;
  const double *x, *c;
  int n;
  __device__ __forceinline__ double operator()(double nu) const {
#pragma clang fp contract(off)
    return f_nu(*e, nu) * bias_2_nu(*e, 0.0, spline_eval(x, c, n, nu), nu);
  }
};

constexpr int kB2NW = 4;
// grid n_epoch, block 64 kB2NW; dynamic LDS b2_lds_doubles(NM)
__host__ __device__ inline int b2_lds_doubles(int NM) {
  return 2 * NM + 4 * (NM - 1) + 9 * NM + romberg_scratch<kB2NW, 1>();
}
__global__ __launch_bounds__(64 * kB2NW) void k_mass_b2(chomp_config cfg, TabLayout L, B2Layout B,
                                                        const Epoch* __restrict__ epochs,
                                                        const double* __restrict__ tab,
                                                        double* __restrict__ b2,
                                                        unsigned* __restrict__ status) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  const int e = (int)blockIdx.x, NM = L.NM;
  double* xs = sm;
  double* ys = xs + NM;
  double* cs = ys + NM;
  double* work = cs + 4 * (NM - 1);
  double* red = work + 9 * NM;
  double* b = b2 + (size_t)e * B.stride;
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(xs, tab + (size_t)e * L.stride + L.off_nu, NM);
  copy_doubles(ys, b + B.off_sigma, NM);
  __syncthreads();
  // _sigma_spline = InterpolatedUnivariateSpline(_nu_array, _sigma_array) (:391-392)
  spline_build_pcr(xs, ys, NM, cs, work, (int)threadIdx.x, 64, threadIdx.x < 64);
  __syncthreads();
  FnuBias2Lin f{&E, xs, cs, NM};
  Scalar1<FnuBias2Lin> w{f};
  const RombergOut<1> r = romberg_group<kB2NW, 1>(w, E.nu_min, E.nu_max, cfg.global_precision,
                                                  cfg.mass_precision, cfg.divmax, red);
  copy_doubles(b + B.off_pp, cs, 4 * (NM - 1));
  if (threadIdx.x == 0) {
    const bool conv = r.converged[0];
    b[B.off_sc + 0] = -r.value[0];
    b[B.off_sc + 1] = (double)r.level[0];
    b[B.off_sc + 2] = conv ? 1.0 : 0.0;
    b[B.off_sc + 3] = 0.0;
    if (!conv) atomicOr(&status[e], CHOMP_ST_B2_DIVMAX);   // scipy: AccuracyWarning
  }
}

// CHOMP_EV_BIAS_2_NU / CHOMP_EV_SIGMA_OF_NU of epoch e
__global__ void k_eval_b2(TabLayout L, B2Layout B, const Epoch* __restrict__ epochs, int e,
                          const double* __restrict__ tab, const double* __restrict__ b2, int what,
                          const double* __restrict__ x, int n, double* __restrict__ out) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  const int NM = L.NM;
  double* xs = sm;
  double* cs = xs + NM;
  const double* b = b2 + (size_t)e * B.stride;
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(xs, tab + (size_t)e * L.stride + L.off_nu, NM);
  copy_doubles(cs, b + B.off_pp, 4 * (NM - 1));
  __syncthreads();
  const double b2norm = b[B.off_sc];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double v = x[i];
    const double sigma = spline_eval(xs, cs, NM, v);
    out[i] = what == CHOMP_EV_SIGMA_OF_NU ? sigma : bias_2_nu(E, b2norm, sigma, v);
  }
}

}  // namespace chomp
