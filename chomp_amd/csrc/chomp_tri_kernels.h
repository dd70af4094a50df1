// chomp_tri_kernels.h -- the one-halo trispectrum (gfx950): halo_trispectrum.HaloTrispectrumOneHalo,
// halo_trispectrum.py:13-151.
//
//   k_tri1h_table    _initialize_i_0_4: the N (N + 1) / 2 distinct I_0^4(k_i, k_i, k_j, k_j) of the
//                    N x N table of each epoch, for an epoch range in one launch, with their
//                    Romberg levels
//   k_tri1h_bicubic  RectBivariateSpline(kx = ky = 3, s = 0) of each epoch's table (bicubic_build)
//   k_tri1h_eval     the spline at (ln k1, ln k2) points, FITPACK's clamp to the knot range
//   k_tri1h_quad     i_0_4(k1, k2, k3, k4) at arbitrary quadruples, one Romberg each
//
// I_0^4 = int_{ln nu_min}^{ln nu_max} nu f(nu) y(k1, M) y(k2, M) y(k3, M) y(k4, M) M^3 n(M) dln nu
// / rho_bar^3 (halo_trispectrum.py:60-95, 133-151), on the raw integrand: the reference computes a
// norm and never passes it, so Romberg's stopping rule sees the unnormalised values.  n(M) is the
// moment of the epoch's HOD that power_spec selects (CHOMP_TRI_*), the 3rd and 4th through the
// product formula of hod.py:68-92.
#pragma once

#include <hip/hip_runtime.h>

#include "chomp_cov_kernels.h"
#include "chomp_pt_kernels.h"

namespace chomp {

constexpr unsigned kStTri1hDivmax = CHOMP_ST_TRI1H_DIVMAX;
constexpr int kTriThreads = 256;   // block of the table kernel: one pair per thread
constexpr int kTriTile = 32;       // Romberg nodes per LDS tile of the table kernel
constexpr int kTriQuadWaves = 4;   // quadruples per block of k_tri1h_quad (one per wavefront)

// Device block of one epoch's table: ln k knots | table | levels | bicubic | scratch of the
// bicubic build | per-block divmax flags of the table launch.
struct TriLayout {
  int N, NP, nchunk, kx, tab, lev, bic, rowt, work, flag, total;
};
inline TriLayout make_tri_layout(int N) {
  TriLayout T;
  T.N = N;
  T.NP = N * (N + 1) / 2;
  T.nchunk = (T.NP + kTriThreads - 1) / kTriThreads;
  int o = 0;
  T.kx = o; o += N;
  T.tab = o; o += N * N;
  T.lev = o; o += N * N;
  T.bic = o; o += 16 * (N - 1) * (N - 1);
  T.rowt = o; o += 4 * (N - 1) * N;
  T.work = o; o += 4 * (N - 1) * (6 * N);
  T.flag = o; o += T.nchunk;
  T.total = (o + 7) & ~7;
  return T;
}
// dynamic LDS of the table kernel, in doubles: nu knots and ln M(nu) pieces, ln k knots, the
// node tile (weights, ln M, y^2 per knot) and the trapezoid estimates T_m of every pair
inline int tri_table_lds_doubles(int NM, int N) {
  return NM + 4 * (NM - 1) + N + kTriTile * (2 + N) + (kMaxDivmax + 1) * kTriThreads;
}
inline int tri_quad_lds_doubles(int NM) { return NM + 4 * (NM - 1); }

// n(M) of halo_trispectrum.py:142-151 (_expected_moment) for the epoch's HOD: 1, <N>,
// <N(N-1)>, and nth_moment(n = 3, 4) (hod.py:68-92): <N>^n prod_{j<n} (j a - j + 1) with
// a = <N(N-1)> / <N>^2, 0 where <N> = 0.
__device__ __forceinline__ double tri_moment(const Epoch& E, double mass, double lnm, int code) {
  if (code == CHOMP_TRI_MMMM) return 1.0;
  double n1, n2;
  hod_node(E, mass, lnm, &n1, &n2);
  if (code == CHOMP_TRI_GMMM) return n1;
  if (code == CHOMP_TRI_GGMM) return n2;
  const int n = code == CHOMP_TRI_GGGM ? 3 : 4;
  double r = n == 3 ? n1 * n1 * n1 : n1 * n1 * n1 * n1;
  const double am2 = n1 != 0.0 ? n2 / (n1 * n1) : 0.0;
  for (int j = 0; j < n; ++j) r *= (double)j * am2 - (double)j + 1.0;
  return r;
}

// The k-independent factor of the integrand at x = ln nu, nu f(nu) M^3 n(M), and ln M.
__device__ __forceinline__ double tri_weight(const Epoch& E, const double* nu_knots,
                                             const double* lnm_pp, int NM, int code, double x,
                                             double* lnm_out) {
  const double nu = exp(x);
  const double lnm = spline_eval(nu_knots, lnm_pp, NM, nu);
  const double mass = exp(lnm);
  double nf, b;
  mf_node(E, nu, x, false, &nf, &b);
  *lnm_out = lnm;
  return nf * mass * mass * mass * tri_moment(E, mass, lnm, code);
}

// grid (T.nchunk, n_epoch), block kTriThreads; LDS tri_table_lds_doubles.  Block (c, e): pairs
// p = 256 c + t of epoch epoch0 + e, p -> (i, j), i <= j, row i of the upper triangle holding
// N - i of them.  Every pair of an epoch integrates over the same [ln nu_min, ln nu_max] and so
// on the same Romberg nodes: each level's new nodes are evaluated once per block -- the weight
// A = nu f M^3 n and y^2 at the knots some unfinished pair of the block still needs, a tile of
// kTriTile nodes at a time in LDS -- and each pair sums A y_i^2 y_j^2 over them.  The Richardson
// rows and the reference's stopping test (tol, rtol, divmax) run per pair on those sums: row i
// is sum_m CHOMP_ROMBERG_C[i][m] T_m, as in romberg_group, with the pair's T_m in LDS.  A pair
// stops at its own level; the block ends when all of its pairs have.
__global__ __launch_bounds__(kTriThreads) void k_tri1h_table(chomp_config cfg, TabLayout L,
                                                             TriLayout T,
                                                             const Epoch* __restrict__ epochs,
                                                             int epoch0,
                                                             const double* __restrict__ tab,
                                                             const SiCiTab* __restrict__ sici_g,
                                                             int code, double* __restrict__ tri) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ SiCiTab S;
  __shared__ int need[64];
  __shared__ int klist[64];
  __shared__ int nneed;
  const int e = epoch0 + (int)blockIdx.y;
  const int N = T.N, NM = L.NM, t = threadIdx.x;
  const double* et = tab + (size_t)e * L.stride;
  double* nu_knots = sm;
  double* lnm_pp = nu_knots + NM;
  double* lnk = lnm_pp + 4 * (NM - 1);
  double* tw = lnk + N;                         // [kTriTile] weights
  double* tl = tw + kTriTile;                   // [kTriTile] ln M
  double* ty = tl + kTriTile;                   // [kTriTile][N] y^2
  double* th = ty + kTriTile * N;               // [kMaxDivmax + 1][kTriThreads] T_m
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&S), reinterpret_cast<const double*>(sici_g),
               (int)(sizeof(SiCiTab) / sizeof(double)));
  copy_doubles(nu_knots, et + L.off_nu, NM);
  copy_doubles(lnm_pp, et + L.off_lnm_pp, 4 * (NM - 1));
  const double ln_k_min = log(cfg.k_min), ln_k_max = log(cfg.k_max);
  double* out = tri + (size_t)e * T.total;
  for (int i = t; i < N; i += blockDim.x) {
    const double x = linspace_at(ln_k_min, ln_k_max, N, i);
    lnk[i] = log(exp(x));                       // (y(numpy.log(k)) of k = exp(_ln_k_array[i]))
    if (blockIdx.x == 0) out[T.kx + i] = x;
  }
  __syncthreads();
  const int p = (int)blockIdx.x * kTriThreads + t;
  const bool live = p < T.NP;
  int pi = 0, pj = 0;
  if (live) {
    int b = p;
    while (b >= N - pi) { b -= N - pi; ++pi; }
    pj = pi + b;
  }
  const double a = log(E.nu_min), bnd = log(E.nu_max), range = bnd - a;
  const double tol = cfg.global_precision, rtol = cfg.halo_precision;
  const int divmax = cfg.divmax;

  // the k knots the unfinished pairs of the block need, as a list (all threads call)
  auto gather_need = [&](bool mine) {
    if (t < N) need[t] = 0;
    __syncthreads();
    if (mine) { need[pi] = 1; need[pj] = 1; }
    __syncthreads();
    if (t == 0) {
      int c = 0;
      for (int i = 0; i < N; ++i)
        if (need[i]) klist[c++] = i;
      nneed = c;
    }
    __syncthreads();
  };
  // y^2 at the listed knots and the weights of nt nodes x_j = x0 + h j (all threads call)
  auto eval_tile = [&](int nt, double x0, double h, long j0, bool ends) {
    __syncthreads();                            // (the previous tile has been consumed)
    if (t < nt) {
      const double x = ends ? (t == 0 ? a : bnd) : x0 + h * (double)(j0 + t);
      tw[t] = tri_weight(E, nu_knots, lnm_pp, NM, code, x, &tl[t]);
    }
    __syncthreads();
    const int nk = nneed;
    for (int q = t; q < nt * nk; q += blockDim.x) {
      const int n = q / nk, k = klist[q - n * nk];
      const double y = y_nfw(E, S, lnk[k], tl[n]);
      ty[n * N + k] = y * y;
    }
    __syncthreads();
  };

  // level 0: the end points (halo_trispectrum.py:89-95 through scipy's _difftrap)
  gather_need(live);
  eval_tile(2, 0.0, 0.0, 0, true);
  double ordsum = 0.0, prev = 0.0, cur = 0.0;
  int level = 0;
  bool done = !live;
  if (live) {
    const double fa = tw[0] * ty[pi] * ty[pj];
    const double fb = tw[1] * ty[N + pi] * ty[N + pj];
    ordsum = 0.5 * (fa + fb);
    cur = range * ordsum;
    prev = cur;
    th[t] = cur;
  }
  for (int i = 1; i <= divmax; ++i) {
    if (!__syncthreads_or(!done)) break;
    gather_need(!done);
    const long numtosum = 1L << (i - 1);
    const double h = ldexp(range, 1 - i);
    const double lox = a + 0.5 * h;
    double part = 0.0;
    for (long j0 = 0; j0 < numtosum; j0 += kTriTile) {
      const int nt = (int)(numtosum - j0 < kTriTile ? numtosum - j0 : kTriTile);
      eval_tile(nt, lox, h, j0, false);
      if (!done)
        for (int n = 0; n < nt; ++n) part += tw[n] * ty[n * N + pi] * ty[n * N + pj];
    }
    if (!done) {
      ordsum += part;
      th[i * kTriThreads + t] = ldexp(range * ordsum, -i);
      double r = 0.0;
      for (int m = 0; m <= i; ++m) r += CHOMP_ROMBERG_C[i][m] * th[m * kTriThreads + t];
      cur = r;
      const double err = fabs(cur - prev);
      prev = cur;
      level = i;
      if (err < tol || err < rtol * fabs(cur)) done = true;
    }
  }
  const bool exhausted = live && !done;
  if (live) {
    const double rb = E.rho_bar;
    const double v = cur / (rb * rb * rb);
    out[T.tab + pi * N + pj] = v;
    out[T.tab + pj * N + pi] = v;
    out[T.lev + pi * N + pj] = (double)level;
    out[T.lev + pj * N + pi] = (double)level;
  }
  const int any = __syncthreads_or(exhausted);
  if (t == 0) out[T.flag + blockIdx.x] = any ? 1.0 : 0.0;
}

// grid n_epoch, block 256: the bicubic of each epoch's table, and the epoch's status bit from
// the table launch's flags (set or cleared: the word says what the last table build did).
__global__ __launch_bounds__(256) void k_tri1h_bicubic(TriLayout T, int epoch0,
                                                       double* __restrict__ tri,
                                                       unsigned* __restrict__ status) {
  const int e = epoch0 + (int)blockIdx.x;
  double* st = tri + (size_t)e * T.total;
  bicubic_build(T.N, st + T.kx, st + T.tab, st + T.rowt, st + T.work, st + T.bic);
  if (threadIdx.x == 0) {
    bool any = false;
    for (int c = 0; c < T.nchunk; ++c) any = any || st[T.flag + c] != 0.0;
    if (any) atomicOr(&status[e], kStTri1hDivmax);
    else atomicAnd(&status[e], ~kStTri1hDivmax);
  }
}

// i_0_4_parallelogram's spline (halo_trispectrum.py:97-102, 125-127) at (ln k1, ln k2): FITPACK's
// bispev clamps each argument into [x_0, x_{N-1}].  The k_min clamp and the k_max mask of the
// reference are the caller's (they decide the grid's shape on the host).
__global__ void k_tri1h_eval(TriLayout T, const double* __restrict__ tri, int e,
                             const double* __restrict__ a, const double* __restrict__ b, int n,
                             double* __restrict__ out) {
  const double* st = tri + (size_t)e * T.total;
  Bicubic K;
  K.x = st + T.kx;
  K.bic = st + T.bic;
  K.N = T.N;
  K.lo = K.x[0];
  K.hi = K.x[T.N - 1];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double u = a[i], v = b[i];
    if (isnan(u) || isnan(v)) { out[i] = NAN; continue; }
    u = u < K.lo ? K.lo : (u > K.hi ? K.hi : u);
    v = v < K.lo ? K.lo : (v > K.hi ? K.hi : v);
    out[i] = K.poly(u, v);
  }
}

// The integrand of i_0_4 (halo_trispectrum.py:133-140) at one quadruple, in the reference's order
// of multiplication; y is evaluated once per distinct k.  ARITY 3: HaloTrispectrum.i_1_3
// (:690-705, 737-745) at a triple, nu f b y1 y2 y3 M^2; a compile-time choice, so that the ARITY 4
// instance is the I_0^4 code as it always was.
template <int ARITY>
struct Tri1hQuadIntegrand {
  const Epoch* E;
  const SiCiTab* S;
  const double *nu_knots, *lnm_pp;
  int NM, code;
  double lk[ARITY];
  int src[ARITY];                  // src[i]: the first index with the same k
  __device__ __forceinline__ double operator()(double x) const {
    const double nu = exp(x);
    const double lnm = spline_eval(nu_knots, lnm_pp, NM, nu);
    const double mass = exp(lnm);
    double nf, b;
    mf_node(*E, nu, x, ARITY == 3, &nf, &b);
    double y[ARITY];
#pragma unroll
    for (int i = 0; i < ARITY; ++i) y[i] = src[i] == i ? y_nfw(*E, *S, lk[i], lnm) : y[src[i]];
    if constexpr (ARITY == 3) return nf * b * y[0] * y[1] * y[2] * mass * mass;
    else
      return nf * y[0] * y[1] * y[2] * y[3] * mass * mass * mass * tri_moment(*E, mass, lnm, code);
  }
};

// grid ceil(n / kTriQuadWaves), block 64 kTriQuadWaves; LDS tri_quad_lds_doubles.  One wavefront
// per quadruple k[q][0..3] of epoch e: i_0_4 with the reference's Romberg (romberg_group), its
// value / rho_bar^3 to out[q] and its level to levels[q] (optional).  ARITY 3: k[q][0..2] and
// i_1_3, / rho_bar^2.  An exhausted divmax raises `bit`.
template <int ARITY>
__global__ __launch_bounds__(64 * kTriQuadWaves) void k_tri1h_quad(
    chomp_config cfg, TabLayout L, const Epoch* __restrict__ epochs, int e,
    const double* __restrict__ tab, const SiCiTab* __restrict__ sici_g, int code,
    const double* __restrict__ k, long n, double* __restrict__ out, double* __restrict__ levels,
    unsigned* __restrict__ status, unsigned bit) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ SiCiTab S;
  const int NM = L.NM;
  const double* et = tab + (size_t)e * L.stride;
  double* nu_knots = sm;
  double* lnm_pp = nu_knots + NM;
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&S), reinterpret_cast<const double*>(sici_g),
               (int)(sizeof(SiCiTab) / sizeof(double)));
  copy_doubles(nu_knots, et + L.off_nu, NM);
  copy_doubles(lnm_pp, et + L.off_lnm_pp, 4 * (NM - 1));
  __syncthreads();
  const long q = (long)blockIdx.x * kTriQuadWaves + (threadIdx.x >> 6);
  if (q >= n) return;                           // (wave-uniform; no barrier follows)
  Tri1hQuadIntegrand<ARITY> f;
  f.E = &E; f.S = &S; f.nu_knots = nu_knots; f.lnm_pp = lnm_pp; f.NM = NM; f.code = code;
  double kv[ARITY];
#pragma unroll
  for (int i = 0; i < ARITY; ++i) {
    kv[i] = k[q * ARITY + i];
    f.lk[i] = log(kv[i]);
    f.src[i] = i;
    for (int m = i - 1; m >= 0; --m)
      if (kv[m] == kv[i]) f.src[i] = m;
  }
  double red[1];
  Scalar1<Tri1hQuadIntegrand<ARITY>> w{f};
  const RombergOut<1> r = romberg_group<1, 1>(w, log(E.nu_min), log(E.nu_max),
                                              cfg.global_precision, cfg.halo_precision,
                                              cfg.divmax, red);
  if ((threadIdx.x & 63) == 0) {
    const double rb = E.rho_bar;
    if constexpr (ARITY == 3) out[q] = r.value[0] / (rb * rb);
    else out[q] = r.value[0] / (rb * rb * rb);
    if (levels) levels[q] = (double)r.level[0];
    if (!r.converged[0]) atomicOr(&status[e], bit);
  }
}

// ===========================================================================================
// HaloTrispectrum (halo_trispectrum.py:153-837): the two- to four-halo terms.
//
//   k_tri_table   _initialize_i_1_2 / _i_1_3 / _i_2_2 / _i_2_1: the mass-integral tables of an
//                 epoch range, the kind on the grid's z axis, with their Romberg levels
//   k_tri_finish  their bicubics (bicubic_build), the not-a-knot spline of _i_2_1 and the
//                 epochs' status bit
//   k_tri_lookup  one table at (k1, k2) points with the reference's clamp and zero rules
//   k_tri_terms   t_1_h .. t_4_h at (k1, k2, z) configurations, one per lane
//   k_tri_proj    tri_spec_proj_integral at (k1, k2) pairs, one wavefront each
//
// The tables (kinds TRI_K*), over the k knots k_i of the halo model:
//   I_1^2[i][j] = int nu f b  y_i y_j M      / rho_bar    (:655-688)
//   I_1^3[i][j] = int nu f b  y_i^2 y_j M^2  / rho_bar^2  (:714-745; i <= j, mirrored as shipped)
//   I_2^2[i][j] = int nu f b2 y_j^2 M        / rho_bar    (:802-836; called with (ln_k2, ln_k2))
//   I_2^1[i]    = int nu f b2 y_i * integrand(ln nu = 0)  (:761-784; Romberg on the raw integrand,
//                 then "/ norm" with norm = 1 / integrand(0))
// The 2-D kinds integrate integrand * norm, norm = 1 / (their integrand at ln nu = 0, for I_2^2 with
// y_i y_j), and divide it out afterwards, as the reference does.  I_0^4 is k_tri1h_table's.
// ===========================================================================================
constexpr unsigned kStTriDivmax = CHOMP_ST_TRI_DIVMAX;
enum { TRI_K12 = 0, TRI_K13 = 1, TRI_K22 = 2, TRI_K21 = 3, TRI_K04 = 4, TRI_K11 = 5 };
constexpr int kTriKinds2d = 3;
constexpr int kTriProjWaves = 4;   // pairs per block of k_tri_proj (one per wavefront)

// Device block of one epoch: a TriLayout block per 2-D kind, then the 1-D table: knots | table |
// levels | pp coefficients | scratch of the spline build | divmax flag.
struct TriTabLayout {
  TriLayout T;
  int N, o1, kx, tab, lev, pp, work, flag, total;
};
inline TriTabLayout make_tri_tab_layout(int N) {
  TriTabLayout Q;
  Q.T = make_tri_layout(N);
  Q.N = N;
  int o = kTriKinds2d * Q.T.total;
  Q.o1 = o;
  Q.kx = o; o += N;
  Q.tab = o; o += N;
  Q.lev = o; o += N;
  Q.pp = o; o += 4 * (N - 1);
  Q.work = o; o += 4 * N;
  Q.flag = o; o += 1;
  Q.total = (o + 7) & ~7;
  return Q;
}
// dynamic LDS of k_tri_table, in doubles (the node tile holds y, not y^2, at the knots)
inline int tri_tab_lds_doubles(int NM, int N) { return tri_table_lds_doubles(NM, N); }

// The k-independent factor of a kind's integrand at x = ln nu, and ln M.  b2pp: the sigma(nu)
// spline of the epoch's second-order mass function (B2Layout), b2norm its bias_2_norm.
__device__ __forceinline__ double tri_tab_weight(const Epoch& E, const double* nu_knots,
                                                 const double* lnm_pp, const double* b2pp,
                                                 double b2norm, int NM, int kind, double x,
                                                 double* lnm_out) {
  const double nu = exp(x);
  const double lnm = spline_eval(nu_knots, lnm_pp, NM, nu);
  const double mass = exp(lnm);
  double nf, b = 0.0;
  mf_node(E, nu, x, kind <= TRI_K13, &nf, &b);
  *lnm_out = lnm;
  if (kind == TRI_K12) return nf * b * mass;
  if (kind == TRI_K13) return nf * b * mass * mass;
  const double b2 = bias_2_nu(E, b2norm, spline_eval(nu_knots, b2pp, NM, nu), nu);
  return kind == TRI_K22 ? nf * b2 * mass : nf * b2;
}
// The profile factor of pair (i, j): of the integrand, and of the norm's integrand.
__device__ __forceinline__ double tri_tab_prod(int kind, double yi, double yj) {
  return kind == TRI_K12 ? yi * yj : kind == TRI_K13 ? yi * yi * yj : kind == TRI_K22 ? yj * yj : yi;
}
__device__ __forceinline__ double tri_tab_norm_prod(int kind, double yi, double yj) {
  return kind == TRI_K22 ? yi * yj : tri_tab_prod(kind, yi, yj);
}

// grid (T.nchunk, n_epoch, 4), block kTriThreads; LDS tri_tab_lds_doubles.  The scheme of
// k_tri1h_table with the kind (blockIdx.z) selecting the weight A(nu) and the powers of y: every
// pair of an epoch shares the Romberg nodes, each level's new nodes are evaluated once per block
// -- A and y at the knots some unfinished pair still needs, kTriTile nodes at a time in LDS --
// and each pair sums A y_i^p y_j^q norm over them, runs the reference's stopping rule on its own
// sums and records its own level.  Level 0 carries a third node, ln nu = 0, for the norms.
// TRI_K21 is the 1-D case: N "pairs" (i, i), chunk 0 only.
__global__ __launch_bounds__(kTriThreads) void k_tri_table(chomp_config cfg, TabLayout L,
                                                           B2Layout B, TriTabLayout Q,
                                                           const Epoch* __restrict__ epochs,
                                                           int epoch0,
                                                           const double* __restrict__ tab,
                                                           const double* __restrict__ b2,
                                                           const SiCiTab* __restrict__ sici_g,
                                                           double* __restrict__ tri) {
  extern __shared__ __align__(16) double sm[];
  __shared__ Epoch E;
  __shared__ SiCiTab S;
  __shared__ int need[64];
  __shared__ int klist[64];
  __shared__ int nneed;
  const int kind = (int)blockIdx.z;
  const TriLayout& T = Q.T;
  const int N = T.N, NM = L.NM, t = threadIdx.x;
  const int NP = kind == TRI_K21 ? N : T.NP;
  if ((int)blockIdx.x * kTriThreads >= NP) return;      // (block-uniform; before any barrier)
  const int e = epoch0 + (int)blockIdx.y;
  const double* et = tab + (size_t)e * L.stride;
  const double* b2e = b2 + (size_t)e * B.stride;
  const double* b2pp = b2e + B.off_pp;
  const double b2norm = b2e[B.off_sc];
  double* nu_knots = sm;
  double* lnm_pp = nu_knots + NM;
  double* lnk = lnm_pp + 4 * (NM - 1);
  double* tw = lnk + N;                         // [kTriTile] weights
  double* tl = tw + kTriTile;                   // [kTriTile] ln M
  double* ty = tl + kTriTile;                   // [kTriTile][N] y
  double* th = ty + kTriTile * N;               // [kMaxDivmax + 1][kTriThreads] T_m
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&S), reinterpret_cast<const double*>(sici_g),
               (int)(sizeof(SiCiTab) / sizeof(double)));
  copy_doubles(nu_knots, et + L.off_nu, NM);
  copy_doubles(lnm_pp, et + L.off_lnm_pp, 4 * (NM - 1));
  const double ln_k_min = log(cfg.k_min), ln_k_max = log(cfg.k_max);
  double* ep = tri + (size_t)e * Q.total;
  double* out = kind == TRI_K21 ? ep : ep + (size_t)kind * T.total;
  const int o_kx = kind == TRI_K21 ? Q.kx : T.kx;
  for (int i = t; i < N; i += blockDim.x) {
    const double x = linspace_at(ln_k_min, ln_k_max, N, i);
    lnk[i] = x;                                 // (the integrands take ln k; i_1_3's log(exp(x)) below)
    if (blockIdx.x == 0) out[o_kx + i] = x;
  }
  __syncthreads();
  if (kind == TRI_K13)
    for (int i = t; i < N; i += blockDim.x) lnk[i] = log(exp(lnk[i]));
  __syncthreads();
  const int p = (int)blockIdx.x * kTriThreads + t;
  const bool live = p < NP;
  int pi = 0, pj = 0;
  if (live) {
    if (kind == TRI_K21) {
      pi = pj = p;
    } else {
      int b = p;
      while (b >= N - pi) { b -= N - pi; ++pi; }
      pj = pi + b;
    }
  }
  const double a = log(E.nu_min), bnd = log(E.nu_max), range = bnd - a;
  const double tol = cfg.global_precision, rtol = cfg.halo_precision;
  const int divmax = cfg.divmax;

  auto gather_need = [&](bool mine) {
    if (t < N) need[t] = 0;
    __syncthreads();
    if (mine) { need[pi] = 1; need[pj] = 1; }
    __syncthreads();
    if (t == 0) {
      int c = 0;
      for (int i = 0; i < N; ++i)
        if (need[i]) klist[c++] = i;
      nneed = c;
    }
    __syncthreads();
  };
  // y at the listed knots and the weights of nt nodes x_j = x0 + h j; ends: a, b and 0
  auto eval_tile = [&](int nt, double x0, double h, long j0, bool ends) {
    __syncthreads();                            // (the previous tile has been consumed)
    if (t < nt) {
      const double x = ends ? (t == 0 ? a : (t == 1 ? bnd : 0.0)) : x0 + h * (double)(j0 + t);
      tw[t] = tri_tab_weight(E, nu_knots, lnm_pp, b2pp, b2norm, NM, kind, x, &tl[t]);
    }
    __syncthreads();
    const int nk = nneed;
    for (int q = t; q < nt * nk; q += blockDim.x) {
      const int n = q / nk, k = klist[q - n * nk];
      ty[n * N + k] = y_nfw(E, S, lnk[k], tl[n]);
    }
    __syncthreads();
  };

  gather_need(live);
  eval_tile(3, 0.0, 0.0, 0, true);
  double ordsum = 0.0, prev = 0.0, cur = 0.0, norm = 1.0, scale = 1.0;
  int level = 0;
  bool done = !live;
  if (live) {
    norm = 1.0 / (tw[2] * tri_tab_norm_prod(kind, ty[2 * N + pi], ty[2 * N + pj]));
    scale = kind == TRI_K21 ? 1.0 : norm;       // (_i_2_1 integrates the raw integrand)
    const double fa = tw[0] * tri_tab_prod(kind, ty[pi], ty[pj]) * scale;
    const double fb = tw[1] * tri_tab_prod(kind, ty[N + pi], ty[N + pj]) * scale;
    ordsum = 0.5 * (fa + fb);
    cur = range * ordsum;
    prev = cur;
    th[t] = cur;
  }
  for (int i = 1; i <= divmax; ++i) {
    if (!__syncthreads_or(!done)) break;
    gather_need(!done);
    const long numtosum = 1L << (i - 1);
    const double h = ldexp(range, 1 - i);
    const double lox = a + 0.5 * h;
    double part = 0.0;
    for (long j0 = 0; j0 < numtosum; j0 += kTriTile) {
      const int nt = (int)(numtosum - j0 < kTriTile ? numtosum - j0 : kTriTile);
      eval_tile(nt, lox, h, j0, false);
      if (!done)
        for (int n = 0; n < nt; ++n)
          part += tw[n] * tri_tab_prod(kind, ty[n * N + pi], ty[n * N + pj]) * scale;
    }
    if (!done) {
      ordsum += part;
      th[i * kTriThreads + t] = ldexp(range * ordsum, -i);
      double r = 0.0;
      for (int m = 0; m <= i; ++m) r += CHOMP_ROMBERG_C[i][m] * th[m * kTriThreads + t];
      cur = r;
      const double err = fabs(cur - prev);
      prev = cur;
      level = i;
      if (err < tol || err < rtol * fabs(cur)) done = true;
    }
  }
  const bool exhausted = live && !done;
  if (live) {
    const double rb = E.rho_bar;
    if (kind == TRI_K21) {
      out[Q.tab + pi] = cur / norm;
      out[Q.lev + pi] = (double)level;
    } else {
      const double v = kind == TRI_K13 ? cur / (rb * rb * norm) : cur / rb / norm;
      out[T.tab + pi * N + pj] = v;
      out[T.tab + pj * N + pi] = v;
      out[T.lev + pi * N + pj] = (double)level;
      out[T.lev + pj * N + pi] = (double)level;
    }
  }
  const int any = __syncthreads_or(exhausted);
  if (t == 0) out[(kind == TRI_K21 ? Q.flag : T.flag) + blockIdx.x] = any ? 1.0 : 0.0;
}

// grid (n_epoch, 4), block 256.  y < 3: the bicubic of 2-D kind y.  y = 3: the not-a-knot spline
// of _i_2_1 (InterpolatedUnivariateSpline, :774-775) and the epoch's status bit from the flags
// of the table launch before this one (set or cleared: the word says what the last build did).
__global__ __launch_bounds__(256) void k_tri_finish(TriTabLayout Q, int epoch0,
                                                    double* __restrict__ tri,
                                                    unsigned* __restrict__ status) {
  const int e = epoch0 + (int)blockIdx.x;
  const TriLayout& T = Q.T;
  double* ep = tri + (size_t)e * Q.total;
  if (blockIdx.y < kTriKinds2d) {
    double* st = ep + (size_t)blockIdx.y * T.total;
    bicubic_build(T.N, st + T.kx, st + T.tab, st + T.rowt, st + T.work, st + T.bic);
    return;
  }
  if (threadIdx.x == 0) {
    spline_build(ep + Q.kx, ep + Q.tab, Q.N, ep + Q.pp, ep + Q.work);
    bool any = ep[Q.flag] != 0.0;
    for (int k = 0; k < kTriKinds2d; ++k)
      for (int c = 0; c < T.nchunk; ++c) any = any || ep[(size_t)k * T.total + T.flag + c] != 0.0;
    if (any) atomicOr(&status[e], kStTriDivmax);
    else atomicAnd(&status[e], ~kStTriDivmax);
  }
}

// The five splines of one epoch with the reference's range rules (:585-590, 649-653, 707-712,
// 757-759, 796-800) and _h_m (halo.py:649-652): k < k_min is clamped to k_min, k > k_max gives 0;
// the bivariate splines clamp ln k into the knot range as FITPACK does, the univariate one
// extrapolates its end pieces.  _h_m is 0 outside [k_min, k_max].
struct TriLook {
  const double *ep, *e1h;          // the epoch's block of the four tables; of k_tri1h_table's I_0^4
  const double *x1, *pp1, *hm_pp;
  int N, kx, bic, stride;
  double k_min, k_max, x0, dx;
  // which: TRI_K12, TRI_K13, TRI_K22, or 3: I_0^4
  __device__ __forceinline__ double two(int which, double k1, double k2) const {
    k1 = k1 < k_min ? k_min : k1;
    k2 = k2 < k_min ? k_min : k2;
    if (!(k1 <= k_max && k2 <= k_max)) return 0.0;
    const double* st = which == 3 ? e1h : ep + (size_t)which * stride;
    Bicubic K;
    K.x = st + kx;
    K.bic = st + bic;
    K.N = N;
    K.lo = K.x[0];
    K.hi = K.x[N - 1];
    double u = log(k1), v = log(k2);
    u = u < K.lo ? K.lo : (u > K.hi ? K.hi : u);
    v = v < K.lo ? K.lo : (v > K.hi ? K.hi : v);
    return K.poly(u, v);
  }
  __device__ __forceinline__ double i_2_1(double k) const {
    k = k < k_min ? k_min : k;
    if (!(k <= k_max)) return 0.0;
    return spline_eval(x1, pp1, N, log(k));
  }
  __device__ __forceinline__ double h_m(double k) const {
    if (!(k >= k_min && k <= k_max)) return 0.0;
    return spline_eval_uniform(x0, dx, hm_pp, N, log(k));
  }
  __device__ __forceinline__ double kind(int kd, double k1, double k2) const {
    if (kd == TRI_K21) return i_2_1(k1);
    if (kd == TRI_K11) return h_m(k1);
    return two(kd == TRI_K04 ? 3 : kd, k1, k2);
  }
};
__device__ __forceinline__ TriLook tri_look(const chomp_config& cfg, const TabLayout& L,
                                            const TriLayout& T, const TriTabLayout& Q,
                                            const double* tab, const double* tri1h,
                                            const double* tri, int e) {
  TriLook K;
  K.ep = tri + (size_t)e * Q.total;
  K.e1h = tri1h + (size_t)e * T.total;
  K.x1 = K.ep + Q.kx;
  K.pp1 = K.ep + Q.pp;
  K.hm_pp = tab + (size_t)e * L.stride + L.off_kpp[F_HM];
  K.N = T.N;
  K.kx = T.kx;
  K.bic = T.bic;
  K.stride = T.total;
  K.k_min = cfg.k_min;
  K.k_max = cfg.k_max;
  K.x0 = log(cfg.k_min);
  K.dx = (log(cfg.k_max) - K.x0) / (double)(T.N - 1);
  return K;
}

__global__ void k_tri_lookup(chomp_config cfg, TabLayout L, TriLayout T, TriTabLayout Q,
                             const double* __restrict__ tab, const double* __restrict__ tri1h,
                             const double* __restrict__ tri, int e, int kind,
                             const double* __restrict__ k1, const double* __restrict__ k2, int n,
                             double* __restrict__ out) {
  const TriLook K = tri_look(cfg, L, T, Q, tab, tri1h, tri, e);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = K.kind(kind, k1[i], k2[i]);
}

// Everything of the terms that depends on k1 and k2 only.
struct TriPair {
  double k1, k2, t1, i12, i13_112, i13_221, i22_11, i22_22, i22_12, i21_1, i21_2, h1, h2, p1, p2;
};
template <bool BAO>
__device__ __forceinline__ TriPair tri_pair(const TriLook& K, const Epoch& E, double k1,
                                            double k2) {
  TriPair P;
  P.k1 = k1; P.k2 = k2;
  P.t1 = K.two(3, k1, k2);
  P.i12 = K.two(TRI_K12, k1, k2);
  P.i13_112 = K.two(TRI_K13, k1, k2);
  P.i13_221 = K.two(TRI_K13, k2, k1);
  P.i22_11 = K.two(TRI_K22, k1, k1);
  P.i22_22 = K.two(TRI_K22, k2, k2);
  P.i22_12 = K.two(TRI_K22, k1, k2);
  P.i21_1 = K.i_2_1(k1);
  P.i21_2 = K.i_2_1(k2);
  P.h1 = K.h_m(k1);
  P.h2 = K.h_m(k2);
  P.p1 = linear_power_t<BAO>(E, k1);
  P.p2 = linear_power_t<BAO>(E, k2);
  return P;
}

// t_2_h, t_3_h, t_4_h (:334-512) at the cosine z, in the reference's order of operations.  E: the
// halo model's epoch (its linear_power); Ep: the PerturbationTheory object's (bispectrum_len,
// trispectrum_parallelogram).  As shipped: perm_4 uses the unguarded bispectrum.
template <bool BAO>
__device__ __forceinline__ void tri_angle(const TriPair& P, const Epoch& E, const Epoch& Ep,
                                          double z, double* t2, double* t3, double* t4) {
#pragma clang fp contract(off)
  const double k1 = P.k1, k2 = P.k2, P1 = P.p1, P2 = P.p2, h1 = P.h1, h2 = P.h2;
  {
    const double T31 = 2.0 * ((P1 * P.i13_221) * h1 + (P2 * P.i13_112) * h2);
    const double k1m2 = sqrt((k1 * k1 + k2 * k2) - ((2.0 * k1) * k2) * z);
    const double k1p2 = sqrt((k1 * k1 + k2 * k2) + ((2.0 * k1) * k2) * z);
    const double T22 = ((2.0 * P.i12) * P.i12) *
                       (linear_power_t<BAO>(E, k1m2) + linear_power_t<BAO>(E, k1p2));
    *t2 = T31 + T22;
  }
  {
    const double lenplus = sqrt((k1 * k1 + ((2.0 * k1) * k2) * z) + k2 * k2);
    const double lenminus = sqrt((k1 * k1 - ((2.0 * k1) * k2) * z) + k2 * k2);
    const double z1plus = lenplus > 0.0 ? (k1 * k1 + (k1 * k2) * z) / (k1 * lenplus) : 0.0;
    const double z2plus = lenplus > 0.0 ? (k2 * k2 + (k1 * k2) * z) / (k2 * lenplus) : 0.0;
    const double z1minus = lenminus > 0.0 ? (k1 * k1 - (k1 * k2) * z) / (k1 * lenminus) : 0.0;
    const double z2minus = lenminus > 0.0 ? (k2 * k2 - (k1 * k2) * z) / (k2 * lenminus) : 0.0;
    const double perm_1 = (((P1 * P1) * P.i22_22) * h1) * h1;
    const double perm_2 = (((P2 * P2) * P.i22_11) * h2) * h2;
    double bp;
    if (lenplus > 1e-8) {
      const double a[6] = {k1, k2, lenplus, z, -z1plus, -z2plus};
      bp = pt_bispectrum_len<BAO>(Ep, a);
    } else {
      bp = 2.0 * ((pt_fs2_len(k1, k2, z) * P1) * P2);
    }
    const double two_h = (((P1 * P2) * P.i22_12) * h1) * h2;
    const double perm_3 = ((bp * P.i12) * h1) * h2 + two_h;
    const double am[6] = {k1, k2, lenminus, -z, -z1minus, -z2minus};
    const double perm_4 = ((pt_bispectrum_len<BAO>(Ep, am) * P.i12) * h1) * h2 + two_h;
    *t3 = (perm_1 + perm_2) + 2.0 * (perm_3 + perm_4);
  }
  *t4 = (((h1 * h1) * h2) * h2) *
        (pt_trispectrum_par<BAO>(Ep, k1, k2, z) +
         2.0 * (((P.i21_1 * P1) * P2) * P2 + ((P.i21_2 * P2) * P1) * P1));
}

// grid gx, block 256: out[4 i + 0..3] = t_1_h .. t_4_h of configuration kkz[3 i + 0..2] =
// (k1, k2, z), one configuration per lane in a grid-stride loop.  e: the halo model's epoch, ep:
// the PerturbationTheory object's.
template <bool BAO>
__global__ __launch_bounds__(256) void k_tri_terms(chomp_config cfg, TabLayout L, TriLayout T,
                                                   TriTabLayout Q,
                                                   const Epoch* __restrict__ epochs, int e, int ep,
                                                   const double* __restrict__ tab,
                                                   const double* __restrict__ tri1h,
                                                   const double* __restrict__ tri,
                                                   const double* __restrict__ kkz, size_t n,
                                                   double* __restrict__ out) {
  __shared__ Epoch E, Ep;
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&Ep), reinterpret_cast<const double*>(&epochs[ep]),
               kEpochDoubles);
  __syncthreads();
  const TriLook K = tri_look(cfg, L, T, Q, tab, tri1h, tri, e);
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const TriPair P = tri_pair<BAO>(K, E, kkz[3 * i], kkz[3 * i + 1]);
    double t2, t3, t4;
    tri_angle<BAO>(P, E, Ep, kkz[3 * i + 2], &t2, &t3, &t4);
    out[4 * i] = P.t1;
    out[4 * i + 1] = t2;
    out[4 * i + 2] = t3;
    out[4 * i + 3] = t4;
  }
}

// _trispectrum_parallelogram_wrap (:315-318): (t_2_h + t_3_h + t_4_h)(cos theta) norm
template <bool BAO>
struct TriProjIntegrand {
  const TriPair* P;
  const Epoch *E, *Ep;
  double norm;
  __device__ __forceinline__ double operator()(double theta) const {
#pragma clang fp contract(off)
    double t2, t3, t4;
    tri_angle<BAO>(*P, *E, *Ep, cos(theta), &t2, &t3, &t4);
    return ((t2 + t3) + t4) * norm;
  }
};

// grid ceil(n / kTriProjWaves), block 64 kTriProjWaves.  One wavefront per pair kk[2 q + 0..1]:
// tri_spec_proj_integral (:267-278), t_1_h + 2 Romberg_0^pi / (norm pi) with norm = 1 / the
// integrand at pi / 2; the k-only factors are looked up once.  A non-finite end point (k1 = k2
// at theta = 0) gives NaN at once -- the value the reference returns after divmax levels --
// with level divmax, flag 1 and the status bit; so does an exhausted divmax.
template <bool BAO>
__global__ __launch_bounds__(64 * kTriProjWaves) void k_tri_proj(
    chomp_config cfg, TabLayout L, TriLayout T, TriTabLayout Q, const Epoch* __restrict__ epochs,
    int e, int ep, const double* __restrict__ tab, const double* __restrict__ tri1h,
    const double* __restrict__ tri, const double* __restrict__ kk, long n,
    double* __restrict__ out, double* __restrict__ levels, double* __restrict__ flags,
    unsigned* __restrict__ status) {
  __shared__ Epoch E, Ep;
  copy_doubles(reinterpret_cast<double*>(&E), reinterpret_cast<const double*>(&epochs[e]),
               kEpochDoubles);
  copy_doubles(reinterpret_cast<double*>(&Ep), reinterpret_cast<const double*>(&epochs[ep]),
               kEpochDoubles);
  __syncthreads();
  const long q = (long)blockIdx.x * kTriProjWaves + (threadIdx.x >> 6);
  if (q >= n) return;                           // (wave-uniform; no barrier follows)
  const TriLook K = tri_look(cfg, L, T, Q, tab, tri1h, tri, e);
  const TriPair P = tri_pair<BAO>(K, E, kk[2 * q], kk[2 * q + 1]);
  TriProjIntegrand<BAO> f{&P, &E, &Ep, 1.0};
  const double norm = 1.0 / f(kPi / 2.0);
  f.norm = norm;
  const double fa = f(0.0), fb = f(kPi);
  double value, level;
  bool bad;
  if (!isfinite(fa) || !isfinite(fb)) {
    value = NAN;
    level = (double)cfg.divmax;
    bad = true;
  } else {
    double red[1];
    Scalar1<TriProjIntegrand<BAO>> w{f};
    const RombergOut<1> r = romberg_group<1, 1>(w, 0.0, kPi, cfg.global_precision,
                                                cfg.halo_precision, cfg.divmax, red);
    value = P.t1 + (2.0 * r.value[0]) / (norm * kPi);
    level = (double)r.level[0];
    bad = !r.converged[0];
  }
  if ((threadIdx.x & 63) == 0) {
    out[q] = value;
    if (levels) levels[q] = level;
    if (flags) flags[q] = bad ? 1.0 : 0.0;
    if (bad) atomicOr(&status[e], kStTriDivmax);
  }
}
}  // namespace chomp
