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
// of multiplication; y is evaluated once per distinct k.
struct Tri1hQuadIntegrand {
  const Epoch* E;
  const SiCiTab* S;
  const double *nu_knots, *lnm_pp;
  int NM, code;
  double lk[4];
  int src[4];                      // src[i]: the first index with the same k
  __device__ __forceinline__ double operator()(double x) const {
    const double nu = exp(x);
    const double lnm = spline_eval(nu_knots, lnm_pp, NM, nu);
    const double mass = exp(lnm);
    double nf, b;
    mf_node(*E, nu, x, false, &nf, &b);
    double y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = src[i] == i ? y_nfw(*E, *S, lk[i], lnm) : y[src[i]];
    return nf * y[0] * y[1] * y[2] * y[3] * mass * mass * mass * tri_moment(*E, mass, lnm, code);
  }
};

// grid ceil(n / kTriQuadWaves), block 64 kTriQuadWaves; LDS tri_quad_lds_doubles.  One wavefront
// per quadruple k[q][0..3] of epoch e: i_0_4 with the reference's Romberg (romberg_group), its
// value / rho_bar^3 to out[q] and its level to levels[q] (optional).
__global__ __launch_bounds__(64 * kTriQuadWaves) void k_tri1h_quad(
    chomp_config cfg, TabLayout L, const Epoch* __restrict__ epochs, int e,
    const double* __restrict__ tab, const SiCiTab* __restrict__ sici_g, int code,
    const double* __restrict__ k, long n, double* __restrict__ out, double* __restrict__ levels,
    unsigned* __restrict__ status) {
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
  Tri1hQuadIntegrand f;
  f.E = &E; f.S = &S; f.nu_knots = nu_knots; f.lnm_pp = lnm_pp; f.NM = NM; f.code = code;
  double kv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    kv[i] = k[q * 4 + i];
    f.lk[i] = log(kv[i]);
    f.src[i] = i;
    for (int m = i - 1; m >= 0; --m)
      if (kv[m] == kv[i]) f.src[i] = m;
  }
  double red[1];
  Scalar1<Tri1hQuadIntegrand> w{f};
  const RombergOut<1> r = romberg_group<1, 1>(w, log(E.nu_min), log(E.nu_max),
                                              cfg.global_precision, cfg.halo_precision,
                                              cfg.divmax, red);
  if ((threadIdx.x & 63) == 0) {
    const double rb = E.rho_bar;
    out[q] = r.value[0] / (rb * rb * rb);
    if (levels) levels[q] = (double)r.level[0];
    if (!r.converged[0]) atomicOr(&status[e], kStTri1hDivmax);
  }
}

}  // namespace chomp
