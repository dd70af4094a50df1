// TEST-ONLY harness: the sixth device counterpart of tests/hostcheck.  One HIP translation unit
// that compiles the product's header chain (chomp_cov_kernels.h down to chomp_math.h) FOR THE
// DEVICE, with the product's compiler flags, and drives three pieces of it on inputs handed in:
//   * the chi-only node table of the C_l route, k_cell_nodes and k_cell_nodes_sets, with the
//     product's block size and dynamic LDS, on a projection set-up (ProjDev scalars and a slab
//     of window / chi(z) / growth cubics) the caller supplies -- no kernel set-up runs;
//   * the parallel not-a-knot spline build, spline_build_pcr and spline_build_staged, in the
//     block shapes the product calls them in (thin kernels: the product has none around them);
//   * the C_l chain itself -- k_cell_nodes, k_cell_ptab, k_cell / k_cell4, k_cell_deep and their
//     _epochs and _sets forms -- with the Romberg levels (LT, split, divmax) as arguments, the
//     hand-over (list and states) read back between the two kernels;
// and returns the host's plan of the C_l work buffer (cell_plan, cell_epoch_stride,
// cell_set_stride).  It includes the headers themselves, never copies of their functions.  Never
// loaded by the chomp_amd package, not in _lib.UNITS, no part of the C ABI.  Built and loaded by
// tests/devcheck_build.py.
//
// Every entry point allocates its buffers, fills every output and work buffer with NaN bytes
// (what a kernel never wrote stays recognisable), launches, synchronises, returns the HIP error
// code (0: success; -1: an argument outside what the buffers were sized for) and frees its
// buffers, unless it is a plain getter.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../chomp_amd/csrc/chomp_cov_kernels.h"
#include "power_setup.h"

using chomp::ProjDev;
using chomp::ProjLayout;
using chomp::ProjLds;

namespace {

using devcheck::Dev;
using devcheck::DevI;
using devcheck::DevT;

constexpr int kPdIn = 8;        // chi_min chi_max me_z_min[0] me_z_max[0] w_chi_min[0] w_chi_max[0]
                                // w_chi_min[1] w_chi_max[1]; every other field of ProjDev zero
constexpr int kMaxSets = 4, kMaxLists = 8, kMaxN = 2048, kMaxPts = 128, kNKT = 8;
constexpr int kMaxSplineN = 128, kMaxWaves = 4;

ProjDev proj_dev(const double* v) {
  ProjDev pd;
  std::memset(&pd, 0, sizeof(pd));
  pd.chi_min = v[0]; pd.chi_max = v[1];
  pd.me_z_min[0] = v[2]; pd.me_z_max[0] = v[3];
  pd.w_chi_min[0] = v[4]; pd.w_chi_max[0] = v[5];
  pd.w_chi_min[1] = v[6]; pd.w_chi_max[1] = v[7];
  return pd;
}

bool proj_ok(int NC, int NWp) { return NC >= 4 && NC <= kMaxPts && NWp >= 4 && NWp <= kMaxPts; }

// block `threads`, dynamic LDS 9 n doubles: one system on the first 64 threads, rows strided by
// 64, knots read where they lie (as k_de_table, k_power_spline and the mass tables call it)
__global__ void k_pcr(const double* x, const double* y, int n, double* c) {
  extern __shared__ __align__(16) double sm[];
  chomp::spline_build_pcr(x, y, n, c, sm, (int)threadIdx.x, 64, threadIdx.x < 64);
}

// block 64 * n_wave, dynamic LDS n_wave * 11 n doubles: one system per wavefront in lockstep,
// wavefront w's at x + w n, y + w n, c + 4 w (n - 1), where bit w of `mask` is set (as
// k_proj_me_splines, k_proj_window_splines and k_proj_kernel_spline call it)
__global__ void k_staged(const double* x, const double* y, int n, double* c, unsigned mask) {
  extern __shared__ __align__(16) double sm[];
  const int wave = threadIdx.x >> 6;
  chomp::spline_build_staged(x + (size_t)wave * n, y + (size_t)wave * n, n,
                             c + (size_t)wave * 4 * (n - 1), sm + (size_t)wave * 11 * n,
                             ((mask >> wave) & 1u) != 0);
}

__global__ void k_logs(const double* x, int n, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = log(x[i]);
}

}  // namespace

extern "C" {

int dl_romberg_dump() { return chomp::kRombergDump; }
int dl_ptab_n() { return chomp::kPTabN; }
int dl_pd_inputs() { return kPdIn; }
// kCellTabLevel, kCellSplitLevel, kCell4Level, kCellDeepThreads, kDeepLds
void dl_constants(int* out) {
  out[0] = chomp::kCellTabLevel; out[1] = chomp::kCellSplitLevel; out[2] = chomp::kCell4Level;
  out[3] = chomp::kCellDeepThreads; out[4] = chomp::kDeepLds;
}

// make_proj_layout(NC, NWp, NKT): out[0] me_chi[0], [1] me_pp_z[0], [2] me_pp_g[0], [3] w_pp[0],
// [4] w_pp[1], [5] total, [6] ProjLds::doubles
int dl_proj_layout(int NC, int NWp, int NKT, int* out) {
  if (!proj_ok(NC, NWp) || NKT < 4 || NKT > kMaxPts) return -1;
  const ProjLayout L = chomp::make_proj_layout(NC, NWp, NKT);
  out[0] = L.me_chi[0]; out[1] = L.me_pp_z[0]; out[2] = L.me_pp_g[0];
  out[3] = L.w_pp[0]; out[4] = L.w_pp[1]; out[5] = L.total; out[6] = ProjLds::doubles(L);
  return 0;
}

// cell_plan(divmax, NK, make_proj_layout(NC, NWp, NKT), n, one_kernel, per_row_nodes): out[0]
// sh_nodes, [1] sh, [2] shd, [3] deep_lds, [4] deep_fits, [5] LT, [6] split, [7] four, [8] n_nodes,
// [9] stride, [10] pk_at, [11] state_at, [12] deep_at, [13] gnodes, [14] gdeep, [15] per_row_nodes,
// [16] doubles(1), [17] doubles(3), [18] cell_epoch_stride(n), [19] cell_set_stride(n, LT)
int dl_plan(int divmax, int NK, int NC, int NWp, int NKT, long long n, long long one_kernel,
            int per_row_nodes, long long* out) {
  if (!proj_ok(NC, NWp) || NKT < 4 || NKT > kMaxPts || divmax < 1 || divmax > 30 || NK < 2 || n < 1)
    return -1;
  const ProjLayout L = chomp::make_proj_layout(NC, NWp, NKT);
  const chomp::CellPlan P = chomp::cell_plan(divmax, NK, L, (size_t)n, one_kernel, per_row_nodes != 0);
  out[0] = (long long)P.sh_nodes; out[1] = (long long)P.sh; out[2] = (long long)P.shd;
  out[3] = P.deep_lds; out[4] = P.deep_fits ? 1 : 0; out[5] = P.LT; out[6] = P.split;
  out[7] = P.four ? 1 : 0; out[8] = (long long)P.n_nodes; out[9] = (long long)P.stride;
  out[10] = (long long)P.pk_at; out[11] = (long long)P.state_at; out[12] = (long long)P.deep_at;
  out[13] = P.gnodes; out[14] = P.gdeep; out[15] = P.per_row_nodes ? 1 : 0;
  out[16] = (long long)P.doubles(1); out[17] = (long long)P.doubles(3);
  out[18] = (long long)chomp::cell_epoch_stride((size_t)n);
  out[19] = (long long)chomp::cell_set_stride((size_t)n, P.LT);
  return 0;
}

// k_cell_nodes on one projection set-up: pdv the kPdIn scalars, tab a slab of
// make_proj_layout(NC, NWp, kNKT).total doubles, growth D_z, level LT, with n_lists lists
// list_stride ints apart.  nodes_out: 3 (2^LT + 1) + extra doubles (the node table and what lies
// behind it); deep_out: (n_lists - 1) list_stride + 2 + extra ints.
int dl_nodes(int NC, int NWp, const double* pdv, const double* tab, double D_z, int LT, int n_lists,
             long long list_stride, int extra, double* nodes_out, int* deep_out) {
  if (!proj_ok(NC, NWp) || LT < 1 || LT > chomp::kCellTabLevel || n_lists < 1 || n_lists > kMaxLists ||
      list_stride < 2 || list_stride > (1 << 20) || extra < 0 || extra > 4096)
    return -1;
  const ProjLayout L = chomp::make_proj_layout(NC, NWp, kNKT);
  const ProjDev pd = proj_dev(pdv);
  const size_t N = ((size_t)1 << LT) + 1;
  const size_t n_deep = (size_t)(n_lists - 1) * (size_t)list_stride + 2 + (size_t)extra;
  DevT<ProjDev> d_pd(1, &pd);
  Dev d_tab((size_t)L.total, tab), d_nodes(3 * N + (size_t)extra, nullptr);
  DevI d_deep(n_deep, nullptr);
  DW_TRY(d_pd.err); DW_TRY(d_tab.err); DW_TRY(d_nodes.err); DW_TRY(d_deep.err);
  DW_TRY(d_nodes.nan_fill());
  DW_TRY(d_deep.nan_fill());
  chomp::k_cell_nodes<<<dim3((unsigned)((N + 255) / 256)), dim3(256),
                        (size_t)ProjLds::doubles(L) * sizeof(double)>>>(
      L, d_pd.p, d_tab.p, D_z, LT, d_nodes.p, d_deep.p, n_lists, (size_t)list_stride);
  DW_SYNC();
  DW_TRY(d_nodes.back(nodes_out, 3 * N + (size_t)extra));
  DW_TRY(d_deep.back(deep_out, n_deep));
  return 0;
}

// k_cell_nodes_sets on n_sets set-ups (pdv: kPdIn scalars each; tab: a slab of the layout's total
// each; D_z each) into one work buffer of n_sets rows of cell_set_stride(n, LT) doubles, the
// first row's list at its plan's deep_at, as chomp_cell_sets places them.  buf_out: the whole
// buffer.
int dl_nodes_sets(int NC, int NWp, int n_sets, const double* pdv, const double* tab,
                  const double* D_z, int LT, int n, double* buf_out) {
  if (!proj_ok(NC, NWp) || LT < 1 || LT > chomp::kCellTabLevel || n_sets < 1 || n_sets > kMaxSets ||
      n < 1 || n > kMaxN)
    return -1;
  const ProjLayout L = chomp::make_proj_layout(NC, NWp, kNKT);
  std::vector<ProjDev> pd(n_sets);
  for (int s = 0; s < n_sets; ++s) pd[s] = proj_dev(pdv + (size_t)s * kPdIn);
  const size_t N = ((size_t)1 << LT) + 1;
  const size_t stride = chomp::cell_set_stride((size_t)n, LT);
  const size_t deep_at = 3 * N + (size_t)chomp::kPTabN + 1 + (size_t)n * chomp::kRombergDump;
  DevT<ProjDev> d_pd(n_sets, pd.data());
  Dev d_tab((size_t)n_sets * L.total, tab), d_D(n_sets, D_z), d_buf((size_t)n_sets * stride, nullptr);
  DW_TRY(d_pd.err); DW_TRY(d_tab.err); DW_TRY(d_D.err); DW_TRY(d_buf.err);
  DW_TRY(d_buf.nan_fill());
  chomp::k_cell_nodes_sets<<<dim3((unsigned)((N + 255) / 256), (unsigned)n_sets), dim3(256),
                             (size_t)ProjLds::doubles(L) * sizeof(double)>>>(
      L, d_pd.p, d_tab.p, (size_t)L.total, d_D.p, LT, d_buf.p,
      reinterpret_cast<int*>(d_buf.p + deep_at), stride);
  DW_SYNC();
  DW_TRY(d_buf.back(buf_out, (size_t)n_sets * stride));
  return 0;
}

// The not-a-knot build on n_sys systems of n knots (x[s n + i], y[s n + i]) in one block.
// staged == 0: spline_build_pcr on the knots where they lie, one system (n_sys = 1), block
// `threads`; staged != 0: spline_build_staged, block 64 n_sys, system s on wavefront s where bit s
// of mine_mask is set.  c_out[s * 4 (n - 1) + 4 i + p]: NaN bytes where nothing was written.
int dl_spline(int staged, const double* x, const double* y, int n, int n_sys, unsigned mine_mask,
              int threads, double* c_out) {
  if (n < 4 || n > kMaxSplineN || n_sys < 1 || n_sys > kMaxWaves) return -1;
  if (staged ? threads != 64 * n_sys : (n_sys != 1 || threads < 64 || threads > 256 || threads % 64))
    return -1;
  Dev d_x((size_t)n_sys * n, x), d_y((size_t)n_sys * n, y), d_c((size_t)n_sys * 4 * (n - 1), nullptr);
  DW_TRY(d_x.err); DW_TRY(d_y.err); DW_TRY(d_c.err);
  DW_TRY(d_c.nan_fill());
  if (staged)
    k_staged<<<dim3(1), dim3((unsigned)threads), (size_t)n_sys * 11 * n * sizeof(double)>>>(
        d_x.p, d_y.p, n, d_c.p, mine_mask);
  else
    k_pcr<<<dim3(1), dim3((unsigned)threads), (size_t)9 * n * sizeof(double)>>>(d_x.p, d_y.p, n,
                                                                                d_c.p);
  DW_SYNC();
  DW_TRY(d_c.back(c_out, (size_t)n_sys * 4 * (n - 1)));
  return 0;
}


// out[i] = log(x[i]) by the device's log (what every kernel here forms ln k_min, ln k_max and
// ln l with)
int dl_logs(const double* x, int n, double* out) {
  if (n < 1 || n > 4096) return -1;
  Dev d_x(n, x), d_o(n, nullptr);
  DW_TRY(d_x.err); DW_TRY(d_o.err);
  DW_TRY(d_o.nan_fill());
  k_logs<<<dim3((unsigned)((n + 63) / 64)), dim3(64)>>>(d_x.p, n, d_o.p);
  DW_SYNC();
  DW_TRY(d_o.back(out, n));
  return 0;
}

// The C_l route as chomp_cell / chomp_cell_epochs / chomp_cell_sets chain it, on the set-ups
// handed in, with the levels as arguments: k_cell_nodes(_sets), k_cell_ptab(_epochs) (use_ptab),
// then kind 0 k_cell<HF, BAO, false>, 1 k_cell<HF, BAO, true>, 2 k_cell4<HF, BAO>, then, with
// deep_blocks > 0 and split < divmax, k_cell_deep<HF, BAO> on deep_blocks blocks (opted in to
// kDeepLds as lds_opt_in does).  form 0: the single kernels (rows = 1); 1: the _epochs forms, row
// y on epoch y; 2: the _sets forms, row y on epoch y and set y.  The work buffer is the plan's:
// [3 N node table, once] (forms 0, 1) then per row [3 N node table (form 2)], kPTabN + 1 doubles
// of P(k), n_ell states, the list; out1 / buf1: the values and the whole buffer after the first
// kernel, out2 / buf2 after k_cell_deep (untouched without it).  Instances: HF with BAO false
// only; BAO (no spectrum table: use_ptab 0) with kinds 1 and 2 and k_cell_deep; forms 1, 2 with
// neither.
int dl_cell(int n_epoch, const double* ein, const double* htab, int NK, double k_min, double k_max,
            int which, int bao, int NC, int NWp, int n_sets, const double* pdv, const double* ptab,
            const double* D_z, const double* ell, int n_ell, double tol, double rtol, int divmax,
            int LT, int split, int kind, int use_ptab, int form, int rows, int deep_blocks,
            double* out1, double* buf1, double* out2, double* buf2) {
  const bool hf = (which & CHOMP_P_HALOFIT) != 0;
  const int w = which & 15;
  if (!devcheck::setup_ok(n_epoch, NK, k_min, k_max) || w < CHOMP_P_LIN || w > CHOMP_P_GG ||
      (which & ~(15 | CHOMP_P_HALOFIT | CHOMP_P_EXTRAPOLATE)) != 0 || !proj_ok(NC, NWp) ||
      n_ell < 1 || n_ell > 64 || divmax < 1 || divmax > chomp::kMaxDivmax || LT < 1 ||
      LT > chomp::kCellTabLevel || split < 1 || split > divmax || kind < 0 || kind > 2 ||
      form < 0 || form > 2 || rows < 1 || rows > kMaxSets || (form == 0 && rows != 1) ||
      n_epoch < rows || n_sets != (form == 2 ? rows : 1) || deep_blocks < 0 || deep_blocks > 512)
    return -1;
  if ((kind != 1 && split > LT) || (kind == 2 && split < 6)) return -1;   // (the lean instances)
  if ((hf && bao) || (bao && (kind == 0 || use_ptab)) || (form != 0 && (hf || bao || kind == 0)))
    return -1;
  const bool deep_run = deep_blocks > 0 && split < divmax;
  if (deep_run && !bao && !use_ptab) return -1;
  devcheck::Setup S(n_epoch, ein, htab, NK, k_min, k_max, nullptr);
  if (const int rc = S.init()) return rc;
  S.cfg.global_precision = tol;
  S.cfg.corr_precision = rtol;
  S.cfg.divmax = divmax;
  const ProjLayout L = chomp::make_proj_layout(NC, NWp, kNKT);
  std::vector<ProjDev> pd(n_sets);
  for (int s = 0; s < n_sets; ++s) pd[s] = proj_dev(pdv + (size_t)s * kPdIn);
  const size_t N = ((size_t)1 << LT) + 1, n = (size_t)n_ell;
  const size_t stride = form == 2 ? chomp::cell_set_stride(n, LT) : chomp::cell_epoch_stride(n);
  const size_t total = (form == 2 ? 0 : 3 * N) + stride * (size_t)rows;
  const size_t pk_at = 3 * N, state_at = pk_at + (size_t)chomp::kPTabN + 1;
  const size_t deep_at = state_at + n * chomp::kRombergDump;
  DevT<ProjDev> d_pd(n_sets, pd.data());
  Dev d_ptab((size_t)n_sets * L.total, ptab), d_D(n_sets, D_z), d_ell(n, ell), d_buf(total, nullptr),
      d_out(n * (size_t)rows, nullptr);
  DW_TRY(d_pd.err); DW_TRY(d_ptab.err); DW_TRY(d_D.err); DW_TRY(d_ell.err); DW_TRY(d_buf.err);
  DW_TRY(d_out.err);
  DW_TRY(d_buf.nan_fill());
  DW_TRY(d_out.nan_fill());
  double* nodes = d_buf.p;
  double* pk_tab = d_buf.p + pk_at;
  double* state = d_buf.p + state_at;
  int* deep = reinterpret_cast<int*>(d_buf.p + deep_at);
  const size_t sh_nodes = (size_t)ProjLds::doubles(L) * sizeof(double);
  const size_t sh = S.lds() + sh_nodes, shd = sh + ((size_t)chomp::kPTabN + 1) * sizeof(double);
  if (shd > (size_t)chomp::kDeepLds) return -1;
  const dim3 gnodes((unsigned)((N + 255) / 256), form == 2 ? (unsigned)rows : 1u);
  const dim3 gtab((chomp::kPTabN + 256) / 256, form == 0 ? 1u : (unsigned)rows);
  const unsigned E = (unsigned)rows;
  const double Dz = D_z[0];
  const size_t pstride = (size_t)L.total;
  if (form == 2)
    chomp::k_cell_nodes_sets<<<gnodes, dim3(256), sh_nodes>>>(L, d_pd.p, d_ptab.p, pstride, d_D.p, LT,
                                                              nodes, deep, stride);
  else
    chomp::k_cell_nodes<<<gnodes, dim3(256), sh_nodes>>>(L, d_pd.p, d_ptab.p, Dz, LT, nodes, deep,
                                                         rows, 2 * stride);
  DW_SYNC();
  const double* pk = use_ptab ? pk_tab : nullptr;
  auto first = [&](auto HF, auto BAO) -> int {
    if (use_ptab) {
      if (form == 0)
        chomp::k_cell_ptab<HF, BAO><<<gtab, dim3(256), S.lds()>>>(S.cfg, S.L, S.ep(), 0, S.d_tab.p,
                                                                  which, pk_tab);
      else
        chomp::k_cell_ptab_epochs<HF, BAO><<<gtab, dim3(256), S.lds()>>>(
            S.cfg, S.L, S.ep(), 0, S.d_tab.p, which, pk_tab, (int*)nullptr, stride);
      DW_SYNC();
    }
    return 0;
  };
  // (every launch below names its instance: only these are compiled)
#define DL_CELL(HF, BAO, DIRECT)                                                                  \
  chomp::k_cell<HF, BAO, DIRECT><<<dim3((unsigned)n), dim3(256), sh>>>(                           \
      S.cfg, S.L, L, S.ep(), 0, S.d_tab.p, which, d_pd.p, d_ptab.p, Dz, d_ell.p, d_out.p, nodes,  \
      LT, pk, split, deep, state)
#define DL_CELL4(HF, BAO)                                                                         \
  chomp::k_cell4<HF, BAO><<<dim3((unsigned)((n + 3) / 4)), dim3(256), sh>>>(                      \
      S.cfg, S.L, L, S.ep(), 0, S.d_tab.p, which, d_pd.p, d_ptab.p, Dz, d_ell.p, n_ell, d_out.p,  \
      nodes, LT, pk, split, deep, state)
  if (form == 0) {
    if (hf) {
      if (const int rc = first(std::true_type{}, std::false_type{})) return rc;
      if (kind == 1) DL_CELL(true, false, true);
      else if (kind == 2) DL_CELL4(true, false);
      else return -1;
    } else if (bao) {           // (wiggles: no spectrum table, at_ln at every node)
      if (kind == 1) DL_CELL(false, true, true);
      else DL_CELL4(false, true);
    } else {
      if (const int rc = first(std::false_type{}, std::false_type{})) return rc;
      if (kind == 0) DL_CELL(false, false, false);
      else if (kind == 1) DL_CELL(false, false, true);
      else DL_CELL4(false, false);
    }
  } else {
    if (const int rc = first(std::false_type{}, std::false_type{})) return rc;
    if (form == 1 && kind == 1)
      chomp::k_cell_epochs<false, false, true><<<dim3((unsigned)n, E), dim3(256), sh>>>(
          S.cfg, S.L, L, S.ep(), 0, S.d_tab.p, which, d_pd.p, d_ptab.p, Dz, d_ell.p, d_out.p, nodes,
          LT, pk, split, deep, state, stride);
    else if (form == 1)
      chomp::k_cell4_epochs<false, false><<<dim3((unsigned)((n + 3) / 4), E), dim3(256), sh>>>(
          S.cfg, S.L, L, S.ep(), 0, S.d_tab.p, which, d_pd.p, d_ptab.p, Dz, d_ell.p, n_ell, d_out.p,
          nodes, LT, pk, split, deep, state, stride);
    else if (kind == 1)
      chomp::k_cell_sets<false, false, true><<<dim3((unsigned)n, E), dim3(256), sh>>>(
          S.cfg, S.L, L, S.ep(), 0, S.d_tab.p, which, d_pd.p, d_ptab.p, pstride, d_D.p, d_ell.p,
          d_out.p, nodes, LT, pk, split, deep, state, stride);
    else
      chomp::k_cell4_sets<false, false><<<dim3((unsigned)((n + 3) / 4), E), dim3(256), sh>>>(
          S.cfg, S.L, L, S.ep(), 0, S.d_tab.p, which, d_pd.p, d_ptab.p, pstride, d_D.p, d_ell.p,
          n_ell, d_out.p, nodes, LT, pk, split, deep, state, stride);
  }
#undef DL_CELL
#undef DL_CELL4
  DW_SYNC();
  DW_TRY(d_out.back(out1, n * (size_t)rows));
  DW_TRY(d_buf.back(buf1, total));
  if (!deep_run) return 0;
  const dim3 gdeep((unsigned)deep_blocks, E), bdeep(chomp::kCellDeepThreads);
#define DL_OPT_IN(K)                                                                              \
  DW_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&K),                                   \
                             hipFuncAttributeMaxDynamicSharedMemorySize, chomp::kDeepLds))
  if (form == 0 && hf) {
    DL_OPT_IN((chomp::k_cell_deep<true, false>));
    chomp::k_cell_deep<true, false><<<gdeep, bdeep, shd>>>(
        S.cfg, S.L, L, S.ep(), 0, S.d_tab.p, which, d_pd.p, d_ptab.p, Dz, d_ell.p, d_out.p, nodes, LT,
        pk, split, deep, state);
  } else if (form == 0 && bao) {
    DL_OPT_IN((chomp::k_cell_deep<false, true>));
    chomp::k_cell_deep<false, true><<<gdeep, bdeep, shd>>>(
        S.cfg, S.L, L, S.ep(), 0, S.d_tab.p, which, d_pd.p, d_ptab.p, Dz, d_ell.p, d_out.p, nodes, LT,
        pk, split, deep, state);
  } else if (form == 0) {
    DL_OPT_IN((chomp::k_cell_deep<false, false>));
    chomp::k_cell_deep<false, false><<<gdeep, bdeep, shd>>>(
        S.cfg, S.L, L, S.ep(), 0, S.d_tab.p, which, d_pd.p, d_ptab.p, Dz, d_ell.p, d_out.p, nodes, LT,
        pk, split, deep, state);
  } else if (form == 1) {
    DL_OPT_IN((chomp::k_cell_deep_epochs<false, false>));
    chomp::k_cell_deep_epochs<false, false><<<gdeep, bdeep, shd>>>(
        S.cfg, S.L, L, S.ep(), 0, S.d_tab.p, which, d_pd.p, d_ptab.p, Dz, d_ell.p, n_ell, d_out.p,
        nodes, LT, pk, split, deep, state, stride);
  } else {
    DL_OPT_IN((chomp::k_cell_deep_sets<false, false>));
    chomp::k_cell_deep_sets<false, false><<<gdeep, bdeep, shd>>>(
        S.cfg, S.L, L, S.ep(), 0, S.d_tab.p, which, d_pd.p, d_ptab.p, pstride, d_D.p, d_ell.p, n_ell,
        d_out.p, nodes, LT, pk, split, deep, state, stride);
  }
#undef DL_OPT_IN
  DW_SYNC();
  DW_TRY(d_out.back(out2, n * (size_t)rows));
  DW_TRY(d_buf.back(buf2, total));
  return 0;
}

}  // extern "C"
