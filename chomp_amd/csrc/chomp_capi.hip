// chomp_capi.hip -- C ABI (include/chomp_mi355x.h) over the HIP kernels.
// Host side only orchestrates: parameter upload, kernel launches on the context's
// stream, staging of host buffers.  No numerical work of the hot path runs on the
// CPU (the only host arithmetic is parameter preparation: the 1.05-step candidate
// mass sequence, erfinv for HODZheng.first_moment_zero, the Tinker parameter
// splines of a fixed 9-row table).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <map>
#include <unordered_map>
#include <vector>

#include "../../include/chomp_mi355x.h"
#include "chomp_buffers.h"
#include "chomp_power_kernels.h"
#include "chomp_proj_kernels.h"
#include "chomp_cov_kernels.h"
#include "chomp_probe_kernel.h"
#include "chomp_de_kernels.h"
#include "chomp_pt_kernels.h"
#include "chomp_tri_kernels.h"
#include "chomp_profile_kernels.h"
#include "chomp_pp_plan.h"

using namespace chomp;

// roctx ranges around the stages (chomp_set_tuning CHOMP_TUNE_ROCTX; rocprofv3 --marker-trace):
// the marker library is looked up at run time, so nothing links against a profiler.
struct RoctxApi {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  bool load() {
    if (push) return true;
    for (const char* lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
      void* h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL);
      if (!h) continue;
      push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
      pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
      if (push && pop) return true;
      push = nullptr; pop = nullptr;
    }
    return false;
  }
};

struct chomp_ctx {
  chomp_config cfg;
  RoctxApi roctx;
  int device = 0;
  hipStream_t stream = nullptr;
  bool owns_stream = false;
  TabLayout L;
  std::string err;

  // Buffers a captured HIP graph may still reference are never freed before the context
  // is destroyed (mem.graph_seen: a call of this context has been captured at least once).
  BufferHome mem;

  // constant tables
  DeviceBuffer<SiCiTab> d_sici;
  DeviceBuffer<BesselTab> d_j0;
  DeviceBuffer<BesselTab> d_j2;
  DeviceBuffer<TinkerTab> d_tinker;
  DeviceBuffer<double> d_gl16;
  DeviceBuffer<double> d_cand;

  // epoch batch
  size_t n_epoch = 0, cap_epoch = 0;
  // (the parameter blocks travel with their shadows: see upload)
  StagedBuffer<chomp_cosmo> d_cosmo;
  StagedBuffer<double> d_z;
  DeviceBuffer<Epoch> d_epochs;
  DeviceBuffer<double> d_search;
  DeviceBuffer<double> d_probe;    // k_epoch_init: certifying probes of the mass-limit search
  DeviceBuffer<int> d_count;       // k_epoch_init: arrivals per epoch (reset by the kernel)
  DeviceBuffer<int> d_pending;     // work list of k_halo_knots_deep (cleared by k_halo_finalize)
  DeviceBuffer<double> d_tab;
  StagedBuffer<chomp_halo_par> d_mass_par;
  StagedBuffer<chomp_halo_par> d_profile;
  StagedBuffer<HodDev> d_hod;
  DeviceBuffer<double> d_nodes;    // node tables of the halo integrals
  DeviceBuffer<double> d_snodes;   // node tables of the sigma(R) integrals (per cosmology slot)
  StagedBuffer<int> d_slot;        // epoch -> cosmology slot
  StagedBuffer<int> d_first;       // slot -> an epoch with that cosmology
  DeviceBuffer<unsigned> d_status; // per-epoch status word (chomp_get_status)
  DeviceBuffer<double> d_endp;     // integrand pairs of the knots at the upper end point
  DeviceBuffer<int> d_npend;       // per epoch: listed knots + 1 token (k_halo_knots_fast)
  long long tune[CHOMP_TUNE_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // chomp_set_tuning
  bool have_epochs = false, have_mass = false, have_halo = false;
  unsigned fam_mask = 0;          // families (F_* bits) with valid splines in every epoch (set-ups)
  std::vector<unsigned> put_mask;  // per epoch: families installed by chomp_put_table since epochs_set
  // HaloSuperSampleCovariance._delta_b per epoch (chomp_set_delta_b), read by CHOMP_P_MM_SSC.
  // chomp_epochs_set only raises delta_b_zero: the buffer is cleared when something next needs
  // it, so that a batch that never asks for the super-sample codes queues nothing for them.
  DeviceBuffer<double> d_delta_b;
  StagedBlock sh_delta_b;
  bool delta_b_zero = true;
  std::vector<char> have_halofit;
  StagedBlock sh_proj, sh_pp[2];   // projection scalars, tabulated redshift distributions
  // pinned host mirrors of the staging buffers of host-pointer calls (chomp_power)
  PinnedBuffer<unsigned> h_status; // chomp_status_post: pinned copy of d_status ...
  size_t n_hstatus = 0;
  hipEvent_t ev_status = nullptr;  // ... complete when this event is
  PinnedBuffer<double> h_stage_in;
  PinnedBuffer<double> h_stage_out;

  // staging for host-pointer calls
  DeviceBuffer<double> d_stage_in;
  DeviceBuffer<double> d_kcache;   // device copy of the last host k grid of chomp_power
  std::vector<double> kcache_shadow;   // ... which is this one (empty: the buffer holds none)
  DeviceBuffer<double> d_stage_out;
  DeviceBuffer<int> d_slow;        // Stage E: 2 counters + list of k groups for the per-lane pass
  DeviceBuffer<int> d_winfo;       // Stage E: per k group knot interval / flags (k_power_prep)
  DeviceBuffer<double> d_ktab;     // Stage E: per-k (offset, shape) table (k_power_prep)
  DeviceBuffer<double> d_wnodes;   // w(theta): theta-independent integrand factor on the Romberg nodes
  DeviceBuffer<double> d_cnodes;   // C_l: chi-only factors on the Romberg nodes
  DeviceBuffer<double> d_samples;  // coarse samples of the listed knots, a slot each (k_halo_knots_samples -> _fast)
  DeviceBuffer<double> d_psum;     // ... and their per-level sums
  DeviceBuffer<DeepPlan> d_plan;   // per (epoch, group): the break-point plan (k_halo_knots -> _fast)
  DeviceBuffer<double> d_deepw;    // k_halo_knots_fast: level weights (deep_weights_host)
  DeviceBuffer<double> d_hf_ainv;  // k_halofit_finalize: inverse collocation matrix of the ln R grid
  DeviceBuffer<int> d_deepstat;    // k_halo_knots_fast: knots done by the fast / literal path
  // chomp_power_plan: the k-only table of a registered k grid, kept across chomp_power calls
  struct PowerPlan {
    bool valid = false;
    const double* k = nullptr;
    size_t nk = 0;
    chomp_cosmo cosmo;             // the cosmology the shape column was computed for
    int bao = 0, parity = 0, n_slow = -1;
  } plan;
  int slow_parity = 0;
  // kernel -> the dynamic LDS it has been opted in to (lds_opt_in; per context: hipFuncSetAttribute
  // applies to the current device, so a process-wide record would skip a second device)
  std::unordered_map<const void*, int> lds_limit;
  bool slow_by_memset = false;     // set once a Stage E call has been captured into a HIP graph
  int precision = CHOMP_PREC_F64;  // chomp_set_precision
  int with_bao = 0;                // chomp_set_transfer
  // w0-wa dark energy (chomp_set_dark_energy): the switch, the knots (ln a_i, then z_i; host-made,
  // sent once), the epochs' and the projection's tables, and per epoch its table (-1: none)
  int dark_energy = 0;
  StagedBuffer<double> d_de_knots;
  DeTables de_ep, de_proj;
  std::vector<int> de_slot;
  StagedBuffer<int> d_de_slot;
  // What chomp_kernel_setup_sets / _pairs take beyond analytic windows in Lambda-CDM
  // (chomp_set_sets_scope: CHOMP_SETS_* bits)
  unsigned sets_scope = 0;
  // MassFunctionSecondOrder (chomp_set_second_order): the switch, and per epoch the sigma knots,
  // the sigma(nu) spline and bias_2_norm (B2Layout); have_b2: the last mass set-up made them
  int second_order = 0;
  bool have_b2 = false;
  B2Layout B2;
  DeviceBuffer<double> d_b2;
  // HaloTrispectrumOneHalo (chomp_tri1h_setup): per epoch the I_0^4 table, its levels and its
  // bicubic (TriLayout); tri_built: the epoch has one since chomp_epochs_set
  TriLayout T3;
  DeviceBuffer<double> d_tri;
  std::vector<char> tri_built;
  int tri_moment = -1;             // the moment of the I_0^4 tables in d_tri (the last chomp_tri1h_setup)
  // HaloTrispectrum (chomp_tri_setup): per epoch the I_1^2, I_1^3, I_2^2 and I_2^1 tables with
  // their levels and splines (TriTabLayout); tri4_built as tri_built
  TriTabLayout Q4;
  DeviceBuffer<double> d_tri4;
  std::vector<char> tri4_built;
  // General-slope halo profiles (chomp_set_general_profile): the switch, per epoch the y(k, M)
  // table with its levels and splines (ProfLayout), and which epochs of the last halo set-up have
  // one (prof_general: alpha != -1 in a set-up that took the general path)
  int general_profile = 0;
  ProfLayout PL;
  DeviceBuffer<double> d_prof;
  std::vector<char> prof_general;
  bool prof_built = false;         // ... and that set-up built knot tables (some family asked for)
  int timing = 0;                  // chomp_set_timing: HIP events around the Stage E launches
  bool timing_valid = false;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  std::vector<int> slot;           // host copy: epoch -> cosmology slot
  size_t n_slots = 1;              // distinct cosmologies of the batch

  // projection
  ProjState proj;
  ProjSets sets;                // chomp_kernel_setup_sets: one projection set-up per cosmology
  CrossState cross;             // Covariance(corr_a, corr_b): the two sides' snapshots and the four tables
  FourierState fourier;         // CovarianceFourier: the four pairs' scalars, Limber tables and splines
  BlocksState blocks;           // chomp_covariance_blocks: one table slab per block of a CovarianceMulti
  SscBlocksState ssc_blocks;    // chomp_covariance_ssc_blocks: one kernel_ssc slab per block
  NgBlocksState ng_blocks;      // chomp_covariance_ng_blocks: one kernel_NG slab per block
  std::vector<double> sets_z_min, sets_z_max;   // per set of `sets`: the redshifts its two windows share
  // The side stream.  The projection set-up (chomp_kernel_setup / chomp_multi_epoch_setup:
  // a chain of six small launches) depends on nothing the halo set-up produces, and C_l on
  // nothing w(theta) produces: they run here, beside the context's stream, ordered against it
  // by events -- behind everything queued on `stream` when they start, and joined back before
  // anything reads what they wrote (proj_pending: lazily, at the next call that looks at the
  // projection tables).  Under stream capture the fork and the join are captured with the rest
  // (the side stream joins the capture through ev_side_go and is joined back before the
  // capture ends: every call that forks also joins, the lazy projection join at the first
  // reader); what must not happen is a join, inside a capture, of side work queued before it.
  hipStream_t side = nullptr;
  hipEvent_t ev_side_go = nullptr, ev_proj_ready = nullptr, ev_side_done = nullptr;
  bool proj_pending = false;
  bool proj_pending_captured = false;   // ... and it was queued inside the capture in progress
  bool status_mirrored = false;    // the last set-up ended with a halo set-up: its finalising blocks
                                   // wrote the status words to the pinned host words themselves
  // (see ensure_hstatus / mirror_next / chomp_status_post)
  PinnedBuffer<unsigned long long> h_mirror;
  unsigned setup_seq = 0, posted_seq = 0;
  int mirror_half = 0, mirror_region = 0, posted_half = 0;
  int posted_kind = 0;             // 0 none, 1 the mirror, 2 the copy, 3 collected into posted_saved
  bool posted_in_capture = false;
  std::vector<unsigned> posted_saved;
};

namespace {

// Scope of one stage on the host timeline (a no-op unless ranges are switched on).
struct StageRange {
  chomp_ctx* ctx;
  StageRange(chomp_ctx* c, const char* name) : ctx(c && c->roctx.push ? c : nullptr) {
    if (ctx) ctx->roctx.push(name);
  }
  ~StageRange() { if (ctx) ctx->roctx.pop(); }
};

int fail(chomp_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

#define HIPCHK(call)                                                              \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess)                                                         \
      return fail(ctx, CHOMP_ERR_HIP,                                             \
                  std::string(#call) + ": " + hipGetErrorString(e_));             \
  } while (0)

bool capturing(chomp_ctx* ctx) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  ctx->mem.capture = false;
  if (hipStreamIsCapturing(ctx->stream, &st) != hipSuccess) return false;
  ctx->mem.capture = st == hipStreamCaptureStatusActive;
  if (ctx->mem.capture) ctx->mem.graph_seen = true;
  return ctx->mem.capture;
}

// Upload `bytes` from `src` to `dst` unless the shadow says the device already holds
// exactly these bytes.  No host synchronisation with the stream (see StagedBlock).
// Under stream capture a changed block is an error: the graph would bake in the staging
// buffer's contents of capture time (include/chomp_mi355x.h, "HIP graphs").
int upload(chomp_ctx* ctx, void* dst, const void* src, size_t bytes, StagedBlock& b) {
  if (b.shadow.size() == bytes && std::memcmp(b.shadow.data(), src, bytes) == 0) return CHOMP_OK;
  if (capturing(ctx))
    return fail(ctx, CHOMP_ERR_STATE,
                "a parameter block changed while the context's stream is being captured: run the "
                "set-up once with these parameters before capturing (HIP graphs replay the "
                "captured parameters)");
  if (bytes > b.cap) {
    // (buffers still in flight are drained by their events first)
    for (int i = 0; i < 2; ++i)
      if (b.used[i]) HIPCHK(hipEventSynchronize(b.done[i]));
    const size_t cap = bytes + bytes / 2;
    for (int i = 0; i < 2; ++i) {
      if (b.pin[i]) HIPCHK(hipHostFree(b.pin[i]));
      b.pin[i] = nullptr;
      HIPCHK(hipHostMalloc(&b.pin[i], cap, hipHostMallocDefault));
      if (!b.done[i]) HIPCHK(hipEventCreateWithFlags(&b.done[i], hipEventDisableTiming));
      b.used[i] = false;
    }
    b.cap = cap;
  }
  const int t = b.turn;
  if (b.used[t]) HIPCHK(hipEventSynchronize(b.done[t]));   // the copy of two uploads ago: long done
  std::memcpy(b.pin[t], src, bytes);
  HIPCHK(hipMemcpyAsync(dst, b.pin[t], bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipEventRecord(b.done[t], ctx->stream));
  b.used[t] = true;
  b.turn = t ^ 1;
  b.shadow.assign(static_cast<const char*>(src), static_cast<const char*>(src) + bytes);
  return CHOMP_OK;
}
template <class T>
int upload(chomp_ctx* ctx, StagedBuffer<T>& b, const void* src, size_t bytes) {
  return upload(ctx, b.dev.get(), src, bytes, b.sh);
}

// -- the side stream ------------------------------------------------------------------
int side_create(chomp_ctx* ctx) {
  if (ctx->side) return CHOMP_OK;
  HIPCHK(hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
  for (hipEvent_t* e : {&ctx->ev_side_go, &ctx->ev_proj_ready, &ctx->ev_side_done})
    HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  return CHOMP_OK;
}

// While alive, everything the context queues goes to the side stream, which first waits for
// what `stream` holds now; on destruction `done` (if any) is recorded there and the context's
// stream restored.  on() is false (nothing redirected) under stream capture or on failure.
struct SideScope {
  chomp_ctx* ctx;
  hipStream_t saved = nullptr;
  hipEvent_t* done;                // (a member of *ctx: the events are created by begin())
  bool active = false;
  bool marks_proj;                 // the work is a projection set-up: proj_pending on EVERY way out
  SideScope(chomp_ctx* c, hipEvent_t* done_, bool marks_proj_ = false)
      : ctx(c), done(done_), marks_proj(marks_proj_) {}
  int begin() {
    // (the side stream and its events exist before any capture: an eager call of the same kind
    //  comes first -- buffers and parameters have to be in place for a capture anyway)
    if (capturing(ctx) && !ctx->side)
      return fail(ctx, CHOMP_ERR_STATE,
                  "the first call that runs work beside the context's stream came while the stream "
                  "is being captured: run the step once eagerly before capturing it");
    const int rc = side_create(ctx);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ctx->ev_side_go, ctx->stream));
    HIPCHK(hipStreamWaitEvent(ctx->side, ctx->ev_side_go, 0));
    saved = ctx->stream;
    ctx->stream = ctx->side;
    active = true;
    return CHOMP_OK;
  }
  bool on() const { return active; }
  void end() {
    if (!active) return;
    (void)hipEventRecord(*done, ctx->side);
    if (marks_proj) {              // (also on an error return: what was queued is still in flight)
      ctx->proj_pending = true;
      ctx->proj_pending_captured = capturing(ctx);
    }
    ctx->stream = saved;
    active = false;
  }
  ~SideScope() { end(); }
};

// Before anything on the context's stream reads (or rewrites) the projection tables: wait for
// a projection set-up still in flight on the side stream.
int proj_join(chomp_ctx* ctx) {
  if (!ctx->proj_pending) return CHOMP_OK;
  if (capturing(ctx) && !ctx->proj_pending_captured)
    return fail(ctx, CHOMP_ERR_STATE,
                "a projection set-up queued BEFORE the capture is still in flight beside the "
                "stream being captured: make any projection call (or chomp_sync) before the "
                "capture begins");
  HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_proj_ready, 0));   // (captured under capture)
  ctx->proj_pending = false;
  ctx->proj_pending_captured = false;
  return CHOMP_OK;
}

// What a growth of one of the context's buffers came to, as a return code.
int grown(chomp_ctx* ctx, BufferGrowth g) {
  if (g == BufferGrowth::refused)
    return fail(ctx, CHOMP_ERR_STATE,
                "a work buffer would have to grow while the context's stream is being captured: "
                "run the call once at this size before capturing");
  if (g == BufferGrowth::failed)
    return fail(ctx, CHOMP_ERR_HIP, std::string("a buffer of the context: ") +
                                        hipGetErrorString((hipError_t)ctx->mem.error));
  return CHOMP_OK;
}

// Room for n elements in `b` (a DeviceBuffer, PinnedBuffer or StagedBuffer); contents are not
// kept.  *moved: the block is a new one, and holds nothing.
template <class B>
int ensure(chomp_ctx* ctx, B& b, size_t n, bool* moved = nullptr) {
  if (moved) *moved = false;
  if (b.fits(n)) return CHOMP_OK;
  (void)capturing(ctx);
  const BufferGrowth g = b.ensure(ctx->mem, n);
  if (moved) *moved = g == BufferGrowth::moved;
  return grown(ctx, g);
}

// Before a launch with more than 64 KiB of dynamic LDS: opt `kernel` in to `bytes`, once per
// context and kernel.
template <class Kernel>
int lds_opt_in(chomp_ctx* ctx, Kernel* kernel, int bytes) {
  int& have = ctx->lds_limit[reinterpret_cast<const void*>(kernel)];
  if (have >= bytes) return CHOMP_OK;
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  have = bytes;
  return CHOMP_OK;
}

// The memory space of a call's arrays: CHOMP_HOST or CHOMP_DEVICE, nothing else
// (include/chomp_mi355x.h, "Memory-space convention").
int check_mem(chomp_ctx* ctx, int mem, const char* who) {
  if (mem == CHOMP_HOST || mem == CHOMP_DEVICE) return CHOMP_OK;
  return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": mem");
}

// The array arguments of one call.  Device arrays are used in place.  Host arrays get a segment
// each, one after another on 16-byte boundaries: inputs in d_stage_in, sent by place(); outputs in
// d_stage_out, copied back by finish(), which then waits for the stream once.  A host output
// without an array (nullptr) keeps its segment but is not copied back.  place(n) also sets aside
// a scratch segment of n doubles of d_stage_in, neither sent nor copied back.
// rc: CHOMP_ERR_ARG when `mem` is neither CHOMP_HOST nor CHOMP_DEVICE; callers return it before any
// other work, and place() refuses to stage anything with it set.
struct Staging {
  template <class T>
  struct Seg { T* host; T** dev; size_t off, n; };
  chomp_ctx* ctx;
  bool host;
  int rc;
  double* scratch = nullptr;
  std::vector<Seg<const double>> ins;
  std::vector<Seg<double>> outs;
  size_t n_in = 0, n_out = 0;

  Staging(chomp_ctx* c, int mem, const char* who)
      : ctx(c), host(mem == CHOMP_HOST), rc(check_mem(c, mem, who)) {}
  static size_t take(size_t* used, size_t n) {
    const size_t off = *used;
    *used += (n + 1) & ~(size_t)1;
    return off;
  }
  // *d: the array the kernels use (for a host array: set by place())
  void in(const double* x, size_t n, const double** d) {
    *d = x;
    if (host) ins.push_back({x, d, take(&n_in, n), n});
  }
  void out(double* y, size_t n, double** d) {
    *d = y;
    if (host) outs.push_back({y, d, take(&n_out, n), n});
  }
  int place(size_t n_scratch = 0) {
    if (rc) return rc;             // (an unknown mem never takes either path)
    const size_t off_scratch = take(&n_in, n_scratch);
    if (n_in) { const int e = ensure(ctx, ctx->d_stage_in, n_in); if (e) return e; }
    if (n_out) { const int e = ensure(ctx, ctx->d_stage_out, n_out); if (e) return e; }
    for (const Seg<const double>& s : ins) {
      *s.dev = ctx->d_stage_in + s.off;
      HIPCHK(hipMemcpyAsync(ctx->d_stage_in + s.off, s.host, s.n * sizeof(double),
                            hipMemcpyHostToDevice, ctx->stream));
    }
    for (const Seg<double>& s : outs) *s.dev = ctx->d_stage_out + s.off;
    if (n_scratch) scratch = ctx->d_stage_in + off_scratch;
    return CHOMP_OK;
  }
  int finish() {
    HIPCHK(hipGetLastError());
    if (!host) return CHOMP_OK;
    for (const Seg<double>& s : outs)
      if (s.host)
        HIPCHK(hipMemcpyAsync(s.host, ctx->d_stage_out + s.off, s.n * sizeof(double),
                              hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return CHOMP_OK;
  }
};

// The 1-D grid of the element-wise kernels: a block per 256 elements, at most 1024 blocks.
dim3 grid_1d(size_t n) { return dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)); }

// erfinv(y) for y in (-1, 1): Newton on erf/erfc (used once per HOD, hod.py:172-175).
double erfinv_host(double y) {
  if (y <= -1.0) return -INFINITY;
  if (y >= 1.0) return INFINITY;
  if (y == 0.0) return 0.0;
  const double a = 0.147;
  const double ln1 = std::log1p(-y * y);
  const double t = 2.0 / (M_PI * a) + 0.5 * ln1;
  double x = std::copysign(std::sqrt(std::sqrt(t * t - ln1 / a) - t), y);
  for (int it = 0; it < 60; ++it) {
    // residual computed in the tail-accurate form
    double r;
    if (y < -0.5) r = std::erfc(-x) - (1.0 + y);
    else if (y > 0.5) r = (1.0 - y) - std::erfc(x);
    else r = std::erf(x) - y;
    const double d = 2.0 / std::sqrt(M_PI) * std::exp(-x * x);
    const double dx = r / d;
    x -= dx;
    if (std::fabs(dx) <= 1e-16 * std::fabs(x)) break;
  }
  return x;
}

// A constant table: allocated once, n elements, and filled from `src`.
template <class T>
int constant(chomp_ctx* ctx, DeviceBuffer<T>& b, const T* src, size_t n) {
  HIPCHK((hipError_t)b.once(n));
  HIPCHK(hipMemcpy(b, src, n * sizeof(T), hipMemcpyHostToDevice));
  return CHOMP_OK;
}

int setup_constants(chomp_ctx* ctx) {
  SiCiTab s;
  BesselTab j0, j2;
  fill_tables(&s, &j0, &j2);
  // (the three blocks first, then their contents: the order the context has always made them in)
  HIPCHK((hipError_t)ctx->d_sici.once(1));
  HIPCHK((hipError_t)ctx->d_j0.once(1));
  HIPCHK((hipError_t)ctx->d_j2.once(1));
  int rc = constant(ctx, ctx->d_sici, &s, 1);
  if (!rc) rc = constant(ctx, ctx->d_j0, &j0, 1);
  if (!rc) rc = constant(ctx, ctx->d_j2, &j2, 1);
  if (!rc) rc = constant(ctx, ctx->d_gl16, CHOMP_GL16, 32);
  if (rc) return rc;
  // Tinker et al. 2010 parameter table (mass_function.py:450-459), splined in
  // ln(Delta) exactly as the reference does (:461-470).
  static const double delta[9] = {200, 300, 400, 600, 800, 1200, 1600, 2400, 3200};
  static const double par[5][9] = {
      {0.368, 0.363, 0.385, 0.389, 0.393, 0.365, 0.379, 0.355, 0.327},       // alpha
      {0.589, 0.585, 0.544, 0.543, 0.564, 0.632, 0.637, 0.673, 0.702},       // beta
      {0.864, 0.922, 0.987, 1.09, 1.20, 1.34, 1.50, 1.68, 1.81},             // gamma
      {-0.729, -0.789, -0.910, -1.05, -1.20, -1.26, -1.45, -1.50, -1.49},    // phi
      {-0.243, -0.261, -0.261, -0.273, -0.278, -0.301, -0.301, -0.319, -0.336}};  // eta
  TinkerTab tt;
  double work[18];
  for (int i = 0; i < 9; ++i) tt.x[i] = std::log(delta[i]);
  for (int q = 0; q < 5; ++q) spline_build(tt.x, par[q], 9, tt.c[q], work);
  rc = constant(ctx, ctx->d_tinker, &tt, 1);
  if (rc) return rc;
  // Candidate masses of the 5 % walk (mass_function.py:161-193), generated by the
  // same repeated multiply/divide so every candidate is bit-identical to the value
  // the reference's loop would hold after j steps.
  std::vector<double> cand(4 * kSearchJ);
  const double start[4] = {1.0e9, 1.0e9, 1.0e16, 1.0e16};
  const bool mul[4] = {false, true, true, false};
  for (int t = 0; t < 4; ++t) {
    double m = start[t];
    for (int j = 0; j < kSearchJ; ++j) {
      cand[t * kSearchJ + j] = m;
      m = mul[t] ? m * 1.05 : m / 1.05;
    }
  }
  {   // level weights of the fast deep-knot sums
    const int top = ctx->cfg.divmax;
    std::vector<double> w((size_t)(top > kDeepCoarse ? top - kDeepCoarse : 1) * kDeepWStride, 0.0);
    if (top > kDeepCoarse) deep_weights_host(kDeepCoarse, top, w.data());
    rc = constant(ctx, ctx->d_deepw, w.data(), w.size());
    if (rc) return rc;
    HIPCHK((hipError_t)ctx->d_deepstat.once(8));
    HIPCHK(hipMemset(ctx->d_deepstat, 0, 8 * sizeof(int)));
  }
  if (ctx->cfg.halo_npoints >= 12) {   // (fewer points: the serial quintic solve of k_halofit_finalize)
    const int nk = ctx->cfg.halo_npoints;
    std::vector<double> ai((size_t)nk * nk);
    halofit_collocation_inverse_host(nk, ai.data());
    rc = constant(ctx, ctx->d_hf_ainv, ai.data(), ai.size());
    if (rc) return rc;
  }
  return constant(ctx, ctx->d_cand, cand.data(), cand.size());
}

int alloc_epochs(chomp_ctx* ctx, size_t n) {
  if (n <= ctx->cap_epoch) return CHOMP_OK;
  if (capturing(ctx))
    return fail(ctx, CHOMP_ERR_STATE,
                "the epoch batch would have to grow while the context's stream is being captured");
  // (every block of the batch is a new one of exactly its size; a parameter block's shadow
  //  goes with the block it described)
  auto fresh = [&](auto& b, size_t count) { return grown(ctx, b.renew(ctx->mem, count)); };
  int rc = fresh(ctx->d_cosmo, n);
  if (!rc) rc = fresh(ctx->d_z, n);
  if (!rc) rc = fresh(ctx->d_epochs, n);
  if (!rc) rc = fresh(ctx->d_search, n * 4);
  if (!rc) rc = fresh(ctx->d_probe, n * kProbeStride);
  if (!rc) rc = fresh(ctx->d_count, n);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(ctx->d_count, 0, n * sizeof(int), ctx->stream));
  rc = fresh(ctx->d_pending, pending_ints(n, ctx->L.NK));
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(ctx->d_pending, 0, kPendingHead * sizeof(int), ctx->stream));
  rc = fresh(ctx->d_endp, n * kGroups * 2 * (size_t)ctx->L.NK);
  if (!rc) rc = fresh(ctx->d_npend, n);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(ctx->d_npend, 0, n * sizeof(int), ctx->stream));
  rc = fresh(ctx->d_tab, n * (size_t)ctx->L.stride);
  if (rc) return rc;
  // (rows of the levels table and knot tables no set-up has written read back as 0, not as
  //  whatever the allocation held: the same for every context)
  HIPCHK(hipMemsetAsync(ctx->d_tab, 0, n * (size_t)ctx->L.stride * sizeof(double), ctx->stream));
  rc = fresh(ctx->d_mass_par, n);
  if (!rc) rc = fresh(ctx->d_profile, n);
  if (!rc) rc = fresh(ctx->d_hod, n);
  if (!rc) rc = fresh(ctx->d_nodes, n * kGroups * (size_t)kNodeStride);
  if (!rc) rc = fresh(ctx->d_snodes, n * (size_t)kSigmaStride);
  if (rc) return rc;
  // (holds the arrival counters of k_sigma_nodes: zero once, the kernel resets them)
  HIPCHK(hipMemsetAsync(ctx->d_snodes, 0, n * (size_t)kSigmaStride * sizeof(double), ctx->stream));
  rc = fresh(ctx->d_slot, n);
  if (!rc) rc = fresh(ctx->d_first, n);
  if (!rc) rc = fresh(ctx->d_status, n);
  if (rc) return rc;
  ctx->cap_epoch = n;
  return CHOMP_OK;
}

}  // namespace

extern "C" {

void chomp_default_config(chomp_config* c) {
  // defaults.py:42-51 and 62-92
  c->k_min = 0.001; c->k_max = 100.0; c->mass_min = -1; c->mass_max = -1;
  c->corr_precision = 1.48e-6; c->cosmo_precision = 1.48e-8; c->dNdz_precision = 1.48e-8;
  c->halo_precision = 1.48e-5; c->kernel_precision = 1.48e-6; c->mass_precision = 1.48e-8;
  c->window_precision = 1.48e-6; c->global_precision = 1.48e-32;
  c->corr_npoints = 50; c->cosmo_npoints = 50; c->halo_npoints = 50;
  c->kernel_npoints = 50; c->kernel_bessel_limit = 8; c->mass_npoints = 50;
  c->window_npoints = 100; c->divmax = 20;
}

int chomp_ctx_create(const chomp_config* cfg, int device, void* hip_stream,
                     chomp_ctx** out) {
  if (!out) return CHOMP_ERR_ARG;
  *out = nullptr;
  chomp_ctx* ctx = new chomp_ctx();
  if (cfg) ctx->cfg = *cfg; else chomp_default_config(&ctx->cfg);
  const chomp_config& c = ctx->cfg;
  // (every way out that is not success: through chomp_ctx_destroy once there is a stream, so
  //  that it and the constants go too; before that the context owns nothing on the device)
  auto leave = [&](int code) {
    if (ctx->stream) chomp_ctx_destroy(ctx); else delete ctx;
    return code;
  };
  auto bad = [&](const char* m) {
    fprintf(stderr, "chomp_ctx_create: %s\n", m);
    return leave(CHOMP_ERR_ARG);
  };
  if (c.mass_npoints < 8 || c.mass_npoints > 256) return bad("mass_npoints out of [8,256]");
  if (c.halo_npoints < 6 || c.halo_npoints > 256) return bad("halo_npoints out of [6,256]");
  if (c.kernel_npoints < 4 || c.kernel_npoints > 512) return bad("kernel_npoints");
  if (c.window_npoints < 4 || c.window_npoints > 1024) return bad("window_npoints");
  if (c.cosmo_npoints < 4 || c.cosmo_npoints > 512) return bad("cosmo_npoints");
  if (c.divmax < 1 || c.divmax > 30) return bad("divmax out of [1,30]");
  if (!(c.k_min > 0.0) || !(c.k_max > c.k_min)) return bad("k limits");
  ctx->device = device;
  ctx->L = make_layout(c.mass_npoints, c.halo_npoints);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    fprintf(stderr, "chomp_ctx_create: no usable HIP device %d (%s) -- this library has "
                    "no CPU fallback\n", device, hipGetErrorString(e));
    return leave(CHOMP_ERR_HIP);
  }
  if (hipSetDevice(device) != hipSuccess) return leave(CHOMP_ERR_HIP);
  if (hip_stream) {
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
  } else {
    if (hipStreamCreate(&ctx->stream) != hipSuccess) return leave(CHOMP_ERR_HIP);
    ctx->owns_stream = true;
  }
  int rc = setup_constants(ctx);
  if (rc != CHOMP_OK) {
    fprintf(stderr, "chomp_ctx_create: %s\n", ctx->err.c_str());
    return leave(rc);
  }
  *out = ctx;
  return CHOMP_OK;
}

// Nothing of the context is in flight once its two streams have drained (every call queues on
// one of them), so the buffers -- which free themselves with the context, after the streams it
// owns are gone -- are freed idle; hipFree does not need the stream.  A caller's stream
// (owns_stream false) is drained the same and left alone.
void chomp_ctx_destroy(chomp_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->side) (void)hipStreamSynchronize(ctx->side);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->ev_status) (void)hipEventDestroy(ctx->ev_status);
  for (hipEvent_t e : ctx->ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : {ctx->ev_side_go, ctx->ev_proj_ready, ctx->ev_side_done})
    if (e) (void)hipEventDestroy(e);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char* chomp_last_error(chomp_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int chomp_set_timing(chomp_ctx* ctx, int on) {
  if (!ctx) return CHOMP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  if (on)
    for (hipEvent_t& e : ctx->ev)
      if (!e) HIPCHK(hipEventCreate(&e));
  ctx->timing = on ? 1 : 0;
  ctx->timing_valid = false;
  return CHOMP_OK;
}

int chomp_get_timing(chomp_ctx* ctx, double* us, size_t n) {
  if (!ctx || !us || n != 3) return fail(ctx, CHOMP_ERR_ARG, "get_timing: us[3]");
  if (!ctx->timing || !ctx->timing_valid)
    return fail(ctx, CHOMP_ERR_STATE,
                "get_timing: no timed streaming chomp_power call (chomp_set_timing, large grid)");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipEventSynchronize(ctx->ev[3]));
  for (int i = 0; i < 3; ++i) {
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[i], ctx->ev[i + 1]));
    us[i] = 1e3 * (double)ms;
  }
  return CHOMP_OK;
}

int chomp_get_stream(chomp_ctx* ctx, void** out) {
  if (!ctx || !out) return CHOMP_ERR_ARG;
  *out = reinterpret_cast<void*>(ctx->stream);
  return CHOMP_OK;
}

int chomp_sync(chomp_ctx* ctx) {
  if (!ctx) return CHOMP_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  { const int rcj = proj_join(ctx); if (rcj) return rcj; }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return CHOMP_OK;
}

int chomp_set_tuning(chomp_ctx* ctx, int what, long long value) {
  if (!ctx) return CHOMP_ERR_ARG;
  // (1 and 9 are the numbers of retired knobs: refused like any unknown one)
  if (what < 0 || what >= CHOMP_TUNE_COUNT || what == 1 || what == 9)
    return fail(ctx, CHOMP_ERR_ARG, "set_tuning: unknown knob");
  ctx->tune[what] = value < 0 ? -1 : value;
  if (what == CHOMP_TUNE_ROCTX) {
    if (value > 0) {
      if (!ctx->roctx.load()) return fail(ctx, CHOMP_ERR_STATE, "set_tuning: no roctx library found");
    } else {
      ctx->roctx.push = nullptr;
    }
  }
  return CHOMP_OK;
}

int chomp_get_deep_stats(chomp_ctx* ctx, long long* out) {
  if (!ctx || !out) return fail(ctx, CHOMP_ERR_ARG, "get_deep_stats: bad args");
  HIPCHK(hipSetDevice(ctx->device));
  int v[8] = {0};
  HIPCHK(hipMemcpyAsync(v, ctx->d_deepstat, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 5; ++i) out[i] = v[i];
  float worst;
  std::memcpy(&worst, &v[5], sizeof worst);
  out[5] = (long long)((double)worst * 1e15);      // largest self-check estimate, in 1e-15
  out[6] = v[6];
  return CHOMP_OK;
}

int chomp_get_status(chomp_ctx* ctx, size_t epoch0, size_t n, unsigned* out) {
  if (!ctx || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "get_status: bad args");
  if (!ctx->have_epochs) return fail(ctx, CHOMP_ERR_STATE, "get_status before epochs_set");
  if (epoch0 + n > ctx->n_epoch) return fail(ctx, CHOMP_ERR_ARG, "get_status: epoch range");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(out, ctx->d_status + epoch0, n * sizeof(unsigned), hipMemcpyDeviceToHost,
                        ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return CHOMP_OK;
}

// The pinned host words of the status posts, large enough for the batch: h_mirror, three regions
// the finalising blocks of the halo set-ups write (sequence number << 32 | word) into in turn
// (known to the kernels through ctx->L), and h_status, where a post without a mirror is copied.
// Not under stream capture (an allocation): returns OK with the words as they are.
static int mirror_collect(chomp_ctx* ctx, int half, unsigned seq, size_t epoch0, size_t n,
                          unsigned* out);
static int ensure_hstatus(chomp_ctx* ctx) {
  if (ctx->h_status.fits(ctx->n_epoch) && ctx->h_mirror) return CHOMP_OK;
  if (capturing(ctx)) return CHOMP_OK;
  HIPCHK(hipStreamSynchronize(ctx->stream));       // (a copy or a kernel's mirror may be in flight)
  // (a post nobody has waited for yet survives the reallocation: its words are there now)
  if (ctx->posted_kind == 1 || ctx->posted_kind == 2) {
    const size_t np = ctx->n_hstatus;
    std::vector<unsigned> keep(np);
    if (ctx->posted_kind == 1) {
      const int rcc = mirror_collect(ctx, ctx->posted_half, ctx->posted_seq, 0, np, keep.data());
      if (rcc) return rcc;
    } else {
      std::memcpy(keep.data(), ctx->h_status, np * sizeof(unsigned));
    }
    ctx->posted_saved.swap(keep);
    ctx->posted_kind = 3;
  }
  const int kept_kind = ctx->posted_kind;
  const size_t kept_n = ctx->n_hstatus;
  ctx->L.h_status = nullptr;
  ctx->posted_kind = kept_kind == 3 ? 3 : 0;
  ctx->n_hstatus = kept_kind == 3 ? kept_n : 0;
  // (a graph may still write the old words: the buffers park them then)
  int rc = grown(ctx, ctx->h_status.renew(ctx->mem, ctx->n_epoch));
  if (!rc) rc = grown(ctx, ctx->h_mirror.renew(ctx->mem, 3 * ctx->n_epoch));
  if (rc) return rc;
  std::memset(ctx->h_mirror, 0, 3 * ctx->n_epoch * sizeof(unsigned long long));
  ctx->mirror_half = 0;
  ctx->mirror_region = 0;
  ctx->L.h_status = ctx->h_mirror;
  ctx->L.h_seq = 0u;
  return CHOMP_OK;
}

// The words of a mirrored post, once every one of them carries the post's sequence number
// (the set-up's finalising blocks have written them).  Spins on the pinned words; gives up with
// an error when the stream has drained and they still do not (a set-up that failed).
static int mirror_collect(chomp_ctx* ctx, int half, unsigned seq, size_t epoch0, size_t n,
                          unsigned* out) {
  const volatile unsigned long long* w = ctx->h_mirror + (size_t)half * ctx->h_status.cap() + epoch0;
  for (size_t i = 0; i < n; ++i) {
    bool drained = false;
    for (;;) {
      const unsigned long long v = w[i];
      if ((unsigned)(v >> 32) == seq) { out[i] = (unsigned)v; break; }
      if (drained)
        return fail(ctx, CHOMP_ERR_STATE, "status_wait: the posted set-up never finalised its epochs");
      if (hipStreamQuery(ctx->stream) == hipSuccess) drained = true;   // (one more look, then give up)
    }
  }
  return CHOMP_OK;
}

// In front of a halo set-up's kernels: the region its finalising blocks will mirror into and its
// sequence number.  Eager set-ups take regions 0 and 1 in turn; a post of the region about to be
// written again that nobody has waited for yet is collected first -- it is the set-up of two
// set-ups ago.  A set-up under stream capture gets region 2 and a number of its own, both fixed
// in the graph's kernel arguments: replays never write where an eager set-up's words are.
static int mirror_next(chomp_ctx* ctx) {
  if (!ctx->h_mirror) return CHOMP_OK;
  int next = 2;
  if (!capturing(ctx)) {
    next = ctx->mirror_half ^ 1;
    ctx->mirror_half = next;
  }
  if (ctx->posted_kind == 1 && ctx->posted_half == next && !capturing(ctx)) {
    ctx->posted_saved.resize(ctx->n_hstatus);
    const int rc = mirror_collect(ctx, next, ctx->posted_seq, 0, ctx->n_hstatus, ctx->posted_saved.data());
    if (rc) return rc;
    ctx->posted_kind = 3;
  }
  ctx->mirror_region = next;
  ctx->L.h_status = ctx->h_mirror + (size_t)next * ctx->h_status.cap();
  ctx->L.h_seq = ++ctx->setup_seq;
  return CHOMP_OK;
}

int chomp_status_post(chomp_ctx* ctx) {
  if (!ctx) return CHOMP_ERR_ARG;
  if (!ctx->have_epochs) return fail(ctx, CHOMP_ERR_STATE, "status_post before epochs_set");
  HIPCHK(hipSetDevice(ctx->device));
  const bool cap = capturing(ctx);
  if (cap && (ctx->n_epoch > ctx->h_status.cap() || !ctx->h_status))
    return fail(ctx, CHOMP_ERR_STATE,
                "status_post during stream capture before any eager set-up of this size (the "
                "pinned words would have to be allocated)");
  { const int rce = ensure_hstatus(ctx); if (rce) return rce; }
  if (ctx->status_mirrored) {
    // Behind a halo set-up the words are on their way already (its finalising blocks write them,
    // with the set-up's sequence number): the post puts nothing on the stream -- it names the
    // region and the number to wait for.
    ctx->posted_kind = 1;
    ctx->posted_half = ctx->mirror_region;
    ctx->posted_seq = ctx->L.h_seq;
  } else {
    if (!ctx->ev_status) {
      if (cap) return fail(ctx, CHOMP_ERR_STATE, "status_post during stream capture before any eager post");
      HIPCHK(hipEventCreateWithFlags(&ctx->ev_status, hipEventDisableTiming));
    }
    if (ctx->posted_kind == 2 && !cap && !ctx->posted_in_capture)
      HIPCHK(hipEventSynchronize(ctx->ev_status));       // (the previous copy into the same words)
    HIPCHK(hipMemcpyAsync(ctx->h_status, ctx->d_status, ctx->n_epoch * sizeof(unsigned),
                          hipMemcpyDeviceToHost, ctx->stream));
    // (under capture the copy is a node of the graph, and whoever looks at the words waits for
    //  the stream the graph was launched on, not for an event)
    if (!cap) HIPCHK(hipEventRecord(ctx->ev_status, ctx->stream));
    ctx->posted_kind = 2;
  }
  ctx->posted_in_capture = cap;
  ctx->n_hstatus = ctx->n_epoch;
  return CHOMP_OK;
}

int chomp_status_wait(chomp_ctx* ctx, size_t epoch0, size_t n, unsigned* out) {
  if (!ctx || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "status_wait: bad args");
  if (!ctx->n_hstatus || !ctx->posted_kind) return fail(ctx, CHOMP_ERR_STATE, "status_wait before status_post");
  if (epoch0 + n > ctx->n_hstatus) return fail(ctx, CHOMP_ERR_ARG, "status_wait: epoch range");
  HIPCHK(hipSetDevice(ctx->device));
  if (capturing(ctx))
    return fail(ctx, CHOMP_ERR_STATE,
                "status_wait while the context's stream is being captured (a wait on the host "
                "cannot be part of a graph): look at the status before the capture or after a replay");
  if (ctx->posted_kind == 3) {                       // (collected when its region was needed again)
    std::memcpy(out, ctx->posted_saved.data() + epoch0, n * sizeof(unsigned));
    return CHOMP_OK;
  }
  if (ctx->posted_in_capture) HIPCHK(hipStreamSynchronize(ctx->stream));
  if (ctx->posted_kind == 1) return mirror_collect(ctx, ctx->posted_half, ctx->posted_seq, epoch0, n, out);
  if (!ctx->posted_in_capture) HIPCHK(hipEventSynchronize(ctx->ev_status));
  std::memcpy(out, ctx->h_status + epoch0, n * sizeof(unsigned));
  return CHOMP_OK;
}

// -- w0-wa dark energy ----------------------------------------------------------------
// The knots of the pressure tables (cosmology.py:98-102) made as numpy makes them:
// a_i = 10 ** linspace(log10(cosmo_precision), 0, n); the tables take ln a_i, the integrals z_i =
// 1 / a_i - 1.  Sent once per context (the configuration is fixed at its creation).
static int de_knots(chomp_ctx* ctx) {
  const int n = ctx->cfg.cosmo_npoints;
  std::vector<double> k(2 * (size_t)n);
  for (int i = 0; i < n; ++i) de_knot(ctx->cfg.cosmo_precision, n, i, &k[i], &k[n + i]);
  const int rc = ensure(ctx, ctx->d_de_knots, k.size());
  if (rc) return rc;
  return upload(ctx, ctx->d_de_knots, k.data(), k.size() * sizeof(double));
}

// The tables of the distinct (w0, wa) of `keys`, queued on the context's stream -- or nothing,
// when T already holds exactly these (the reference-shaped loop sets one epoch per z up).
static int de_build(chomp_ctx* ctx, DeTables& T, const std::vector<DePar>& keys) {
  const int n = ctx->cfg.cosmo_npoints;
  const size_t nk = keys.size();
  if (T.valid && T.keys.size() == nk &&
      std::memcmp(T.keys.data(), keys.data(), nk * sizeof(DePar)) == 0)
    return CHOMP_OK;
  if (n < 4 || n > 240) return fail(ctx, CHOMP_ERR_ARG, "dark energy: cosmo_npoints must be 4..240");
  if (nk > 65535) return fail(ctx, CHOMP_ERR_ARG, "dark energy: more than 65535 distinct (w0, wa)");
  T.valid = false;
  int rc = de_knots(ctx);
  if (rc) return rc;
  rc = ensure(ctx, T.d_par, nk);
  if (rc) return rc;
  rc = ensure(ctx, T.d_tab, nk * (size_t)de_stride(n));
  if (rc) return rc;
  rc = upload(ctx, T.d_par, keys.data(), nk * sizeof(DePar));
  if (rc) return rc;
  hipLaunchKernelGGL(k_de_table, dim3((unsigned)n, (unsigned)nk), dim3(64 * kDeNW), 0, ctx->stream,
                     ctx->cfg, T.d_par, ctx->d_de_knots, T.d_tab);
  hipLaunchKernelGGL(k_de_spline, dim3((unsigned)nk), dim3(64), (size_t)(11 * n) * sizeof(double),
                     ctx->stream, ctx->cfg, T.d_tab);
  HIPCHK(hipGetLastError());
  T.keys = keys;
  T.valid = true;
  return CHOMP_OK;
}

int chomp_set_dark_energy(chomp_ctx* ctx, int on) {
  if (!ctx) return CHOMP_ERR_ARG;
  ctx->dark_energy = on != 0;
  return CHOMP_OK;
}

int chomp_set_sets_scope(chomp_ctx* ctx, unsigned flags) {
  if (!ctx) return CHOMP_ERR_ARG;
  if (flags & ~(unsigned)(CHOMP_SETS_TABULATED | CHOMP_SETS_DARK_ENERGY))
    return fail(ctx, CHOMP_ERR_ARG, "set_sets_scope: unknown flag");
  ctx->sets_scope = flags;
  return CHOMP_OK;
}

int chomp_set_general_profile(chomp_ctx* ctx, int on) {
  if (!ctx) return CHOMP_ERR_ARG;
  ctx->general_profile = on != 0;
  return CHOMP_OK;
}

int chomp_get_de_table(chomp_ctx* ctx, int source, size_t index, int what, double* out, size_t n) {
  if (!ctx || !out) return fail(ctx, CHOMP_ERR_ARG, "get_de_table: bad args");
  const int np = ctx->cfg.cosmo_npoints;
  int off;
  size_t want = (size_t)np;
  switch (what) {
    case CHOMP_DE_LN_A: off = de_off_ln_a(np); break;
    case CHOMP_DE_PRESSURE: off = de_off_p(np); break;
    case CHOMP_DE_LEVELS: off = de_off_level(np); break;
    case CHOMP_DE_CONVERGED: off = de_off_conv(np); break;
    case CHOMP_DE_PP: off = de_off_pp(np); want = 4 * (size_t)(np - 1); break;
    default: return fail(ctx, CHOMP_ERR_ARG, "get_de_table: unknown table part");
  }
  if (n != want) return fail(ctx, CHOMP_ERR_ARG, "get_de_table: n must be cosmo_npoints (4 (cosmo_npoints - 1) for the coefficients)");
  HIPCHK(hipSetDevice(ctx->device));
  const double* src;
  if (source == CHOMP_DE_EPOCH) {
    if (!ctx->have_epochs || index >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_STATE, "get_de_table: epoch");
    if (index >= ctx->de_slot.size() || ctx->de_slot[index] < 0)
      return fail(ctx, CHOMP_ERR_STATE, "get_de_table: the epoch's cosmology has no dark energy");
    src = ctx->de_ep.d_tab + (size_t)ctx->de_slot[index] * de_stride(np);
  } else if (source == CHOMP_DE_PROJ) {
    if (!ctx->proj.me_ready || !ctx->proj.de)
      return fail(ctx, CHOMP_ERR_STATE, "get_de_table: no projection set-up with dark energy");
    { const int rcj = proj_join(ctx); if (rcj) return rcj; }
    src = ctx->de_proj.d_tab;
  } else {
    return fail(ctx, CHOMP_ERR_ARG, "get_de_table: unknown source");
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(out, src + off, n * sizeof(double), hipMemcpyDeviceToHost));
  return CHOMP_OK;
}

int chomp_epochs_set(chomp_ctx* ctx, size_t n_epoch, const chomp_cosmo* cosmo,
                     const double* z) {
  StageRange range_(ctx, "chomp:epochs_set (Stage K: sigma tables, mass-limit search)");
  if (!ctx || !cosmo || !z || n_epoch == 0) return fail(ctx, CHOMP_ERR_ARG, "epochs_set: bad args");
  for (size_t i = 0; i < n_epoch; ++i) {
    if (!ctx->dark_energy && has_dark_energy(cosmo[i].w0, cosmo[i].wa))
      return fail(ctx, CHOMP_ERR_SCOPE,
                  "w0 != -1 or wa != 0: dynamical dark energy (cosmology.py:96-104) needs "
                  "chomp_set_dark_energy(ctx, 1)");
    if (!(cosmo[i].omega_m0 > 0.0) || !(cosmo[i].h > 0.0) || !(cosmo[i].sigma_8 > 0.0))
      return fail(ctx, CHOMP_ERR_ARG, "epochs_set: omega_m0, h, sigma_8 must be > 0");
  }
  HIPCHK(hipSetDevice(ctx->device));
  int rc = alloc_epochs(ctx, n_epoch);
  if (rc) return rc;
  ctx->n_epoch = n_epoch;
  ctx->status_mirrored = false;     // (until a halo set-up of these epochs has finalised them)
  { const int rch = ensure_hstatus(ctx); if (rch) return rch; }
  ctx->have_mass = ctx->have_halo = false;
  ctx->fam_mask = 0;
  ctx->put_mask.assign(n_epoch, 0u);
  ctx->delta_b_zero = true;
  ctx->have_halofit.assign(n_epoch, 0);
  ctx->tri_built.assign(n_epoch, 0);
  ctx->tri4_built.assign(n_epoch, 0);
  ctx->prof_general.assign(n_epoch, 0);
  rc = upload(ctx, ctx->d_cosmo, cosmo, n_epoch * sizeof(chomp_cosmo));
  if (rc) return rc;
  rc = upload(ctx, ctx->d_z, z, n_epoch * sizeof(double));
  if (rc) return rc;
  // cosmology-only work (sigma node table, sigma_8 integral) is shared by the epochs of
  // one cosmology: slot = index of the first epoch with identical parameters
  // (hashed: a design of a thousand distinct cosmologies must not cost n^2 comparisons per step)
  std::vector<int> slot(n_epoch), first;
  {
    std::unordered_multimap<uint64_t, int> seen;     // hash of the parameter bytes -> slot
    seen.reserve(n_epoch * 2);
    for (size_t i = 0; i < n_epoch; ++i) {
      uint64_t h = 1469598103934665603ull;           // FNV-1a over the 10 doubles
      const unsigned char* b = reinterpret_cast<const unsigned char*>(&cosmo[i]);
      for (size_t j = 0; j < sizeof(chomp_cosmo); ++j) { h ^= b[j]; h *= 1099511628211ull; }
      int s_found = -1;
      auto range = seen.equal_range(h);
      for (auto it = range.first; it != range.second; ++it)
        if (std::memcmp(&cosmo[first[it->second]], &cosmo[i], sizeof(chomp_cosmo)) == 0) {
          s_found = it->second;
          break;
        }
      if (s_found < 0) {
        s_found = (int)first.size();
        first.push_back((int)i);
        seen.emplace(h, s_found);
      }
      slot[i] = s_found;
    }
  }
  const size_t n_slots = first.size();
  ctx->n_slots = n_slots;
  ctx->slot = slot;
  first.resize(n_epoch, 0);
  rc = upload(ctx, ctx->d_slot, slot.data(), n_epoch * sizeof(int));
  if (rc) return rc;
  rc = upload(ctx, ctx->d_first, first.data(), n_epoch * sizeof(int));
  if (rc) return rc;
  // w0-wa dark energy: one pressure table per distinct (w0, wa), epoch -> table (-1: none).  A
  // batch without dark energy queues nothing here.
  std::vector<DePar> de_keys;
  ctx->de_slot.assign(n_epoch, -1);
  if (ctx->dark_energy) {
    std::map<std::pair<double, double>, int> seen;
    for (size_t i = 0; i < n_epoch; ++i) {
      if (!has_dark_energy(cosmo[i].w0, cosmo[i].wa)) continue;
      auto it = seen.emplace(std::make_pair(cosmo[i].w0, cosmo[i].wa), (int)de_keys.size());
      if (it.second) de_keys.push_back(DePar{cosmo[i].w0, cosmo[i].wa});
      ctx->de_slot[i] = it.first->second;
    }
  }
  const bool any_de = !de_keys.empty();
  if (any_de) {
    rc = de_build(ctx, ctx->de_ep, de_keys);
    if (rc) return rc;
    rc = ensure(ctx, ctx->d_de_slot, n_epoch);
    if (rc) return rc;
    rc = upload(ctx, ctx->d_de_slot, ctx->de_slot.data(), n_epoch * sizeof(int));
    if (rc) return rc;
  }
  // (one cosmology or a few: most blocks, shortest launch; a batch of many: four nodes per
  //  thread and the ln S integrals one per wavefront -- see k_sigma_nodes)
  // (the probes as one launch -- n_epoch < 128, launch_epoch_probe -- take chi from this launch:
  //  its chi rows, one block per epoch; a large batch integrates it in its probing phase)
  const bool chi_here = n_epoch < (size_t)kProbeLargeBatch;
  rc = with_flag(ctx->with_bao, n_slots >= 16, [&](auto BAO, auto MANY) {
    constexpr int NPT = MANY ? 4 : 1;
    constexpr int gx = sigma_node_blocks<NPT>() + sigma_lns_blocks<NPT>() + sigma_gtab_blocks<NPT>();
    const unsigned gy = (unsigned)(n_slots + sigma_epoch_rows((int)n_epoch) +
                                   (chi_here ? sigma_chi_rows((int)n_epoch, gx) : 0));
    hipLaunchKernelGGL((k_sigma_nodes<BAO, NPT>), dim3(gx, gy),
                       dim3(256), 0, ctx->stream, ctx->cfg, ctx->d_cosmo, ctx->d_z, ctx->d_first,
                       ctx->d_slot, (int)n_slots, (int)n_epoch, ctx->d_epochs, ctx->d_snodes,
                       ctx->d_status, chi_here ? ctx->d_probe : nullptr);
    if (!MANY) return CHOMP_OK;
    // ... and the aiming tables behind them (the g table of a cosmology staged in LDS; the
    // instance with BAO stages none)
    const size_t shl = BAO ? 0 : (size_t)kGTabCount * sizeof(double);
    if constexpr (!BAO) {
      const int rcl = lds_opt_in(ctx, &k_sigma_lns<BAO>, (int)shl);
      if (rcl) return rcl;
    }
    hipLaunchKernelGGL(k_sigma_lns<BAO>, dim3((unsigned)n_slots), dim3(kLnsThreads), shl, ctx->stream,
                       ctx->cfg, ctx->d_cosmo, ctx->d_z, ctx->d_first, ctx->d_snodes);
    return CHOMP_OK;
  });
  if (rc) return rc;
  // (dark energy: E0(z) and its dependents -- delta_c steers the mass-limit search below)
  if (any_de)
    hipLaunchKernelGGL(k_de_epochs, dim3((unsigned)((n_epoch + 63) / 64)), dim3(64), 0, ctx->stream,
                       ctx->cfg, ctx->d_de_slot, (int)n_epoch, ctx->de_ep.d_tab, ctx->d_epochs,
                       ctx->d_status);
  // (k_epoch_probe lives in chomp_probe.hip: the one kernel that is faster WITH machine LICM --
  //  but for the probing phase of a large batch, one wavefront per probe, compiled here)
  if (n_epoch >= (size_t)kProbeLargeBatch)
    with_flag(ctx->with_bao, [&](auto BAO) {
      hipLaunchKernelGGL((k_epoch_probe<BAO, 1, 1>), dim3((unsigned)n_epoch, 2 * kProbes), dim3(64), 0,
                         ctx->stream, ctx->cfg, ctx->d_epochs, ctx->d_search, ctx->d_cand, ctx->d_snodes,
                         ctx->d_probe, ctx->d_count, ctx->d_status);
    });
  chomp::launch_epoch_probe(ctx->with_bao != 0, (unsigned)n_epoch, ctx->stream, ctx->cfg,
                            ctx->d_epochs, ctx->d_search, ctx->d_cand, ctx->d_snodes,
                            ctx->d_probe, ctx->d_count, ctx->d_status);
  if (any_de)
    hipLaunchKernelGGL(k_de_chi, dim3((unsigned)n_epoch), dim3(64), 0, ctx->stream, ctx->cfg,
                       ctx->d_de_slot, ctx->de_ep.d_tab, ctx->d_epochs);
  HIPCHK(hipGetLastError());
  ctx->have_epochs = true;
  return CHOMP_OK;
}

// Host half of a halo set-up: argument checks, the HOD-derived constants (hod.py:172-186; one
// erfinv per epoch), the parameter uploads, and the integration groups the requested
// families need.
struct HaloPlan {
  unsigned fam = 0, kmask = 0;
  int groups[4] = {-1, -1, -1, -1};
  int ng = 0;
  int want_nbar = 1;
  bool eval = false;     // some epoch's HOD has alpha != 1: the deep-level sums evaluate nodes
  bool general = false;  // some epoch's profile has alpha != -1 (chomp_set_general_profile)
  bool has_hod() const {
    return group_hod(groups[0]) || group_hod(groups[1]) || group_hod(groups[2]) ||
           group_hod(groups[3]);
  }
};
// The tagged models of n Zheng parameter sets (the entry points that predate chomp_hod_model).
static std::vector<chomp_hod_model> zheng_models(const chomp_hod_par* hod, size_t n) {
  std::vector<chomp_hod_model> m(n);
  for (size_t i = 0; i < n; ++i) {
    m[i] = chomp_hod_model{};
    m[i].kind = CHOMP_HOD_ZHENG;
    m[i].zheng = hod[i];
  }
  return m;
}
static_assert(kHodZheng == CHOMP_HOD_ZHENG && kHodMandelbaum == CHOMP_HOD_MANDELBAUM,
              "chomp_math.h's model numbers are the header's");
static_assert(PT_FS2 == CHOMP_PT_FS2 && PT_FS2_LEN == CHOMP_PT_FS2_LEN &&
                  PT_FS2_KDIFF == CHOMP_PT_FS2_KDIFF && PT_FS3 == CHOMP_PT_FS3 &&
                  PT_FS3_PARALLELOGRAM == CHOMP_PT_FS3_PARALLELOGRAM && PT_F3 == CHOMP_PT_F3 &&
                  PT_FS3_BCGS == CHOMP_PT_FS3_BCGS && PT_BISPECTRUM == CHOMP_PT_BISPECTRUM &&
                  PT_BISPECTRUM_LEN == CHOMP_PT_BISPECTRUM_LEN &&
                  PT_TRISPECTRUM == CHOMP_PT_TRISPECTRUM &&
                  PT_TRISPECTRUM_PARALLELOGRAM == CHOMP_PT_TRISPECTRUM_PARALLELOGRAM &&
                  kPtForms == CHOMP_PT_TRISPECTRUM_PARALLELOGRAM + 1,
              "chomp_pt_kernels.h's form numbers are the header's");
static int halo_prepare(chomp_ctx* ctx, const chomp_halo_par* profile, const chomp_hod_model* hod,
                        unsigned tables, HaloPlan* P) {
  const size_t n = ctx->n_epoch;
  for (size_t i = 0; i < n; ++i) {
    if (profile[i].alpha == -1.0) continue;
    if (!ctx->general_profile)
      return fail(ctx, CHOMP_ERR_SCOPE,
                  "halo alpha != -1: the general-profile transform y_general "
                  "(halo.py:491-559) is outside the hot-path scope (NFW only) unless "
                  "chomp_set_general_profile(ctx, 1)");
    // (the profile's mass integral, halo.py:887, diverges at the centre for alpha <= -3)
    // (... and profile_mass_integral is validated to 1e-13 up to alpha = 3.5: the cancellation in
    //  its second series grows with alpha, 7e-10 at alpha = 15.5)
    if (!(profile[i].alpha > -3.0) || !(profile[i].alpha <= kProfileAlphaMax))
      return fail(ctx, CHOMP_ERR_ARG, "halo_setup: alpha must lie in (-3, 3.5]");
    P->general = true;
  }
  for (size_t i = 0; i < n; ++i)
    if ((hod[i].kind != CHOMP_HOD_ZHENG && hod[i].kind != CHOMP_HOD_MANDELBAUM) ||
        hod[i].reserved != 0)
      return fail(ctx, CHOMP_ERR_ARG, "halo_setup: unknown HOD model");
  std::vector<HodDev> hd(n);
  for (size_t i = 0; i < n; ++i) {
    HodDev& d = hd[i];
    d.model = hod[i].kind;
    d.pad_ = 0;
    d.w = 0.0;
    d.M_min = 0.0;
    if (hod[i].kind == CHOMP_HOD_MANDELBAUM) {
      // hod.py:248-259: no HOD.__init__ values of its own beyond -1 (no moment zeros, no safe
      // norm: every integral over the whole nu range); sigma = 0 and alpha = 1 keep the Zheng
      // fields out of the way (alpha = 1: no node evaluation, see HaloPlan::eval)
      d.log_M_0 = hod[i].log_M_0;
      mandelbaum_constants(hod[i].log_M_0, &d.log_M_min, &d.M_min);
      d.w = hod[i].w;
      d.sigma = 0.0; d.log_M_1p = 0.0; d.alpha = 1.0;
      d.first_zero = d.second_zero = d.safe_norm = -1.0;
      continue;
    }
    const chomp_hod_par& h = hod[i].zheng;
    d.log_M_min = h.log_M_min; d.sigma = h.sigma; d.log_M_0 = h.log_M_0;
    d.log_M_1p = h.log_M_1p; d.alpha = h.alpha;
    // hod.py:172-186; the `secon_moment_zero` typo there means second_moment_zero
    // is never clamped to first_moment_zero.
    d.first_zero = std::pow(10.0, h.log_M_min +
                                      h.sigma * erfinv_host(2.0 * ctx->cfg.halo_precision - 1.0));
    d.second_zero = std::pow(10.0, h.log_M_0);
    d.safe_norm = std::pow(10.0, h.log_M_min + 1.0 * h.sigma);
    if (h.alpha != 1.0) P->eval = true;
  }
  int rcu = upload(ctx, ctx->d_profile, profile, n * sizeof(chomp_halo_par));
  if (rcu) return rcu;
  rcu = upload(ctx, ctx->d_hod, hd.data(), n * sizeof(HodDev));
  if (rcu) return rcu;
  // header bits CHOMP_T_* are (1 << F_*) by construction
  P->fam = tables & ((1u << kFamilies) - 1u);
  P->kmask = P->fam | ((tables & CHOMP_T_EXCLUSION) ? kMaskExclusion : 0u);
  P->ng = 0;
  if (P->fam & ((1u << F_HM) | (1u << F_PPMM))) P->groups[P->ng++] = 0;
  if (P->fam & ((1u << F_HG) | (1u << F_PPGM))) P->groups[P->ng++] = 1;
  if (P->fam & (1u << F_PPGG)) P->groups[P->ng++] = 2;
  if (P->fam & (1u << F_I12)) P->groups[P->ng++] = 3;
  // integrands that can run beyond the node tables (the HOD ones): one level more in the tables
  if (P->has_hod() && ctx->cfg.divmax > kNodeLevel)
    P->kmask |= kMaskDeepNodes;
  return CHOMP_OK;
}

// k_nu_table, then k_mass_nodes; plan != nullptr: the halo node tables in the same launch.
static int launch_nu_mass(chomp_ctx* ctx, int mf_kind, const HaloPlan* plan) {
  ctx->status_mirrored = false;    // (the mass function's status bits: mirrored by the halo set-up behind it, if any)
  const size_t n = ctx->n_epoch;
  const TabLayout& L = ctx->L;
  // (one cosmology or a few: epochs fastest in dispatch order, the longest integrals first;
  //  a cosmology per epoch: an epoch's masses side by side -- see k_nu_table)
  //  (the epochs as the grid's y axis: at most 65535 of them)
  const int ef = (ctx->n_slots < 16 || n > 65535) ? 1 : 0;
  // (fewer integrals than SIMDs to put them on: four wavefronts to an integral)
  ctx->have_b2 = false;
  if (ctx->second_order) {
    ctx->B2 = make_b2_layout(L.NM);
    const int rcb = ensure(ctx, ctx->d_b2, n * (size_t)ctx->B2.stride);
    if (rcb) return rcb;
  }
  with_flag(ctx->with_bao, (size_t)L.NM * n <= 512, [&](auto BAO, auto FEW) {
    constexpr int NW = FEW ? 4 : 1;
    const dim3 grid = ef ? dim3((unsigned)n, L.NM) : dim3(L.NM, (unsigned)n);
    if (ctx->second_order)      // (the sigma knots of MassFunctionSecondOrder as well)
      hipLaunchKernelGGL((k_nu_table<BAO, NW, true>), grid, dim3(64 * NW), 0, ctx->stream, ctx->cfg,
                         L, ctx->d_epochs, ctx->d_search, ctx->d_snodes, ctx->d_tab, ctx->d_status,
                         ef, ctx->d_b2, ctx->B2.stride);
    else
      hipLaunchKernelGGL((k_nu_table<BAO, NW>), grid, dim3(64 * NW), 0, ctx->stream, ctx->cfg, L,
                         ctx->d_epochs, ctx->d_search, ctx->d_snodes, ctx->d_tab, ctx->d_status, ef,
                         nullptr, 0);
  });
  const size_t sh = (size_t)mass_lds_doubles(L.NM) * sizeof(double);
  const int ng = plan && plan->ng > 0 ? plan->ng : 1;
  // (node-table chunks: as many blocks per (epoch, group) as keep the launch under ~2 blocks
  //  per CU -- below that the chip is idle anyway and each block's node loop gets shorter)
  //  (measured: twice the chunks for the tables that are one level deeper -- 1024 blocks, each
  //   repeating the mass function part, for 768 resident -- 58 against 37 us on configs[2])
  unsigned chunks = plan ? (unsigned)(512 / (n * ng)) : 1u;
  chunks = chunks < 1 ? 1 : (chunks > 12 ? 12 : chunks);
  hipLaunchKernelGGL(k_mass_nodes, dim3((unsigned)n, (unsigned)ng, chunks), dim3(256), sh, ctx->stream,
                     ctx->cfg, L, ctx->d_epochs, ctx->d_search, ctx->d_tab, ctx->d_mass_par, mf_kind,
                     ctx->d_tinker, ctx->d_gl16, plan ? 1 : 0, ctx->d_profile, ctx->d_hod,
                     ctx->d_sici, ctx->d_nodes, ctx->d_endp, plan ? plan->groups[0] : -1,
                     plan ? plan->groups[1] : -1, plan ? plan->groups[2] : -1,
                     plan ? plan->groups[3] : -1, plan ? plan->kmask : 0u, ctx->d_status, ctx->d_npend, ctx->d_pending);
  if (ctx->second_order) {
    // MassFunctionSecondOrder._normalize's third integral (mass_function.py:408-414), behind the
    // epochs' f_norm and bias_norm
    hipLaunchKernelGGL(k_mass_b2, dim3((unsigned)n), dim3(64 * kB2NW),
                       (size_t)b2_lds_doubles(L.NM) * sizeof(double), ctx->stream, ctx->cfg, L,
                       ctx->B2, ctx->d_epochs, ctx->d_tab, ctx->d_b2, ctx->d_status);
    ctx->have_b2 = true;
  }
  HIPCHK(hipGetLastError());
  return CHOMP_OK;
}

// The launches of k_halo_knots_fast in a halo set-up (launch_halo_knots): what they share, and
// one launch on the listed knots in the sample buffer's slots [lo, hi) of round `round`
// (from_eval: on the knots the lean instance handed on).
extern "C++" struct KnotsFast {
  chomp_ctx* ctx;
  const HaloPlan& P;
  size_t lds;                      // dynamic LDS of every instance
  int all_literal;
  double deep_tol;
  int max_rough, max_fine, parts;
  template <int NT, bool SELF, bool EVAL, bool LIT = false>
  int launch(unsigned grid, int round, int lo, int hi, int from_eval) const {
    if (lds > 64 * 1024) {
      const int rc = lds_opt_in(ctx, &k_halo_knots_fast<kDeepCoarse, NT, SELF, EVAL, LIT>, 80 * 1024);
      if (rc) return rc;
    }
    hipLaunchKernelGGL((k_halo_knots_fast<kDeepCoarse, NT, SELF, EVAL, LIT>), dim3(grid), dim3(NT), lds,
                       ctx->stream, ctx->cfg, ctx->L, ctx->d_epochs, ctx->d_tab, ctx->d_sici, P.groups[0],
                       P.groups[1], P.groups[2], P.groups[3], P.kmask, (int)ctx->n_epoch, ctx->d_pending, ctx->d_npend,
                       ctx->d_epochs, P.fam, ctx->d_status, ctx->d_deepw, all_literal, deep_tol, max_rough,
                       max_fine, ctx->d_deepstat, ctx->d_samples, ctx->d_psum, parts, round, lo, hi,
                       from_eval, ctx->d_plan, ctx->d_profile, ctx->d_hod);
    return CHOMP_OK;
  }
};

// The knot integrals and everything after them (k_halo_knots, k_halo_knots_fast with the
// per-epoch finalisation).
static int launch_halo_knots(chomp_ctx* ctx, const HaloPlan& P) {
  { const int rcm = mirror_next(ctx); if (rcm) return rcm; }
  const size_t n = ctx->n_epoch;
  const TabLayout& L = ctx->L;
  const int ng = P.ng > 0 ? P.ng : 1;
  // (a block per knot pair when the whole launch is a few hundred knots: one or a few epochs)
  const bool wide = (size_t)L.NK * n * ng <= 512;
  // (... single-wavefront blocks when the knots outnumber the chip's wavefront slots about twice:
  //  a finished knot then frees its slot at once -- C3 89 -> 78 us; below that, four knots to a
  //  256-thread block, whose n_bar block also keeps its four wavefronts -- C2 37 vs 39 us)
  const bool lone = !wide && (size_t)L.NK * n * ng > 4096;
  const unsigned kb = (wide || lone) ? (unsigned)L.NK : (unsigned)((L.NK + 3) / 4);
  const size_t shk = (size_t)(L.NM + 8 * (L.NM - 1) + kKnotScratch) * sizeof(double);
  // The knots of the HOD groups that do not converge within the node tables are listed; every
  // listed knot gets a slot of the sample buffer (k_halo_knots_samples fills it, k_halo_knots_fast
  // sums the knot's levels from it).  The buffer holds every knot that CAN be listed while that
  // stays under the budget; beyond it the two kernels work the list off in rounds of `slots`.
  const bool hod_groups = P.has_hod();
  const bool deep_route = hod_groups && ctx->cfg.divmax > kNodeLevel;
  size_t slots = 0;
  int rounds = 1;
  if (deep_route) {
    const size_t worst = (size_t)ng * n * (size_t)L.NK;
    const size_t budget = ((size_t)1 << 30) / ((size_t)kDeepSlot * sizeof(double));
    slots = worst < budget ? worst : budget;
    if (ctx->tune[CHOMP_TUNE_DEEP_SLOTS] > 0 && (size_t)ctx->tune[CHOMP_TUNE_DEEP_SLOTS] < slots)
      slots = (size_t)ctx->tune[CHOMP_TUNE_DEEP_SLOTS];
    if ((worst + slots - 1) / slots > (size_t)kPendingRounds)
      slots = (worst + kPendingRounds - 1) / kPendingRounds;
    rounds = (int)((worst + slots - 1) / slots);
    int rck = ensure(ctx, ctx->d_samples, slots * (size_t)kDeepSlot);
    if (rck) return rck;
    rck = ensure(ctx, ctx->d_psum, slots * (size_t)(kDeepChunks * kDeepPsum));
    if (rck) return rck;
  }
  // (a set-up of one or a few epochs -- every launch lasts as long as its slowest unit -- leaves
  //  the table at level 9; a batch, where the ~11 % of knots that converge AT level 10 would each
  //  take a slot, a sampling work item and a summing block, walks the whole table: 888 against
  //  1001 listed knots and -6.6 us per configs[2] step)
  const bool few = (size_t)L.NK * n * ng <= 768;
  const int hod_cap = few ? kHodCapLevel : kNodeLevel;
  // chomp_set_tuning: the checker (every listed knot by literal evaluation) and the two
  // thresholds at which a knot leaves the fast path by itself
  const int all_literal = ctx->tune[CHOMP_TUNE_DEEP_LITERAL] > 0 ? 1 : 0;
  const double deep_tol = ctx->tune[CHOMP_TUNE_DEEP_TOL] >= 0
                              ? (double)ctx->tune[CHOMP_TUNE_DEEP_TOL] * 1e-15 : kDeepTol;
  int max_rough = ctx->tune[CHOMP_TUNE_DEEP_MAX_BREAKS] >= 0 ? (int)ctx->tune[CHOMP_TUNE_DEEP_MAX_BREAKS]
                                                             : kDeepMaxRough;
  if (max_rough > kDeepMaxRough) max_rough = kDeepMaxRough;
  int max_fine = ctx->tune[CHOMP_TUNE_DEEP_MAX_FINE] >= 0 ? (int)ctx->tune[CHOMP_TUNE_DEEP_MAX_FINE]
                                                          : kDeepMaxFine;
  if (max_fine > kDeepMaxFine) max_fine = kDeepMaxFine;
  // (the break-point plans of the (epoch, group)s: an extra block row of k_halo_knots)
  const int want_plan = deep_route ? 1 : 0;
  if (want_plan) {
    const int rcp = ensure(ctx, ctx->d_plan, n * kGroups);
    if (rcp) return rcp;
  }
  auto knots = [&](auto KNW) {
    hipLaunchKernelGGL((k_halo_knots<KNW>), dim3((unsigned)n, kb + (P.want_nbar ? 1u : 0u) + (unsigned)want_plan, (unsigned)ng),
                       dim3(KNW == 0 ? 64 : 256), shk, ctx->stream, ctx->cfg, L, ctx->d_epochs, ctx->d_tab,
                       ctx->d_profile, ctx->d_hod, ctx->d_sici, ctx->d_nodes, ctx->d_endp,
                       P.groups[0], P.groups[1], P.groups[2], P.groups[3], P.kmask, P.want_nbar, ctx->d_pending,
                       ctx->d_npend, ctx->d_status, hod_cap, want_plan, max_rough, max_fine,
                       ctx->d_plan);
  };
  if (wide) knots(int_c<4>{}); else if (lone) knots(int_c<0>{}); else knots(int_c<1>{});
  // blocks 0..n-1 take the epochs' tokens; with integrands that can run beyond the node
  // tables (the HOD ones) enough further blocks to fill the chip draw from the list
  unsigned gd = (unsigned)n;
  if (deep_route) {
    // (as many blocks as are resident at once -- two of 256 threads or one of 512 per CU, 256
    //  CUs: a block loops over the list until it is empty, and one that starts after that only
    //  stages its tables to find nothing left)
    // (three of 256 threads -- the lean instance: 164 registers, 51 KB of LDS -- or one of 512)
    unsigned want = (unsigned)(L.NK * n * ng);
    const unsigned resident = few ? 256u : (P.eval ? 512u : 768u);
    if (want > resident) want = resident;
    if (want > gd) gd = want;
  }
  size_t shf = deep_fast_lds<kDeepCoarse>(L.NM, ctx->cfg.divmax);
  if (shf < (size_t)finalize_lds_doubles(L.NK) * sizeof(double))
    shf = (size_t)finalize_lds_doubles(L.NK) * sizeof(double);
  // (the sampling launch: a listed knot's 2^11 + 1 samples in `parts` work items -- the fewer
  //  knots there can be, the finer, so that a single epoch's handful still spreads over the chip)
  const int parts = few ? 8 : ((size_t)L.NK * n * ng <= 8192 ? 4 : 2);
  const KnotsFast fast{ctx, P, shf, all_literal, deep_tol, max_rough, max_fine, parts};
  constexpr int NT = kDeepThreads, NF = kDeepThreadsFew;
  int rc = CHOMP_OK;
  if (!hod_groups) {                // (group 0 alone: listed knots are done in the same launch)
    rc = fast.launch<NT, true, true>(gd, 0, 0, 0x7fffffff, 0);
  } else if (!deep_route) {         // (divmax within the node tables: nothing is ever listed)
    rc = few ? fast.launch<NF, false, false>(gd, 0, 0, 0, 0) : fast.launch<NT, false, false>(gd, 0, 0, 0, 0);
  } else {
    for (int r = 0; r < rounds && !rc; ++r) {
      const int lo = (int)((size_t)r * slots), hi = (int)((size_t)(r + 1) * slots);
      size_t gs = slots * (size_t)parts;
      if (gs > 1536) gs = 1536;
      hipLaunchKernelGGL((k_halo_knots_samples<kDeepCoarse>), dim3((unsigned)gs), dim3(256), 0, ctx->stream,
                         ctx->cfg, L, ctx->d_sici, P.groups[0], P.groups[1], P.groups[2], P.groups[3], P.kmask,
                         (int)n, ctx->d_pending, ctx->d_nodes, ctx->d_endp, ctx->d_samples, ctx->d_psum,
                         parts, lo, hi);
      const unsigned g = r == 0 ? gd : (gd < 512u ? gd : 512u);
      if (P.eval) {
        rc = few ? fast.launch<NF, false, true>(g < 256u ? g : 256u, r, lo, hi, 0)
                 : fast.launch<NT, false, true>(g < 512u ? g : 512u, r, lo, hi, 0);
      } else {
        // (the lean instance, and behind it ONE launch for what it hands on: the knots that
        //  need node evaluations -- few and long: 512 threads each -- and, in the last round,
        //  those that go to the literal evaluation)
        const bool last_round = r == rounds - 1;
        const unsigned ge = all_literal ? g : (g < 256u ? g : 256u);
        rc = few ? fast.launch<NF, false, false>(g, r, lo, hi, 0) : fast.launch<NT, false, false>(g, r, lo, hi, 0);
        if (!rc)
          rc = last_round ? fast.launch<NT, false, true, true>(ge, r, lo, hi, 1)
                          : fast.launch<NT, false, true>(ge, r, lo, hi, 1);
      }
    }
  }
  if (rc) return rc;
  // knots can only be handed on when some HOD Romberg may run beyond the node tables
  if (deep_route && P.eval) {       // (alpha != 1: no launch behind the fast sums that could take the list)
    // (an empty list is the rule: few blocks, each returns after one read)
    const unsigned gl = all_literal ? gd : (gd < 256u ? gd : 256u);
    hipLaunchKernelGGL((k_halo_knots_literal<NT>), dim3(gl), dim3(NT), deep_literal_lds(L.NM, L.NK),
                       ctx->stream, ctx->cfg, L, ctx->d_epochs, ctx->d_tab, ctx->d_profile, ctx->d_hod,
                       ctx->d_sici, P.groups[0], P.groups[1], P.groups[2], P.groups[3], P.kmask, (int)n, ctx->d_pending,
                       ctx->d_npend, ctx->d_epochs, P.fam, ctx->d_status, ctx->d_deepstat);
  }
  HIPCHK(hipGetLastError());
  ctx->have_halo = true;
  ctx->fam_mask |= P.fam;
  ctx->status_mirrored = ctx->L.h_status != nullptr;
  return CHOMP_OK;
}

// The halo set-up of a batch with some alpha != -1 (chomp_set_general_profile), behind the stage
// that put the epochs' halo / HOD constants into their records: the y(k, M) tables and their
// splines, the knot integrals with the literal integrands, the epochs' finalisation.  Every
// epoch of the batch goes this way, those with alpha = -1 with y_nfw inline.
static int launch_halo_general(chomp_ctx* ctx, const HaloPlan& P, const chomp_halo_par* profile) {
  { const int rcm = mirror_next(ctx); if (rcm) return rcm; }
  const size_t n = ctx->n_epoch;
  const TabLayout& L = ctx->L;
  if (n > 65535) return fail(ctx, CHOMP_ERR_ARG, "halo_setup: at most 65535 epochs with a general profile");
  ctx->PL = make_prof_layout(L.NM, L.NK);
  const ProfLayout& PL = ctx->PL;
  int rc = ensure(ctx, ctx->d_prof, n * (size_t)PL.stride);
  if (rc) return rc;
  if (P.fam) {                      // (a set-up for n_bar alone integrates no y)
    hipLaunchKernelGGL(k_y_general_table, dim3((unsigned)L.NM, (unsigned)L.NK, (unsigned)n), dim3(64), 0,
                       ctx->stream, ctx->cfg, L, PL, ctx->d_epochs, 0, ctx->d_tab, ctx->d_profile, 0, 0.0,
                       1, ctx->d_prof, ctx->d_status);
    hipLaunchKernelGGL(k_y_general_splines, dim3((unsigned)L.NK, (unsigned)n), dim3(64),
                       (size_t)(11 * L.NM) * sizeof(double), ctx->stream, L, PL, 0, ctx->d_tab,
                       ctx->d_profile, 0, 1, 0, ctx->d_prof);
  }
  const unsigned ng = (unsigned)(P.ng > 0 ? P.ng : 1);
  hipLaunchKernelGGL(k_halo_knots_general, dim3((unsigned)n, (unsigned)L.NK + 1u, ng), dim3(256),
                     (size_t)knots_general_lds_doubles(L.NM) * sizeof(double), ctx->stream, ctx->cfg, L,
                     PL, ctx->d_epochs, ctx->d_tab, ctx->d_profile, ctx->d_hod, ctx->d_sici, ctx->d_prof,
                     P.groups[0], P.groups[1], P.groups[2], P.groups[3], P.kmask, ctx->d_status);
  hipLaunchKernelGGL(k_halo_finalize_general, dim3((unsigned)n), dim3(256),
                     (size_t)finalize_lds_doubles(L.NK) * sizeof(double), ctx->stream, ctx->cfg, L,
                     ctx->d_epochs, ctx->d_tab, P.fam, ctx->d_status);
  HIPCHK(hipGetLastError());
  for (size_t i = 0; i < n; ++i) ctx->prof_general[i] = profile[i].alpha != -1.0;
  ctx->prof_built = P.fam != 0;
  ctx->have_halo = true;
  ctx->fam_mask |= P.fam;
  ctx->status_mirrored = ctx->L.h_status != nullptr;
  return CHOMP_OK;
}

// The plan of the stage in front of launch_halo_general: the epochs' constants and nothing else
// (no integration group: no node tables).
static HaloPlan constants_only(const HaloPlan& P) {
  HaloPlan Q = P;
  Q.ng = 0;
  Q.groups[0] = Q.groups[1] = Q.groups[2] = Q.groups[3] = -1;
  return Q;
}

int chomp_mass_setup(chomp_ctx* ctx, const chomp_halo_par* par, int mf_kind) {
  StageRange range_(ctx, "chomp:mass_setup (Stage K: nu table, mass function)");
  if (!ctx || !par) return fail(ctx, CHOMP_ERR_ARG, "mass_setup: bad args");
  if (!ctx->have_epochs) return fail(ctx, CHOMP_ERR_STATE, "mass_setup before epochs_set");
  if (mf_kind != CHOMP_MF_ST && mf_kind != CHOMP_MF_TINKER)
    return fail(ctx, CHOMP_ERR_ARG, "mass_setup: unknown mass function kind");
  HIPCHK(hipSetDevice(ctx->device));
  int rc = upload(ctx, ctx->d_mass_par, par, ctx->n_epoch * sizeof(chomp_halo_par));
  if (rc) return rc;
  rc = launch_nu_mass(ctx, mf_kind, nullptr);
  if (rc) return rc;
  ctx->have_mass = true;
  // Knot tables already built stay as they are (the reference's MassFunction.set_halo
  // does not reset Halo._initialized_h_m / _pp_mm, halo.py:220-235).
  return CHOMP_OK;
}

int chomp_halo_setup_hod(chomp_ctx* ctx, const chomp_halo_par* profile,
                         const chomp_hod_model* hod, unsigned tables) {
  StageRange range_(ctx, "chomp:halo_setup (Stage K: node tables, knot integrals)");
  if (!ctx || !profile || !hod) return fail(ctx, CHOMP_ERR_ARG, "halo_setup: bad args");
  if (!ctx->have_mass) return fail(ctx, CHOMP_ERR_STATE, "halo_setup before mass_setup");
  HIPCHK(hipSetDevice(ctx->device));
  HaloPlan P;
  int rc = halo_prepare(ctx, profile, hod, tables, &P);
  if (rc) return rc;
  const size_t n = ctx->n_epoch;
  const TabLayout& L = ctx->L;
  const size_t sh = (size_t)(L.NM + 8 * (L.NM - 1) + kKnotScratch) * sizeof(double);
  if (P.general) {
    hipLaunchKernelGGL(k_halo_nodes, dim3((unsigned)n, 1, 1), dim3(256), sh, ctx->stream, ctx->cfg, L,
                       ctx->d_epochs, ctx->d_tab, ctx->d_profile, ctx->d_hod, ctx->d_sici,
                       ctx->d_nodes, ctx->d_endp, -1, -1, -1, -1, 0u, ctx->d_status, ctx->d_npend,
                       ctx->d_pending);
    return launch_halo_general(ctx, P, profile);
  }
  std::fill(ctx->prof_general.begin(), ctx->prof_general.end(), 0);
  // (few epochs: the table's nodes over several blocks each)
  const unsigned ngy = (unsigned)(P.ng > 0 ? P.ng : 1);
  unsigned nchunks = (unsigned)(512 / (n * ngy));
  nchunks = nchunks < 1 ? 1 : (nchunks > 8 ? 8 : nchunks);
  hipLaunchKernelGGL(k_halo_nodes, dim3((unsigned)n, ngy, nchunks), dim3(256), sh,
                     ctx->stream, ctx->cfg, L, ctx->d_epochs, ctx->d_tab, ctx->d_profile,
                     ctx->d_hod, ctx->d_sici, ctx->d_nodes, ctx->d_endp, P.groups[0], P.groups[1],
                     P.groups[2], P.groups[3], P.kmask, ctx->d_status, ctx->d_npend, ctx->d_pending);
  return launch_halo_knots(ctx, P);
}

int chomp_stage_k_hod(chomp_ctx* ctx, const chomp_halo_par* mass_par, int mf_kind,
                      const chomp_halo_par* profile, const chomp_hod_model* hod, unsigned tables) {
  StageRange range_(ctx, "chomp:stage_k (Stage K: mass function + halo model)");
  if (!ctx || !mass_par || !profile || !hod) return fail(ctx, CHOMP_ERR_ARG, "stage_k: bad args");
  if (!ctx->have_epochs) return fail(ctx, CHOMP_ERR_STATE, "stage_k before epochs_set");
  if (mf_kind != CHOMP_MF_ST && mf_kind != CHOMP_MF_TINKER)
    return fail(ctx, CHOMP_ERR_ARG, "stage_k: unknown mass function kind");
  HIPCHK(hipSetDevice(ctx->device));
  int rc = upload(ctx, ctx->d_mass_par, mass_par, ctx->n_epoch * sizeof(chomp_halo_par));
  if (rc) return rc;
  HaloPlan P;
  rc = halo_prepare(ctx, profile, hod, tables, &P);
  if (rc) return rc;
  if (P.general) {
    const HaloPlan Q = constants_only(P);
    rc = launch_nu_mass(ctx, mf_kind, &Q);
    if (rc) return rc;
    ctx->have_mass = true;
    return launch_halo_general(ctx, P, profile);
  }
  std::fill(ctx->prof_general.begin(), ctx->prof_general.end(), 0);
  rc = launch_nu_mass(ctx, mf_kind, &P);
  if (rc) return rc;
  ctx->have_mass = true;
  return launch_halo_knots(ctx, P);
}

int chomp_halo_setup(chomp_ctx* ctx, const chomp_halo_par* profile,
                     const chomp_hod_par* hod, unsigned tables) {
  if (!ctx || !profile || !hod) return fail(ctx, CHOMP_ERR_ARG, "halo_setup: bad args");
  const std::vector<chomp_hod_model> m = zheng_models(hod, ctx->n_epoch);
  return chomp_halo_setup_hod(ctx, profile, m.data(), tables);
}

int chomp_stage_k(chomp_ctx* ctx, const chomp_halo_par* mass_par, int mf_kind,
                  const chomp_halo_par* profile, const chomp_hod_par* hod, unsigned tables) {
  if (!ctx || !mass_par || !profile || !hod) return fail(ctx, CHOMP_ERR_ARG, "stage_k: bad args");
  const std::vector<chomp_hod_model> m = zheng_models(hod, ctx->n_epoch);
  return chomp_stage_k_hod(ctx, mass_par, mf_kind, profile, m.data(), tables);
}

int chomp_set_transfer(chomp_ctx* ctx, int kind) {
  if (!ctx) return CHOMP_ERR_ARG;
  if (kind != CHOMP_TRANSFER_EH && kind != CHOMP_TRANSFER_EH_BAO)
    return fail(ctx, CHOMP_ERR_ARG, "set_transfer: unknown transfer function");
  if (ctx->with_bao != (kind == CHOMP_TRANSFER_EH_BAO)) {
    ctx->with_bao = kind == CHOMP_TRANSFER_EH_BAO;
    ctx->have_epochs = ctx->have_mass = ctx->have_halo = false;   // every table depends on T(k)
    ctx->fam_mask = 0;
    ctx->put_mask.assign(ctx->put_mask.size(), 0u);
    ctx->tri_built.assign(ctx->tri_built.size(), 0);
    ctx->tri4_built.assign(ctx->tri4_built.size(), 0);
  }
  return CHOMP_OK;
}

int chomp_hod_stats(chomp_ctx* ctx, size_t epoch0, size_t n, double* out) {
  if (!ctx || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "hod_stats: bad args");
  if (!ctx->have_halo) return fail(ctx, CHOMP_ERR_STATE, "hod_stats before halo_setup");
  if (epoch0 + n > ctx->n_epoch) return fail(ctx, CHOMP_ERR_ARG, "hod_stats: epoch range");
  HIPCHK(hipSetDevice(ctx->device));
  int rc = ensure(ctx, ctx->d_stage_out, 3 * n);
  if (rc) return rc;
  const TabLayout& L = ctx->L;
  const size_t sh = (size_t)(L.NM + 8 * (L.NM - 1) + kKnotScratch) * sizeof(double);
  hipLaunchKernelGGL(k_hod_stats, dim3(3, (unsigned)n), dim3(256), sh, ctx->stream, ctx->cfg, L,
                     ctx->d_epochs, (int)epoch0, ctx->d_tab, ctx->d_profile, ctx->d_hod,
                     ctx->d_sici, ctx->d_stage_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, ctx->d_stage_out, 3 * n * sizeof(double), hipMemcpyDeviceToHost,
                        ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return CHOMP_OK;
}

// ssc: the caller serves the super-sample codes (chomp_power / chomp_power_range; the projections
// take the spectra of Halo / HaloFit only).
static int check_power(chomp_ctx* ctx, int which, size_t epoch0, size_t n, bool ssc = false) {
  if (!ctx) return CHOMP_ERR_ARG;
  if (!ctx->have_epochs) return fail(ctx, CHOMP_ERR_STATE, "power before epochs_set");
  if (epoch0 + n > ctx->n_epoch || n == 0) return fail(ctx, CHOMP_ERR_ARG, "power: epoch range");
  const int w = which & 15;
  const bool hf = (which & CHOMP_P_HALOFIT) != 0;
  const bool w_ssc = w == CHOMP_P_SSC_RESPONSE || w == CHOMP_P_MM_SSC;
  if (w < CHOMP_P_LIN || w > (ssc ? CHOMP_P_MM_SSC : CHOMP_P_GG)) return fail(ctx, CHOMP_ERR_ARG, "power: unknown spectrum");
  if (hf && w == CHOMP_P_LIN) return fail(ctx, CHOMP_ERR_ARG, "power: halofit|lin");
  // HaloSuperSampleCovariance is a Halo that never extrapolates (halo.py:1102-1108) and no HaloFit
  if (w_ssc && (which & (CHOMP_P_HALOFIT | CHOMP_P_EXTRAPOLATE)))
    return fail(ctx, CHOMP_ERR_ARG, "power: the super-sample spectra take no HALOFIT / EXTRAPOLATE");
  unsigned need = 0;
  if (w_ssc) need = (1u << F_HM) | (1u << F_PPMM) | (1u << F_I12);
  if (w == CHOMP_P_MM && !hf) need = (1u << F_HM) | (1u << F_PPMM);
  if (w == CHOMP_P_GM) need = (1u << F_HM) | (1u << F_HG) | (1u << F_PPGM);
  if (w == CHOMP_P_GG) need = (1u << F_HG) | (1u << F_PPGG);
  // (a set-up builds a family for every epoch; chomp_put_table for the one epoch it is given)
  if ((ctx->fam_mask & need) != need)
    for (size_t i = epoch0; i < epoch0 + n; ++i)
      if (((ctx->fam_mask | ctx->put_mask[i]) & need) != need)
        return fail(ctx, CHOMP_ERR_STATE, "power: knot tables of this spectrum were not built "
                                          "(chomp_halo_setup families, or chomp_put_table) for "
                                          "every epoch of the range");
  if (hf)
    for (size_t i = epoch0; i < epoch0 + n; ++i)
      if (!ctx->have_halofit[i])
        return fail(ctx, CHOMP_ERR_STATE, "power: chomp_halofit_setup not called for epoch");
  return CHOMP_OK;
}

// Halo(extrapolate=True): refresh the constants of the continuation above k_max for the
// epochs about to be evaluated (cheap: one 64-thread block per epoch).
static int prepare_extrapolation(chomp_ctx* ctx, int which, size_t epoch0, size_t n) {
  const int w = which & 15;
  if (!(which & CHOMP_P_EXTRAPOLATE) || (which & CHOMP_P_HALOFIT) || w == CHOMP_P_LIN)
    return CHOMP_OK;
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_power_extrap<BAO>, dim3((unsigned)n), dim3(64), 0, ctx->stream, ctx->cfg,
                       ctx->L, ctx->d_epochs, ctx->d_tab, w, (int)epoch0);
  });
  HIPCHK(hipGetLastError());
  return CHOMP_OK;
}

// k_power_prep of the streaming shape: the k-only table (d_ktab, d_winfo) and the list of k
// groups for the per-lane pass (d_slow, through counter *parity).
static int stage_e_prep(chomp_ctx* ctx, size_t epoch0, int w, const double* dk, size_t nk,
                        int* parity) {
  const TabLayout& L = ctx->L;
  const unsigned gx = (unsigned)((nk + 511) / 512);
  const size_t groups = (nk + 127) / 128;
  // k groups that cannot take the streaming kernel go on a compact list for the per-lane
  // pass.  Its counters ping-pong on a host-side parity bit (a launch appends through one
  // and clears the other for the next streaming call).  A call captured into a HIP graph
  // would replay ONE parity for ever and run its counter past the list, so under capture
  // the call clears both counters itself (a memset node) and keeps the bit still.
  bool fresh = false;
  int rc = ensure(ctx, ctx->d_slow, groups + 2, &fresh);
  if (rc) return rc;
  if (fresh)                                     // fresh buffer: clear both counters
    HIPCHK(hipMemsetAsync(ctx->d_slow, 0, 2 * sizeof(int), ctx->stream));
  *parity = ctx->slow_parity;
  if (capturing(ctx)) ctx->slow_by_memset = true;
  if (ctx->slow_by_memset) {     // (sticky: a graph may be replayed between any two calls)
    HIPCHK(hipMemsetAsync(ctx->d_slow, 0, 2 * sizeof(int), ctx->stream));
    *parity = 0;
  } else {
    ctx->slow_parity ^= 1;
  }
  const unsigned gx8 = (gx + 7) / 8 * 8;
  rc = ensure(ctx, ctx->d_winfo, (size_t)gx8 * 4);
  if (rc) return rc;
  rc = ensure(ctx, ctx->d_ktab, (size_t)gx8 * 1024);
  if (rc) return rc;
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_power_prep<BAO>, dim3(gx8), dim3(256), 0, ctx->stream, ctx->cfg, L,
                       ctx->d_epochs, (int)epoch0, w, dk, nk, ctx->d_ktab, ctx->d_winfo,
                       ctx->d_slow, *parity);
  });
  HIPCHK(hipGetLastError());
  return CHOMP_OK;
}

// The per-epoch delta_b buffer, cleared if chomp_epochs_set has been called since it was last
// written.
static int ensure_delta_b(chomp_ctx* ctx) {
  bool fresh = false;
  const int rc = ensure(ctx, ctx->d_delta_b, ctx->n_epoch, &fresh);
  if (rc) return rc;
  if (ctx->delta_b_zero || fresh) {
    HIPCHK(hipMemsetAsync(ctx->d_delta_b, 0, ctx->d_delta_b.cap() * sizeof(double), ctx->stream));
    ctx->delta_b_zero = false;
  }
  return CHOMP_OK;
}

int chomp_set_delta_b(chomp_ctx* ctx, size_t epoch0, size_t n, const double* delta_b, int mem) {
  if (!ctx || !delta_b || n == 0) return fail(ctx, CHOMP_ERR_ARG, "set_delta_b: bad args");
  int rc = check_mem(ctx, mem, "set_delta_b");
  if (rc) return rc;
  if (!ctx->have_epochs) return fail(ctx, CHOMP_ERR_STATE, "set_delta_b before epochs_set");
  if (epoch0 + n > ctx->n_epoch) return fail(ctx, CHOMP_ERR_ARG, "set_delta_b: epoch range");
  HIPCHK(hipSetDevice(ctx->device));
  rc = ensure_delta_b(ctx);
  if (rc) return rc;
  if (mem == CHOMP_DEVICE) {
    HIPCHK(hipMemcpyAsync(ctx->d_delta_b + epoch0, delta_b, n * sizeof(double),
                          hipMemcpyDeviceToDevice, ctx->stream));
  } else {
    // (through the pinned staging pair, no host synchronisation; every call uploads -- the
    //  shadow cannot know what chomp_epochs_set has cleared since)
    ctx->sh_delta_b.reset();
    rc = upload(ctx, ctx->d_delta_b + epoch0, delta_b, n * sizeof(double), ctx->sh_delta_b);
    if (rc) return rc;
  }
  return CHOMP_OK;
}

static bool plan_matches(chomp_ctx* ctx, size_t epoch0, const double* dk, size_t nk) {
  const chomp_ctx::PowerPlan& P = ctx->plan;
  if (!P.valid || P.k != dk || P.nk != nk || P.bao != ctx->with_bao) return false;
  if (ctx->d_cosmo.sh.shadow.size() < (epoch0 + 1) * sizeof(chomp_cosmo)) return false;
  return std::memcmp(&P.cosmo, ctx->d_cosmo.sh.shadow.data() + epoch0 * sizeof(chomp_cosmo),
                     sizeof(chomp_cosmo)) == 0;
}

int chomp_power_plan(chomp_ctx* ctx, size_t epoch0, const double* k, size_t nk) {
  if (!ctx || !k || nk == 0) return fail(ctx, CHOMP_ERR_ARG, "power_plan: bad args");
  if (!ctx->have_epochs || epoch0 >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_STATE, "power_plan: epoch");
  if (nk % 2 != 0 || reinterpret_cast<uintptr_t>(k) % 16 != 0)
    return fail(ctx, CHOMP_ERR_ARG, "power_plan: k must be 16-byte aligned with an even length");
  HIPCHK(hipSetDevice(ctx->device));
  ctx->plan.valid = false;
  int parity = 0;
  int rc = stage_e_prep(ctx, epoch0, CHOMP_P_MM, k, nk, &parity);
  if (rc) return rc;
  int n_slow = 0;
  HIPCHK(hipMemcpyAsync(&n_slow, ctx->d_slow + parity, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->plan.k = k;
  ctx->plan.nk = nk;
  std::memcpy(&ctx->plan.cosmo, ctx->d_cosmo.sh.shadow.data() + epoch0 * sizeof(chomp_cosmo),
              sizeof(chomp_cosmo));
  ctx->plan.bao = ctx->with_bao;
  ctx->plan.parity = parity;
  ctx->plan.n_slow = n_slow;
  ctx->plan.valid = true;
  return CHOMP_OK;
}

int chomp_power_range(chomp_ctx* ctx, int which, size_t epoch0, size_t n, const double* k,
                      size_t nk, double* out, int mem) {
  StageRange range_(ctx, "chomp:power (Stage E)");
  int rc = check_power(ctx, which, epoch0, n, true);
  if (rc) return rc;
  if (!k || !out || nk == 0) return fail(ctx, CHOMP_ERR_ARG, "power: null buffer");
  rc = check_mem(ctx, mem, "power");
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  const bool ssc = (which & 15) == CHOMP_P_SSC_RESPONSE || (which & 15) == CHOMP_P_MM_SSC;
  if (ssc) {
    rc = ensure_delta_b(ctx);
    if (rc) return rc;
  }
  rc = prepare_extrapolation(ctx, which, epoch0, n);
  if (rc) return rc;
  const bool extrap = (which & CHOMP_P_EXTRAPOLATE) && !(which & CHOMP_P_HALOFIT);
  const double* dk = k;
  double* dout = out;
  if (mem == CHOMP_HOST) {
    rc = ensure(ctx, ctx->d_stage_out, nk * n);
    if (rc) return rc;
    // through pinned mirrors: a pageable buffer would be staged by the runtime in small
    // synchronous pieces (no refusal of their own under capture: d_stage_out has made it)
    if (!ctx->h_stage_in.fits(nk)) rc = grown(ctx, ctx->h_stage_in.renew(ctx->mem, nk));
    if (rc) return rc;
    if (!ctx->h_stage_out.fits(nk * n)) rc = grown(ctx, ctx->h_stage_out.renew(ctx->mem, nk * n));
    if (rc) return rc;
    // The reference-shaped loop asks for the same k array at every redshift: the device copy of
    // the last host k grid is kept (a buffer of its own; 32 KB compared in ~1 us) and the upload
    // -- which would sit behind the set-up on the stream, in front of the evaluation -- skipped.
    bool moved = false;
    rc = ensure(ctx, ctx->d_kcache, nk, &moved);
    if (rc) return rc;
    if (moved) ctx->kcache_shadow.clear();
    if (ctx->kcache_shadow.size() != nk ||
        std::memcmp(ctx->kcache_shadow.data(), k, nk * sizeof(double)) != 0) {
      if (capturing(ctx))
        return fail(ctx, CHOMP_ERR_STATE, "power: a new host k grid while the stream is being captured");
      std::memcpy(ctx->h_stage_in, k, nk * sizeof(double));
      HIPCHK(hipMemcpyAsync(ctx->d_kcache, ctx->h_stage_in, nk * sizeof(double),
                            hipMemcpyHostToDevice, ctx->stream));
      ctx->kcache_shadow.assign(k, k + nk);
    }
    dk = ctx->d_kcache;
    dout = ctx->d_stage_out;
  }
  const TabLayout& L = ctx->L;
  if ((which & CHOMP_P_HALOFIT) == 0 &&
      (reinterpret_cast<uintptr_t>(dk) % 16 == 0) && (reinterpret_cast<uintptr_t>(dout) % 16 == 0)) {
    const unsigned gx = (unsigned)((nk + 511) / 512);
    bool one_cosmology = true;
    for (size_t i = 1; i < n; ++i) one_cosmology &= ctx->slot[epoch0 + i] == ctx->slot[epoch0];
    const int w = which & 15;
    size_t stream_min = (size_t)1 << 22;           // samples; below this the launches dominate
    // (chomp_set_tuning: the tests force either launch shape on small grids)
    if (ctx->tune[CHOMP_TUNE_E_STREAM_MIN] >= 0) stream_min = (size_t)ctx->tune[CHOMP_TUNE_E_STREAM_MIN];
    if (one_cosmology && w != CHOMP_P_LIN && nk % 2 == 0 && nk * n >= stream_min) {
      int parity = 0;
      bool lanes_needed = true;
      // (a k grid registered with chomp_power_plan keeps its k-only table: no prep launch)
      const bool planned = mem == CHOMP_DEVICE && plan_matches(ctx, epoch0, dk, nk);
      const bool timed = ctx->timing != 0;
      ctx->timing_valid = false;
      if (timed) HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
      if (planned) {
        parity = ctx->plan.parity;
        lanes_needed = ctx->plan.n_slow != 0;
      } else {
        ctx->plan.valid = false;                   // (this call overwrites the table)
        rc = stage_e_prep(ctx, epoch0, w, dk, nk, &parity);
        if (rc) return rc;
      }
      if (timed) HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
      const unsigned gx8 = (gx + 7) / 8 * 8;
      // (two rows per block of the streaming kernel where the rows pair up: measured best on MI355X)
      with_flag(n % 2 == 0, ssc, [&](auto PAIRS, auto SSC) {
        constexpr int PER = PAIRS ? 2 : 1;
        hipLaunchKernelGGL((k_power_stream<PER, SSC>), dim3(gx8, (unsigned)(n / PER)), dim3(256), 0,
                           ctx->stream, L, ctx->d_tab, w, (int)epoch0, ctx->d_ktab, ctx->d_winfo, nk,
                           dout, ctx->d_delta_b);
      });
      if (timed) {
        HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
        ctx->timing_valid = true;
      }
      // per-lane pass over the listed k groups (a planned grid knows whether it has any)
      if (lanes_needed)
        with_flag(ctx->with_bao, ssc, [&](auto BAO, auto SSC) {
          hipLaunchKernelGGL((k_power_grid_lanes<BAO, SSC>), dim3(1024), dim3(256), 0, ctx->stream,
                             ctx->cfg, L, ctx->d_epochs, ctx->d_tab, w, extrap, (int)epoch0, (int)n,
                             dk, nk, dout, ctx->d_slow, parity, ctx->d_delta_b);
        });
    } else {
      // enough blocks to fill 256 CUs: split the epochs over blockIdx.y when nk is small
      unsigned gy = (2048 + gx - 1) / gx;
      if (gy > n) gy = (unsigned)n;
      const int epy = (int)((n + gy - 1) / gy);
      gy = (unsigned)((n + epy - 1) / epy);
      with_flag(ctx->with_bao, ssc, [&](auto BAO, auto SSC) {
        hipLaunchKernelGGL((k_power_grid<BAO, SSC>), dim3(gx, gy), dim3(256), 0, ctx->stream, ctx->cfg,
                           L, ctx->d_epochs, ctx->d_tab, w, (int)epoch0, (int)n, epy, dk, nk, dout,
                           extrap, ctx->d_delta_b);
      });
    }
    if (ctx->timing_valid) HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
  } else {
    unsigned gx = (unsigned)((nk + 255) / 256);
    if (gx > 2048) gx = 2048;
    const size_t sh = (size_t)(12 * (L.NK - 1)) * sizeof(double);
    with_flag(ctx->with_bao, [&](auto BAO) {
      hipLaunchKernelGGL(k_power<BAO>, dim3(gx, (unsigned)n), dim3(256), sh, ctx->stream, ctx->cfg,
                         L, ctx->d_epochs, ctx->d_tab, which, (int)epoch0, dk, nk, dout,
                         ctx->d_delta_b);
    });
  }
  HIPCHK(hipGetLastError());
  if (mem == CHOMP_HOST) {
    HIPCHK(hipMemcpyAsync(ctx->h_stage_out, dout, nk * n * sizeof(double), hipMemcpyDeviceToHost,
                          ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::memcpy(out, ctx->h_stage_out, nk * n * sizeof(double));
  }
  return CHOMP_OK;
}

int chomp_power(chomp_ctx* ctx, int which, const double* k, size_t nk, double* out, int mem) {
  if (!ctx) return CHOMP_ERR_ARG;
  return chomp_power_range(ctx, which, 0, ctx->n_epoch, k, nk, out, mem);
}

int chomp_sigma_r(chomp_ctx* ctx, size_t epoch, const double* scale, size_t n, double* out) {
  if (!ctx || !scale || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "sigma_r: bad args");
  if (!ctx->have_epochs || epoch >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_STATE, "sigma_r: epoch");
  HIPCHK(hipSetDevice(ctx->device));
  Staging st(ctx, CHOMP_HOST, "sigma_r");
  const double* d_scale;
  double* d_out;
  st.in(scale, n, &d_scale);
  st.out(out, n, &d_out);
  const int rc = st.place();
  if (rc) return rc;
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_sigma_r<BAO>, dim3((unsigned)n), dim3(256), 0, ctx->stream, ctx->cfg,
                       ctx->d_epochs, (int)epoch, d_scale, ctx->d_snodes, d_out);
  });
  return st.finish();
}

int chomp_y_nfw(chomp_ctx* ctx, size_t epoch, const double* ln_k, const double* mass, size_t n,
                double* out) {
  if (!ctx || !ln_k || !mass || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "y_nfw: bad args");
  if (!ctx->have_halo || epoch >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_STATE, "y_nfw before halo_setup");
  HIPCHK(hipSetDevice(ctx->device));
  Staging st(ctx, CHOMP_HOST, "y_nfw");
  const double *d_ln_k, *d_mass;
  double* d_out;
  st.in(ln_k, n, &d_ln_k);
  st.in(mass, n, &d_mass);
  st.out(out, n, &d_out);
  const int rc = st.place();
  if (rc) return rc;
  hipLaunchKernelGGL(k_y_nfw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                     ctx->d_epochs, (int)epoch, ctx->d_sici, d_ln_k, d_mass, (int)n, d_out);
  return st.finish();
}

// The context's general-profile buffer for the current batch (a set-up with alpha != -1 has made
// it; an NFW-only one has not).
static int ensure_prof(chomp_ctx* ctx) {
  ctx->PL = make_prof_layout(ctx->L.NM, ctx->L.NK);
  return ensure(ctx, ctx->d_prof, ctx->n_epoch * (size_t)ctx->PL.stride);
}

int chomp_y_general(chomp_ctx* ctx, size_t epoch, double ln_k, const double* mass, size_t n,
                    double* out) {
  if (!ctx || !mass || !out || n == 0 || n > (size_t)INT32_MAX)
    return fail(ctx, CHOMP_ERR_ARG, "y_general: bad args");
  if (!ctx->have_halo || epoch >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_STATE, "y_general before halo_setup");
  HIPCHK(hipSetDevice(ctx->device));
  int rc = ensure_prof(ctx);
  if (rc) return rc;
  Staging st(ctx, CHOMP_HOST, "y_general");
  const double* d_mass;
  double* d_out;
  st.in(mass, n, &d_mass);
  st.out(out, n, &d_out);
  rc = st.place();
  if (rc) return rc;
  const TabLayout& L = ctx->L;
  const ProfLayout& PL = ctx->PL;
  // (the table of _initialize_y_spline at this ln k -- the epoch's scratch row -- and its spline)
  hipLaunchKernelGGL(k_y_general_table, dim3((unsigned)L.NM, 1, 1), dim3(64), 0, ctx->stream, ctx->cfg,
                     L, PL, ctx->d_epochs, (int)epoch, ctx->d_tab, ctx->d_profile, L.NK, ln_k, 0,
                     ctx->d_prof, ctx->d_status);
  hipLaunchKernelGGL(k_y_general_splines, dim3(1, 1), dim3(64), (size_t)(11 * L.NM) * sizeof(double),
                     ctx->stream, L, PL, (int)epoch, ctx->d_tab, ctx->d_profile, L.NK, 0, 0, ctx->d_prof);
  hipLaunchKernelGGL(k_y_general_eval, grid_1d(n), dim3(256), (size_t)(5 * L.NM - 4) * sizeof(double),
                     ctx->stream, L, PL, ctx->d_epochs, (int)epoch, ctx->d_tab, ctx->d_prof, L.NK,
                     d_mass, (int)n, d_out);
  return st.finish();
}

int chomp_y_general_table(chomp_ctx* ctx, size_t epoch, double* out_y, double* out_level) {
  if (!ctx || (!out_y && !out_level)) return fail(ctx, CHOMP_ERR_ARG, "y_general_table: bad args");
  if (!ctx->have_halo || epoch >= ctx->n_epoch || !ctx->prof_general[epoch] || !ctx->prof_built)
    return fail(ctx, CHOMP_ERR_STATE, "y_general_table: the last halo set-up built no general-profile "
                                      "table for this epoch (alpha = -1, or no chomp_set_general_profile)");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const ProfLayout& PL = ctx->PL;
  const size_t nn = (size_t)PL.NK * PL.NM;
  const double* b = ctx->d_prof + epoch * (size_t)PL.stride;
  if (out_y) HIPCHK(hipMemcpy(out_y, b + PL.off_y, nn * sizeof(double), hipMemcpyDeviceToHost));
  if (out_level) HIPCHK(hipMemcpy(out_level, b + PL.off_level, nn * sizeof(double), hipMemcpyDeviceToHost));
  return CHOMP_OK;
}

int chomp_halo_normalization(chomp_ctx* ctx, size_t epoch, const double* mass, size_t n, double* out) {
  if (!ctx || !mass || !out || n == 0 || n > (size_t)INT32_MAX)
    return fail(ctx, CHOMP_ERR_ARG, "halo_normalization: bad args");
  if (!ctx->have_halo || epoch >= ctx->n_epoch)
    return fail(ctx, CHOMP_ERR_STATE, "halo_normalization before halo_setup");
  HIPCHK(hipSetDevice(ctx->device));
  int rc = ensure_prof(ctx);
  if (rc) return rc;
  Staging st(ctx, CHOMP_HOST, "halo_normalization");
  const double* d_mass;
  double* d_out;
  st.in(mass, n, &d_mass);
  st.out(out, n, &d_out);
  rc = st.place();
  if (rc) return rc;
  const TabLayout& L = ctx->L;
  const ProfLayout& PL = ctx->PL;
  hipLaunchKernelGGL(k_halo_normalization_knots, dim3(1), dim3(64), 0, ctx->stream, L, PL, ctx->d_epochs,
                     (int)epoch, ctx->d_tab, ctx->d_profile, ctx->d_prof);
  hipLaunchKernelGGL(k_y_general_splines, dim3(1, 1), dim3(64), (size_t)(11 * L.NM) * sizeof(double),
                     ctx->stream, L, PL, (int)epoch, ctx->d_tab, ctx->d_profile, 0, 0, 1, ctx->d_prof);
  hipLaunchKernelGGL(k_halo_normalization_eval, grid_1d(n), dim3(256),
                     (size_t)(5 * L.NM - 4) * sizeof(double), ctx->stream, L, PL, (int)epoch, ctx->d_tab,
                     ctx->d_prof, d_mass, (int)n, d_out);
  return st.finish();
}

int chomp_eval(chomp_ctx* ctx, size_t epoch, int what, const double* x, size_t n, double* out,
               int mem) {
  if (!ctx || !x || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "eval: bad args");
  Staging st(ctx, mem, "eval");
  if (st.rc) return st.rc;
  if (what < 0 || what > CHOMP_EV_SIGMA_OF_NU) return fail(ctx, CHOMP_ERR_ARG, "eval: unknown function");
  if (!ctx->have_epochs || epoch >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_STATE, "eval: epoch");
  const bool second = what == CHOMP_EV_BIAS_2_NU || what == CHOMP_EV_SIGMA_OF_NU;
  const bool needs_mass = what <= CHOMP_EV_BIAS_NU || second;
  const bool needs_halo = what >= CHOMP_EV_HOD_FIRST && what <= CHOMP_EV_CONCENTRATION;
  if (needs_mass && !ctx->have_mass) return fail(ctx, CHOMP_ERR_STATE, "eval before mass_setup");
  if (needs_halo && !ctx->have_halo) return fail(ctx, CHOMP_ERR_STATE, "eval before halo_setup");
  if (second && !ctx->have_b2)
    return fail(ctx, CHOMP_ERR_STATE, "eval: the last mass set-up was not second-order "
                                      "(chomp_set_second_order)");
  HIPCHK(hipSetDevice(ctx->device));
  const double* dx;
  double* dout;
  st.in(x, n, &dx);
  st.out(out, n, &dout);
  const int rc = st.place();
  if (rc) return rc;
  const TabLayout& L = ctx->L;
  const size_t sh = (size_t)(L.NM + 8 * (L.NM - 1)) * sizeof(double);
  if (second)
    hipLaunchKernelGGL(k_eval_b2, grid_1d(n), dim3(256), (size_t)(L.NM + 4 * (L.NM - 1)) * sizeof(double),
                       ctx->stream, L, ctx->B2, ctx->d_epochs, (int)epoch, ctx->d_tab, ctx->d_b2,
                       what, dx, (int)n, dout);
  else
    hipLaunchKernelGGL(k_eval, grid_1d(n), dim3(256), sh, ctx->stream, L, ctx->d_epochs, (int)epoch,
                       ctx->d_tab, what, dx, (int)n, dout);
  return st.finish();
}

int chomp_set_second_order(chomp_ctx* ctx, int on) {
  if (!ctx) return CHOMP_ERR_ARG;
  ctx->second_order = on != 0;
  return CHOMP_OK;
}

int chomp_get_second_order(chomp_ctx* ctx, size_t epoch, double* out, size_t n) {
  if (!ctx || !out) return fail(ctx, CHOMP_ERR_ARG, "get_second_order: bad args");
  if (!ctx->have_mass || !ctx->have_b2 || epoch >= ctx->n_epoch)
    return fail(ctx, CHOMP_ERR_STATE, "get_second_order: no second-order mass set-up of this epoch");
  const int NM = ctx->L.NM;
  if (n != (size_t)NM + 3) return fail(ctx, CHOMP_ERR_ARG, "get_second_order: length mismatch");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const double* b = ctx->d_b2 + epoch * (size_t)ctx->B2.stride;
  HIPCHK(hipMemcpy(out, b + ctx->B2.off_sigma, NM * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out + NM, b + ctx->B2.off_sc, 3 * sizeof(double), hipMemcpyDeviceToHost));
  return CHOMP_OK;
}

int chomp_pt_eval(chomp_ctx* ctx, int form, size_t epoch0, size_t n_epoch, const double* args,
                  size_t n, double* out, int mem) {
  StageRange range_(ctx, "chomp:pt_eval");
  if (!ctx || !args || !out || n == 0 || n_epoch == 0) return fail(ctx, CHOMP_ERR_ARG, "pt_eval: bad args");
  if (form < 0 || form >= kPtForms) return fail(ctx, CHOMP_ERR_ARG, "pt_eval: unknown form");
  Staging st(ctx, mem, "pt_eval");
  if (st.rc) return st.rc;
  if (!ctx->have_epochs) return fail(ctx, CHOMP_ERR_STATE, "pt_eval before epochs_set");
  if (epoch0 + n_epoch > ctx->n_epoch || n_epoch > 65535)
    return fail(ctx, CHOMP_ERR_ARG, "pt_eval: epoch range");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t na = (size_t)pt_arity(form);
  const double* dargs;
  double* dout;
  st.in(args, n * na, &dargs);
  st.out(out, n * n_epoch, &dout);
  const int rc = st.place();
  if (rc) return rc;
  // (a grid-stride loop: about 4096 blocks over the whole launch -- 16 per CU -- with the epochs
  //  as the y axis, so that a block stages its epoch once and then streams configurations)
  size_t gx = (n + kPtThreads - 1) / kPtThreads;
  size_t cap = 4096 / n_epoch;
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  const dim3 grid((unsigned)gx, (unsigned)n_epoch);
  with_flag(ctx->with_bao, [&](auto BAO) {
    auto go = [&](auto F) {
      hipLaunchKernelGGL((k_pt<BAO, decltype(F)::value>), grid, dim3(kPtThreads), 0, ctx->stream,
                         ctx->d_epochs, (int)epoch0, dargs, n, dout);
    };
    switch (form) {
      case PT_FS2: go(int_c<PT_FS2>{}); break;
      case PT_FS2_LEN: go(int_c<PT_FS2_LEN>{}); break;
      case PT_FS2_KDIFF: go(int_c<PT_FS2_KDIFF>{}); break;
      case PT_FS3: go(int_c<PT_FS3>{}); break;
      case PT_FS3_PARALLELOGRAM: go(int_c<PT_FS3_PARALLELOGRAM>{}); break;
      case PT_F3: go(int_c<PT_F3>{}); break;
      case PT_FS3_BCGS: go(int_c<PT_FS3_BCGS>{}); break;
      case PT_BISPECTRUM: go(int_c<PT_BISPECTRUM>{}); break;
      case PT_BISPECTRUM_LEN: go(int_c<PT_BISPECTRUM_LEN>{}); break;
      case PT_TRISPECTRUM: go(int_c<PT_TRISPECTRUM>{}); break;
      default: go(int_c<PT_TRISPECTRUM_PARALLELOGRAM>{}); break;
    }
  });
  return st.finish();
}

// -- HaloTrispectrumOneHalo (halo_trispectrum.py:13-151) ------------------------------------------
static bool tri_moment_ok(int moment) { return moment >= CHOMP_TRI_MMMM && moment <= CHOMP_TRI_GGGG; }

// Replaces _initialize_i_0_4 (halo_trispectrum.py:104-129): the 1275 i_0_4 calls of its loop
// (:60-95, one scipy Romberg each) and the RectBivariateSpline fit, for a range of epochs.
// The trispectrum tables integrate y_nfw at k that are no knots of the halo tables: an epoch whose
// last halo set-up had alpha != -1 is outside their scope.
static int nfw_only(chomp_ctx* ctx, size_t epoch0, size_t n, const char* who) {
  for (size_t e = epoch0; e < epoch0 + n && e < ctx->prof_general.size(); ++e)
    if (ctx->prof_general[e])
      return fail(ctx, CHOMP_ERR_SCOPE, std::string(who) + ": halo alpha != -1 (NFW only)");
  return CHOMP_OK;
}

int chomp_tri1h_setup(chomp_ctx* ctx, size_t epoch0, size_t n_epoch, int moment,
                      double* table_out, double* levels_out) {
  StageRange range_(ctx, "chomp:tri1h_setup");
  if (!ctx || n_epoch == 0) return fail(ctx, CHOMP_ERR_ARG, "tri1h_setup: bad args");
  if (!tri_moment_ok(moment)) return fail(ctx, CHOMP_ERR_ARG, "tri1h_setup: unknown moment");
  if (!ctx->have_halo) return fail(ctx, CHOMP_ERR_STATE, "tri1h_setup before a halo set-up");
  { const int rcs = nfw_only(ctx, epoch0, n_epoch, "tri1h_setup"); if (rcs) return rcs; }
  if (epoch0 + n_epoch > ctx->n_epoch || n_epoch > 65535)
    return fail(ctx, CHOMP_ERR_ARG, "tri1h_setup: epoch range");
  const int N = ctx->L.NK;
  if (N < 4 || N > 64)
    return fail(ctx, CHOMP_ERR_SCOPE, "tri1h_setup: halo_npoints must lie in [4, 64]");
  if (ctx->cfg.divmax > kMaxDivmax) return fail(ctx, CHOMP_ERR_ARG, "tri1h_setup: divmax");
  HIPCHK(hipSetDevice(ctx->device));
  ctx->T3 = make_tri_layout(N);
  const TriLayout& T = ctx->T3;
  const size_t need = ctx->n_epoch * (size_t)T.total;
  bool moved = false;
  { const int rc = ensure(ctx, ctx->d_tri, need, &moved); if (rc) return rc; }
  if (moved) ctx->tri_built.assign(ctx->n_epoch, 0);   // (a grown buffer holds no epoch's table)
  const int lds = tri_table_lds_doubles(ctx->L.NM, N) * (int)sizeof(double);
  { const int rc = lds_opt_in(ctx, &k_tri1h_table, lds); if (rc) return rc; }
  hipLaunchKernelGGL(k_tri1h_table, dim3((unsigned)T.nchunk, (unsigned)n_epoch), dim3(kTriThreads),
                     (size_t)lds, ctx->stream, ctx->cfg, ctx->L, T, ctx->d_epochs, (int)epoch0,
                     ctx->d_tab, ctx->d_sici, moment, ctx->d_tri);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_tri1h_bicubic, dim3((unsigned)n_epoch), dim3(256), 0, ctx->stream, T,
                     (int)epoch0, ctx->d_tri, ctx->d_status);
  HIPCHK(hipGetLastError());
  if (ctx->tri_moment != moment) {     // (tables of another moment are not this call's)
    for (size_t e = 0; e < ctx->tri_built.size(); ++e)
      if (e < epoch0 || e >= epoch0 + n_epoch) ctx->tri_built[e] = 0;
    ctx->tri_moment = moment;
  }
  for (size_t e = epoch0; e < epoch0 + n_epoch; ++e) ctx->tri_built[e] = 1;
  if (table_out || levels_out) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const size_t nn = (size_t)N * N;
    for (size_t e = 0; e < n_epoch; ++e) {
      const double* b = ctx->d_tri + (epoch0 + e) * (size_t)T.total;
      if (table_out)
        HIPCHK(hipMemcpy(table_out + e * nn, b + T.tab, nn * sizeof(double), hipMemcpyDeviceToHost));
      if (levels_out)
        HIPCHK(hipMemcpy(levels_out + e * nn, b + T.lev, nn * sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  return CHOMP_OK;
}

// Replaces the _i_0_4_spline(ln k1, ln k2) look-ups of i_0_4_parallelogram
// (halo_trispectrum.py:97-102).
int chomp_tri1h_eval(chomp_ctx* ctx, size_t epoch, const double* ln_k1, const double* ln_k2,
                     size_t n, double* out, int mem) {
  StageRange range_(ctx, "chomp:tri1h_eval");
  if (!ctx || !ln_k1 || !ln_k2 || !out || n == 0 || n > (size_t)INT32_MAX)
    return fail(ctx, CHOMP_ERR_ARG, "tri1h_eval: bad args");
  Staging st(ctx, mem, "tri1h_eval");
  if (st.rc) return st.rc;
  if (epoch >= ctx->n_epoch || epoch >= ctx->tri_built.size() || !ctx->tri_built[epoch])
    return fail(ctx, CHOMP_ERR_STATE, "tri1h_eval: no trispectrum table of this epoch (chomp_tri1h_setup)");
  HIPCHK(hipSetDevice(ctx->device));
  const double *da, *db;
  double* dout;
  st.in(ln_k1, n, &da);
  st.in(ln_k2, n, &db);
  st.out(out, n, &dout);
  const int rc = st.place();
  if (rc) return rc;
  hipLaunchKernelGGL(k_tri1h_eval, grid_1d(n), dim3(256), 0, ctx->stream, ctx->T3, ctx->d_tri,
                     (int)epoch, da, db, (int)n, dout);
  return st.finish();
}

// Replaces i_0_4 / trispectrum (halo_trispectrum.py:57-95): one scipy Romberg per call.
int chomp_tri1h_quad(chomp_ctx* ctx, size_t epoch, int moment, const double* k, size_t n,
                     double* out, double* levels, int mem) {
  StageRange range_(ctx, "chomp:tri1h_quad");
  if (!ctx || !k || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "tri1h_quad: bad args");
  if (!tri_moment_ok(moment)) return fail(ctx, CHOMP_ERR_ARG, "tri1h_quad: unknown moment");
  Staging st(ctx, mem, "tri1h_quad");
  if (st.rc) return st.rc;
  if (!ctx->have_halo || epoch >= ctx->n_epoch)
    return fail(ctx, CHOMP_ERR_STATE, "tri1h_quad before a halo set-up of this epoch");
  { const int rcs = nfw_only(ctx, epoch, 1, "tri1h_quad"); if (rcs) return rcs; }
  const size_t nb = (n + kTriQuadWaves - 1) / kTriQuadWaves;
  if (nb > (size_t)INT32_MAX) return fail(ctx, CHOMP_ERR_ARG, "tri1h_quad: too many quadruples");
  HIPCHK(hipSetDevice(ctx->device));
  const double* dk;
  double* dout;
  double* dlev = nullptr;
  st.in(k, 4 * n, &dk);
  st.out(out, n, &dout);
  if (levels) st.out(levels, n, &dlev);
  const int rc = st.place();
  if (rc) return rc;
  const int lds = tri_quad_lds_doubles(ctx->L.NM) * (int)sizeof(double);
  hipLaunchKernelGGL(k_tri1h_quad<4>, dim3((unsigned)nb), dim3(64 * kTriQuadWaves), (size_t)lds,
                     ctx->stream, ctx->cfg, ctx->L, ctx->d_epochs, (int)epoch, ctx->d_tab,
                     ctx->d_sici, moment, dk, (long)n, dout, dlev, ctx->d_status,
                     kStTri1hDivmax);
  return st.finish();
}

// -- HaloTrispectrum (halo_trispectrum.py:153-837) -------------------------------------------------
// Replaces the five _initialize_i_* loops (:592-836): 4 x 1275 + 50 scipy Rombergs and the spline
// fits, for a range of epochs.
int chomp_tri_setup(chomp_ctx* ctx, size_t epoch0, size_t n_epoch, double* tables_out,
                    double* levels_out) {
  StageRange range_(ctx, "chomp:tri_setup");
  if (!ctx || n_epoch == 0) return fail(ctx, CHOMP_ERR_ARG, "tri_setup: bad args");
  if (!ctx->have_halo) return fail(ctx, CHOMP_ERR_STATE, "tri_setup before a halo set-up");
  { const int rcs = nfw_only(ctx, epoch0, n_epoch, "tri_setup"); if (rcs) return rcs; }
  if (!ctx->have_b2)
    return fail(ctx, CHOMP_ERR_STATE, "tri_setup: the last mass set-up was not second-order "
                                      "(chomp_set_second_order)");
  {
    const int rc = chomp_tri1h_setup(ctx, epoch0, n_epoch, CHOMP_TRI_MMMM, nullptr, nullptr);
    if (rc) return rc;
  }
  const int N = ctx->L.NK;
  ctx->Q4 = make_tri_tab_layout(N);
  const TriTabLayout& Q = ctx->Q4;
  const size_t need = ctx->n_epoch * (size_t)Q.total;
  bool moved = false;
  { const int rc = ensure(ctx, ctx->d_tri4, need, &moved); if (rc) return rc; }
  if (moved || ctx->tri4_built.size() != ctx->n_epoch) ctx->tri4_built.assign(ctx->n_epoch, 0);
  const int lds = tri_tab_lds_doubles(ctx->L.NM, N) * (int)sizeof(double);
  { const int rc = lds_opt_in(ctx, &k_tri_table, lds); if (rc) return rc; }
  hipLaunchKernelGGL(k_tri_table, dim3((unsigned)Q.T.nchunk, (unsigned)n_epoch, 4u),
                     dim3(kTriThreads), (size_t)lds, ctx->stream, ctx->cfg, ctx->L, ctx->B2, Q,
                     ctx->d_epochs, (int)epoch0, ctx->d_tab, ctx->d_b2, ctx->d_sici, ctx->d_tri4);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_tri_finish, dim3((unsigned)n_epoch, 4u), dim3(256), 0, ctx->stream, Q,
                     (int)epoch0, ctx->d_tri4, ctx->d_status);
  HIPCHK(hipGetLastError());
  for (size_t e = epoch0; e < epoch0 + n_epoch; ++e) ctx->tri4_built[e] = 1;
  if (tables_out || levels_out) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const size_t nn = (size_t)N * N, per = 4 * nn + (size_t)N;
    for (size_t e = 0; e < n_epoch; ++e) {
      const double* b1 = ctx->d_tri + (epoch0 + e) * (size_t)ctx->T3.total;
      const double* b4 = ctx->d_tri4 + (epoch0 + e) * (size_t)Q.total;
      for (int w = 0; w < 2; ++w) {
        double* o = w == 0 ? tables_out : levels_out;
        if (!o) continue;
        o += e * per;
        const int o2 = w == 0 ? Q.T.tab : Q.T.lev;
        HIPCHK(hipMemcpy(o, b1 + o2, nn * sizeof(double), hipMemcpyDeviceToHost));
        for (int k = 0; k < kTriKinds2d; ++k)
          HIPCHK(hipMemcpy(o + (k + 1) * nn, b4 + (size_t)k * Q.T.total + o2, nn * sizeof(double),
                           hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(o + 4 * nn, b4 + (w == 0 ? Q.tab : Q.lev), N * sizeof(double),
                         hipMemcpyDeviceToHost));
      }
    }
  }
  return CHOMP_OK;
}

static int tri_ready(chomp_ctx* ctx, size_t epoch, const char* who) {
  if (epoch >= ctx->n_epoch || epoch >= ctx->tri4_built.size() || !ctx->tri4_built[epoch] ||
      epoch >= ctx->tri_built.size() || !ctx->tri_built[epoch] ||
      ctx->tri_moment != CHOMP_TRI_MMMM)
    return fail(ctx, CHOMP_ERR_STATE, std::string(who) + ": no HaloTrispectrum tables of this epoch (chomp_tri_setup)");
  return CHOMP_OK;
}

// Replaces the spline look-ups of i_0_4_parallelogram, i_1_2, i_1_3_parallelogram, i_2_1, i_2_2.
int chomp_tri_table_eval(chomp_ctx* ctx, size_t epoch, int table, const double* k1,
                         const double* k2, size_t n, double* out, int mem) {
  StageRange range_(ctx, "chomp:tri_table_eval");
  if (!ctx || !k1 || !k2 || !out || n == 0 || n > (size_t)INT32_MAX)
    return fail(ctx, CHOMP_ERR_ARG, "tri_table_eval: bad args");
  if (table < CHOMP_TRI_TAB_I_1_2 || table > CHOMP_TRI_TAB_I_1_1)
    return fail(ctx, CHOMP_ERR_ARG, "tri_table_eval: unknown table");
  Staging st(ctx, mem, "tri_table_eval");
  if (st.rc) return st.rc;
  { const int rc = tri_ready(ctx, epoch, "tri_table_eval"); if (rc) return rc; }
  if (table == CHOMP_TRI_TAB_I_1_1 && !((ctx->fam_mask | ctx->put_mask[epoch]) & (1u << F_HM)))
    return fail(ctx, CHOMP_ERR_STATE, "tri_table_eval: the h_m knot table was not built (chomp_halo_setup)");
  HIPCHK(hipSetDevice(ctx->device));
  const double *da, *db;
  double* dout;
  st.in(k1, n, &da);
  st.in(k2, n, &db);
  st.out(out, n, &dout);
  const int rc = st.place();
  if (rc) return rc;
  hipLaunchKernelGGL(k_tri_lookup, grid_1d(n), dim3(256), 0, ctx->stream, ctx->cfg, ctx->L, ctx->T3,
                     ctx->Q4, ctx->d_tab, ctx->d_tri, ctx->d_tri4, (int)epoch, table, da, db,
                     (int)n, dout);
  return st.finish();
}

static int tri_terms_ready(chomp_ctx* ctx, size_t epoch, size_t pt_epoch, const char* who) {
  const int rc = tri_ready(ctx, epoch, who);
  if (rc) return rc;
  if (pt_epoch >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_ARG, std::string(who) + ": pt_epoch");
  if (!((ctx->fam_mask | ctx->put_mask[epoch]) & (1u << F_HM)))
    return fail(ctx, CHOMP_ERR_STATE, std::string(who) + ": the h_m knot table was not built (chomp_halo_setup)");
  return CHOMP_OK;
}

// Replaces t_1_h .. t_4_h (:320-512), one Python call chain per configuration.
int chomp_tri_terms(chomp_ctx* ctx, size_t epoch, size_t pt_epoch, const double* kkz, size_t n,
                    double* out, int mem) {
  StageRange range_(ctx, "chomp:tri_terms");
  if (!ctx || !kkz || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "tri_terms: bad args");
  Staging st(ctx, mem, "tri_terms");
  if (st.rc) return st.rc;
  { const int rc = tri_terms_ready(ctx, epoch, pt_epoch, "tri_terms"); if (rc) return rc; }
  HIPCHK(hipSetDevice(ctx->device));
  const double* dk;
  double* dout;
  st.in(kkz, 3 * n, &dk);
  st.out(out, 4 * n, &dout);
  const int rc = st.place();
  if (rc) return rc;
  size_t gx = (n + 255) / 256;
  if (gx > 4096) gx = 4096;
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_tri_terms<BAO>, dim3((unsigned)gx), dim3(256), 0, ctx->stream, ctx->cfg,
                       ctx->L, ctx->T3, ctx->Q4, ctx->d_epochs, (int)epoch, (int)pt_epoch,
                       ctx->d_tab, ctx->d_tri, ctx->d_tri4, dk, n, dout);
  });
  return st.finish();
}

// Replaces tri_spec_proj_integral (:267-278): one scipy Romberg over theta per pair.
int chomp_tri_proj(chomp_ctx* ctx, size_t epoch, size_t pt_epoch, const double* kk, size_t n,
                   double* out, double* levels, double* flags, int mem) {
  StageRange range_(ctx, "chomp:tri_proj");
  if (!ctx || !kk || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "tri_proj: bad args");
  Staging st(ctx, mem, "tri_proj");
  if (st.rc) return st.rc;
  { const int rc = tri_terms_ready(ctx, epoch, pt_epoch, "tri_proj"); if (rc) return rc; }
  const size_t nb = (n + kTriProjWaves - 1) / kTriProjWaves;
  if (nb > (size_t)INT32_MAX) return fail(ctx, CHOMP_ERR_ARG, "tri_proj: too many pairs");
  HIPCHK(hipSetDevice(ctx->device));
  const double* dk;
  double* dout;
  double* dlev = nullptr;
  double* dflag = nullptr;
  st.in(kk, 2 * n, &dk);
  st.out(out, n, &dout);
  if (levels) st.out(levels, n, &dlev);
  if (flags) st.out(flags, n, &dflag);
  const int rc = st.place();
  if (rc) return rc;
  with_flag(ctx->with_bao, [&](auto BAO) {
    hipLaunchKernelGGL(k_tri_proj<BAO>, dim3((unsigned)nb), dim3(64 * kTriProjWaves), 0,
                       ctx->stream, ctx->cfg, ctx->L, ctx->T3, ctx->Q4, ctx->d_epochs, (int)epoch,
                       (int)pt_epoch, ctx->d_tab, ctx->d_tri, ctx->d_tri4, dk, (long)n, dout, dlev,
                       dflag, ctx->d_status);
  });
  return st.finish();
}

// Replaces i_1_3 (:690-705): one scipy Romberg per call.
int chomp_tri_triple(chomp_ctx* ctx, size_t epoch, const double* k, size_t n, double* out,
                     double* levels, int mem) {
  StageRange range_(ctx, "chomp:tri_triple");
  if (!ctx || !k || !out || n == 0) return fail(ctx, CHOMP_ERR_ARG, "tri_triple: bad args");
  Staging st(ctx, mem, "tri_triple");
  if (st.rc) return st.rc;
  if (!ctx->have_halo || epoch >= ctx->n_epoch)
    return fail(ctx, CHOMP_ERR_STATE, "tri_triple before a halo set-up of this epoch");
  const size_t nb = (n + kTriQuadWaves - 1) / kTriQuadWaves;
  if (nb > (size_t)INT32_MAX) return fail(ctx, CHOMP_ERR_ARG, "tri_triple: too many triples");
  HIPCHK(hipSetDevice(ctx->device));
  const double* dk;
  double* dout;
  double* dlev = nullptr;
  st.in(k, 3 * n, &dk);
  st.out(out, n, &dout);
  if (levels) st.out(levels, n, &dlev);
  const int rc = st.place();
  if (rc) return rc;
  const int lds = tri_quad_lds_doubles(ctx->L.NM) * (int)sizeof(double);
  hipLaunchKernelGGL(k_tri1h_quad<3>, dim3((unsigned)nb), dim3(64 * kTriQuadWaves), (size_t)lds,
                     ctx->stream, ctx->cfg, ctx->L, ctx->d_epochs, (int)epoch, ctx->d_tab,
                     ctx->d_sici, CHOMP_TRI_MMMM, dk, (long)n, dout, dlev, ctx->d_status,
                     kStTriDivmax);
  return st.finish();
}

int chomp_halofit_get(chomp_ctx* ctx, size_t epoch, double* out) {
  if (!ctx || !out) return fail(ctx, CHOMP_ERR_ARG, "halofit_get: bad args");
  if (!ctx->have_epochs || epoch >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_STATE, "halofit_get: epoch");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  Epoch E;
  HIPCHK(hipMemcpy(&E, ctx->d_epochs + epoch, sizeof(Epoch), hipMemcpyDeviceToHost));
  std::memcpy(out, &E.hf_f1, CHOMP_HF_COUNT * sizeof(double));
  return CHOMP_OK;
}

int chomp_halofit_put(chomp_ctx* ctx, size_t epoch, const double* in) {
  if (!ctx || !in) return fail(ctx, CHOMP_ERR_ARG, "halofit_put: bad args");
  if (!ctx->have_epochs || epoch >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_STATE, "halofit_put: epoch");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  char* dst = reinterpret_cast<char*>(ctx->d_epochs + epoch) + offsetof(Epoch, hf_f1);
  HIPCHK(hipMemcpy(dst, in, CHOMP_HF_COUNT * sizeof(double), hipMemcpyHostToDevice));
  ctx->have_halofit[epoch] = 1;
  return CHOMP_OK;
}

int chomp_get_scalars(chomp_ctx* ctx, size_t epoch, double* out) {
  if (!ctx || !out) return fail(ctx, CHOMP_ERR_ARG, "get_scalars: bad args");
  if (!ctx->have_epochs || epoch >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_STATE, "get_scalars: epoch");
  HIPCHK(hipSetDevice(ctx->device));
  Epoch E;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(&E, ctx->d_epochs + epoch, sizeof(Epoch), hipMemcpyDeviceToHost));
  for (int i = 0; i < CHOMP_SC_COUNT; ++i) out[i] = 0.0;
  out[CHOMP_SC_Z] = E.z; out[CHOMP_SC_CHI] = E.chi; out[CHOMP_SC_GROWTH] = E.growth;
  out[CHOMP_SC_OMEGA_M] = E.omega_m_z; out[CHOMP_SC_OMEGA_L] = E.omega_l_z;
  out[CHOMP_SC_DELTA_C] = E.delta_c; out[CHOMP_SC_DELTA_V] = E.delta_v;
  out[CHOMP_SC_RHO_BAR] = E.rho_bar; out[CHOMP_SC_SIGMA_NORM] = E.sigma_norm;
  out[CHOMP_SC_LN_MASS_MIN] = E.ln_mass_min; out[CHOMP_SC_LN_MASS_MAX] = E.ln_mass_max;
  out[CHOMP_SC_NU_MIN] = E.nu_min; out[CHOMP_SC_NU_MAX] = E.nu_max;
  out[CHOMP_SC_M_STAR] = E.m_star; out[CHOMP_SC_F_NORM] = E.f_norm;
  out[CHOMP_SC_BIAS_NORM] = E.bias_norm; out[CHOMP_SC_N_BAR] = E.n_bar;
  out[CHOMP_SC_N_BAR_OVER_RHO_BAR] = E.n_bar_over_rho_bar;
  out[CHOMP_SC_N_SEARCH] = (double)E.n_search; out[CHOMP_SC_MF_DELTA_V] = E.mf_delta_v;
  out[CHOMP_SC_T_ALPHA] = E.t_alpha; out[CHOMP_SC_T_BETA] = E.t_beta;
  out[CHOMP_SC_T_GAMMA] = E.t_gamma; out[CHOMP_SC_T_PHI] = E.t_phi;
  out[CHOMP_SC_T_ETA] = E.t_eta; out[CHOMP_SC_GROWTH_NORM] = E.growth_norm;
  out[CHOMP_SC_DELTA_H] = E.delta_H; out[CHOMP_SC_HF_K_S] = E.hf_k_s;
  out[CHOMP_SC_HF_N_EFF] = E.hf_n_eff; out[CHOMP_SC_HF_C] = E.hf_C;
  return CHOMP_OK;
}

int chomp_get_table(chomp_ctx* ctx, size_t epoch, int table, double* out, size_t n) {
  if (!ctx || !out) return fail(ctx, CHOMP_ERR_ARG, "get_table: bad args");
  if (!ctx->have_mass || epoch >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_STATE, "get_table before mass_setup");
  const TabLayout& L = ctx->L;
  int off = -1;
  size_t len = 0;
  unsigned need = 0;                 // knot family that must have been built
  bool need_hf = false;
  switch (table) {
    case CHOMP_TAB_LN_MASS: off = L.off_ln_mass; len = L.NM; break;
    case CHOMP_TAB_NU: off = L.off_nu; len = L.NM; break;
    case CHOMP_TAB_H_M: off = L.off_knot[F_HM]; len = L.NK; need = 1u << F_HM; break;
    case CHOMP_TAB_PP_MM: off = L.off_knot[F_PPMM]; len = L.NK; need = 1u << F_PPMM; break;
    case CHOMP_TAB_H_G: off = L.off_knot[F_HG]; len = L.NK; need = 1u << F_HG; break;
    case CHOMP_TAB_PP_GM: off = L.off_knot[F_PPGM]; len = L.NK; need = 1u << F_PPGM; break;
    case CHOMP_TAB_PP_GG: off = L.off_knot[F_PPGG]; len = L.NK; need = 1u << F_PPGG; break;
    case CHOMP_TAB_LEVELS:
      off = L.off_levels; len = 5 * (size_t)L.NK;
      if (!ctx->fam_mask) return fail(ctx, CHOMP_ERR_STATE, "get_table: no knot table built yet");
      break;
    case CHOMP_TAB_HF_LN_SIGMA2: off = L.off_hf_lns2; len = L.NK; need_hf = true; break;
    case CHOMP_TAB_I_1_2: off = L.off_knot[F_I12]; len = L.NK; need = 1u << F_I12; break;
    case CHOMP_TAB_LEVELS_I_1_2:
      off = L.off_levels + F_I12 * L.NK; len = L.NK; need = 1u << F_I12; break;
    default: return fail(ctx, CHOMP_ERR_ARG, "get_table: unknown table");
  }
  // (the levels rows come from a set-up only: chomp_put_table installs knots, not levels)
  const bool levels = table == CHOMP_TAB_LEVELS_I_1_2;
  if (((ctx->fam_mask | (levels ? 0u : ctx->put_mask[epoch])) & need) != need)
    return fail(ctx, CHOMP_ERR_STATE, "get_table: this knot table was not built (chomp_halo_setup)");
  if (need_hf && !ctx->have_halofit[epoch])
    return fail(ctx, CHOMP_ERR_STATE, "get_table: chomp_halofit_setup not called for this epoch");
  if (n != len) return fail(ctx, CHOMP_ERR_ARG, "get_table: length mismatch");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(out, ctx->d_tab + epoch * (size_t)L.stride + off, len * sizeof(double),
                   hipMemcpyDeviceToHost));
  return CHOMP_OK;
}

int chomp_put_table(chomp_ctx* ctx, size_t epoch, int table, const double* in, size_t n) {
  if (!ctx || !in) return fail(ctx, CHOMP_ERR_ARG, "put_table: bad args");
  if (!ctx->have_mass || epoch >= ctx->n_epoch) return fail(ctx, CHOMP_ERR_STATE, "put_table before mass_setup");
  int f = -1;
  switch (table) {
    case CHOMP_TAB_H_M: f = F_HM; break;
    case CHOMP_TAB_PP_MM: f = F_PPMM; break;
    case CHOMP_TAB_H_G: f = F_HG; break;
    case CHOMP_TAB_PP_GM: f = F_PPGM; break;
    case CHOMP_TAB_PP_GG: f = F_PPGG; break;
    case CHOMP_TAB_I_1_2: f = F_I12; break;
    default: return fail(ctx, CHOMP_ERR_ARG, "put_table: not a knot table");
  }
  const TabLayout& L = ctx->L;
  if (n != (size_t)L.NK) return fail(ctx, CHOMP_ERR_ARG, "put_table: length mismatch");
  if (capturing(ctx))
    return fail(ctx, CHOMP_ERR_STATE, "put_table: synchronises the host; not while the stream is being captured");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(ctx->d_tab + epoch * (size_t)L.stride + L.off_knot[f], in, n * sizeof(double),
                   hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_put_spline, dim3(1), dim3(64), (size_t)(11 * L.NK) * sizeof(double), ctx->stream,
                     ctx->cfg, L, ctx->d_tab, (int)epoch, f);
  HIPCHK(hipGetLastError());
  ctx->put_mask[epoch] |= 1u << f;
  return CHOMP_OK;
}

#include "chomp_capi_proj.inc"

}  // extern "C"
