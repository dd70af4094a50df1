/*
 * chomp_mi355x.h -- C ABI of libchomp_mi355x.so, the MI355X (gfx950) implementation
 * of CHOMP's halo-model + Limber-projection hot path.
 *
 * The reference (morriscb/chomp) has no FFI: its boundary for this path is the
 * Python method surface of halo.Halo / kernel.Kernel / correlation.Correlation.
 * Each entry point below names the reference interface it replaces (file:line in
 * /root/reference).  The chomp_amd Python package binds these with ctypes and mirrors the
 * reference classes; INTEGRATION.md shows the stub a reference maintainer would
 * add.  All functions return CHOMP_OK (0) or a negative error code; the message
 * is available from chomp_last_error().  Plain pointers and sizes only.
 *
 * Memory-space convention: every array argument is paired with (or covered by) a
 * `mem` argument: CHOMP_HOST (pointer is host memory; the library stages it) or
 * CHOMP_DEVICE (pointer is HBM on the context's device, e.g. torch
 * tensor.data_ptr(); no copy, the call is asynchronous on the context's stream).
 * Any other `mem` is refused with CHOMP_ERR_ARG before anything is copied or launched.
 *
 * Threading: one HIP stream per context; calls on one context must be serialised
 * by the caller; distinct contexts are independent.
 */
#ifndef CHOMP_MI355X_H
#define CHOMP_MI355X_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHOMP_OK 0
#define CHOMP_ERR_ARG (-1)      /* bad argument (KeyError/ValueError analogue)   */
#define CHOMP_ERR_HIP (-2)      /* HIP runtime failure                            */
#define CHOMP_ERR_STATE (-3)    /* stage called before its prerequisite           */
#define CHOMP_ERR_SCOPE (-4)    /* feature outside the hot-path scope (w != -1)   */

#define CHOMP_HOST 0
#define CHOMP_DEVICE 1

typedef struct chomp_ctx chomp_ctx;

/* defaults.default_cosmo_dict (defaults.py:6-18).  w0/wa other than -1/0 (w0-wa dark energy)
 * need chomp_set_dark_energy(ctx, 1); without it the set-ups refuse them (CHOMP_ERR_SCOPE). */
typedef struct chomp_cosmo {
  double omega_m0, omega_b0, omega_l0, omega_r0, cmb_temp, h, sigma_8, n_scalar,
      w0, wa;
} chomp_cosmo;

/* defaults.default_halo_dict (defaults.py:21-29). */
typedef struct chomp_halo_par {
  double stq, st_little_a, c0, beta, alpha, delta_v;
} chomp_halo_par;

/* hod.HODZheng parameters (hod.py:156-186, defaults.py:33-39). */
typedef struct chomp_hod_par {
  double log_M_min, sigma, log_M_0, log_M_1p, alpha;
} chomp_hod_par;

/* Occupation models (chomp_hod_model.kind). */
#define CHOMP_HOD_ZHENG 0
#define CHOMP_HOD_MANDELBAUM 1

/* One epoch's HOD, tagged by its model: hod.HODZheng (CHOMP_HOD_ZHENG: `zheng`) or
 * hod.HODMandelbaum (hod.py:232-299, CHOMP_HOD_MANDELBAUM: log_M_0 and w; the library derives
 * log_M_min = log10(3) + log_M_0 and 10**log_M_min as the reference does, and -- the HOD has no
 * moment zeros and no safe norm -- integrates every HOD integral over the whole nu range).
 * `reserved` must be 0; the fields of the other model are ignored. */
typedef struct chomp_hod_model {
  int kind, reserved;
  chomp_hod_par zheng;
  double log_M_0, w;
} chomp_hod_model;

/* Snapshot of defaults.default_limits + defaults.default_precision
 * (defaults.py:42-51, 62-92), taken when the context is created. */
typedef struct chomp_config {
  double k_min, k_max, mass_min, mass_max;
  double corr_precision, cosmo_precision, dNdz_precision, halo_precision,
      kernel_precision, mass_precision, window_precision, global_precision;
  int corr_npoints, cosmo_npoints, halo_npoints, kernel_npoints,
      kernel_bessel_limit, mass_npoints, window_npoints, divmax;
} chomp_config;

/* Mass functions: mass_function.MassFunction (Sheth-Tormen, mass_function.py:25)
 * and mass_function.TinkerMassFunction (:436). */
#define CHOMP_MF_ST 0
#define CHOMP_MF_TINKER 1

/* Knot tables built by chomp_halo_setup (bit mask): one bit per lazily
 * initialised spline of the reference's Halo (halo.py:96-101), so a caller can
 * mirror which of them a setter invalidates (halo.py:165-170, 186-189). */
#define CHOMP_T_H_M 1u    /* Halo._initialize_h_m    halo.py:904-927   */
#define CHOMP_T_PP_MM 2u  /* Halo._initialize_pp_mm  halo.py:971-994   */
#define CHOMP_T_H_G 4u    /* Halo._initialize_h_g    halo.py:929-969   */
#define CHOMP_T_PP_GM 8u  /* Halo._initialize_pp_gm  halo.py:1043-1086 */
#define CHOMP_T_PP_GG 16u /* Halo._initialize_pp_gg  halo.py:996-1041  */
/* HaloSuperSampleCovariance._initialize_i_1_2 (halo.py:1176-1199): I_1^2 = int dln nu
 * nu f(nu) b(nu) y(k, M)^2 M / rho_bar over [nu_min, nu_max], the range of h_m / pp_mm. */
#define CHOMP_T_I_1_2 32u
/* OR-ed in: the object is a HaloExclusion (halo.py:1201-1233): h_m and h_g are built
 * with the halo-exclusion mass window in their integrands. */
#define CHOMP_T_EXCLUSION 64u
#define CHOMP_FAM_MM (CHOMP_T_H_M | CHOMP_T_PP_MM)               /* power_mm */
#define CHOMP_FAM_GM (CHOMP_T_H_M | CHOMP_T_H_G | CHOMP_T_PP_GM) /* power_gm */
#define CHOMP_FAM_GG (CHOMP_T_H_G | CHOMP_T_PP_GG)               /* power_gg */
#define CHOMP_FAM_SSC (CHOMP_FAM_MM | CHOMP_T_I_1_2)               /* dln_power_ddelta_b */

/* Power spectra served by chomp_power. */
#define CHOMP_P_LIN 0 /* Halo.linear_power  halo.py:266-275 */
#define CHOMP_P_MM 1  /* Halo.power_mm      halo.py:277-320 */
#define CHOMP_P_GM 2  /* Halo.power_gm/mg   halo.py:322-389 */
#define CHOMP_P_GG 3  /* Halo.power_gg      halo.py:391-439 */
/* HaloSuperSampleCovariance (halo.py:1089-1199); need CHOMP_FAM_SSC, refuse HALOFIT and
 * EXTRAPOLATE (the class never extrapolates, halo.py:1102-1108).  Inside [k_min, k_max]
 * (inclusive) dlnP/ddelta_b = (68/21 h_m^2 P_lin + I_1^2) / P_mm, outside exactly 0
 * (halo.py:1136-1156); P_mm_ssc = P_mm (1 + delta_b dlnP/ddelta_b) with the epoch's delta_b
 * (chomp_set_delta_b): P_mm itself below k_min, 0 above k_max (halo.py:1158-1169). */
#define CHOMP_P_SSC_RESPONSE 4 /* dln_power_ddelta_b halo.py:1136-1156 */
#define CHOMP_P_MM_SSC 5       /* power_mm_ssc       halo.py:1158-1169 */
#define CHOMP_P_HALOFIT 16 /* OR-ed in: HaloFit.power_* halo.py:1325-1413 */
/* OR-ed in: Halo(extrapolate=True) -- above k_max P_mm continues as a rescaled linear
 * spectrum, P_gm / P_gg as power laws (halo.py:300-312, 341-367, 405-431); HaloFit
 * ignores it, as in the reference. */
#define CHOMP_P_EXTRAPOLATE 32

void chomp_default_config(chomp_config* cfg);

/* Create a context on `device` using HIP stream `hip_stream` (NULL -> a new
 * stream owned by the context).  Replaces the import-time snapshot of
 * defaults.py that every reference constructor reads. */
int chomp_ctx_create(const chomp_config* cfg, int device, void* hip_stream,
                     chomp_ctx** out);
void chomp_ctx_destroy(chomp_ctx* ctx);
const char* chomp_last_error(chomp_ctx* ctx);
/* Measurement aid (no counterpart in the reference).  With timing on, the streaming shape
 * of chomp_power / chomp_power_range (large grid of one cosmology) brackets its three
 * launches -- k_power_prep, k_power_stream, k_power_grid_lanes -- with HIP events on the
 * context's stream; chomp_get_timing waits for the last such call and returns their
 * durations in microseconds (us[3], n = 3).  CHOMP_ERR_STATE when the last call took
 * another launch shape or timing is off. */
int chomp_set_timing(chomp_ctx* ctx, int on);
int chomp_get_timing(chomp_ctx* ctx, double* us, size_t n);

/* The HIP stream every call of this context is queued on (the one given to chomp_ctx_create,
 * or the one it created): a caller that works on another stream orders the two with events
 * (hipEventRecord / hipStreamWaitEvent) around calls that pass device buffers. */
int chomp_get_stream(chomp_ctx* ctx, void** out);

/* Block until everything queued on the context's stream has finished. */
int chomp_sync(chomp_ctx* ctx);

/* ---- Stage K: per-(cosmology, z) tables -------------------------------------
 * An "epoch" is one (cosmology, redshift) pair = one cosmology.SingleEpoch
 * (cosmology.py:39-119).  A batch of n epochs is set up together; this is the
 * z-axis of the (k, z) grid and the design-point axis of SimulationDesign. */

/* SingleEpoch.__init__/_initialize_defaults for every epoch (cosmology.py:39-119):
 * flatness flags, delta_H, chi(z), growth, sigma_8 normalisation. */
int chomp_epochs_set(chomp_ctx* ctx, size_t n_epoch, const chomp_cosmo* cosmo,
                     const double* z);

/* MassFunction.__init__ (mass_function.py:38-61; Tinker :448-492): mass-limit
 * search (:160-203), nu table + splines (:205-223), normalisation (:225-241).
 * `par[i]` are the halo_dict values the mass function sees for epoch i. */
int chomp_mass_setup(chomp_ctx* ctx, const chomp_halo_par* par, int mf_kind);

/* Halo.__init__ + lazy initialisers (halo.py:41-104, 674-707, 839-1086): n_bar,
 * then the 50-knot tables selected by `tables` (CHOMP_T_* bits) and their
 * splines; tables not selected keep their previous contents.
 * `profile[i]` are the halo_dict values the profile (c0, beta, delta_v) sees;
 * they differ from chomp_mass_setup's only after Halo.set_halo (halo.py:220-235,
 * which does not rebuild the profile splines). */
int chomp_halo_setup(chomp_ctx* ctx, const chomp_halo_par* profile,
                     const chomp_hod_par* hod, unsigned tables);
/* The same with one tagged HOD model per epoch (the models may differ from epoch to epoch);
 * chomp_halo_setup(hod) is chomp_halo_setup_hod with CHOMP_HOD_ZHENG models of hod. */
int chomp_halo_setup_hod(chomp_ctx* ctx, const chomp_halo_par* profile,
                         const chomp_hod_model* hod, unsigned tables);

/* chomp_mass_setup followed by chomp_halo_setup in fewer launches (the mass function's tail
 * and the halo model's node tables share a kernel): what a batch that always builds both --
 * the (k, z) grid, a SimulationDesign -- calls per set-up.  Same results, bit for bit. */
int chomp_stage_k(chomp_ctx* ctx, const chomp_halo_par* mass_par, int mf_kind,
                  const chomp_halo_par* profile, const chomp_hod_par* hod,
                  unsigned tables);
/* The same with one tagged HOD model per epoch (see chomp_halo_setup_hod). */
int chomp_stage_k_hod(chomp_ctx* ctx, const chomp_halo_par* mass_par, int mf_kind,
                      const chomp_halo_par* profile, const chomp_hod_model* hod,
                      unsigned tables);

/* chomp_stage_k followed by chomp_halofit_setup(epoch, epoch, ...) in one call -- a HaloFit
 * object's first set-up (halo.py:1236-1266 then 1268-1319).  Same results, bit for bit; the
 * HaloFit sigma table and fit run on a second HIP stream beside the halo model's knot
 * integrals (neither needs the other's results) and are joined before the call returns. */
int chomp_stage_k_halofit(chomp_ctx* ctx, const chomp_halo_par* mass_par, int mf_kind,
                          const chomp_halo_par* profile, const chomp_hod_par* hod,
                          unsigned tables, size_t epoch, double f_1, double f_2, double f_3,
                          double omega_l, double w);
/* The same with one tagged HOD model per epoch (see chomp_halo_setup_hod). */
int chomp_stage_k_halofit_hod(chomp_ctx* ctx, const chomp_halo_par* mass_par, int mf_kind,
                              const chomp_halo_par* profile, const chomp_hod_model* hod,
                              unsigned tables, size_t epoch, double f_1, double f_2,
                              double f_3, double omega_l, double w);

/* HaloFit._initialize_sigma_spline (halo.py:1268-1319) for epoch `src_epoch`,
 * stored as the HaloFit coefficient set of epoch `dst_epoch`; f_1..f_3, omega_l
 * and w are passed explicitly because the reference fixes them at construction
 * (halo.py:1261-1266) and never refreshes them on set_redshift. */
int chomp_halofit_setup(chomp_ctx* ctx, size_t dst_epoch, size_t src_epoch,
                        double f_1, double f_2, double f_3, double omega_l,
                        double w);

/* ---- Stage E: grid evaluation ------------------------------------------------
 * Halo.linear_power / power_mm / power_gm / power_gg (halo.py:266-439) for every
 * epoch of the batch: out[i*nk + j] = P_which(k[j]; epoch i), row-major (z-major).
 * k in h/Mpc, P in (Mpc/h)^3.  extrapolate=False semantics: k < k_min -> scaled
 * linear spectrum, k > k_max -> 0. */
int chomp_power(chomp_ctx* ctx, int which, const double* k, size_t nk,
                double* out, int mem);
/* Same for the epoch range [epoch0, epoch0 + n). */
int chomp_power_range(chomp_ctx* ctx, int which, size_t epoch0, size_t n,
                      const double* k, size_t nk, double* out, int mem);

/* HaloSuperSampleCovariance._delta_b (halo.py:1104-1107) of epochs [epoch0, epoch0 + n): one
 * value per epoch, read by CHOMP_P_MM_SSC.  chomp_epochs_set resets every epoch's to 0. */
int chomp_set_delta_b(chomp_ctx* ctx, size_t epoch0, size_t n, const double* delta_b, int mem);

/* Register a k grid (device memory, 16-byte aligned, even length) for repeated chomp_power /
 * chomp_power_range calls over the same cosmology: everything that depends on k alone -- ln k,
 * its knot interval, the Eisenstein-Hu shape of the linear spectrum (halo.py:649-672,
 * cosmology.py:449-472) -- is tabulated now, and calls that pass the same pointer and length
 * for epochs of the same cosmology skip that step.  The caller promises not to modify k[]
 * while the registration lasts; it ends with the next chomp_power call on another grid (or a
 * host buffer) that takes the streaming launch shape, or with the context.  No counterpart in
 * the reference, where every power_mm(k) call recomputes log(k) and the linear spectrum. */
int chomp_power_plan(chomp_ctx* ctx, size_t epoch0, const double* k, size_t nk);

/* SingleEpoch.sigma_r (cosmology.py:602-642) at n scales for one epoch (host). */
int chomp_sigma_r(chomp_ctx* ctx, size_t epoch, const double* scale, size_t n,
                  double* out);
/* Halo.y (NFW, halo.py:561-585) at (ln_k[i], mass[i]) pairs for one epoch (host). */
int chomp_y_nfw(chomp_ctx* ctx, size_t epoch, const double* ln_k,
                const double* mass, size_t n, double* out);

/* Element-wise lookups of one epoch (host or device buffers):
 * MassFunction.nu / ln_mass / f_nu / bias_nu (mass_function.py:243-346),
 * the moments of the epoch's HOD model (HODZheng hod.py:189-230, HODMandelbaum hod.py:261-299),
 * Halo.virial_radius / concentration
 * (halo.py:441-463), SingleEpoch.delta_k (cosmology.py:574-587). */
#define CHOMP_EV_NU_OF_MASS 0
#define CHOMP_EV_LN_MASS_OF_NU 1
#define CHOMP_EV_F_NU 2
#define CHOMP_EV_BIAS_NU 3
#define CHOMP_EV_HOD_FIRST 4
#define CHOMP_EV_HOD_SECOND 5
#define CHOMP_EV_HOD_CENTRAL 6
#define CHOMP_EV_HOD_SATELLITE 7
#define CHOMP_EV_VIRIAL_RADIUS 8
#define CHOMP_EV_CONCENTRATION 9
#define CHOMP_EV_DELTA_K 10
/* MassFunctionSecondOrder (mass_function.py:365-434; needs a mass set-up with
 * chomp_set_second_order on): bias_2_nu (:423-429) and _sigma_spline, the not-a-knot sigma(nu)
 * spline over the nu knots (:391-392), extrapolated by its end pieces as FITPACK does. */
#define CHOMP_EV_BIAS_2_NU 11
#define CHOMP_EV_SIGMA_OF_NU 12
int chomp_eval(chomp_ctx* ctx, size_t epoch, int what, const double* x, size_t n,
               double* out, int mem);

/* HaloFit coefficient block of one epoch (f_1, f_2, f_3, k_s, n_eff, C, a_n, b_n,
 * c_n, gamma_n, alpha_n, beta_n, mu_n, nu_n): read it back / write it.  The
 * reference keeps these across set_redshift (halo.py:1254-1259 never resets
 * _initialized_sigma_spline), so a caller mirroring that re-installs them after
 * chomp_epochs_set. */
#define CHOMP_HF_COUNT 14
int chomp_halofit_get(chomp_ctx* ctx, size_t epoch, double* out);
int chomp_halofit_put(chomp_ctx* ctx, size_t epoch, const double* in);

/* ---- Introspection (per-stage parity tests, write() mirrors) ---------------- */
#define CHOMP_SC_Z 0
#define CHOMP_SC_CHI 1
#define CHOMP_SC_GROWTH 2
#define CHOMP_SC_OMEGA_M 3
#define CHOMP_SC_OMEGA_L 4
#define CHOMP_SC_DELTA_C 5
#define CHOMP_SC_DELTA_V 6
#define CHOMP_SC_RHO_BAR 7
#define CHOMP_SC_SIGMA_NORM 8
#define CHOMP_SC_LN_MASS_MIN 9
#define CHOMP_SC_LN_MASS_MAX 10
#define CHOMP_SC_NU_MIN 11
#define CHOMP_SC_NU_MAX 12
#define CHOMP_SC_M_STAR 13
#define CHOMP_SC_F_NORM 14
#define CHOMP_SC_BIAS_NORM 15
#define CHOMP_SC_N_BAR 16
#define CHOMP_SC_N_BAR_OVER_RHO_BAR 17
#define CHOMP_SC_N_SEARCH 18
#define CHOMP_SC_MF_DELTA_V 19
#define CHOMP_SC_T_ALPHA 20
#define CHOMP_SC_T_BETA 21
#define CHOMP_SC_T_GAMMA 22
#define CHOMP_SC_T_PHI 23
#define CHOMP_SC_T_ETA 24
#define CHOMP_SC_GROWTH_NORM 25
#define CHOMP_SC_DELTA_H 26
#define CHOMP_SC_HF_K_S 27
#define CHOMP_SC_HF_N_EFF 28
#define CHOMP_SC_HF_C 29
#define CHOMP_SC_COUNT 30
/* out[CHOMP_SC_COUNT] <- scalars of one epoch (SingleEpoch / MassFunction / Halo
 * attributes: _chi, _growth, omega_m(), delta_c(), ..., f_norm, n_bar). */
int chomp_get_scalars(chomp_ctx* ctx, size_t epoch, double* out);

/* Per-epoch status word: what the reference would have told its user through a warning (or
 * through never returning), reported instead of computed around.  Bits accumulate over the
 * stages of an epoch; chomp_epochs_set clears the word, chomp_halo_setup the HALO / NONFINITE
 * bits.  out[n] <- status of epochs [epoch0, epoch0 + n) (host buffer; synchronises).
 *
 * MASS_MIN_SATURATED: MassFunction._set_mass_limits' 5 % walk (mass_function.py:171-181) ended
 *   at a mass so small that k R < 0.2 over the whole k range of sigma_r (clamped at 100 k_max,
 *   cosmology.py:627-632).  There nu(M) has converged to a constant above the band -- in exact
 *   arithmetic the walk would never end -- and what ends the reference's walk is the rounding
 *   error of 3 (sin x / x^3 - cos x / x^2) at x << 1 (its variance biases sigma^2 upwards like
 *   eps^2 / x^4): the step it stops at is a property of the libm in use, not of the model.
 *   Results for such an epoch can differ from the reference's by percents (either answer is
 *   equally arbitrary); low sigma_8 / Omega_m at z >~ 0.8, M_min ~ 1e-8 M_sun/h.
 * MASS_MAX_SATURATED: the mass_max walk ended with sigma_r's k range clamped at k_min / 100
 *   (cosmology.py:617-622, behind the reference's commented-out extrapolation warning).
 * MASS_SEARCH_EXHAUSTED: the walk did not end within 2047 steps (the reference loops on).
 * SIGMA_DIVMAX: a sigma(R) Romberg of the nu table exhausted divmax (scipy: AccuracyWarning).
 * DE_DIVMAX: a knot of the epoch's dark-energy pressure table exhausted divmax
 *   (cosmology.py:196-213; with the default precision the deepest 22 of the 50 knots do).
 * HALO_DIVMAX_*: some knot of that table exhausted divmax (halo.py:909-915, 951-957, 976-982,
 *   1018-1024, 1065-1071, 1182-1189; scipy returns the last row with an AccuracyWarning -- with the
 *   default precision the discontinuous HOD integrands of pp_gm / pp_gg do this routinely).
 * NONFINITE: a knot table holds a NaN or an infinity. */
#define CHOMP_ST_MASS_MIN_SATURATED 1u
#define CHOMP_ST_MASS_MAX_SATURATED 2u
#define CHOMP_ST_MASS_SEARCH_EXHAUSTED 4u
#define CHOMP_ST_SIGMA_DIVMAX 8u
#define CHOMP_ST_DE_DIVMAX 0x10u
/* B2_DIVMAX: the bias_2_norm Romberg of a second-order set-up exhausted divmax
 * (mass_function.py:408-414). */
#define CHOMP_ST_B2_DIVMAX 0x20u
/* TRI1H_DIVMAX: an I_0^4 Romberg of the last one-halo trispectrum table of the epoch
 * (chomp_tri1h_setup; halo_trispectrum.py:89-95), or of a chomp_tri1h_quad call since, exhausted
 * divmax.  Each table set-up sets or clears it for its epochs. */
#define CHOMP_ST_TRI1H_DIVMAX 0x40u
/* COV_NG_DIVMAX: on the context's first epoch -- a raw_kernel_NG Romberg of the last
 * chomp_kernel_ng_setup (kernel.py:1067-1072), of a chomp_kernel_ng_raw call or a k_b Romberg of
 * a chomp_covariance_ng call (covariance.py:665-671) since, exhausted divmax.  The set-up
 * clears it first. */
#define CHOMP_ST_COV_NG_DIVMAX 0x80u
/* TRI_DIVMAX: a Romberg of the last HaloTrispectrum tables of the epoch (chomp_tri_setup;
 * halo_trispectrum.py:655-836), or of a chomp_tri_proj / chomp_tri_triple call since, exhausted
 * divmax; for chomp_tri_proj also a non-finite end point (k1 = k2), where the result is NaN. */
#define CHOMP_ST_TRI_DIVMAX 0x4000u
#define CHOMP_ST_HALO_DIVMAX_H_M 0x100u   /* << 0..5: H_M, PP_MM, H_G, PP_GM, PP_GG, I_1_2 */
#define CHOMP_ST_HALO_DIVMAX_PP_MM 0x200u
#define CHOMP_ST_HALO_DIVMAX_H_G 0x400u
#define CHOMP_ST_HALO_DIVMAX_PP_GM 0x800u
#define CHOMP_ST_HALO_DIVMAX_PP_GG 0x1000u
#define CHOMP_ST_HALO_DIVMAX_I_1_2 0x2000u  /* halo.py:1182-1189 */
#define CHOMP_ST_NONFINITE 0x10000u
int chomp_get_status(chomp_ctx* ctx, size_t epoch0, size_t n, unsigned* out);
/* The same words without draining the stream.  chomp_status_post makes every epoch's word, as
 * it is behind the work enqueued so far (call it right after a set-up), available in pinned host
 * memory; chomp_status_wait blocks until THOSE words have landed -- not until the stream is idle
 * -- and returns them as they were then, whatever has been set up since.  Behind a halo set-up
 * (chomp_stage_k, chomp_halo_setup) a post puts nothing on the stream: the set-up's finalising
 * blocks have written the words, tagged with the set-up's sequence number, to the pinned words
 * themselves, and the wait polls for that number (an event record alone costs a step ~10 us on
 * this stack).  Behind any other set-up it is a copy and an event.  A caller that keeps its
 * samples on the device posts after each set-up and waits whenever it next has a reason to look
 * (the reference printed its AccuracyWarning at the time of the integral; here the time of
 * looking is the caller's choice).
 * ERR_STATE: wait before any post; wait while the stream is being captured; wait for a set-up
 * that never finalised its epochs (it failed). */
int chomp_status_post(chomp_ctx* ctx);
int chomp_status_wait(chomp_ctx* ctx, size_t epoch0, size_t n, unsigned* out);

/* Test / tuning hooks (no counterpart in the reference; not needed by a caller): override a
 * launch-shape decision of this context.  value < 0 restores the default.  Numbers 1 and 9
 * belonged to retired knobs and are refused (CHOMP_ERR_ARG) like any unknown one.
 *   CHOMP_TUNE_E_STREAM_MIN  samples from which chomp_power takes the streaming launch shape
 *   CHOMP_TUNE_DEEP_LITERAL  1: knots beyond the node tables by literal evaluation of every
 *                            Romberg node (the checker of the fast deep-level sums)
 *   CHOMP_TUNE_DEEP_TOL      self-check threshold of the fast deep-level sums, in units of 1e-15
 *                            relative (default 1 000 000 = 1e-9): a knot whose estimate is above
 *                            it is handed to the literal evaluation.  0 sends every knot that
 *                            reaches the self-check there
 *   CHOMP_TUNE_DEEP_MAX_BREAKS  break points of the integrand (changes of its discrete state
 *                            along ln nu) a knot may have and still take the fast sums (default
 *                            and maximum 8); a knot with more goes to the literal evaluation
 *   CHOMP_TUNE_DEEP_MAX_FINE coarse intervals a knot may evaluate node by node (break points,
 *                            the margin above a singular satellite onset, segments shorter
 *                            than a stencil) and still take the fast sums (default and
 *                            maximum 64)
 *   CHOMP_TUNE_DEEP_SLOTS    slots of the sample buffer of the listed knots (default: one per
 *                            knot that can be listed, up to 1 GiB): with fewer slots than
 *                            listed knots the sampling and summing launches work the list off
 *                            in rounds (the path of a batch of hundreds of epochs, for a test)
 *   CHOMP_TUNE_WTHETA_DIRECT 1: w(theta) by evaluating the kernel spline at every Romberg node
 *                            (the checker of the moment route of chomp_wtheta)
 *   CHOMP_TUNE_WTHETA_EPOCH_CHUNK  epochs that chomp_wtheta_epochs evaluates per round of
 *                            launches (default 16, at most 256; its work buffer holds one chunk,
 *                            about 12 MiB per epoch at divmax = 20): a small value lets a test
 *                            cross the seam between two chunks with a handful of epochs.  It serves
 *                            both batched projections: chomp_cell_epochs takes its chunk from it
 *                            too (64 KiB + 276 bytes per multipole for every epoch of a chunk)
 *   CHOMP_TUNE_CELL_ONE_KERNEL 1: C_l with every Romberg level in the per-multipole kernel (the
 *                            checker of the hand-over to k_cell_deep)
 *   CHOMP_TUNE_ROCTX         1: roctx ranges around the stages on the host timeline (one per
 *                            entry point: "chomp:epochs_set", "chomp:stage_k", "chomp:power",
 *                            "chomp:wtheta", ...; rocprofv3 --marker-trace shows them over
 *                            the kernels they queued).  The marker library is looked up with
 *                            dlopen; CHOMP_ERR_STATE if none is installed. */
#define CHOMP_TUNE_E_STREAM_MIN 0
#define CHOMP_TUNE_DEEP_LITERAL 2
#define CHOMP_TUNE_ROCTX 3
#define CHOMP_TUNE_WTHETA_DIRECT 4
#define CHOMP_TUNE_CELL_ONE_KERNEL 5
#define CHOMP_TUNE_DEEP_TOL 6
#define CHOMP_TUNE_DEEP_MAX_BREAKS 7
#define CHOMP_TUNE_DEEP_MAX_FINE 8
#define CHOMP_TUNE_DEEP_SLOTS 10
#define CHOMP_TUNE_WTHETA_EPOCH_CHUNK 11
#define CHOMP_TUNE_COUNT 12
int chomp_set_tuning(chomp_ctx* ctx, int what, long long value);
/* Measurement aid: out[7] <- knots beyond the node tables done so far (since the context was
 * created) by [0] the fast deep-level sums, [1] literal evaluation of every node; why literal:
 * [2] too many break points, [3] too many node-by-node intervals, [4] the self-check of the
 * interpolation; [5] the largest self-check error estimate seen, in units of 1e-15; [6] why
 * literal, continued: the knot needed the integrand at a node off the coarse grid in a set-up
 * whose kernel instance carries none (every HOD with alpha = 1). */
int chomp_get_deep_stats(chomp_ctx* ctx, long long* out);

#define CHOMP_TAB_LN_MASS 0 /* MassFunction._ln_mass_array  [mass_npoints] */
#define CHOMP_TAB_NU 1      /* MassFunction._nu_array       [mass_npoints] */
#define CHOMP_TAB_H_M 2     /* knots of Halo._h_m_spline    [halo_npoints] */
#define CHOMP_TAB_PP_MM 3
#define CHOMP_TAB_H_G 4
#define CHOMP_TAB_PP_GM 5
#define CHOMP_TAB_PP_GG 6
#define CHOMP_TAB_LEVELS 7  /* Romberg levels reached, 5 x halo_npoints, as doubles */
#define CHOMP_TAB_HF_LN_SIGMA2 8 /* HaloFit._ln_sigma2_array [halo_npoints] */
#define CHOMP_TAB_I_1_2 9   /* knots of HaloSuperSampleCovariance._i_1_2_spline [halo_npoints] */
#define CHOMP_TAB_LEVELS_I_1_2 10 /* Romberg levels of the I_1^2 knots [halo_npoints], as doubles */
int chomp_get_table(chomp_ctx* ctx, size_t epoch, int table, double* out,
                    size_t n);
/* Install the knot values of one knot table (CHOMP_TAB_H_M .. CHOMP_TAB_PP_GG, CHOMP_TAB_I_1_2;
 * n = halo_npoints, host buffer) for one epoch, rebuild its not-a-knot spline over ln k with the
 * routine of the set-up and mark the table built: a get -> put round trip leaves every spectrum
 * bit for bit as it was.  What a mirror of the reference's copied or stale splines needs once
 * another object has set the epoch up again (halo.py:1116-1132: init_from_halo copies the
 * input's splines; :135-235: no setter resets _initialized_i_1_2).  The table counts as built for
 * THAT epoch only (until the next chomp_epochs_set): chomp_power refuses (CHOMP_ERR_STATE) a
 * range with an epoch that neither a set-up nor a put has given the table.  Synchronises the
 * host with the context's stream, so it is refused while the stream is being captured. */
int chomp_put_table(chomp_ctx* ctx, size_t epoch, int table, const double* in, size_t n);

/* ---- Second-order bias and perturbation theory ------------------------------ */

/* mass_function.MassFunctionSecondOrder (mass_function.py:365-434), an opt-in of the context
 * (off at creation).  With it on, every mass set-up (chomp_mass_setup, chomp_stage_k*) also keeps
 * sigma(M) at the mass_npoints knots -- the integrals that give nu (:383-386) -- builds the
 * not-a-knot sigma(nu) spline (:391-392) and integrates bias_2_norm = -int f(nu) b2(nu) dnu over
 * [nu_min, nu_max] with bias_2_norm = 0 inside (:408-414; mass_precision, global_precision and
 * divmax, the Romberg of the other normalisations; CHOMP_ST_B2_DIVMAX when divmax runs out).
 * The nu table itself stays the Sheth-Tormen one, (delta_c / sigma)^2; the subclass writes
 * delta_c / sigma * delta_c / sigma (:386), which differs from it by rounding.  Off, a set-up
 * launches what it launched before. */
int chomp_set_second_order(chomp_ctx* ctx, int on);
/* out[n] of one epoch after a second-order set-up, n = mass_npoints + 3:
 * _sigma_array [mass_npoints], bias_2_norm, its Romberg level, 1 if that Romberg converged. */
int chomp_get_second_order(chomp_ctx* ctx, size_t epoch, double* out, size_t n);

/* perturbation_spectra.PerturbationTheory (perturbation_spectra.py:59-345): the tree-level forms
 * for n configurations over the epochs [epoch0, epoch0 + n_epoch) of the batch,
 * out[(e - epoch0) n + i] (fp64).  args[i] holds the doubles of configuration i, row-major:
 *   FS2                  (:89-105)   k1[3], k2[3]                        6
 *   FS2_LEN              (:107-123)  k1, k2, z                           3
 *   FS2_KDIFF            (:125-132)  k1, k2, mu                          3
 *   FS3                  (:147-180)  k1[3], k2[3], k3[3]                 9
 *   FS3_PARALLELOGRAM    (:182-199)  k1, k2, mu                          3
 *   F3                   (:201-223)  k1[3], k2[3], k3[3]                 9
 *   FS3_BCGS             (:225-229)  k1[3], k2[3], k3[3] (default F3)    9
 *   BISPECTRUM           (:231-249)  k1[3], k2[3], k3[3]                 9
 *   BISPECTRUM_LEN       (:251-259)  k1, k2, k3, z12, z13, z23           6
 *   TRISPECTRUM          (:261-310)  k1[3], k2[3], k3[3], k4[3]         12
 *   TRISPECTRUM_PARALLELOGRAM (:312-345) k1, k2, mu                      3
 * The reference's operation order, thresholds and branches are kept (Fs3 and Fs3_BCGS disagree
 * as shipped); every P_lin is the epoch's linear spectrum as CHOMP_P_LIN computes it.  Needs
 * chomp_epochs_set only.  mem: CHOMP_HOST (staged, synchronous) or CHOMP_DEVICE (args and out in
 * HBM, asynchronous on the context's stream). */
#define CHOMP_PT_FS2 0
#define CHOMP_PT_FS2_LEN 1
#define CHOMP_PT_FS2_KDIFF 2
#define CHOMP_PT_FS3 3
#define CHOMP_PT_FS3_PARALLELOGRAM 4
#define CHOMP_PT_F3 5
#define CHOMP_PT_FS3_BCGS 6
#define CHOMP_PT_BISPECTRUM 7
#define CHOMP_PT_BISPECTRUM_LEN 8
#define CHOMP_PT_TRISPECTRUM 9
#define CHOMP_PT_TRISPECTRUM_PARALLELOGRAM 10
int chomp_pt_eval(chomp_ctx* ctx, int form, size_t epoch0, size_t n_epoch, const double* args,
                  size_t n, double* out, int mem);

/* ---- One-halo trispectrum ---------------------------------------------------- */

/* halo_trispectrum.HaloTrispectrumOneHalo (halo_trispectrum.py:13-151).  moment: the n(M) of the
 * integrand, the HOD moment its power_spec selects (:142-151) of the epoch's HOD model (the one
 * the last halo set-up installed):
 *   MMMM 1 ('power_mmmm' and any other string), GMMM <N>, GGMM <N(N-1)>, GGGM and GGGG
 *   nth_moment(n = 3, 4) by the product formula of hod.py:68-92. */
#define CHOMP_TRI_MMMM 0
#define CHOMP_TRI_GMMM 1
#define CHOMP_TRI_GGMM 2
#define CHOMP_TRI_GGGM 3
#define CHOMP_TRI_GGGG 4
/* _initialize_i_0_4 (halo_trispectrum.py:104-129) for the epochs [epoch0, epoch0 + n_epoch):
 * the N x N table (N = halo_npoints <= 64) of I_0^4(k_i, k_i, k_j, k_j) over the knots
 * ln k_i = linspace(ln k_min, ln k_max, N) -- i_0_4 (:60-95): the Romberg over
 * [ln nu_min, ln nu_max] of nu f(nu) y^2(k_i, M) y^2(k_j, M) M^3 n(M) with halo_precision,
 * global_precision and divmax, / rho_bar^3 -- the upper triangle integrated and mirrored, each
 * entry's Romberg level, and the bicubic RectBivariateSpline(kx = ky = 3, s = 0) of the table.
 * Needs a halo set-up of those epochs (chomp_halo_setup*, chomp_stage_k*; no knot table has to
 * be built).  table_out, levels_out (optional, host): n_epoch N N doubles, epoch-major,
 * row-major (synchronises).  CHOMP_ST_TRI1H_DIVMAX reports an exhausted divmax. */
int chomp_tri1h_setup(chomp_ctx* ctx, size_t epoch0, size_t n_epoch, int moment,
                      double* table_out, double* levels_out);
/* i_0_4_parallelogram's spline (halo_trispectrum.py:97-102) of one epoch's table at n points
 * (ln_k1[i], ln_k2[i]): each argument is clamped into [ln k_min, ln k_max] as FITPACK's bispev
 * does; the reference's k_min clamp and k_max mask (which shape the result) are the caller's.
 * mem: CHOMP_HOST (staged, synchronous) or CHOMP_DEVICE. */
int chomp_tri1h_eval(chomp_ctx* ctx, size_t epoch, const double* ln_k1, const double* ln_k2,
                     size_t n, double* out, int mem);
/* i_0_4 / trispectrum (halo_trispectrum.py:57-95) at n quadruples k[i][0..3] of one epoch, one
 * Romberg each (the reference's rule); out[n], levels[n] (optional) the Romberg levels.  Needs a
 * halo set-up of the epoch.  mem: CHOMP_HOST (staged, synchronous) or CHOMP_DEVICE (k, out and
 * levels in HBM, asynchronous on the context's stream). */
int chomp_tri1h_quad(chomp_ctx* ctx, size_t epoch, int moment, const double* k, size_t n,
                     double* out, double* levels, int mem);

/* ---- HaloTrispectrum (halo_trispectrum.py:153-837): the two- to four-halo terms ----
 * Tables of chomp_tri_setup / chomp_tri_table_eval. */
#define CHOMP_TRI_TAB_I_1_2 0
#define CHOMP_TRI_TAB_I_1_3 1
#define CHOMP_TRI_TAB_I_2_2 2
#define CHOMP_TRI_TAB_I_2_1 3
#define CHOMP_TRI_TAB_I_0_4 4
#define CHOMP_TRI_TAB_I_1_1 5   /* _h_m(k1): 0 outside [k_min, k_max], no clamp (halo.py:649-652) */
/* _initialize_i_0_4 / _i_1_2 / _i_1_3 / _i_2_1 / _i_2_2 (halo_trispectrum.py:592-836) for the
 * epochs [epoch0, epoch0 + n_epoch): the four N x N tables (upper triangle integrated and
 * mirrored) and the N-knot table of I_2^1, every integral's Romberg level, the bicubics and the
 * not-a-knot spline.  I_0^4 is chomp_tri1h_setup's with CHOMP_TRI_MMMM (called from here).
 * Needs a second-order mass set-up (chomp_set_second_order) and a halo set-up of those epochs.
 * tables_out, levels_out (optional, host): per epoch 4 N N + N doubles in the order I_0^4,
 * I_1^2, I_1^3, I_2^2 (row-major) and I_2^1 (synchronises).  CHOMP_ST_TRI_DIVMAX (and, for
 * I_0^4, CHOMP_ST_TRI1H_DIVMAX) reports an exhausted divmax.
 * The I_0^4 table is the context's one-halo table: a later chomp_tri1h_setup with another moment
 * replaces it, and the calls below then return CHOMP_ERR_STATE until chomp_tri_setup is called
 * again.  As for chomp_tri1h_setup, the tables belong to the mass and halo set-up they were built
 * from: after a new chomp_mass_setup / chomp_halo_setup* on the same context call this again
 * (chomp_epochs_set forgets the tables by itself). */
int chomp_tri_setup(chomp_ctx* ctx, size_t epoch0, size_t n_epoch, double* tables_out,
                    double* levels_out);
/* One table's spline (table: CHOMP_TRI_TAB_*) of one epoch at n points (k1[i], k2[i]) with the
 * reference's rules: k < k_min is clamped to k_min, k > k_max gives 0 (I_2^1 reads k1 only).
 * mem: CHOMP_HOST (staged, synchronous) or CHOMP_DEVICE. */
int chomp_tri_table_eval(chomp_ctx* ctx, size_t epoch, int table, const double* k1,
                         const double* k2, size_t n, double* out, int mem);
/* t_1_h, t_2_h, t_3_h, t_4_h (halo_trispectrum.py:320-512) at n configurations kkz[i][0..2] =
 * (k1, k2, cos theta): out[i][0..3].  epoch: the halo model's (tables of chomp_tri_setup and the
 * h_m knot table); pt_epoch: the PerturbationTheory object's, whose linear spectrum the
 * bispectrum and trispectrum forms use.  mem as above. */
int chomp_tri_terms(chomp_ctx* ctx, size_t epoch, size_t pt_epoch, const double* kkz, size_t n,
                    double* out, int mem);
/* tri_spec_proj_integral (halo_trispectrum.py:267-278) at n pairs kk[i][0..1]: out[n], and
 * (optional) levels[n], the Romberg levels, and flags[n], 1 where the result is NaN from a
 * non-finite end point or divmax ran out (CHOMP_ST_TRI_DIVMAX is raised then).  mem as above. */
int chomp_tri_proj(chomp_ctx* ctx, size_t epoch, size_t pt_epoch, const double* kk, size_t n,
                   double* out, double* levels, double* flags, int mem);
/* i_1_3(k1, k2, k3) (halo_trispectrum.py:690-705) at n triples k[i][0..2] of one epoch, one
 * Romberg each: out[n], levels[n] (optional).  Needs a halo set-up of the epoch.  mem as above. */
int chomp_tri_triple(chomp_ctx* ctx, size_t epoch, const double* k, size_t n, double* out,
                     double* levels, int mem);

/* ---- Projection: MultiEpoch, windows, kernel, correlation --------------------
 * One projection set-up per context. */

/* kernel.dNdz family (kernel.py:26-179). kind: CHOMP_DNDZ_*; p[] per kind:
 * MAGLIM {a, z0, b}; GAUSSIAN {z0, sigma_z}; BOXCAR {} -- the base class dNdz, whose
 * raw_dndz is 1 (kernel.py:56-65).  z_min/z_max are the values AFTER the constructor's
 * clipping (kernel.py:101-104, 164-173), done by the caller.
 * PPOLY: dNdzInterpolation (kernel.py:181-208), a p(z) tabulated by the caller.  The
 * reference fits a FITPACK spline of order 2 (or a smoothing spline) to the table in its
 * constructor; the caller does the same and hands the spline over as a piecewise
 * polynomial: pp_n pieces, piece i on [pp_breaks[i], pp_breaks[i + 1]] with value
 * sum_m pp_coef[i (pp_order + 1) + m] (z - pp_breaks[i])^m (host pointers, copied by
 * chomp_kernel_setup; pp_order <= 5); z_min / z_max = the table's first / last z. */
#define CHOMP_DNDZ_MAGLIM 0
#define CHOMP_DNDZ_GAUSSIAN 1
#define CHOMP_DNDZ_BOXCAR 2
#define CHOMP_DNDZ_PPOLY 3
typedef struct chomp_dndz {
  int kind;
  int pad_;
  double z_min, z_max;
  double p[4];
  const double* pp_breaks;   /* [pp_n + 1] */
  const double* pp_coef;     /* [pp_n][pp_order + 1] */
  int pp_n, pp_order;
} chomp_dndz;

/* kernel.WindowFunctionGalaxy (kernel.py:358-387) / WindowFunctionConvergence
 * (:410-484). */
#define CHOMP_WINDOW_GALAXY 0
#define CHOMP_WINDOW_CONVERGENCE 1
/* WindowFunctionFlatConvergence (kernel.py:487-513): constant 3/2 Omega_m H0^2 1907.71
 * between dist.z_min and dist.z_max; WindowFunctionConvergenceDelta (:516-556): sources on
 * one plane at z = dist.z_max.  Both take only z_min / z_max from `dist`. */
#define CHOMP_WINDOW_FLAT_CONVERGENCE 2
#define CHOMP_WINDOW_CONVERGENCE_DELTA 3
typedef struct chomp_window {
  int kind;
  int pad_;
  chomp_dndz dist;
} chomp_window;

/* cosmology.MultiEpoch(z_min, z_max, cosmo) (cosmology.py:747-817) +
 * kernel.Kernel / GalaxyGalaxyLensingKernel.__init__ and _initialize_spline
 * (kernel.py:584-649, 803-839): window tables, z_bar, 50 kernel knots.
 * bessel_order 0 (J0) or 2 (J2). */
int chomp_kernel_setup(chomp_ctx* ctx, const chomp_cosmo* cosmo, double me_z_min,
                       double me_z_max, double ktheta_min, double ktheta_max,
                       const chomp_window* a, const chomp_window* b,
                       int bessel_order);

/* cosmology.MultiEpoch alone (cosmology.py:747-817): the 50-point chi(z), z(chi),
 * D(z) tables and splines, without windows or kernel. */
int chomp_multi_epoch_setup(chomp_ctx* ctx, const chomp_cosmo* cosmo, double z_min,
                            double z_max);
/* MultiEpoch.comoving_distance / redshift / growth_factor (cosmology.py:873-953)
 * of the context's MultiEpoch (after chomp_multi_epoch_setup or chomp_kernel_setup). */
#define CHOMP_ME_CHI_OF_Z 0
#define CHOMP_ME_Z_OF_CHI 1
#define CHOMP_ME_GROWTH_OF_Z 2
int chomp_me_eval(chomp_ctx* ctx, int what, const double* x, size_t n, double* out,
                  int mem);

#define CHOMP_KI_Z_BAR 0
#define CHOMP_KI_CHI_MIN 1
#define CHOMP_KI_CHI_MAX 2
#define CHOMP_KI_Z_MIN 3
#define CHOMP_KI_Z_MAX 4
#define CHOMP_KI_D_ZBAR 5 /* MultiEpoch.growth_factor(z_bar), correlation.py:94 */
#define CHOMP_KI_NORM_A 6 /* dNdz.norm of window a's distribution */
#define CHOMP_KI_NORM_B 7
#define CHOMP_KI_WA_CHI_MIN 8 /* WindowFunction.chi_min / chi_max of window a, b */
#define CHOMP_KI_WA_CHI_MAX 9
#define CHOMP_KI_WB_CHI_MIN 10
#define CHOMP_KI_WB_CHI_MAX 11
#define CHOMP_KI_J_LIMIT 12   /* Kernel._j0_limit / _j2_limit */
#define CHOMP_KI_COUNT 13
int chomp_kernel_info(chomp_ctx* ctx, double* out);

#define CHOMP_KTAB_LN_KTHETA 0 /* Kernel._ln_ktheta_array [kernel_npoints]   */
#define CHOMP_KTAB_KERNEL 1    /* Kernel._kernel_array    [kernel_npoints]   */
#define CHOMP_KTAB_WA_CHI 2    /* window a _chi_array     [window_npoints]   */
#define CHOMP_KTAB_WA 3        /* window a _wf_array                          */
#define CHOMP_KTAB_WB_CHI 4
#define CHOMP_KTAB_WB 5
#define CHOMP_KTAB_ME_Z 6      /* MultiEpoch._z_array     [cosmo_npoints]    */
#define CHOMP_KTAB_ME_CHI 7
#define CHOMP_KTAB_ME_GROWTH 8
#define CHOMP_KTAB_LEVELS 9
int chomp_kernel_table(chomp_ctx* ctx, int table, double* out, size_t n);

/* The cosmology axis of the projection set-up.  A design or chain over cosmology calls
 * Kernel.set_cosmology once per point (kernel.py:657-676, from Correlation.set_cosmology,
 * correlation.py:161-171, in the loop of simulation_design.py:116-155): new MultiEpoch tables,
 * windows, chi limits, z_bar and kernel knots each time.  chomp_kernel_setup_sets builds n_set
 * such set-ups that differ in cosmology only -- windows, redshift distributions, k theta range
 * and Bessel order are shared -- with the six launches of chomp_kernel_setup run once, on the
 * context's stream.  The sets live beside the single set-up of chomp_kernel_setup, which (with
 * the covariance, ssc and NG tables built on it) is left as it was; their buffers are kept
 * across calls.  Set s holds, bit for bit, what chomp_kernel_setup(ctx, &cosmo[s], ...) builds.
 * Validates what chomp_kernel_setup validates; in addition CHOMP_ERR_SCOPE, before anything is
 * launched, for a CHOMP_DNDZ_PPOLY distribution and for any cosmology with w0/wa != -1/0 (both
 * are set up by chomp_kernel_setup, one cosmology at a time) unless chomp_set_sets_scope, below,
 * has let them in, and CHOMP_ERR_ARG for n_set = 0 or n_set > CHOMP_KERNEL_SETS_MAX (callers
 * work longer designs off in blocks of that size). */
#define CHOMP_KERNEL_SETS_MAX 1024
int chomp_kernel_setup_sets(chomp_ctx* ctx, size_t n_set, const chomp_cosmo* cosmo /*[n_set]*/,
                            double me_z_min, double me_z_max, double ktheta_min,
                            double ktheta_max, const chomp_window* a, const chomp_window* b,
                            int bessel_order);
/* The kernel axis of the projection set-up.  A tomographic analysis is the opposite case: one
 * cosmology, many window pairs (five lens bins give 15 galaxy-galaxy kernels, every lens x source
 * pair a galaxy-galaxy-lensing one: a Kernel / GalaxyGalaxyLensingKernel each, kernel.py:559-839),
 * and a chain over photo-z nuisance parameters rebuilds them all at every step.
 * chomp_kernel_setup_pairs builds
 * n_set projection set-ups that may differ in everything but the k theta range and the Bessel
 * order: set s holds, bit for bit, what chomp_kernel_setup(ctx, &cosmo[s], me_z_min[s],
 * me_z_max[s], ktheta_min, ktheta_max, &a[s], &b[s], bessel_order) builds.
 * It fills the same sets as chomp_kernel_setup_sets with the same six launches (the later of the
 * two calls holds), so chomp_kernel_info_sets, chomp_kernel_table_set, chomp_wtheta_sets and
 * chomp_cell_sets serve either set-up.  Every set is validated before anything is launched and a
 * refusal names the set ("set 1"): what chomp_kernel_setup_sets validates, with all four window
 * kinds of chomp_kernel_setup; CHOMP_ERR_SCOPE for a CHOMP_DNDZ_PPOLY distribution or a w0/wa !=
 * -1/0 cosmology in any set (unless chomp_set_sets_scope has let them in); CHOMP_ERR_ARG for
 * n_set = 0, n_set > CHOMP_KERNEL_SETS_MAX and null arrays. */
int chomp_kernel_setup_pairs(chomp_ctx* ctx, size_t n_set, const chomp_cosmo* cosmo /*[n_set]*/,
                             const double* me_z_min /*[n_set]*/, const double* me_z_max /*[n_set]*/,
                             double ktheta_min, double ktheta_max,
                             const chomp_window* a /*[n_set]*/, const chomp_window* b /*[n_set]*/,
                             int bessel_order);
/* What the two calls above take beyond analytic distributions in Lambda-CDM, opt-in (flags: an
 * OR of CHOMP_SETS_*, 0 at creation; CHOMP_ERR_ARG for an unknown bit).  With a flag off, the
 * calls refuse that input as they always did, with the same text; nothing else reads the flags.
 *   CHOMP_SETS_TABULATED    CHOMP_DNDZ_PPOLY distributions.  The distinct tables of a call -- equal
 *     in pp_n, pp_order and bytes, whatever their addresses: five bins behind 15 kernels are five
 *     tables -- are copied, during the call, into an arena of the sets' own, which is kept across
 *     calls and only grows.  CHOMP_ERR_ARG when they exceed 2^22 doubles (32 MiB: nine tables of
 *     65536 pieces of order 5); nothing is allocated or copied then.
 *   CHOMP_SETS_DARK_ENERGY  cosmologies with w0/wa != -1/0, whatever chomp_set_dark_energy says.
 *     The distinct (w0, wa) of a call get pressure tables of the sets' own (as chomp_set_dark_energy
 *     describes them), and the two launches that evaluate E(z) run in a form that looks its set's
 *     table up; a Lambda-CDM set beside them does the arithmetic of a Lambda-CDM batch, and a
 *     batch without a w0-wa cosmology makes the launches it makes with the flag off.
 * Either way set s holds, bit for bit, what chomp_kernel_setup builds for it (with
 * chomp_set_dark_energy(ctx, 1) where its cosmology needs that), and the single set-up, its
 * tables behind it and its pressure table stay as they are. */
#define CHOMP_SETS_TABULATED 1u
#define CHOMP_SETS_DARK_ENERGY 2u
int chomp_set_sets_scope(chomp_ctx* ctx, unsigned flags);
/* chomp_kernel_info of every set of the last set-up of sets: out[s * CHOMP_KI_COUNT +
 * CHOMP_KI_*], in ONE synchronising read-back.  CHOMP_ERR_STATE before any such set-up. */
int chomp_kernel_info_sets(chomp_ctx* ctx, double* out /*[n_set * CHOMP_KI_COUNT]*/);
/* chomp_kernel_table of set `set` (CHOMP_ERR_ARG beyond the last set-up's sets). */
int chomp_kernel_table_set(chomp_ctx* ctx, size_t set, int table, double* out, size_t n);

/* Kernel.raw_kernel(ln_ktheta) (kernel.py:678-704): the projection integral itself, not
 * its 50-knot spline. */
int chomp_kernel_raw(chomp_ctx* ctx, const double* ln_ktheta, size_t n,
                     double* out, int mem);
/* Kernel.kernel(ln_ktheta) (kernel.py:714-729); argument is ln(k*theta). */
int chomp_kernel_eval(chomp_ctx* ctx, const double* ln_ktheta, size_t n,
                      double* out, int mem);
/* WindowFunction.window_function(chi) (kernel.py:326-340) of window 0 (a) / 1 (b). */
int chomp_window_eval(chomp_ctx* ctx, int which_window, const double* chi,
                      size_t n, double* out, int mem);

/* Correlation.correlation(theta_rad) (correlation.py:242-275):
 * w(theta) = int dlnk k^2/(2 pi) P(k)/D_z^2 K(ln k theta), one wavefront-group per
 * theta.  P is `which` of halo epoch `epoch` (the caller has moved the halo to
 * z_bar as Correlation.__init__ does, correlation.py:102-103). */
int chomp_wtheta(chomp_ctx* ctx, int which, size_t epoch, double k_min,
                 double k_max, double D_z, const double* theta, size_t n,
                 double* out, int mem);
/* Correlation.correlation(theta) for epochs epoch0 .. epoch0 + n_epoch - 1 of one context that
 * share the projection set-up, k range and D_z: out[e * n + i] = what chomp_wtheta(ctx, which,
 * epoch0 + e, ..., theta, n, ...) returns at i, bit for bit.  The batch axis of an HOD design or
 * chain (the loop of set_hod + correlation in the reference's example script, and
 * simulation_design.py:116-155 over HOD parameters): the epochs differ in their halo-model
 * tables only, and the three launches of chomp_wtheta run once per chunk of 16 epochs
 * (CHOMP_TUNE_WTHETA_EPOCH_CHUNK) instead of once per epoch.  fp64 only; CHOMP_ERR_SCOPE for the
 * narrowed precision modes, for HaloFit spectra (CHOMP_P_HALOFIT), for spectra extrapolated
 * beyond the halo's k range (CHOMP_P_EXTRAPOLATE on a halo-model spectrum) and for a context with
 * the wiggle transfer function (chomp_set_transfer): chomp_wtheta serves those, one epoch at a
 * time. */
int chomp_wtheta_epochs(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, double k_min,
                        double k_max, double D_z, const double* theta, size_t n, double* out,
                        int mem);
/* Correlation.correlation(theta) over cosmologies: epoch epoch0 + e of the context is integrated
 * against projection set e of the last set-up of sets with growth D_z[e] (a HOST array
 * whatever `mem` says; the caller has moved epoch e to set e's z_bar, correlation.py:161-171):
 * out[e * n + i] = what chomp_wtheta(ctx, which, epoch0 + e, k_min, k_max, D_z[e], theta, n, ...)
 * returns at i after chomp_kernel_setup with cosmo[e], bit for bit -- both run the same bodies on
 * the same inputs.  The scope, routes and chunking of chomp_wtheta_epochs (fp64 only;
 * CHOMP_ERR_SCOPE for HaloFit codes, extrapolated halo-model spectra and the wiggle transfer
 * function; CHOMP_TUNE_WTHETA_EPOCH_CHUNK).  n_epoch must be the number of sets
 * (CHOMP_ERR_ARG); CHOMP_ERR_STATE before any set-up of sets.  chomp_cell_sets is the same call
 * for C_l. */
int chomp_wtheta_sets(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, double k_min,
                      double k_max, const double* D_z /*[n_epoch], host*/, const double* theta,
                      size_t n, double* out, int mem);
/* Gaussian covariance of w(theta), Covariance(corr, corr) with nongaussian_cov=False.
 *
 * chomp_covariance_table replaces Covariance._initialize_halo_splines (covariance.py:455-543,
 * the matching_corrs branch): on kernel_npoints knots in ln K, from ln(k_min chi_min) to
 * ln(k_max chi_max) (covariance.py:159-175), the projected spectrum
 *   int dchi P(K/chi) W_a(chi) W_b(chi) D(chi)^2 / chi^2
 * of `which` of halo epoch `epoch` (moved to the kernel's z_bar by the caller, :460) with
 * the reference's limits, normalisation and Romberg tolerances, and its spline.  D_z is
 * MultiEpoch.growth_factor(z_bar) (:464).  ln_K / proj / levels (each [n = kernel_npoints],
 * host, may be NULL) receive the knots, the table and the Romberg levels reached.
 *
 * chomp_covariance_gaussian replaces Covariance.covariance_G (covariance.py:361-453) for n
 * pairs of bin centres: theta holds theta_a[n] then theta_b[n] (radians).  j0_limit is
 * Covariance._j0_limit (:188-189), area the survey area in steradians, poisson_a /
 * poisson_b the shot-noise terms proj_power_poisson(0) / (2) of the integrand (:427-432). */
int chomp_covariance_table(chomp_ctx* ctx, int which, size_t epoch, double D_z,
                           double* ln_K, double* proj, double* levels, size_t n);
int chomp_covariance_gaussian(chomp_ctx* ctx, double j0_limit, double area,
                              double poisson_a, double poisson_b,
                              const double* theta, size_t n, double* out, int mem);

/* Gaussian cross-covariance of two w(theta), Covariance(corr_a, corr_b) with two different
 * correlations and nongaussian_cov=False: the matching_corrs == False branch
 * (covariance.py:422-453, 495-541).
 *
 * A cross block reads four windows and two P(k) epochs, and a context holds one projection
 * set-up and -- for one Halo object -- one epoch.  chomp_covariance_cross_stage therefore takes
 * a snapshot of one side into `ctx`: slot 0 is correlation a, slot 1 correlation b.  `src` (which
 * may be `ctx` itself) is the context that holds that side now: its kernel_setup (windows,
 * MultiEpoch, z range) and spectrum `which` of its halo epoch `epoch`, moved to that
 * correlation's z_bar by the caller (:465-466).  Later changes of `src` do not reach the
 * snapshot.  Both contexts must be on one device and share configuration and transfer function
 * (CHOMP_ERR_SCOPE otherwise).  When src is another context the call waits for both streams.
 * which = CHOMP_CROSS_WINDOWS takes the projection set-up alone (src needs no halo epoch): enough
 * for the kernels of the four windows, chomp_kernel_ssc_setup_cross and what follows it.
 *
 * chomp_covariance_table_cross replaces Covariance._initialize_halo_splines for the block: on
 * kernel_npoints knots in ln K from ln(k_min min(chi_min_a, chi_min_b)) to
 * ln(k_max max(chi_max_a, chi_max_b)) (:162-167) the four projected spectra
 *   a:  P_a W_a1 W_a2,  b:  P_b W_b1 W_b2,  ab: sqrt(P_a P_b) W_a1 W_b2,  ba: sqrt(P_a P_b) W_a2 W_b1
 * (each times D^2 / chi^2, over chi) with the reference's limits -- a's range, b's range, and for
 * ab / ba b's clamped again to a's -- normalisations and Romberg tolerances, and their splines.
 * Growth factor, z(chi) and the chi limits of both sides are those of slot 0's MultiEpoch
 * (Covariance.kernel.cosmo is correlation a's).  D_a / D_b are its growth_factor(z_bar_a / b)
 * (:468-469).  ln_K [n], tables [4][n] and levels [4][n] (n = kernel_npoints, host, may be
 * NULL; rows in the order a, b, ab, ba) receive the knots, the tables and the Romberg levels.
 *
 * chomp_covariance_gaussian_cross replaces Covariance.covariance_G for n pairs of bin centres
 * of the block: theta holds theta_a[n] then theta_b[n] (radians); poisson_p is
 * proj_power_poisson(window_pair = p) (:427-428, 443-444); j0_limit and area as in
 * chomp_covariance_gaussian. */
#define CHOMP_CROSS_WINDOWS (-1)
int chomp_covariance_cross_stage(chomp_ctx* ctx, int slot, chomp_ctx* src, int which,
                                 size_t epoch);
int chomp_covariance_table_cross(chomp_ctx* ctx, double D_a, double D_b, double* ln_K,
                                 double* tables, double* levels, size_t n);
int chomp_covariance_gaussian_cross(chomp_ctx* ctx, double j0_limit, double area,
                                    double poisson_0, double poisson_1, double poisson_2,
                                    double poisson_3, const double* theta, size_t n,
                                    double* out, int mem);

/* Every Gaussian block of a CovarianceMulti (covariance.py:796-871) in one call.
 *
 * Correlation c (c < n_corr) is projection set c of the last chomp_kernel_setup_pairs (or
 * chomp_kernel_setup_sets) of Bessel order 0 and P(k) epoch epoch[c] of this context, moved to
 * that set's z_bar by the caller.  The n_blocks = n_corr (n_corr + 1) / 2 blocks (i, j), i <= j,
 * are in the row-major order of the upper triangle -- (0,0), (0,1) ... (0,n-1), (1,1) ... --, the
 * order of CovarianceMulti.covariance_list.  A diagonal block is what chomp_kernel_setup (kernel
 * i) + chomp_covariance_table(which, epoch[i], D_zbar of set i) + chomp_covariance_gaussian with
 * poisson[b][0] and poisson[b][2] return; a cross block what chomp_covariance_cross_stage of
 * (kernel i, epoch[i]) and (kernel j, epoch[j]) + chomp_covariance_table_cross(D_a, D_b) +
 * chomp_covariance_gaussian_cross with poisson[b][0..3] return, D_a = D_zbar of set i and D_b the
 * growth factor of set i's MultiEpoch at set j's z_bar (:468-469): bit for bit, the blocks being
 * a grid dimension of kernels that run the single calls' code.  Both sides of a block are read
 * where they lie (no snapshot), and the call touches neither the context's single projection
 * set-up nor the state of chomp_covariance_table / chomp_covariance_cross_stage.
 *
 * theta holds theta_a[n_pairs] then theta_b[n_pairs] (radians), the same pairs for every block;
 * out [n_blocks][n_pairs].  theta, poisson and out are host or device arrays as `mem` says
 * ("Memory-space convention"); epoch is a host array.  j0_limit and area as in
 * chomp_covariance_gaussian; the transfer function and `which` as in chomp_covariance_table
 * (an extrapolated spectrum has its constants refreshed first).
 * CHOMP_ERR_STATE: no set-up of sets, one of another number of sets than n_corr, or of Bessel
 * order 2.  CHOMP_ERR_ARG: an epoch out of range, more than 65535 blocks (they are a grid's z
 * dimension), j0_limit or area not positive, a host theta not positive.
 *
 * chomp_covariance_blocks_table reads the tables of block `block` of the last call: ln_K [n],
 * tables [4][n] and levels [4][n] (n = kernel_npoints; rows a, b, ab, ba -- of a diagonal block
 * row 0 alone, the others zero) and scalars [8]: {ln_K_min, ln_K_max, D_a, D_b, chi_peak_a,
 * chi_peak_b} of a cross block, {ln_K_min, ln_K_max, D_z, chi_peak, 0, 0} of a diagonal one, then
 * D_a and D_b as the call's first kernel found them.  Host arrays; any may be NULL. */
int chomp_covariance_blocks(chomp_ctx* ctx, int which, size_t n_corr,
                            const size_t* epoch /*[n_corr]*/, double j0_limit, double area,
                            const double* poisson /*[n_blocks][4]*/,
                            const double* theta /*[2][n_pairs]: theta_a then theta_b*/,
                            size_t n_pairs, double* out /*[n_blocks][n_pairs]*/, int mem);
int chomp_covariance_blocks_table(chomp_ctx* ctx, size_t block, double* ln_K,
                                  double* tables /*[4][N]*/, double* levels /*[4][N]*/,
                                  double* scalars /*[8]*/, size_t n);

/* Super-sample covariance of w(theta), Covariance(corr, corr, nongaussian_cov=False,
 * ssc_cov=True), with a1 = b1 = window a and a2 = b2 = window b of the context's
 * kernel_setup.  Host memory throughout.
 *
 * chomp_kernel_ssc_setup replaces KernelCovariance._find_z_bar (kernel.py:961-972),
 * _initialize_sigma2_spline (:1208-1222) and _initialize_ssc_spline (:1132-1153).  The
 * sigma^2 knots (ln chi[n_sigma], sigma2[n_sigma]: MultiEpoch.sigma_r(chi, 0)^2 on
 * logspace(log10 chi_min, log10 chi_max, corr_npoints)) get their not-a-knot spline; the
 * kernel_npoints x kernel_npoints table of raw_kernel_ssc over linspace(ln_ktheta_min,
 * ln_ktheta_max, kernel_npoints) is integrated (upper triangle, mirrored) with the J0 limit
 * j0_ssc_limit (kernel.py:951-952) and fitted with the tensor-product bicubic of
 * RectBivariateSpline(s=0).  with_table = 0 stops after the sigma^2 spline and z_bar_NG (what
 * chomp_kernel_ssc_raw needs); the table, its bicubic and the other two calls need 1.
 * info[3] (z_bar_NG, chi(z_bar_NG), growth_factor(z_bar_NG)), table and levels (each
 * [kernel_npoints^2], row-major in ln(k theta_a); with_table only) may be NULL.
 *
 * chomp_kernel_ssc_raw replaces raw_kernel_ssc (kernel.py:1155-1206) and
 * chomp_kernel_ssc_eval kernel_ssc (:1113-1130) at n points: ln_ktheta holds ln(k theta_a)[n]
 * then ln(k theta_b)[n].
 *
 * chomp_covariance_ssc replaces Covariance.covariance_ssc (covariance.py:685-776) for n pairs
 * of bin centres: theta holds theta_a[n] then theta_b[n] (radians); the response
 * dlnP_mm/ddelta_b is that of halo epoch `epoch` (HaloSuperSampleCovariance's tables).  area
 * is in steradians.  kb_knots / kb_levels ([n * kernel_npoints], may be NULL) receive each
 * pair's k_b integrals at the k_a knots and their Romberg levels. */
int chomp_kernel_ssc_setup(chomp_ctx* ctx, double ln_ktheta_min, double ln_ktheta_max,
                           double j0_ssc_limit, const double* ln_chi, const double* sigma2,
                           size_t n_sigma, int with_table, double* info, double* table,
                           double* levels);
int chomp_kernel_ssc_raw(chomp_ctx* ctx, const double* ln_ktheta, size_t n, double* out);
int chomp_kernel_ssc_eval(chomp_ctx* ctx, const double* ln_ktheta, size_t n, double* out);
int chomp_covariance_ssc(chomp_ctx* ctx, size_t epoch, double area, const double* theta,
                         size_t n, double* out, double* kb_knots, double* kb_levels);

/* The super-sample and trispectrum terms of a cross block, Covariance(corr_a, corr_b,
 * cross_terms=True): KernelCovariance with a1 != b1 or a2 != b2 (kernel.py:893-972, 1035-1111,
 * 1155-1206) and _kb_ssc_integrand with halo_a at k_a and halo_b at k_b (covariance.py:763-776).
 * Everything works from the two slots of chomp_covariance_cross_stage: slot 0 holds a1, a2 and
 * the MultiEpoch (correlation a's throughout, kernel.py:918-931), slot 1 holds b1, b2.  The window
 * product is a1 a2 b1 b2 in that order.  Host memory throughout.
 *
 * chomp_covariance_cross_range gives info[4] = z_min, z_max, chi_min, chi_max of the four windows:
 * z_min the largest of their z_min, z_max the smallest of their z_max, chi_min =
 * max(window_precision, chi(z_min)), chi_max = chi(z_max) (kernel.py:910-931) -- the range the
 * caller lays the sigma^2 knots over.  Windows with no redshift in common (z_min >= z_max) are
 * CHOMP_ERR_SCOPE, here and in the calls below, before anything is launched.
 *
 * chomp_kernel_ssc_setup_cross is chomp_kernel_ssc_setup for those four windows: same
 * arguments, limits, norm, tolerances and outputs.  The kernel_ssc state of the context is
 * then the block's: chomp_kernel_ssc_raw / _eval, chomp_kernel_ng_setup / _raw / _eval and
 * chomp_covariance_ng serve it unchanged (chomp_kernel_ng_setup takes its windows from where the
 * kernel_ssc state took them).  Staging a slot again drops it.
 *
 * chomp_covariance_ssc_cross is chomp_covariance_ssc with two responses: dlnP_mm/ddelta_b of
 * slot 0's epoch at k_a and of slot 1's at k_b (both snapshots must have been taken with the
 * families h_m, pp_mm and i_1_2 built: CHOMP_ERR_STATE otherwise).  The order of the arguments
 * matters: (theta_a, theta_b) is not (theta_b, theta_a). */
int chomp_covariance_cross_range(chomp_ctx* ctx, double* info);
int chomp_kernel_ssc_setup_cross(chomp_ctx* ctx, double ln_ktheta_min, double ln_ktheta_max,
                                 double j0_ssc_limit, const double* ln_chi, const double* sigma2,
                                 size_t n_sigma, int with_table, double* info, double* table,
                                 double* levels);
int chomp_covariance_ssc_cross(chomp_ctx* ctx, double area, const double* theta, size_t n,
                               double* out, double* kb_knots, double* kb_levels);

/* The super-sample term of every block of a CovarianceMulti(ssc_cov=True, cross_terms=True) in
 * one call, beside chomp_covariance_blocks: the same correlations (projection set c of the last
 * chomp_kernel_setup_pairs of Bessel order 0, halo epoch epoch[c] of this context at that set's
 * z_bar, holding the families h_m, pp_mm and i_1_2), the same n_blocks = n_corr (n_corr + 1) / 2
 * blocks (i, j), i <= j, in the row-major order of the upper triangle.  A diagonal block is what
 * chomp_kernel_setup (kernel i) + chomp_kernel_ssc_setup + chomp_covariance_ssc(epoch[i]) return;
 * a cross block what chomp_covariance_cross_stage of (kernel i, epoch[i]) and (kernel j, epoch[j])
 * + chomp_kernel_ssc_setup_cross + chomp_covariance_ssc_cross return -- a1, a2 and the MultiEpoch
 * from set i, b1, b2 from set j, the response of epoch[i] at k_a and of epoch[j] at k_b, so the
 * order of the two angles matters: bit for bit, the blocks being a grid dimension of kernels that
 * run the single calls' code.  Both sides of a block are read where they lie (no snapshot); the
 * call keeps a state of its own and touches neither the context's kernel_ssc state, nor the two
 * slots of chomp_covariance_cross_stage, nor the state of chomp_covariance_blocks.
 *
 * chomp_covariance_ssc_blocks_range gives info[n_blocks][4] = z_min, z_max, chi_min, chi_max of
 * every block's windows -- a diagonal block's as chomp_kernel_info returns them, a cross block's
 * as chomp_covariance_cross_range does -- in one launch and one read-back: the ranges the caller
 * lays the blocks' sigma^2 knots over.  A block whose windows have no redshift in common is
 * CHOMP_ERR_SCOPE naming the block, here and in chomp_covariance_ssc_blocks, before anything is
 * launched.
 *
 * chomp_covariance_ssc_blocks: ln_ktheta_min, ln_ktheta_max, j0_ssc_limit and n_sigma as in
 * chomp_kernel_ssc_setup; ln_chi and sigma2 (host, [n_blocks][n_sigma]) hold every block's own
 * sigma^2 knots; area and theta (theta_a[n_pairs] then theta_b[n_pairs], the same pairs for every
 * block) as in chomp_covariance_ssc; out [n_blocks][n_pairs].  theta and out are host or device
 * arrays as `mem` says ("Memory-space convention"); epoch, ln_chi and sigma2 are host arrays.
 * CHOMP_ERR_STATE: no set-up of sets, one of another number of sets than n_corr or of Bessel
 * order 2, an epoch without the response's knot tables.  CHOMP_ERR_ARG: an epoch out of range,
 * more than 65535 blocks or pairs, what chomp_kernel_ssc_setup refuses (per block for the knots),
 * area or a host theta not positive, a configuration whose windows or responses do not fit a
 * workgroup's LDS.
 *
 * chomp_covariance_ssc_blocks_table reads block `block` of the last call: info[7] = z_bar_NG,
 * chi(z_bar_NG), growth_factor(z_bar_NG), z_min, z_max, chi_min, chi_max; table and levels
 * [kernel_npoints^2]; kb_knots and kb_levels [n_pairs * kernel_npoints].  Host arrays; any may
 * be NULL. */
int chomp_covariance_ssc_blocks_range(chomp_ctx* ctx, size_t n_corr,
                                      double* info /*[n_blocks][4]*/);
int chomp_covariance_ssc_blocks(chomp_ctx* ctx, size_t n_corr, const size_t* epoch /*[n_corr]*/,
                                double ln_ktheta_min, double ln_ktheta_max, double j0_ssc_limit,
                                const double* ln_chi /*[n_blocks][n_sigma]*/,
                                const double* sigma2 /*[n_blocks][n_sigma]*/, size_t n_sigma,
                                double area,
                                const double* theta /*[2][n_pairs]: theta_a then theta_b*/,
                                size_t n_pairs, double* out /*[n_blocks][n_pairs]*/, int mem);
int chomp_covariance_ssc_blocks_table(chomp_ctx* ctx, size_t block, double* info /*[7]*/,
                                      double* table, double* levels, double* kb_knots,
                                      double* kb_levels);

/* Gaussian covariance of C_l, covariance.CovarianceFourier (covariance.py:874-1083): four Limber
 * tables over ln l, one per window pair X = a1a2, b1b2, a1b2, b1a2 (that order throughout), each
 * from the P_mm of a halo epoch at that pair's z_bar.
 *
 * The four windows come from the two slots of chomp_covariance_cross_stage (CHOMP_CROSS_WINDOWS is
 * enough): slot 0 holds a1, a2 and the MultiEpoch, slot 1 holds b1, b2.  The three calls below keep
 * a state of their own in `ctx`; they read the slots and the context's epochs and change neither.
 * Staging a slot again after chomp_covariance_fourier_zbar makes the scalars stale: call it again.
 *
 * chomp_covariance_fourier_zbar replaces _calculate_zbar (:1067-1075) for the four pairs: on the
 * caller's grid z[n_z] (CovarianceFourier._z_array, n_z <= 256) the first maximum of
 * w1 w2 / chi^2 D(z(chi))^2 at chi = comoving_distance(z), as numpy.argmax finds it.  A pair whose
 * two windows have no redshift in common is CHOMP_ERR_SCOPE before anything is launched.  info[4][7]
 * (host, may be NULL) receives per pair z_min (the larger of its windows' z_min), z_max (the
 * smaller of their z_max), z_bar, comoving_distance(z_bar), comoving_distance(z_min),
 * comoving_distance(z_max) and growth_factor(z_bar), all of slot 0's MultiEpoch.  Synchronises.
 *
 * chomp_covariance_fourier_table replaces _initialize_pl (:958-1065): for every knot ln_l[n]
 * (host, increasing, n = corr_npoints) and pair the Romberg integral over [chi(z_min_X),
 * chi(z_max_X)] of norm_X w1 w2 D^2 / chi^2 P(l / chi) at global_precision / corr_precision /
 * divmax, divided by growth_factor(z_bar_X)^2, and the not-a-knot spline of its logarithm.  `which`
 * is CHOMP_P_MM, with CHOMP_P_EXTRAPOLATE or without (anything else: CHOMP_ERR_SCOPE); epoch[X] is
 * the context's halo epoch that carries pair X's spectrum -- the caller has moved it to z_bar_X;
 * pairs may share an epoch.  norm_X is formed as the reference forms it, quirks included
 * (:987-1006): the reciprocal of the integrand at chi(z_bar_X) with l = chi, the windows a1 and a2
 * whatever the pair, and the spectrum of epoch[X] -- except for a1b2, which takes epoch[0]'s
 * (halo_a1a2).  A norm integrand that is not positive and finite leaves that pair's table NaN and
 * its norm as 1 / integrand; the caller decides.  norms[4], tables[4][n] and levels[4][n] (host,
 * may be NULL) receive the norms, the tables (integral / D^2, before the logarithm) and the
 * Romberg levels reached.  Synchronises.
 *
 * chomp_covariance_fourier_gaussian replaces _pl_a1a2 .. _pl_b1a2 (:934-956) and covariance_G
 * (:928-932) at n multipoles: l holds ln l[n] then l[n] -- the logarithms are the caller's, so the
 * range rule ln_l[0] <= ln l <= ln_l[n-1] is decided by the caller's arithmetic -- and out[5][n]
 * receives the four _pl_X = exp(spline_X(ln l)) / norm_X (exactly 0 outside the range) and
 * covariance_G = (pl_a1a2 pl_b1b2 + pl_a1b2 pl_b1a2) / (2 l + 1). */
int chomp_covariance_fourier_zbar(chomp_ctx* ctx, const double* z, size_t n_z, double* info);
int chomp_covariance_fourier_table(chomp_ctx* ctx, int which, const size_t epoch[4],
                                   const double* ln_l, size_t n, double* norms, double* tables,
                                   double* levels);
int chomp_covariance_fourier_gaussian(chomp_ctx* ctx, const double* l, size_t n, double* out,
                                      int mem);

/* One-halo trispectrum term of the covariance of w(theta), Covariance(corr, corr,
 * nongaussian_cov=True, input_halo_trispectrum=HaloTrispectrumOneHalo), with a1 = b1 = window a
 * and a2 = b2 = window b of the context's kernel_setup.  Host memory throughout.
 *
 * chomp_kernel_ng_setup replaces KernelCovariance._initialize_NG_spline (kernel.py:1016-1030).
 * It needs chomp_kernel_ssc_setup (with_table 0 is enough) for z_bar_NG, chi(z_bar_NG),
 * growth_factor(z_bar_NG) and the ln(k theta) knots, and keeps its own copy of them.  The
 * kernel_npoints x kernel_npoints table of raw_kernel_NG (:1035-1073: the Romberg over chi up
 * to max(j0_limit / k theta_a, j0_limit / k theta_b), j0_limit being _j0_limit, :944-945) is
 * integrated (upper triangle, mirrored); min = min(table), and log(table - 10 min) gets the
 * tensor-product bicubic of RectBivariateSpline(s=0).  with_table = 0 stops before the table
 * (what chomp_kernel_ng_raw needs); the other two calls need 1.  table and levels (each
 * [kernel_npoints^2], row-major in ln(k theta_a)) and table_min[1] may be NULL (with_table
 * only).
 *
 * chomp_kernel_ng_raw replaces raw_kernel / raw_kernel_NG and chomp_kernel_ng_eval kernel /
 * kernel_NG (:996-1014: exp(spline) + 10 min; ln(k theta) below the range is clamped, above it
 * the value is 0) at n points: ln_ktheta holds ln(k theta_a)[n] then ln(k theta_b)[n].
 *
 * chomp_covariance_ng replaces Covariance.covariance_NG (covariance.py:593-683) for n pairs of
 * bin centres: theta holds theta_a[n] then theta_b[n] (radians), area is in steradians.  The
 * trispectrum is trispectrum_parallelogram of a HaloTrispectrumOneHalo (halo_trispectrum.py:
 * 100-106): tri_table[n_tri^2] is its I_0^4 table (chomp_tri1h_setup's, row-major) over
 * linspace(ln tri_k_min, ln tri_k_max, n_tri); the call rebuilds that table's bicubic with the
 * routine of chomp_tri1h_setup and applies the k_min clamp and the k_max mask.  kb_knots /
 * kb_levels ([n * kernel_npoints], may be NULL) receive each pair's k_b integrals at the k_a
 * knots (divided by growth_factor(z_bar_NG)^4) and their Romberg levels.
 * CHOMP_ST_COV_NG_DIVMAX reports an exhausted divmax. */
int chomp_kernel_ng_setup(chomp_ctx* ctx, double j0_limit, int with_table, double* table,
                          double* levels, double* table_min);
int chomp_kernel_ng_raw(chomp_ctx* ctx, const double* ln_ktheta, size_t n, double* out);
int chomp_kernel_ng_eval(chomp_ctx* ctx, const double* ln_ktheta, size_t n, double* out);
int chomp_covariance_ng(chomp_ctx* ctx, double area, const double* tri_table, size_t n_tri,
                        double tri_k_min, double tri_k_max, const double* theta, size_t n,
                        double* out, double* kb_knots, double* kb_levels);

/* The one-halo trispectrum term of EVERY block of a CovarianceMulti(nongaussian_cov=True,
 * cross_terms=True) in one call: the block axis of chomp_covariance_blocks and
 * chomp_covariance_ssc_blocks for the third term.  Correlation c is projection set c of the last
 * chomp_kernel_setup_pairs (Bessel order 0); block (i, j), i <= j, in the row-major order of the
 * upper triangle, reads set i and set j where they lie.  The term reads no halo epoch and no
 * sigma^2 knot: the host sends neither knots nor a range, and nothing is read back before the
 * result.
 *
 * A diagonal block is, bit for bit, what chomp_kernel_setup, chomp_kernel_ssc_setup(with_table 0),
 * chomp_kernel_ng_setup and chomp_covariance_ng return for kernel i; a cross block what two
 * chomp_covariance_cross_stage, chomp_kernel_ssc_setup_cross(with_table 0), chomp_kernel_ng_setup
 * and chomp_covariance_ng do: the table, its levels and minimum, the scalars, the k_b knots, their
 * levels and the values.
 *
 * ln_ktheta_min / ln_ktheta_max and j0_limit (_j0_limit) are those of chomp_kernel_ssc_setup and
 * chomp_kernel_ng_setup, area, tri_table (a host array), n_tri, tri_k_min and tri_k_max those of
 * chomp_covariance_ng: the I_0^4 table's bicubic is built once for all blocks.  theta holds
 * theta_a[n_pairs] then theta_b[n_pairs] and out [n_blocks][n_pairs], both host or device arrays
 * as `mem` says.  epoch ([n_corr], or NULL: no status) only says where the status bit goes: a
 * block (i, j) that exhausts divmax sets CHOMP_ST_COV_NG_DIVMAX on epoch[i]'s word; the call
 * clears the bit on every epoch[i] first.
 *
 * The call keeps a state of its own (one kernel_NG block per block, the k_b knots, the I_0^4
 * table, an index block) and touches neither the context's kernel_ssc / kernel_NG state nor the
 * two cross slots nor the state of chomp_covariance_blocks or chomp_covariance_ssc_blocks.
 *
 * CHOMP_ERR_STATE: no sets, another number of sets than n_corr, sets of order 2.  CHOMP_ERR_ARG:
 * more than 65535 blocks or pairs, a bad ln(k theta) range or J0 limit, n_tri outside 4..64, a bad
 * trispectrum k range, an area or a host theta that is not positive, an epoch the context does not
 * have, tables too large for the 64 kB of LDS.  CHOMP_ERR_SCOPE, naming the block and before
 * anything is launched: a block whose four windows share no redshift (decided on the host from
 * the sets' ranges).
 *
 * chomp_covariance_ng_blocks_table reads block `block` of the last call (host arrays, any may be
 * NULL): info[7] = z_bar_NG, chi(z_bar_NG), growth_factor(z_bar_NG), z_min, z_max, chi_min,
 * chi_max; table and levels [kernel_npoints^2], table_min[1]; kb_knots and kb_levels
 * [n_pairs * kernel_npoints].
 *
 * chomp_covariance_ng_blocks_plan is host arithmetic and needs neither a context nor a device:
 * what a call of n_corr correlations and n_pairs pairs keeps on the device, in elements --
 * sizes[6] = n_blocks, one kernel_NG block (n_ktheta knots a side), all of them, the k_b buffer
 * (knots then levels, n_k knots a pair), the I_0^4 block, the index block -- and, if asked for,
 * that index block, index[n_corr + 3 n_blocks] ints: epoch[n_corr] (NULL: 0 .. n_corr - 1) |
 * (i, j)[n_blocks] | the diagonal blocks [n_corr] | the cross blocks [n_blocks - n_corr].
 * CHOMP_ERR_ARG beyond the sizes the call itself takes (more than 65535 blocks or pairs
 * included). */
int chomp_covariance_ng_blocks(chomp_ctx* ctx, size_t n_corr, const size_t* epoch /*[n_corr] or NULL*/,
                               double ln_ktheta_min, double ln_ktheta_max, double j0_limit,
                               double area, const double* tri_table, size_t n_tri,
                               double tri_k_min, double tri_k_max,
                               const double* theta /*[2][n_pairs]*/, size_t n_pairs,
                               double* out /*[n_blocks][n_pairs]*/, int mem);
int chomp_covariance_ng_blocks_table(chomp_ctx* ctx, size_t block, double* info /*[7]*/,
                                     double* table, double* levels, double* table_min,
                                     double* kb_knots, double* kb_levels);
int chomp_covariance_ng_blocks_plan(size_t n_corr, const size_t* epoch /*[n_corr] or NULL*/,
                                    size_t n_pairs, size_t n_ktheta, size_t n_k, size_t n_tri,
                                    size_t* sizes /*[6]*/,
                                    int* index /*[n_corr + 3 n_blocks] or NULL*/);

/* CorrelationFourier.correlation(l) (correlation.py:360-392): Limber C_l. */
int chomp_cell(chomp_ctx* ctx, int which, size_t epoch, double D_z,
               const double* ell, size_t n, double* out, int mem);
/* CorrelationFourier.correlation(l) for epochs epoch0 .. epoch0 + n_epoch - 1 of one context that
 * share the projection set-up and D_z: out[e * n + i] = what chomp_cell(ctx, which, epoch0 + e,
 * D_z, ell, n, ...) returns at i, bit for bit.  The batch axis of an HOD design or chain over C_l
 * (the loop of set_hod + correlation, as chomp_wtheta_epochs for w(theta)): the chi-only node
 * table is built once per call, and the spectrum table, the per-multipole Romberg and the deep
 * levels run once per chunk of 16 epochs (CHOMP_TUNE_WTHETA_EPOCH_CHUNK) instead of once per
 * epoch, every epoch taking the route chomp_cell would take.  fp64 only; CHOMP_ERR_SCOPE for the
 * narrowed precision modes, for HaloFit spectra (CHOMP_P_HALOFIT), for spectra extrapolated
 * beyond the halo's k range (CHOMP_P_EXTRAPOLATE on a halo-model spectrum) and for a context with
 * the wiggle transfer function (chomp_set_transfer): chomp_cell serves those, one epoch at a
 * time. */
int chomp_cell_epochs(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, double D_z,
                      const double* ell, size_t n, double* out, int mem);
/* C_l of epoch epoch0 + e against projection set e with growth D_z[e] (host array whatever `mem`
 * says, as in chomp_wtheta_sets): out[e * n + i] = what chomp_cell(ctx, which, epoch0 + e, D_z[e],
 * ell, n, ...) returns at i after chomp_kernel_setup of set e's inputs, bit for bit.
 * The sets are those of the last chomp_kernel_setup_sets / chomp_kernel_setup_pairs: the batch
 * over kernels (window pairs, MultiEpoch ranges) and over cosmologies of C_l.  The chi-only node
 * table belongs to a set, so every row of a chunk has its own (1.5 MiB at the default divmax)
 * before its spectrum table, Romberg states and deep list; otherwise the scope, argument checks,
 * chunking (CHOMP_TUNE_WTHETA_EPOCH_CHUNK) and routes of chomp_cell_epochs.  In addition
 * CHOMP_ERR_STATE before any set-up of sets and CHOMP_ERR_ARG when n_epoch is not the number of
 * sets or some D_z[e] <= 0. */
int chomp_cell_sets(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch,
                    const double* D_z /*[n_epoch], host*/, const double* ell, size_t n,
                    double* out, int mem);

/* Both observables of one survey set-up -- Correlation.correlation(theta) (correlation.py:
 * 242-275) and CorrelationFourier.correlation(l) (correlation.py:360-392) on the same kernel,
 * halo and spectrum -- in one call: the results of chomp_wtheta and chomp_cell, bit for bit,
 * with C_l computed beside w(theta) on a second HIP stream when the buffers are device
 * memory (neither integral needs anything of the other).  In the order of the context's
 * stream the call is complete when it returns. */
int chomp_wtheta_cell(chomp_ctx* ctx, int which, size_t epoch, double k_min, double k_max,
                      double D_z, const double* theta, size_t n_theta, double* w_out,
                      const double* ell, size_t n_ell, double* c_out, int mem);

/* SingleEpoch(..., with_bao=...) (cosmology.py:39, 87, 556-572): which Eisenstein & Hu
 * transfer function the context's epochs use -- the no-wiggle fit (default,
 * cosmology.py:449-472) or the one with baryon wiggles (cosmology.py:474-538).  Call it
 * before chomp_epochs_set; changing it invalidates every table. */
#define CHOMP_TRANSFER_EH 0
#define CHOMP_TRANSFER_EH_BAO 1
int chomp_set_transfer(chomp_ctx* ctx, int kind);

/* w0-wa dark energy (cosmology.py:96-104, 165-213), opt-in: with `on` set, chomp_epochs_set,
 * chomp_multi_epoch_setup and chomp_kernel_setup accept w0 != -1 or wa != 0 (off, the default:
 * they refuse them with CHOMP_ERR_SCOPE).  For each distinct (w0, wa) the library tabulates
 * P(a) = 3 int_0^z (1 + w(z')) / (1 + z') dz', w = w0 + wa (1 - a), with scipy's Romberg rule at
 * the cosmo_npoints knots a_i = logspace(log10(cosmo_precision), 0, cosmo_npoints), splines it
 * in ln a and evaluates E0(z) = Omega_L0 exp(P(ln a)) + Omega_m0 / a^3 + Omega_r0 / a^4 wherever
 * E enters: chi, omega_m(z), delta_c, delta_v, rho_bar, the windows' dz/dchi and the lensing
 * efficiency.  omega_l(z) stays Omega_L0 / E0 and the growth factor stays the Carroll et al.
 * approximation, as in the reference.  A Lambda-CDM cosmology takes exactly the path (and gives
 * the bits) it takes with the switch off.  A table is kept while its (w0, wa) recur. */
int chomp_set_dark_energy(chomp_ctx* ctx, int on);
/* One dark-energy table: source CHOMP_DE_EPOCH (the cosmology of epoch `index` of the last
 * chomp_epochs_set) or CHOMP_DE_PROJ (the projection set-up's; index ignored).  what: the knots
 * ln a_i, the pressures P_i, the Romberg levels, 1/0 for converged / divmax exhausted (n =
 * cosmo_npoints each), or the spline's coefficients (n = 4 (cosmo_npoints - 1): piece i on
 * [ln a_i, ln a_{i+1}] is sum_m pp[4 i + m] (ln a - ln a_i)^m).  Host buffer; synchronises.
 * CHOMP_ERR_STATE when that cosmology has no dark energy. */
#define CHOMP_DE_EPOCH 0
#define CHOMP_DE_PROJ 1
#define CHOMP_DE_LN_A 0
#define CHOMP_DE_PRESSURE 1
#define CHOMP_DE_LEVELS 2
#define CHOMP_DE_CONVERGED 3
#define CHOMP_DE_PP 4
int chomp_get_de_table(chomp_ctx* ctx, int source, size_t index, int what, double* out, size_t n);

/* Halo profiles with a general inner slope, halo_dict["alpha"] != -1 (y_general,
 * halo.py:491-559), opt-in: with `on` set the halo set-ups (chomp_halo_setup*, chomp_stage_k*)
 * accept alpha != -1 (off, the default: they refuse it with CHOMP_ERR_SCOPE) in (-3, 3.5]: alpha <= -3,
 * where the profile's mass diverges, and alpha > 3.5, beyond which the profile's mass integral is
 * not validated to 1e-13, are CHOMP_ERR_ARG.  For every ln k knot of the halo tables the
 * library then tabulates y(k, M) at the mass_npoints mass knots -- one integral of
 * x^(2 + alpha) (1 + x)^-(3 + alpha) sinc(k r_s x / pi) over [1e-8, c] each, scipy's Romberg rule
 * with rtol = halo_precision, normalised as the reference normalises it -- splines it in ln M and
 * integrates h_m .. pp_gg, I_1^2 and n_bar with that spline (zero outside the mass table) in
 * place of the NFW transform.  The knot tables land where the NFW ones do: chomp_power, the
 * projections and everything else that reads P(k) run unchanged.
 * A set-up whose epochs all have alpha = -1 takes exactly the launches (and gives the bits) it
 * takes with the switch off.  A set-up with ANY alpha != -1 takes the general path for all its
 * epochs, those with alpha = -1 with the NFW transform inline: their tables agree with the NFW
 * path's to the last digits, not bit for bit.  A y(k, M) integral that exhausts divmax raises
 * CHOMP_ST_HALO_DIVMAX_H_M.  The trispectrum set-ups (chomp_tri1h_setup, chomp_tri1h_quad,
 * chomp_tri_setup) keep refusing an epoch with alpha != -1 (CHOMP_ERR_SCOPE). */
int chomp_set_general_profile(chomp_ctx* ctx, int on);
/* Halo.y_general(ln_k, mass) of one epoch at ONE ln k (any value) and n masses (host): the
 * table of y over the mass knots is integrated at that ln k with the alpha of the epoch's last
 * halo set-up (alpha = -1 included: the Romberg value, not the closed form), splined in ln M and
 * evaluated; 0 outside [mass_min, mass_max] of the mass table (halo.py:496-498). */
int chomp_y_general(chomp_ctx* ctx, size_t epoch, double ln_k, const double* mass, size_t n,
                    double* out);
/* The y(k, M) table of one epoch as the last general-profile set-up built it, and the Romberg
 * level of each of its integrals: halo_npoints x mass_npoints doubles each, ln k slowest (either
 * pointer may be NULL).  Host buffers; synchronises.  CHOMP_ERR_STATE for an epoch without one. */
int chomp_y_general_table(chomp_ctx* ctx, size_t epoch, double* out_y, double* out_level);
/* Halo.halo_normalization(mass) (halo.py:465-474, 880-897) of one epoch at n masses (host): exp
 * of the not-a-knot spline over ln M of ln(rho_s / rho_norm) at the mass knots, for the alpha of
 * the epoch's last halo set-up (any alpha > -3, -1 included). */
int chomp_halo_normalization(chomp_ctx* ctx, size_t epoch, const double* mass, size_t n,
                             double* out);

/* Halo.calculate_bias / calculate_m_eff / calculate_f_sat (halo.py:709-838) of epochs
 * [epoch0, epoch0 + n): out[3 i + {0, 1, 2}] = effective bias, effective halo mass,
 * satellite fraction (host buffer), each with the epoch's HOD model.  Needs chomp_halo_setup
 * (n_bar). */
int chomp_hod_stats(chomp_ctx* ctx, size_t epoch0, size_t n, double* out);

/* Correlation3d.raw_correlation(r) (correlation.py:470-499): xi(r) = int dlnk k^2/(2 pi)
 * P(k) J0(k r) over [k_min, k_max] -- the cylindrical J0, as the reference has it.  One
 * wavefront-group per r; P is `which` of halo epoch `epoch`. */
int chomp_xi3d(chomp_ctx* ctx, int which, size_t epoch, double k_min, double k_max,
               const double* r, size_t n, double* out, int mem);
/* xi(r) of the epochs epoch0 .. epoch0 + n_epoch - 1 in one call (the loop of set_hod or of fresh
 * halos + raw_correlation over an HOD or cosmology design): out[e * n + i] is what
 * chomp_xi3d(ctx, which, epoch0 + e, k_min, k_max, r, n, ...) returns at i, bit for bit.  The
 * r-independent factor k^2/(2 pi) P(k) of the integrand is tabulated once per epoch on the Romberg
 * nodes (the node table of chomp_wtheta_epochs with D_z = 1, in its work buffer: 8 MiB per epoch
 * of a chunk at divmax = 20; CHOMP_TUNE_WTHETA_EPOCH_CHUNK sets the chunk), and one launch with
 * an epoch axis integrates it against J0(k r).  Needs no chomp_kernel_setup.  r / out: host or
 * device arrays (mem).  CHOMP_ERR_SCOPE (chomp_xi3d serves these): a narrowed precision mode, a
 * HaloFit code, CHOMP_P_EXTRAPOLATE on a halo-model spectrum, a context with the wiggle
 * transfer function, a context whose divmax exceeds 20 (the level of the node table). */
int chomp_xi3d_epochs(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, double k_min,
                      double k_max, const double* r, size_t n, double* out, int mem);
/* scipy InterpolatedUnivariateSpline(xk, yk)(x) (k = 3, not-a-knot), host buffers: the
 * 50-knot xi(r) spline of Correlation3d.compute_correlation / correlation
 * (correlation.py:459-468, 501-510).  x outside [xk[0], xk[nk-1]] extrapolates the end
 * pieces, as FITPACK does.  deriv = 0: values; 1: first derivative (the
 * InterpolatedUnivariateSpline.derivatives(x)[1] of MassFunction.dndm,
 * mass_function.py:268-287). */
int chomp_spline_eval(chomp_ctx* ctx, const double* xk, const double* yk, size_t nk,
                      const double* x, size_t n, int deriv, double* out);

/* Arithmetic of the w(theta) integral (BASELINE.json configs[4]: "mixed fp32/fp64 with
 * tolerance sweep").  The reference computes everything in fp64; F64 is the
 * default and the only mode held to the 1e-4 parity bar -- the others exist so that the
 * cost of each narrowing can be measured against the same golden vectors
 * (tests/test_gpu_projection.py::test_c5_precision_sweep). */
enum {
  CHOMP_PREC_F64 = 0,        /* tables, evaluation and sums in fp64 */
  CHOMP_PREC_F32_EVAL = 1,   /* fp32 integrand evaluation, fp64 tables and sums */
  CHOMP_PREC_F32_TABLES = 2, /* spline coefficients rounded to fp32, fp64 evaluation and sums */
  CHOMP_PREC_F32_ALL = 3     /* fp32 tables, evaluation, sums and Richardson extrapolation */
};
int chomp_set_precision(chomp_ctx* ctx, int mode);

#ifdef __cplusplus
}
#endif
#endif /* CHOMP_MI355X_H */
