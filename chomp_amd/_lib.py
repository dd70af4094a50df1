"""ctypes binding of libchomp_mi355x.so (include/chomp_mi355x.h).

The HIP library is the only compute path of this package: if it cannot be loaded
(or built in-tree with hipcc) importing the binding raises -- there is no CPU
fallback.
"""
import ctypes
import operator
import os
import subprocess
import threading

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.join(HERE, "libchomp_mi355x.so")

OK, ERR_ARG, ERR_HIP, ERR_STATE, ERR_SCOPE = 0, -1, -2, -3, -4
HOST, DEVICE = 0, 1
MF_ST, MF_TINKER = 0, 1
T_H_M, T_PP_MM, T_H_G, T_PP_GM, T_PP_GG = 1, 2, 4, 8, 16
T_I_1_2 = 32
T_EXCLUSION = 64
FAM_MM, FAM_GM, FAM_GG = T_H_M | T_PP_MM, T_H_M | T_H_G | T_PP_GM, T_H_G | T_PP_GG
FAM_SSC = FAM_MM | T_I_1_2
P_LIN, P_MM, P_GM, P_GG, P_HALOFIT, P_EXTRAPOLATE = 0, 1, 2, 3, 16, 32
P_SSC_RESPONSE, P_MM_SSC = 4, 5
CROSS_WINDOWS = -1   # chomp_covariance_cross_stage: the projection set-up alone
PREC_F64, PREC_F32_EVAL, PREC_F32_TABLES, PREC_F32_ALL = 0, 1, 2, 3
DNDZ_MAGLIM, DNDZ_GAUSSIAN, DNDZ_BOXCAR, DNDZ_PPOLY = 0, 1, 2, 3
WINDOW_GALAXY, WINDOW_CONVERGENCE, WINDOW_FLAT_CONVERGENCE, WINDOW_CONVERGENCE_DELTA = 0, 1, 2, 3

SC = {name: i for i, name in enumerate([
    "z", "chi", "growth", "omega_m", "omega_l", "delta_c", "delta_v", "rho_bar",
    "sigma_norm", "ln_mass_min", "ln_mass_max", "nu_min", "nu_max", "m_star",
    "f_norm", "bias_norm", "n_bar", "n_bar_over_rho_bar", "n_search",
    "mf_delta_v", "t_alpha", "t_beta", "t_gamma", "t_phi", "t_eta",
    "growth_norm", "delta_H", "hf_k_s", "hf_n_eff", "hf_C"])}
SC_COUNT = 30
TAB = {"ln_mass": 0, "nu": 1, "h_m": 2, "pp_mm": 3, "h_g": 4, "pp_gm": 5,
       "pp_gg": 6, "levels": 7, "hf_ln_sigma2": 8, "i_1_2": 9, "levels_i_1_2": 10}
EV = {"nu_of_mass": 0, "ln_mass_of_nu": 1, "f_nu": 2, "bias_nu": 3,
      "hod_first": 4, "hod_second": 5, "hod_central": 6, "hod_satellite": 7,
      "virial_radius": 8, "concentration": 9, "delta_k": 10, "bias_2_nu": 11,
      "sigma_of_nu": 12}
# chomp_pt_eval forms (CHOMP_PT_*) and the doubles of one configuration
PT = {"Fs2": 0, "Fs2_len": 1, "Fs2_kdiff": 2, "Fs3": 3, "Fs3_parallelogram": 4, "F3": 5,
      "Fs3_BCGS": 6, "bispectrum": 7, "bispectrum_len": 8, "trispectrum": 9,
      "trispectrum_parallelogram": 10}
PT_ARITY = {"Fs2": 6, "Fs2_len": 3, "Fs2_kdiff": 3, "Fs3": 9, "Fs3_parallelogram": 3, "F3": 9,
            "Fs3_BCGS": 9, "bispectrum": 9, "bispectrum_len": 6, "trispectrum": 12,
            "trispectrum_parallelogram": 3}
HF_COUNT = 14
KI = {name: i for i, name in enumerate([
    "z_bar", "chi_min", "chi_max", "z_min", "z_max", "D_zbar", "norm_a", "norm_b",
    "wa_chi_min", "wa_chi_max", "wb_chi_min", "wb_chi_max", "j_limit"])}
KI_COUNT = 13
KERNEL_SETS_MAX = 1024      # CHOMP_KERNEL_SETS_MAX: the sets of one chomp_kernel_setup_sets / _pairs
SETS_TABULATED = 1          # CHOMP_SETS_*: what chomp_set_sets_scope lets into those two calls
SETS_DARK_ENERGY = 2
ME = {"chi_of_z": 0, "z_of_chi": 1, "growth_of_z": 2}
KTAB = {"ln_ktheta": 0, "kernel": 1, "wa_chi": 2, "wa": 3, "wb_chi": 4, "wb": 5,
        "me_z": 6, "me_chi": 7, "me_growth": 8, "levels": 9}

c_double_p = ctypes.POINTER(ctypes.c_double)


class Cosmo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in (
        "omega_m0", "omega_b0", "omega_l0", "omega_r0", "cmb_temp", "h",
        "sigma_8", "n_scalar", "w0", "wa")]


class HaloPar(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in (
        "stq", "st_little_a", "c0", "beta", "alpha", "delta_v")]


class HodPar(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in (
        "log_M_min", "sigma", "log_M_0", "log_M_1p", "alpha")]


HOD_ZHENG, HOD_MANDELBAUM = 0, 1
# CHOMP_TRI_*: the n(M) of the one-halo trispectrum for each power_spec (halo_trispectrum.py:142-151);
# any other string integrates with n = 1
TRI_MOMENT = {"power_mmmm": 0, "power_gmmm": 1, "power_ggmm": 2, "power_gggm": 3, "power_gggg": 4}
DE_EPOCH, DE_PROJ = 0, 1       # chomp_get_de_table sources


class HodModel(ctypes.Structure):
    """chomp_hod_model: one epoch's HOD, tagged by its model (CHOMP_HOD_*)."""
    _fields_ = [("kind", ctypes.c_int), ("reserved", ctypes.c_int), ("zheng", HodPar),
                ("log_M_0", ctypes.c_double), ("w", ctypes.c_double)]


class Config(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_double) for n in (
        "k_min", "k_max", "mass_min", "mass_max", "corr_precision",
        "cosmo_precision", "dNdz_precision", "halo_precision",
        "kernel_precision", "mass_precision", "window_precision",
        "global_precision")] +
        [(n, ctypes.c_int) for n in (
            "corr_npoints", "cosmo_npoints", "halo_npoints", "kernel_npoints",
            "kernel_bessel_limit", "mass_npoints", "window_npoints", "divmax")])


class Dndz(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("pad_", ctypes.c_int),
                ("z_min", ctypes.c_double), ("z_max", ctypes.c_double),
                ("p", ctypes.c_double * 4),
                ("pp_breaks", ctypes.POINTER(ctypes.c_double)),
                ("pp_coef", ctypes.POINTER(ctypes.c_double)),
                ("pp_n", ctypes.c_int), ("pp_order", ctypes.c_int)]


class Window(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("pad_", ctypes.c_int), ("dist", Dndz)]


EXPORTS = [
    "chomp_default_config", "chomp_ctx_create", "chomp_ctx_destroy",
    "chomp_last_error", "chomp_sync", "chomp_epochs_set", "chomp_mass_setup",
    "chomp_halo_setup", "chomp_halofit_setup", "chomp_power", "chomp_power_range",
    "chomp_sigma_r", "chomp_y_nfw", "chomp_get_scalars", "chomp_get_table",
    "chomp_eval", "chomp_halofit_get", "chomp_halofit_put",
    "chomp_multi_epoch_setup", "chomp_me_eval",
    "chomp_kernel_setup", "chomp_kernel_info", "chomp_kernel_table",
    "chomp_kernel_eval", "chomp_window_eval", "chomp_wtheta", "chomp_wtheta_epochs",
    "chomp_cell", "chomp_cell_epochs",
    "chomp_kernel_setup_sets", "chomp_kernel_info_sets", "chomp_kernel_table_set",
    "chomp_wtheta_sets", "chomp_kernel_setup_pairs", "chomp_cell_sets", "chomp_set_sets_scope",
    "chomp_set_precision", "chomp_xi3d", "chomp_xi3d_epochs", "chomp_spline_eval",
    "chomp_hod_stats",
    "chomp_set_transfer", "chomp_kernel_raw",
    "chomp_covariance_table", "chomp_covariance_gaussian",
    "chomp_covariance_cross_stage", "chomp_covariance_table_cross",
    "chomp_covariance_gaussian_cross",
    "chomp_covariance_blocks", "chomp_covariance_blocks_table",
    "chomp_covariance_ssc_blocks_range", "chomp_covariance_ssc_blocks",
    "chomp_covariance_ssc_blocks_table",
    "chomp_set_timing", "chomp_get_timing", "chomp_get_status", "chomp_status_post",
    "chomp_status_wait", "chomp_set_tuning",
    "chomp_get_deep_stats", "chomp_stage_k", "chomp_power_plan", "chomp_get_stream",
    "chomp_wtheta_cell", "chomp_stage_k_halofit", "chomp_set_delta_b", "chomp_put_table",
    "chomp_kernel_ssc_setup", "chomp_kernel_ssc_raw", "chomp_kernel_ssc_eval",
    "chomp_covariance_ssc",
    "chomp_halo_setup_hod", "chomp_stage_k_hod", "chomp_stage_k_halofit_hod",
    "chomp_set_dark_energy", "chomp_get_de_table",
    "chomp_set_second_order", "chomp_get_second_order", "chomp_pt_eval",
    "chomp_tri1h_setup", "chomp_tri1h_eval", "chomp_tri1h_quad",
    "chomp_tri_setup", "chomp_tri_table_eval", "chomp_tri_terms", "chomp_tri_proj",
    "chomp_tri_triple",
    "chomp_kernel_ng_setup", "chomp_kernel_ng_raw", "chomp_kernel_ng_eval",
    "chomp_covariance_ng", "chomp_covariance_ng_blocks", "chomp_covariance_ng_blocks_table",
    "chomp_covariance_ng_blocks_plan",
    "chomp_covariance_cross_range", "chomp_kernel_ssc_setup_cross", "chomp_covariance_ssc_cross",
    "chomp_set_general_profile", "chomp_y_general", "chomp_y_general_table",
    "chomp_halo_normalization",
    "chomp_covariance_fourier_zbar", "chomp_covariance_fourier_table",
    "chomp_covariance_fourier_gaussian",
]

# chomp_get_status bits (include/chomp_mi355x.h)
ST_MASS_MIN_SATURATED, ST_MASS_MAX_SATURATED, ST_MASS_SEARCH_EXHAUSTED, ST_SIGMA_DIVMAX = 1, 2, 4, 8
ST_DE_DIVMAX = 0x10
ST_B2_DIVMAX = 0x20
ST_TRI1H_DIVMAX = 0x40
ST_COV_NG_DIVMAX = 0x80
ST_HALO_DIVMAX = {"h_m": 0x100, "pp_mm": 0x200, "h_g": 0x400, "pp_gm": 0x800, "pp_gg": 0x1000,
                  "i_1_2": 0x2000}
ST_TRI_DIVMAX = 0x4000
ST_NONFINITE = 0x10000
TRI_TAB = {"i_1_2": 0, "i_1_3": 1, "i_2_2": 2, "i_2_1": 3, "i_0_4": 4, "i_1_1": 5}
ST_SATURATED = ST_MASS_MIN_SATURATED | ST_MASS_MAX_SATURATED
TUNE_E_STREAM_MIN, TUNE_DEEP_LITERAL, TUNE_ROCTX, TUNE_WTHETA_DIRECT = 0, 2, 3, 4
TUNE_CELL_ONE_KERNEL = 5
TUNE_DEEP_TOL, TUNE_DEEP_MAX_BREAKS, TUNE_DEEP_MAX_FINE, TUNE_DEEP_SLOTS = 6, 7, 8, 10
TUNE_WTHETA_EPOCH_CHUNK = 11
TUNE_COUNT = 12   # (1 and 9: retired knobs, refused like any unknown number)


class ChompAccuracyWarning(UserWarning):
    """What scipy.integrate.romberg's AccuracyWarning (divmax exceeded) was in the reference."""


class ChompParityWarning(UserWarning):
    """The result is well defined but the reference's own answer for this input is decided by
    rounding noise (saturated mass-limit search): the two may differ by percents."""


def describe_status(word):
    """Human-readable list of the bits of a chomp_get_status word."""
    out = []
    if word & ST_MASS_MIN_SATURATED:
        out.append("mass_min search ended in the saturated regime of sigma_r (k R < 0.2 over "
                   "its whole k range, cosmology.py:627-632): the reference's own limit is "
                   "decided by rounding error there")
    if word & ST_MASS_MAX_SATURATED:
        out.append("mass_max search ended in the saturated regime of sigma_r "
                   "(k range clamped at k_min / 100, cosmology.py:617-622)")
    if word & ST_MASS_SEARCH_EXHAUSTED:
        out.append("mass-limit search did not end within 2047 steps of 5 %")
    if word & ST_SIGMA_DIVMAX:
        out.append("a sigma(R) Romberg of the nu table exhausted divmax")
    if word & ST_DE_DIVMAX:
        out.append("a Romberg of the dark-energy pressure table exhausted divmax")
    if word & ST_B2_DIVMAX:
        out.append("the bias_2_norm Romberg exhausted divmax (mass_function.py:408-414)")
    if word & ST_TRI1H_DIVMAX:
        out.append("an I_0^4 Romberg of the one-halo trispectrum exhausted divmax "
                   "(halo_trispectrum.py:89-95)")
    if word & ST_TRI_DIVMAX:
        out.append("a Romberg of the HaloTrispectrum tables or of tri_spec_proj_integral exhausted "
                   "divmax, or an end point of the latter was not finite (k1 = k2: the result is "
                   "NaN, halo_trispectrum.py:267-278, 655-836)")
    if word & ST_COV_NG_DIVMAX:
        out.append("a Romberg of the trispectrum term of the covariance (raw_kernel_NG, "
                   "kernel.py:1067-1072, or a k_b integral, covariance.py:665-671) exhausted "
                   "divmax")
    for name, bit in ST_HALO_DIVMAX.items():
        if word & bit:
            out.append("%s: Romberg exhausted divmax at some knots (last row kept)" % name)
    if word & ST_NONFINITE:
        out.append("a knot table holds NaN / infinity")
    return out


def sources():
    return [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))
            if f.endswith((".hip", ".h", ".inc"))] + [
        os.path.join(HERE, "..", "include", "chomp_mi355x.h")]


HASH_PATH = LIB_PATH + ".srchash"


# Compiler flags of the device code.  -disable-machine-licm: LLVM's machine-level loop-invariant
# code motion hoists the materialisation of every double constant of the inlined libm / special-
# function polynomials (a v_mov pair each) out of the kernels' outer loops, where they stay live
# across everything and -- the scalar registers being exhausted -- end up in VGPRs or even
# spilled to scratch and re-loaded INSIDE the dependent FMA chains (k_halo_knots_fast: 256 VGPRs +
# 652 B of scratch per lane).  Without it: k_halo_knots 231 -> 168 VGPRs, k_epoch_probe 215 -> 152,
# k_nu_table 128 -> 98, k_power_grid 166 -> 106, no spills left in k_cell / k_cell_deep / k_wtheta
# (tools/kernel_regs.py); same arithmetic, bit-identical results.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
NO_LICM = ["-mllvm", "-disable-machine-licm"]
# translation units: (source, extra flags).  k_epoch_probe is the one kernel that is faster
# with machine LICM (38.5 against 41.8 us per C2 launch) and has a unit of its own.
UNITS = [("chomp_capi.hip", NO_LICM), ("chomp_probe.hip", [])]


def source_hash():
    """Content hash of everything the library is compiled from (mtimes do not survive a
    copy of the tree to another box; contents do), compiler flags included."""
    import hashlib
    h = hashlib.sha256()
    h.update(repr((HIPCC_FLAGS, UNITS)).encode())
    for path in sources():
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def built_hash():
    """The source hash the shipped library was built from (None if not recorded)."""
    try:
        with open(HASH_PATH) as f:
            return f.read().strip() or None
    except OSError:
        return None


def build(force=False, verbose=False, extra_flags=(), out=None):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a
    GPU).  Rebuilds when the sources differ from the ones the .so was built from (their
    hash is kept beside it).  extra_flags / out: a development build with other compiler flags
    somewhere else (e.g. build_exp/), leaving the product library alone."""
    want = source_hash()
    if out is None and not force and os.path.exists(LIB_PATH):
        try:
            with open(HASH_PATH) as f:
                if f.read().strip() == want:
                    return LIB_PATH
        except OSError:
            pass
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tmp = LIB_PATH + ".tmp%d" % os.getpid()
    import tempfile
    with tempfile.TemporaryDirectory(prefix="chomp_build_") as objdir:
        procs = []
        for src, extra in UNITS:                      # (the units compile side by side)
            obj = os.path.join(objdir, src.replace(".hip", ".o"))
            cmd = [hipcc] + HIPCC_FLAGS + list(extra) + list(extra_flags) + ["-c", "-o", obj,
                                                                             os.path.join(CSRC, src)]
            if verbose:
                print(" ".join(cmd))
            procs.append((cmd, obj, subprocess.Popen(cmd, cwd=CSRC)))
        for cmd, obj, pr in procs:
            if pr.wait() != 0:
                raise subprocess.CalledProcessError(pr.returncode, cmd)
        link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + [o for _, o, _ in procs]
        if verbose:
            print(" ".join(link))
        subprocess.check_call(link, cwd=CSRC)
    if out is not None:
        os.replace(tmp, out)
        return out
    os.replace(tmp, LIB_PATH)
    with open(HASH_PATH, "w") as f:
        f.write(want + "\n")
    return LIB_PATH


_lib = None
_lock = threading.Lock()


def _preload_hip_runtime():
    """One HIP runtime per process: PyTorch-ROCm wheels bundle their own
    libamdhip64.so (same SONAME as /opt/rocm's).  If our library were loaded first it
    would bind the system runtime and a later `import torch` would bring in a second
    one, which then fails to open the GPU.  Loading torch's copy first (without
    importing torch) makes both resolve to the same runtime, in either import order."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        cand = os.path.join(libdir, name)
        if os.path.exists(cand):
            try:
                ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                pass


def lib():
    """Load (building if necessary) the HIP library.  Raises if impossible."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        # build() is a no-op when the library was built from exactly these sources (content
        # hash beside it).  A library that was built from OTHER sources is never loaded
        # silently: a test run would certify a binary that is not the tree.
        try:
            build()
        except Exception as exc:   # noqa: BLE001
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    "chomp_amd: libchomp_mi355x.so is missing and could not be "
                    "built with hipcc (%s). This package has no CPU fallback."
                    % exc) from exc
            have = built_hash()
            msg = ("chomp_amd: libchomp_mi355x.so was built from other sources (library %s, "
                   "tree %s) and the rebuild failed (%s)"
                   % (have or "unknown", source_hash(), exc))
            if os.environ.get("CHOMP_ALLOW_STALE_LIB") != "1":
                raise ImportError(msg + "; set CHOMP_ALLOW_STALE_LIB=1 to load it all the "
                                  "same (a box without hipcc)") from exc
            import warnings
            warnings.warn(msg + "; CHOMP_ALLOW_STALE_LIB=1: using the existing library")
        _preload_hip_runtime()
        L = ctypes.CDLL(LIB_PATH)
        for name in EXPORTS:
            if not hasattr(L, name):
                raise ImportError("chomp_amd: %s lacks symbol %s" % (LIB_PATH, name))
        vp, sz, i, d = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double
        L.chomp_default_config.argtypes = [ctypes.POINTER(Config)]
        L.chomp_default_config.restype = None
        L.chomp_ctx_create.argtypes = [ctypes.POINTER(Config), i, vp,
                                       ctypes.POINTER(vp)]
        L.chomp_ctx_destroy.argtypes = [vp]
        L.chomp_ctx_destroy.restype = None
        L.chomp_last_error.argtypes = [vp]
        L.chomp_last_error.restype = ctypes.c_char_p
        L.chomp_sync.argtypes = [vp]
        L.chomp_get_stream.argtypes = [vp, ctypes.POINTER(vp)]
        L.chomp_epochs_set.argtypes = [vp, sz, ctypes.POINTER(Cosmo), c_double_p]
        L.chomp_mass_setup.argtypes = [vp, ctypes.POINTER(HaloPar), i]
        L.chomp_halo_setup.argtypes = [vp, ctypes.POINTER(HaloPar),
                                       ctypes.POINTER(HodPar), ctypes.c_uint]
        L.chomp_stage_k.argtypes = [vp, ctypes.POINTER(HaloPar), i, ctypes.POINTER(HaloPar),
                                    ctypes.POINTER(HodPar), ctypes.c_uint]
        L.chomp_halo_setup_hod.argtypes = [vp, ctypes.POINTER(HaloPar),
                                           ctypes.POINTER(HodModel), ctypes.c_uint]
        L.chomp_stage_k_hod.argtypes = [vp, ctypes.POINTER(HaloPar), i, ctypes.POINTER(HaloPar),
                                        ctypes.POINTER(HodModel), ctypes.c_uint]
        L.chomp_stage_k_halofit_hod.argtypes = [vp, ctypes.POINTER(HaloPar), i,
                                                ctypes.POINTER(HaloPar), ctypes.POINTER(HodModel),
                                                ctypes.c_uint, sz, d, d, d, d, d]
        L.chomp_halofit_setup.argtypes = [vp, sz, sz, d, d, d, d, d]
        L.chomp_stage_k_halofit.argtypes = [vp, ctypes.POINTER(HaloPar), i, ctypes.POINTER(HaloPar),
                                            ctypes.POINTER(HodPar), ctypes.c_uint, sz, d, d, d, d, d]
        L.chomp_power.argtypes = [vp, i, vp, sz, vp, i]
        L.chomp_power_range.argtypes = [vp, i, sz, sz, vp, sz, vp, i]
        L.chomp_power_plan.argtypes = [vp, sz, vp, sz]
        L.chomp_sigma_r.argtypes = [vp, sz, vp, sz, vp]
        L.chomp_y_nfw.argtypes = [vp, sz, vp, vp, sz, vp]
        L.chomp_get_scalars.argtypes = [vp, sz, c_double_p]
        L.chomp_get_table.argtypes = [vp, sz, i, c_double_p, sz]
        L.chomp_put_table.argtypes = [vp, sz, i, c_double_p, sz]
        L.chomp_set_delta_b.argtypes = [vp, sz, sz, vp, i]
        L.chomp_eval.argtypes = [vp, sz, i, vp, sz, vp, i]
        L.chomp_halofit_get.argtypes = [vp, sz, c_double_p]
        L.chomp_halofit_put.argtypes = [vp, sz, c_double_p]
        L.chomp_kernel_setup.argtypes = [vp, ctypes.POINTER(Cosmo), d, d, d, d,
                                         ctypes.POINTER(Window),
                                         ctypes.POINTER(Window), i]
        L.chomp_multi_epoch_setup.argtypes = [vp, ctypes.POINTER(Cosmo), d, d]
        L.chomp_me_eval.argtypes = [vp, i, vp, sz, vp, i]
        L.chomp_kernel_info.argtypes = [vp, c_double_p]
        L.chomp_kernel_table.argtypes = [vp, i, c_double_p, sz]
        L.chomp_kernel_eval.argtypes = [vp, vp, sz, vp, i]
        L.chomp_kernel_raw.argtypes = [vp, vp, sz, vp, i]
        L.chomp_window_eval.argtypes = [vp, i, vp, sz, vp, i]
        L.chomp_wtheta.argtypes = [vp, i, sz, d, d, d, vp, sz, vp, i]
        L.chomp_wtheta_epochs.argtypes = [vp, i, sz, sz, d, d, d, vp, sz, vp, i]
        L.chomp_kernel_setup_sets.argtypes = [vp, sz, ctypes.POINTER(Cosmo), d, d, d, d,
                                              ctypes.POINTER(Window), ctypes.POINTER(Window), i]
        L.chomp_kernel_info_sets.argtypes = [vp, c_double_p]
        L.chomp_kernel_table_set.argtypes = [vp, sz, i, c_double_p, sz]
        L.chomp_wtheta_sets.argtypes = [vp, i, sz, sz, d, d, vp, vp, sz, vp, i]
        L.chomp_cell.argtypes = [vp, i, sz, d, vp, sz, vp, i]
        L.chomp_cell_epochs.argtypes = [vp, i, sz, sz, d, vp, sz, vp, i]
        L.chomp_kernel_setup_pairs.argtypes = [vp, sz, ctypes.POINTER(Cosmo), c_double_p, c_double_p,
                                               d, d, ctypes.POINTER(Window), ctypes.POINTER(Window), i]
        L.chomp_cell_sets.argtypes = [vp, i, sz, sz, vp, vp, sz, vp, i]
        L.chomp_wtheta_cell.argtypes = [vp, i, sz, d, d, d, vp, sz, vp, vp, sz, vp, i]
        L.chomp_set_precision.argtypes = [vp, i]
        L.chomp_hod_stats.argtypes = [vp, sz, sz, c_double_p]
        L.chomp_set_transfer.argtypes = [vp, i]
        L.chomp_set_dark_energy.argtypes = [vp, i]
        L.chomp_set_sets_scope.argtypes = [vp, ctypes.c_uint]
        L.chomp_set_general_profile.argtypes = [vp, i]
        L.chomp_y_general.argtypes = [vp, sz, d, vp, sz, vp]
        L.chomp_y_general_table.argtypes = [vp, sz, vp, vp]
        L.chomp_halo_normalization.argtypes = [vp, sz, vp, sz, vp]
        L.chomp_get_de_table.argtypes = [vp, i, sz, i, c_double_p, sz]
        L.chomp_set_second_order.argtypes = [vp, i]
        L.chomp_get_second_order.argtypes = [vp, sz, c_double_p, sz]
        L.chomp_pt_eval.argtypes = [vp, i, sz, sz, vp, sz, vp, i]
        L.chomp_tri1h_setup.argtypes = [vp, sz, sz, i, vp, vp]
        L.chomp_tri1h_eval.argtypes = [vp, sz, vp, vp, sz, vp, i]
        L.chomp_tri1h_quad.argtypes = [vp, sz, i, vp, sz, vp, vp, i]
        L.chomp_tri_setup.argtypes = [vp, sz, sz, vp, vp]
        L.chomp_tri_table_eval.argtypes = [vp, sz, i, vp, vp, sz, vp, i]
        L.chomp_tri_terms.argtypes = [vp, sz, sz, vp, sz, vp, i]
        L.chomp_tri_proj.argtypes = [vp, sz, sz, vp, sz, vp, vp, vp, i]
        L.chomp_tri_triple.argtypes = [vp, sz, vp, sz, vp, vp, i]
        L.chomp_set_timing.argtypes = [vp, i]
        L.chomp_get_timing.argtypes = [vp, c_double_p, sz]
        L.chomp_get_status.argtypes = [vp, sz, sz, ctypes.POINTER(ctypes.c_uint)]
        L.chomp_status_post.argtypes = [vp]
        L.chomp_status_wait.argtypes = [vp, sz, sz, ctypes.POINTER(ctypes.c_uint)]
        L.chomp_set_tuning.argtypes = [vp, i, ctypes.c_longlong]
        L.chomp_get_deep_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
        L.chomp_covariance_table.argtypes = [vp, i, sz, d, c_double_p, c_double_p,
                                             c_double_p, sz]
        L.chomp_covariance_gaussian.argtypes = [vp, d, d, d, d, vp, sz, vp, i]
        L.chomp_covariance_cross_stage.argtypes = [vp, i, vp, i, sz]
        L.chomp_covariance_table_cross.argtypes = [vp, d, d, c_double_p, c_double_p,
                                                   c_double_p, sz]
        L.chomp_covariance_gaussian_cross.argtypes = [vp, d, d, d, d, d, d, vp, sz, vp, i]
        L.chomp_covariance_blocks.argtypes = [vp, i, sz, ctypes.POINTER(sz), d, d, vp, vp, sz, vp, i]
        L.chomp_covariance_blocks_table.argtypes = [vp, sz, c_double_p, c_double_p, c_double_p,
                                                    c_double_p, sz]
        L.chomp_kernel_ssc_setup.argtypes = [vp, d, d, d, c_double_p, c_double_p, sz, i,
                                             c_double_p, c_double_p, c_double_p]
        L.chomp_kernel_ssc_raw.argtypes = [vp, vp, sz, vp]
        L.chomp_kernel_ssc_eval.argtypes = [vp, vp, sz, vp]
        L.chomp_covariance_ssc.argtypes = [vp, sz, d, vp, sz, vp, vp, vp]
        L.chomp_covariance_cross_range.argtypes = [vp, c_double_p]
        L.chomp_kernel_ssc_setup_cross.argtypes = L.chomp_kernel_ssc_setup.argtypes
        L.chomp_covariance_ssc_cross.argtypes = [vp, d, vp, sz, vp, vp, vp]
        L.chomp_covariance_ssc_blocks_range.argtypes = [vp, sz, c_double_p]
        L.chomp_covariance_ssc_blocks.argtypes = [vp, sz, ctypes.POINTER(sz), d, d, d, c_double_p,
                                                  c_double_p, sz, d, vp, sz, vp, i]
        L.chomp_covariance_ssc_blocks_table.argtypes = [vp, sz, c_double_p, c_double_p, c_double_p,
                                                        c_double_p, c_double_p]
        L.chomp_covariance_fourier_zbar.argtypes = [vp, c_double_p, sz, c_double_p]
        L.chomp_covariance_fourier_table.argtypes = [vp, i, ctypes.POINTER(sz), c_double_p, sz,
                                                     c_double_p, c_double_p, c_double_p]
        L.chomp_covariance_fourier_gaussian.argtypes = [vp, vp, sz, vp, i]
        L.chomp_kernel_ng_setup.argtypes = [vp, d, i, c_double_p, c_double_p, c_double_p]
        L.chomp_kernel_ng_raw.argtypes = [vp, vp, sz, vp]
        L.chomp_kernel_ng_eval.argtypes = [vp, vp, sz, vp]
        L.chomp_covariance_ng.argtypes = [vp, d, vp, sz, d, d, vp, sz, vp, vp, vp]
        L.chomp_covariance_ng_blocks.argtypes = [vp, sz, ctypes.POINTER(sz), d, d, d, d, c_double_p,
                                                 sz, d, d, vp, sz, vp, i]
        L.chomp_covariance_ng_blocks_table.argtypes = [vp, sz] + [c_double_p] * 6
        L.chomp_covariance_ng_blocks_plan.argtypes = [sz, ctypes.POINTER(sz), sz, sz, sz, sz,
                                                      ctypes.POINTER(sz), ctypes.POINTER(i)]
        L.chomp_xi3d.argtypes = [vp, i, sz, d, d, vp, sz, vp, i]
        L.chomp_xi3d_epochs.argtypes = [vp, i, sz, sz, d, d, vp, sz, vp, i]
        L.chomp_spline_eval.argtypes = [vp, vp, vp, sz, vp, sz, i, vp]
        for name in EXPORTS:
            if name not in ("chomp_default_config", "chomp_ctx_destroy",
                            "chomp_last_error"):
                getattr(L, name).restype = i
        _lib = L
        return _lib


def covariance_ng_blocks_plan(n_corr, n_pairs, n_ktheta, n_k, n_tri, epochs=None):
    """What Context.covariance_ng_blocks keeps on the device for n_corr correlations and n_pairs
    pairs of angles (chomp_covariance_ng_blocks_plan; host arithmetic, no device): (sizes, index) --
    sizes a dict of element counts (n_blocks, slab, slabs, kb, tri, index), index the call's index
    block: epoch[n_corr] | (i, j)[n_blocks] | the diagonal blocks | the cross blocks."""
    n_corr = int(n_corr)
    sizes = (ctypes.c_size_t * 6)()
    index = numpy.empty(n_corr + 3 * (n_corr * (n_corr + 1) // 2), dtype=numpy.intc)
    ep = None
    if epochs is not None:
        ep = numpy.ascontiguousarray(epochs, dtype=numpy.uintp).ravel()
        if ep.size != n_corr:
            raise ValueError("covariance_ng_blocks_plan: epochs must be [n_corr]")
    rc = lib().chomp_covariance_ng_blocks_plan(
        n_corr, ep.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)) if ep is not None else None,
        int(n_pairs), int(n_ktheta), int(n_k), int(n_tri), sizes,
        index.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    if rc:
        raise ValueError("covariance_ng_blocks_plan: sizes beyond what covariance_ng_blocks takes")
    names = ("n_blocks", "slab", "slabs", "kb", "tri", "index")
    return dict(zip(names, (int(v) for v in sizes))), index


def current_device():
    """HIP ordinal for new contexts: CHOMP_DEVICE, else LOCAL_RANK (one process
    per GPU under torch.distributed.run), else 0."""
    for key in ("CHOMP_DEVICE", "LOCAL_RANK"):
        if key in os.environ:
            return int(os.environ[key])
    return 0


class ChompError(RuntimeError):
    pass


class ChompScopeError(NotImplementedError):
    """Feature of the reference that is outside the accelerated hot path."""


def make_config(limits, precision):
    """Snapshot defaults.default_limits / default_precision into a Config."""
    c = Config()
    for k in ("k_min", "k_max", "mass_min", "mass_max"):
        setattr(c, k, float(limits[k]))
    for k in ("corr_precision", "cosmo_precision", "dNdz_precision",
              "halo_precision", "kernel_precision", "mass_precision",
              "window_precision", "global_precision"):
        setattr(c, k, float(precision[k]))
    for k in ("corr_npoints", "cosmo_npoints", "halo_npoints", "kernel_npoints",
              "kernel_bessel_limit", "mass_npoints", "window_npoints", "divmax"):
        setattr(c, k, int(precision[k]))
    return c


def cosmo_struct(cosmo_dict):
    """KeyError on a missing key, like the reference (cosmology.py:49-58)."""
    return Cosmo(*[float(cosmo_dict[k]) for k in (
        "omega_m0", "omega_b0", "omega_l0", "omega_r0", "cmb_temp", "h",
        "sigma_8", "n_scalar", "w0", "wa")])


def halo_struct(halo_dict):
    return HaloPar(*[float(halo_dict[k]) for k in (
        "stq", "st_little_a", "c0", "beta", "alpha", "delta_v")])


def hod_struct(hod):
    return HodPar(float(hod.log_M_min), float(hod.sigma), float(hod.log_M_0),
                  float(hod.log_M_1p), float(hod.alpha))


def hod_model(hod):
    """The chomp_hod_model of an HOD object: hod.HODMandelbaum by its class (log_M_0, w; the
    library derives the rest); every other object is read as HODZheng's five numbers, so an
    object without them fails here with AttributeError, as before."""
    from . import hod as hod_mod
    if isinstance(hod, hod_mod.HODMandelbaum):
        return HodModel(HOD_MANDELBAUM, 0, HodPar(), float(hod.log_M_0), float(hod.w))
    return HodModel(HOD_ZHENG, 0, hod_struct(hod), 0.0, 0.0)


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _numel(x):
    """Elements of a numpy array or a torch tensor."""
    return x.size if isinstance(x, numpy.ndarray) else x.numel()


_host_address = operator.attrgetter("ctypes.data")


def _elementwise(*pre, shape=None):
    """Context._run's body of an element-wise entry point fn(handle, *pre, x, n, out, mem): out
    shaped like x (or `shape`)."""
    return lambda mem, new, x: pre + (x, _numel(x), new(x.shape if shape is None else shape), mem)


def _rows(n_epoch, *pre):
    """Context._run's body of a batched entry point fn(handle, *pre, x, n, out, mem): out
    [n_epoch, x.size], a row per epoch."""
    n_epoch = int(n_epoch)
    return lambda mem, new, x: pre + (x, _numel(x), new((n_epoch, _numel(x))), mem)


def _row_growth(who, D_z, n_epoch):
    """The per-row growth factors of `who` (a *_sets call): a host array, one per epoch."""
    D = numpy.ascontiguousarray(D_z, dtype=numpy.float64).ravel()
    if D.size != int(n_epoch):
        raise ValueError("%s: D_z must hold one growth factor per epoch" % who)
    return D


def _pairs(a, b):
    """The pairs of the covariance calls: two host arrays of one length, one after the other."""
    a = numpy.ascontiguousarray(a, dtype=numpy.float64).ravel()
    b = numpy.ascontiguousarray(b, dtype=numpy.float64).ravel()
    assert a.size == b.size
    return numpy.concatenate([a, b])


def _ptr(a):
    """A host array as a double pointer argument; None stays None (the C calls' optional outputs)."""
    return a.ctypes.data_as(c_double_p) if a is not None else None


def _torch_current_stream(device):
    """torch's current HIP stream on `device`, if torch is in use in this process (never
    imports torch or initialises the GPU through it by itself)."""
    import sys
    torch = sys.modules.get("torch")
    if torch is None or not hasattr(torch, "cuda") or not torch.cuda.is_initialized():
        return None
    return torch.cuda.current_stream(device)


class Context(object):
    """Owns one chomp_ctx.  device: HIP ordinal; stream: raw hipStream_t or None.

    stream=None: torch's current stream of the device when torch is already driving the GPU
    in this process (so that tensors handed to power() / wtheta() / ... are produced and
    consumed in stream order with the caller's other work), else a stream of the library's
    own.  Calls that pass torch tensors from ANOTHER current stream are ordered against it
    with events on both sides (_torch_enter / _torch_leave)."""

    def __init__(self, config, device=0, stream=None):
        self._L = lib()
        self._h = ctypes.c_void_p()
        self.config = config
        self.device = int(device)
        if stream is None:
            cur = _torch_current_stream(self.device)
            if cur is not None:
                stream = cur.cuda_stream
        rc = self._L.chomp_ctx_create(ctypes.byref(config), self.device,
                                      ctypes.c_void_p(stream or 0),
                                      ctypes.byref(self._h))
        if rc != OK:
            raise ChompError("chomp_ctx_create failed (%d): no usable MI355X / HIP "
                             "device; chomp_amd has no CPU fallback" % rc)
        sp = ctypes.c_void_p()
        self._L.chomp_get_stream(self._h, ctypes.byref(sp))
        self.stream_ptr = sp.value or 0
        self.n_epoch = 0
        self._proj_ssc = None            # the KernelCovariance whose kernel_ssc table is here
        self._proj_ng = None             # ... and whose kernel_NG table is
        self._plan_k = None

    # -- ordering against the caller's torch stream ------------------------------------
    def _torch_enter(self):
        """Before a call that reads torch tensors: the context's stream waits for what the
        caller's current stream has queued.  Returns the pair of streams for _torch_leave
        (None when both are the same stream: nothing to do)."""
        import torch
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream == self.stream_ptr:
            return None
        mine = torch.cuda.ExternalStream(self.stream_ptr, device=self.device)
        mine.wait_stream(cur)
        return cur, mine

    @staticmethod
    def _torch_leave(pair):
        """After it: the caller's stream waits for the context's (the outputs)."""
        if pair is not None:
            pair[0].wait_stream(pair[1])

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.chomp_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()
            self._plan_k = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001
            pass

    def _check(self, rc):
        if rc == OK:
            return
        msg = self._L.chomp_last_error(self._h).decode()
        if rc == ERR_SCOPE:
            raise ChompScopeError(msg)
        if rc == ERR_ARG:
            raise ValueError(msg)
        raise ChompError("%s (code %d)" % (msg, rc))

    # -- Stage K -------------------------------------------------------------
    # Each call takes either Python dictionaries / objects (converted here) or the
    # ctypes arrays built once by pack_* (the batched path does that: converting 64
    # dictionaries per step costs more host time than the kernels take).
    @staticmethod
    def pack_cosmo(cosmo_dicts, n):
        """One dict (for all n epochs), a list of n dicts, or a float64 array [n, 10] in the
        field order of chomp_cosmo (omega_m0, omega_b0, omega_l0, omega_r0, cmb_temp, h,
        sigma_8, n_scalar, w0, wa) -- what a sampler that draws thousands of points per step
        hands over without building dictionaries."""
        if isinstance(cosmo_dicts, numpy.ndarray):
            a = numpy.ascontiguousarray(cosmo_dicts, dtype=numpy.float64)
            if a.shape != (n, 10):
                raise ValueError("cosmology array must be [%d, 10], got %r" % (n, a.shape))
            return (Cosmo * n).from_buffer_copy(a.tobytes())
        if isinstance(cosmo_dicts, dict):
            cosmo_dicts = [cosmo_dicts] * n
        return (Cosmo * n)(*[cosmo_struct(c) for c in cosmo_dicts])

    @staticmethod
    def pack_halo(halo_dicts, n):
        if isinstance(halo_dicts, dict):
            halo_dicts = [halo_dicts] * n
        return (HaloPar * n)(*[halo_struct(h) for h in halo_dicts])

    @staticmethod
    def pack_hod(hods, n):
        """One HOD object (for all n epochs) or a list of n, of either model: the tagged
        chomp_hod_model array the *_hod entry points take."""
        if not isinstance(hods, (list, tuple)):
            hods = [hods] * n
        return (HodModel * n)(*[hod_model(h) for h in hods])

    def epochs_set(self, cosmo, z, with_bao=False, dark_energy=False):
        """with_bao: SingleEpoch(with_bao=True), the E&H transfer function with wiggles.
        dark_energy: accept w0-wa cosmologies (chomp_set_dark_energy); off, they raise
        ChompScopeError."""
        self._check(self._L.chomp_set_transfer(self._h, 1 if with_bao else 0))
        self._check(self._L.chomp_set_dark_energy(self._h, 1 if dark_energy else 0))
        z = numpy.ascontiguousarray(numpy.atleast_1d(z), dtype=numpy.float64)
        n = z.size
        arr = cosmo if isinstance(cosmo, ctypes.Array) else self.pack_cosmo(cosmo, n)
        assert len(arr) == n
        self._check(self._L.chomp_epochs_set(self._h, n, arr,
                                             z.ctypes.data_as(c_double_p)))
        self.n_epoch = n

    def set_transfer(self, with_bao):
        """The transfer function alone (epochs_set sets it as well): contexts that exchange
        snapshots must agree on it."""
        self._check(self._L.chomp_set_transfer(self._h, 1 if with_bao else 0))

    def mass_setup(self, halo, mf_kind):
        arr = halo if isinstance(halo, ctypes.Array) else self.pack_halo(halo, self.n_epoch)
        assert len(arr) == self.n_epoch
        self._check(self._L.chomp_mass_setup(self._h, arr, int(mf_kind)))

    def halo_setup(self, profile, hods, tables, general_profile=False):
        """general_profile: accept halo dictionaries with alpha != -1 (chomp_set_general_profile);
        off, they raise ChompScopeError."""
        self._check(self._L.chomp_set_general_profile(self._h, 1 if general_profile else 0))
        n = self.n_epoch
        pa = profile if isinstance(profile, ctypes.Array) else self.pack_halo(profile, n)
        ha = hods if isinstance(hods, ctypes.Array) else self.pack_hod(hods, n)
        assert len(pa) == n and len(ha) == n
        self._check(self._L.chomp_halo_setup_hod(self._h, pa, ha, int(tables)))

    def stage_k(self, mass_halo, mf_kind, profile, hods, tables, general_profile=False):
        """mass_setup + halo_setup in one call (chomp_stage_k)."""
        self._check(self._L.chomp_set_general_profile(self._h, 1 if general_profile else 0))
        n = self.n_epoch
        ma = mass_halo if isinstance(mass_halo, ctypes.Array) else self.pack_halo(mass_halo, n)
        pa = profile if isinstance(profile, ctypes.Array) else self.pack_halo(profile, n)
        ha = hods if isinstance(hods, ctypes.Array) else self.pack_hod(hods, n)
        assert len(ma) == n and len(pa) == n and len(ha) == n
        self._check(self._L.chomp_stage_k_hod(self._h, ma, int(mf_kind), pa, ha, int(tables)))

    def stage_k_halofit(self, mass_halo, mf_kind, profile, hods, tables, epoch, f1, f2, f3,
                        omega_l, w, general_profile=False):
        """stage_k + halofit_setup(epoch, epoch, ...) in one call (chomp_stage_k_halofit)."""
        self._check(self._L.chomp_set_general_profile(self._h, 1 if general_profile else 0))
        n = self.n_epoch
        ma = mass_halo if isinstance(mass_halo, ctypes.Array) else self.pack_halo(mass_halo, n)
        pa = profile if isinstance(profile, ctypes.Array) else self.pack_halo(profile, n)
        ha = hods if isinstance(hods, ctypes.Array) else self.pack_hod(hods, n)
        assert len(ma) == n and len(pa) == n and len(ha) == n
        self._check(self._L.chomp_stage_k_halofit_hod(self._h, ma, int(mf_kind), pa, ha,
                                                      int(tables), epoch, f1, f2, f3, omega_l, w))

    def set_second_order(self, on=True):
        """MassFunctionSecondOrder set-ups from now on (chomp_set_second_order)."""
        self._check(self._L.chomp_set_second_order(self._h, 1 if on else 0))

    def second_order(self, epoch=0):
        """{"sigma": sigma(M) at the mass knots, "bias_2_norm", "level", "converged"} of the last
        (second-order) mass set-up (chomp_get_second_order)."""
        nm = self.config.mass_npoints
        out = numpy.empty(nm + 3)
        self._check(self._L.chomp_get_second_order(self._h, epoch,
                                                    out.ctypes.data_as(c_double_p), out.size))
        return {"sigma": out[:nm], "bias_2_norm": float(out[nm]), "level": int(out[nm + 1]),
                "converged": bool(out[nm + 2])}

    def pt_eval(self, form, args, epoch0=0, n=None):
        """PerturbationTheory form `form` (a PT key) of configurations args [N, arity] over the
        epochs [epoch0, epoch0 + n): [n, N].  args numpy (host path) or a contiguous float64 torch
        cuda tensor (device path, asynchronous on the context's stream; returns a tensor)."""
        n = self.n_epoch - epoch0 if n is None else n
        na = PT_ARITY[form]

        def body(mem, new, a):
            m, rest = divmod(_numel(a), na)
            if rest:
                raise ValueError("pt_eval: %s takes %d numbers a configuration" % (form, na))
            return PT[form], epoch0, n, a, m, new((n, m)), mem
        return self._run(self._L.chomp_pt_eval, [args], body)[0]

    # -- one-halo trispectrum -------------------------------------------------------
    def tri1h_setup(self, moment, epoch0=0, n=None, copy_out=False):
        """The I_0^4 table, its levels and its bicubic of the epochs [epoch0, epoch0 + n)
        (chomp_tri1h_setup; moment: a CHOMP_TRI_* code).  copy_out: return (table, levels), each
        [n, N, N] (synchronises); else None, asynchronous."""
        n = self.n_epoch - epoch0 if n is None else n
        if not copy_out:
            self._check(self._L.chomp_tri1h_setup(self._h, epoch0, n, int(moment), None, None))
            return None
        nk = self.config.halo_npoints
        tab = numpy.empty((n, nk, nk))
        lev = numpy.empty((n, nk, nk))
        self._check(self._L.chomp_tri1h_setup(self._h, epoch0, n, int(moment),
                                              ctypes.c_void_p(tab.ctypes.data),
                                              ctypes.c_void_p(lev.ctypes.data)))
        return tab, lev

    def tri1h_eval(self, ln_k1, ln_k2, epoch=0):
        """The table's bicubic at the points (ln_k1[i], ln_k2[i]) (chomp_tri1h_eval), each
        argument clamped into the knot range: numpy (host path) or contiguous float64 torch cuda
        tensors (device path, asynchronous; returns a tensor)."""
        def body(mem, new, a, b):
            assert _numel(a) == _numel(b)
            return epoch, a, b, _numel(a), new(_numel(a)), mem
        return self._run(self._L.chomp_tri1h_eval, [ln_k1, ln_k2], body)[0]

    def tri1h_quad(self, moment, k, epoch=0, levels=False):
        """i_0_4 at the quadruples k [N, 4] (chomp_tri1h_quad): numpy (host path) or a contiguous
        float64 torch cuda tensor (device path, asynchronous; returns tensors).  levels: also
        return the Romberg levels."""
        def body(mem, new, a):
            m, rest = divmod(_numel(a), 4)
            if rest:
                raise ValueError("tri1h_quad: k must be [N, 4]")
            return epoch, int(moment), a, m, new(m), new(m) if levels else None, mem
        outs = self._run(self._L.chomp_tri1h_quad, [k], body)
        return tuple(outs) if levels else outs[0]

    # -- two- to four-halo trispectrum ------------------------------------------------
    def tri_setup(self, epoch0=0, n=None, copy_out=False):
        """The five mass-integral tables of HaloTrispectrum, their levels and splines of the
        epochs [epoch0, epoch0 + n) (chomp_tri_setup).  copy_out: return (tables, levels), each a
        dictionary name -> [n, N, N] ([n, N] for "i_2_1") (synchronises); else None."""
        n = self.n_epoch - epoch0 if n is None else n
        if not copy_out:
            self._check(self._L.chomp_tri_setup(self._h, epoch0, n, None, None))
            return None
        nk = self.config.halo_npoints
        per = 4 * nk * nk + nk
        raw = [numpy.empty((n, per)), numpy.empty((n, per))]
        self._check(self._L.chomp_tri_setup(self._h, epoch0, n,
                                            ctypes.c_void_p(raw[0].ctypes.data),
                                            ctypes.c_void_p(raw[1].ctypes.data)))
        outs = []
        for r in raw:
            d = {}
            for j, name in enumerate(("i_0_4", "i_1_2", "i_1_3", "i_2_2")):
                d[name] = r[:, j * nk * nk:(j + 1) * nk * nk].reshape(n, nk, nk).copy()
            d["i_2_1"] = r[:, 4 * nk * nk:].copy()
            outs.append(d)
        return tuple(outs)

    def tri_table_eval(self, table, k1, k2, epoch=0):
        """Table `table` (a TRI_TAB key) at the points (k1[i], k2[i]) with the reference's clamp
        and zero rules (chomp_tri_table_eval); numpy or contiguous float64 torch cuda tensors."""
        def body(mem, new, a, b):
            if _numel(a) != _numel(b):
                raise ValueError("tri_table_eval: k1 and k2 differ in length")
            return epoch, TRI_TAB[table], a, b, _numel(a), new(_numel(a)), mem
        return self._run(self._L.chomp_tri_table_eval, [k1, k2], body)[0]

    def tri_terms(self, kkz, epoch=0, pt_epoch=0):
        """t_1_h .. t_4_h [N, 4] at the configurations kkz [N, 3] = (k1, k2, z)
        (chomp_tri_terms); numpy or a contiguous float64 torch cuda tensor."""
        def body(mem, new, a):
            m, rest = divmod(_numel(a), 3)
            if rest:
                raise ValueError("tri_terms: kkz must be [N, 3]")
            return epoch, pt_epoch, a, m, new((m, 4)), mem
        return self._run(self._L.chomp_tri_terms, [kkz], body)[0]

    def tri_proj(self, kk, epoch=0, pt_epoch=0, levels=False):
        """tri_spec_proj_integral at the pairs kk [N, 2] (chomp_tri_proj).  levels: also return
        the Romberg levels and the per-pair flags (1: NaN end point or divmax)."""
        def body(mem, new, a):
            m, rest = divmod(_numel(a), 2)
            if rest:
                raise ValueError("tri_proj: kk must be [N, 2]")
            return (epoch, pt_epoch, a, m, new(m), new(m) if levels else None,
                    new(m) if levels else None, mem)
        outs = self._run(self._L.chomp_tri_proj, [kk], body)
        return tuple(outs) if levels else outs[0]

    def tri_triple(self, k, epoch=0, levels=False):
        """i_1_3 at the triples k [N, 3] (chomp_tri_triple)."""
        def body(mem, new, a):
            m, rest = divmod(_numel(a), 3)
            if rest:
                raise ValueError("tri_triple: k must be [N, 3]")
            return epoch, a, m, new(m), new(m) if levels else None, mem
        outs = self._run(self._L.chomp_tri_triple, [k], body)
        return tuple(outs) if levels else outs[0]

    def halofit_setup(self, dst, src, f1, f2, f3, omega_l, w):
        self._check(self._L.chomp_halofit_setup(self._h, dst, src, f1, f2, f3,
                                                omega_l, w))

    # -- Stage E -------------------------------------------------------------
    def power(self, which, k, epoch0=0, n=None, out=None):
        """k: numpy array (host path) or torch cuda tensor (device path, async on
        the context's stream).  Returns [n, nk] in the same kind of container."""
        n = self.n_epoch - epoch0 if n is None else n
        return self._run(self._L.chomp_power_range, [k], lambda mem, new, k: (
            which, epoch0, n, k, _numel(k), new((n, _numel(k)), out), mem))[0]

    def power_plan(self, k, epoch0=0):
        """Register a torch cuda k grid for repeated power() calls (chomp_power_plan): the
        k-only work is done once; the caller keeps k unchanged meanwhile."""
        assert _is_torch(k) and k.is_cuda and k.is_contiguous()
        self._check(self._L.chomp_power_plan(self._h, epoch0, ctypes.c_void_p(k.data_ptr()),
                                             k.numel()))
        # The library recognises the registered grid by (address, length, cosmology).  Keeping
        # the tensor alive for as long as the context may hold that registration means the
        # caching allocator can never hand the same address to a different k grid.
        self._plan_k = k

    def sigma_r(self, epoch, scale):
        return self._run(self._L.chomp_sigma_r, [numpy.atleast_1d(scale)],
                         lambda mem, new, s: (epoch, s, s.size, new(s.shape)))[0]

    def y_nfw(self, epoch, ln_k, mass):
        a, b = numpy.broadcast_arrays(numpy.asarray(ln_k, dtype=numpy.float64),
                                      numpy.asarray(mass, dtype=numpy.float64))
        return self._run(self._L.chomp_y_nfw, [a, b],
                         lambda mem, new, a, b: (epoch, a, b, a.size, new(a.size)))[0]

    def y_general(self, epoch, ln_k, mass):
        """Halo.y_general at one scalar ln k (chomp_y_general): the table of y over the mass knots
        is integrated at that ln k, splined in ln M and evaluated at `mass` (0 outside the mass
        table)."""
        m = numpy.atleast_1d(numpy.asarray(mass, dtype=numpy.float64))
        return self._run(self._L.chomp_y_general, [m],
                         lambda mem, new, m: (epoch, float(ln_k), m, m.size, new(m.shape)))[0]

    def y_general_table(self, epoch=0):
        """(y[k][M], Romberg levels) of the epoch's general-profile table (chomp_y_general_table),
        each [halo_npoints, mass_npoints].  Synchronises."""
        shape = (self.config.halo_npoints, self.config.mass_npoints)
        y, lev = numpy.empty(shape), numpy.empty(shape)
        self._check(self._L.chomp_y_general_table(self._h, epoch, ctypes.c_void_p(y.ctypes.data),
                                                  ctypes.c_void_p(lev.ctypes.data)))
        return y, lev

    def halo_normalization(self, mass, epoch=0):
        """Halo.halo_normalization (chomp_halo_normalization) at `mass`."""
        m = numpy.atleast_1d(numpy.asarray(mass, dtype=numpy.float64))
        return self._run(self._L.chomp_halo_normalization, [m],
                         lambda mem, new, m: (epoch, m, m.size, new(m.shape)))[0]

    def scalars(self, epoch=0):
        out = numpy.empty(SC_COUNT)
        self._check(self._L.chomp_get_scalars(self._h, epoch,
                                              out.ctypes.data_as(c_double_p)))
        return {name: out[i] for name, i in SC.items()}

    def table(self, name, epoch=0):
        cfg = self.config
        n = {"ln_mass": cfg.mass_npoints, "nu": cfg.mass_npoints,
             "levels": 5 * cfg.halo_npoints}.get(name, cfg.halo_npoints)
        out = numpy.empty(n)
        self._check(self._L.chomp_get_table(self._h, epoch, TAB[name],
                                            out.ctypes.data_as(c_double_p), n))
        return out

    def put_table(self, name, values, epoch=0):
        """Install the knots of one knot table ("h_m" .. "pp_gg", "i_1_2") and rebuild its
        spline (chomp_put_table): get -> put leaves every spectrum bit for bit as it was."""
        v = numpy.ascontiguousarray(values, dtype=numpy.float64).ravel()
        self._check(self._L.chomp_put_table(self._h, epoch, TAB[name],
                                            v.ctypes.data_as(c_double_p), v.size))

    def set_delta_b(self, delta_b, epoch0=0):
        """HaloSuperSampleCovariance._delta_b of epochs [epoch0, epoch0 + len) (chomp_set_delta_b);
        numpy array / sequence (host) or torch cuda tensor (device, async on the stream)."""
        self._run(self._L.chomp_set_delta_b, [delta_b],
                  lambda mem, new, v: (epoch0, _numel(v), v, mem))

    def eval(self, what, x, epoch=0):
        """Element-wise lookup; x numpy (any shape) or torch cuda tensor."""
        return self._run(self._L.chomp_eval, [x],
                         _elementwise(epoch, EV[what], shape=numpy.shape(x)))[0]

    def halofit_get(self, epoch=0):
        out = numpy.empty(HF_COUNT)
        self._check(self._L.chomp_halofit_get(self._h, epoch,
                                              out.ctypes.data_as(c_double_p)))
        return out

    def halofit_put(self, coef, epoch=0):
        c = numpy.ascontiguousarray(coef, dtype=numpy.float64)
        assert c.size == HF_COUNT
        self._check(self._L.chomp_halofit_put(self._h, epoch,
                                              c.ctypes.data_as(c_double_p)))

    def sync(self):
        self._check(self._L.chomp_sync(self._h))

    def status(self, epoch0=0, n=None):
        """Per-epoch status words (uint32 array; bits ST_*, describe_status).  Synchronises."""
        n = self.n_epoch - epoch0 if n is None else n
        out = numpy.zeros(n, dtype=numpy.uint32)
        if n:
            self._check(self._L.chomp_get_status(
                self._h, epoch0, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint))))
        return out

    def status_post(self):
        """Enqueue a copy of the status words to pinned host memory (chomp_status_post): no
        synchronisation; status_wait / warn_status(posted=True) pick it up."""
        self._check(self._L.chomp_status_post(self._h))

    def status_wait(self, epoch0=0, n=None):
        """The words of the last status_post (waits for that copy only, not for the stream)."""
        n = self.n_epoch - epoch0 if n is None else n
        out = numpy.zeros(n, dtype=numpy.uint32)
        if n:
            self._check(self._L.chomp_status_wait(
                self._h, epoch0, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint))))
        return out

    def warn_status(self, epoch0=0, n=None, stacklevel=3, posted=False):
        """Turn the status words of the epochs into Python warnings, as the reference's
        scipy.integrate.romberg did for an exhausted divmax (AccuracyWarning); a saturated
        mass-limit search gets a ChompParityWarning.  Returns the words.  posted: the words of
        the last status_post instead of a fresh (synchronising) read."""
        import warnings
        words = self.status_wait(epoch0, n) if posted else self.status(epoch0, n)
        for i, w in enumerate(words):
            w = int(w)
            if not w:
                continue
            kind = (ChompParityWarning if w & (ST_SATURATED | ST_MASS_SEARCH_EXHAUSTED)
                    else ChompAccuracyWarning)
            warnings.warn("epoch %d: %s" % (epoch0 + i, "; ".join(describe_status(w))), kind,
                          stacklevel=stacklevel)
        return words

    def deep_stats(self):
        """(knots done by the fast deep-level sums, knots done by literal evaluation) so far."""
        out = (ctypes.c_longlong * 7)()
        self._check(self._L.chomp_get_deep_stats(self._h, out))
        self.deep_detail = {"too_many_breaks": int(out[2]), "too_many_fine": int(out[3]),
                            "self_check": int(out[4]), "worst_estimate": out[5] * 1e-15,
                            "needs_node_evaluation": int(out[6])}
        return int(out[0]), int(out[1])

    def set_tuning(self, what, value):
        """Test / tuning hook (chomp_set_tuning); value None or < 0 restores the default."""
        self._check(self._L.chomp_set_tuning(self._h, int(what), -1 if value is None else int(value)))

    # -- projection ------------------------------------------------------------
    def kernel_setup(self, cosmo_dict, me_z_min, me_z_max, ktheta_min, ktheta_max,
                     wa, wb, bessel_order, dark_energy=False):
        c = cosmo_struct(cosmo_dict)
        self._check(self._L.chomp_set_dark_energy(self._h, 1 if dark_energy else 0))
        # (a projection set-up drops the kernel_ssc and kernel_NG tables)
        self._proj_ssc = self._proj_ng = None
        self._check(self._L.chomp_kernel_setup(
            self._h, ctypes.byref(c), me_z_min, me_z_max, ktheta_min, ktheta_max,
            ctypes.byref(wa), ctypes.byref(wb), int(bessel_order)))

    def multi_epoch_setup(self, cosmo_dict, z_min, z_max, dark_energy=False):
        c = cosmo_struct(cosmo_dict)
        self._check(self._L.chomp_set_dark_energy(self._h, 1 if dark_energy else 0))
        self._proj_ssc = self._proj_ng = None
        self._check(self._L.chomp_multi_epoch_setup(self._h, ctypes.byref(c),
                                                    float(z_min), float(z_max)))

    def de_table(self, source="epoch", epoch=0):
        """The dark-energy pressure table of epoch `epoch`'s cosmology (source "epoch") or of
        the projection set-up's (source "proj"): dict of ln_a, pressure, levels (int),
        converged (bool) [cosmo_npoints] and the spline's coefficients pp [cosmo_npoints - 1, 4]."""
        n = self.config.cosmo_npoints
        src = {"epoch": DE_EPOCH, "proj": DE_PROJ}[source]
        out = {}
        for name, what, size in (("ln_a", 0, n), ("pressure", 1, n), ("levels", 2, n),
                                 ("converged", 3, n), ("pp", 4, 4 * (n - 1))):
            v = numpy.empty(size)
            self._check(self._L.chomp_get_de_table(self._h, src, epoch, what,
                                                   v.ctypes.data_as(c_double_p), size))
            out[name] = v
        out["levels"] = out["levels"].astype(numpy.int64)
        out["converged"] = out["converged"] != 0.0
        out["pp"] = out["pp"].reshape(n - 1, 4)
        return out

    def me_eval(self, what, x):
        return self._run(self._L.chomp_me_eval, [x], _elementwise(ME[what], shape=numpy.shape(x)))[0]

    def kernel_info(self):
        out = numpy.empty(KI_COUNT)
        self._check(self._L.chomp_kernel_info(self._h, out.ctypes.data_as(c_double_p)))
        return {name: out[i] for name, i in KI.items()}

    def kernel_table(self, name):
        cfg = self.config
        n = {"ln_ktheta": cfg.kernel_npoints, "kernel": cfg.kernel_npoints,
             "levels": cfg.kernel_npoints, "me_z": cfg.cosmo_npoints,
             "me_chi": cfg.cosmo_npoints, "me_growth": cfg.cosmo_npoints}.get(
                 name, cfg.window_npoints)
        out = numpy.empty(n)
        self._check(self._L.chomp_kernel_table(self._h, KTAB[name],
                                               out.ctypes.data_as(c_double_p), n))
        return out

    # -- the cosmology axis of the projection set-up --------------------------
    def _sets_call(self, call, args, tabulated, dark_energy):
        """One of the two set-ups of sets.  With an opt-in, chomp_set_sets_scope goes before the
        call and is taken back after it, also when it raised: the opt-in never sticks to the
        context.  Without one there is no call but the set-up's own."""
        flags = (SETS_TABULATED if tabulated else 0) | (SETS_DARK_ENERGY if dark_energy else 0)
        if not flags:
            self._check(call(*args))
            return
        self._check(self._L.chomp_set_sets_scope(self._h, flags))
        try:
            self._check(call(*args))
        finally:
            self._L.chomp_set_sets_scope(self._h, 0)

    def kernel_setup_sets(self, cosmo_dicts, me_z_min, me_z_max, ktheta_min, ktheta_max,
                          wa, wb, bessel_order, tabulated=False, dark_energy=False):
        """One projection set-up per cosmology (chomp_kernel_setup_sets): cosmo_dicts a list of
        dictionaries, a float64 array [n, 10] or the packed ctypes array (pack_cosmo).  The sets
        live beside the single set-up of kernel_setup, which stays as it is.  At most
        KERNEL_SETS_MAX sets per call (ValueError); ChompScopeError for a w0-wa cosmology unless
        dark_energy=True, and for a tabulated redshift distribution unless tabulated=True (the
        opt-ins hold for this call only: chomp_set_sets_scope)."""
        arr = (cosmo_dicts if isinstance(cosmo_dicts, ctypes.Array)
               else self.pack_cosmo(cosmo_dicts, len(cosmo_dicts)))
        self._sets_call(self._L.chomp_kernel_setup_sets,
                        (self._h, len(arr), arr, me_z_min, me_z_max, ktheta_min, ktheta_max,
                         ctypes.byref(wa), ctypes.byref(wb), int(bessel_order)),
                        tabulated, dark_energy)
        self._n_sets = len(arr)

    def kernel_setup_pairs(self, cosmo_dicts, me_z_min, me_z_max, ktheta_min, ktheta_max,
                           windows_a, windows_b, bessel_order, tabulated=False, dark_energy=False):
        """One projection set-up per kernel (chomp_kernel_setup_pairs): set s is what
        kernel_setup(cosmo_dicts[s], me_z_min[s], me_z_max[s], ktheta_min, ktheta_max,
        windows_a[s], windows_b[s], bessel_order) builds, bit for bit.  cosmo_dicts as in
        kernel_setup_sets; windows_a / windows_b lists of Window structs.  The sets replace those of
        the last kernel_setup_sets / kernel_setup_pairs; the single set-up stays as it is.
        ValueError for lists of other lengths and for more than KERNEL_SETS_MAX sets;
        ChompScopeError, naming the set, for a w0-wa cosmology unless dark_energy=True and for a
        tabulated distribution unless tabulated=True (as in kernel_setup_sets; equal tables are
        sent to the device once)."""
        arr = (cosmo_dicts if isinstance(cosmo_dicts, ctypes.Array)
               else self.pack_cosmo(cosmo_dicts, len(cosmo_dicts)))
        n = len(arr)
        z0 = numpy.ascontiguousarray(me_z_min, dtype=numpy.float64).ravel()
        z1 = numpy.ascontiguousarray(me_z_max, dtype=numpy.float64).ravel()
        if not (z0.size == z1.size == len(windows_a) == len(windows_b) == n):
            raise ValueError("kernel_setup_pairs: one cosmology, MultiEpoch range and window pair "
                             "per set")
        # (the structs are copied into two contiguous arrays; a tabulated distribution's arrays
        #  stay alive in the caller's structs for the duration of the call)
        wa = (Window * max(n, 1))(*windows_a)
        wb = (Window * max(n, 1))(*windows_b)
        self._sets_call(self._L.chomp_kernel_setup_pairs,
                        (self._h, n, arr, z0.ctypes.data_as(c_double_p), z1.ctypes.data_as(c_double_p),
                         float(ktheta_min), float(ktheta_max), wa, wb, int(bessel_order)),
                        tabulated, dark_energy)
        self._n_sets = n

    def kernel_info_sets(self):
        """kernel_info() of every set, as a dictionary of arrays [n_set]; one synchronising
        read-back."""
        n = getattr(self, "_n_sets", 0)
        out = numpy.empty((max(n, 1), KI_COUNT))
        self._check(self._L.chomp_kernel_info_sets(self._h, out.ctypes.data_as(c_double_p)))
        return {name: out[:n, i].copy() for name, i in KI.items()}

    def kernel_table_set(self, set_index, name):
        """kernel_table(name) of one set."""
        cfg = self.config
        n = {"ln_ktheta": cfg.kernel_npoints, "kernel": cfg.kernel_npoints,
             "levels": cfg.kernel_npoints, "me_z": cfg.cosmo_npoints,
             "me_chi": cfg.cosmo_npoints, "me_growth": cfg.cosmo_npoints}.get(
                 name, cfg.window_npoints)
        out = numpy.empty(n)
        self._check(self._L.chomp_kernel_table_set(self._h, int(set_index), KTAB[name],
                                                   out.ctypes.data_as(c_double_p), n))
        return out

    def wtheta_sets(self, which, epoch0, n_epoch, k_min, k_max, D_z, theta):
        """w(theta) of the epochs epoch0 .. epoch0 + n_epoch - 1, epoch epoch0 + e against
        projection set e with growth D_z[e] (chomp_wtheta_sets): [n_epoch, theta.size], row e what
        kernel_setup(<cosmology e>) + wtheta(which, epoch0 + e, ..., D_z[e], theta) returns, bit
        for bit.  D_z is a host array; theta a host array or a torch cuda tensor, as in
        wtheta_epochs."""
        D = _row_growth("wtheta_sets", D_z, n_epoch)
        return self._run(self._L.chomp_wtheta_sets, [theta], _rows(
            n_epoch, int(which), int(epoch0), int(n_epoch), float(k_min), float(k_max),
            _host_address(D)))[0]

    def cell_sets(self, which, epoch0, n_epoch, D_z, ell):
        """C_l of the epochs epoch0 .. epoch0 + n_epoch - 1, epoch epoch0 + e against projection
        set e with growth D_z[e] (chomp_cell_sets): [n_epoch, ell.size], row e what
        kernel_setup(<the inputs of set e>) + cell(which, epoch0 + e, D_z[e], ell) returns, bit for
        bit.  D_z is a host array; ell a host array or a torch cuda tensor, as in cell_epochs."""
        D = _row_growth("cell_sets", D_z, n_epoch)
        return self._run(self._L.chomp_cell_sets, [ell], _rows(
            n_epoch, int(which), int(epoch0), int(n_epoch), _host_address(D)))[0]

    def _run(self, fn, xs, body):
        """Call the array entry point fn on host or device arrays; returns the list of outputs.

        The first of the inputs xs decides.  A torch tensor (every input then a contiguous float64
        cuda tensor) is used in place: DEVICE, asynchronous on the context's stream and ordered
        against the caller's.  Anything else goes through numpy.ascontiguousarray(float64): HOST.
        body(mem, new, *xs) returns fn's arguments after the context handle, its arrays as they
        are (they are passed as pointers); new(shape) allocates an output of the same kind
        (new(shape, given): the caller's own array instead), and the outputs are returned in the
        order of those calls.  The library is not called when an input is empty."""
        outs = []
        if _is_torch(xs[0]):
            import torch
            for x in xs:
                assert x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()
            mem, empty, array, address = DEVICE, xs[0].new_empty, torch.Tensor, torch.Tensor.data_ptr
            called = all(x.numel() for x in xs)
        else:
            xs = [numpy.ascontiguousarray(x, dtype=numpy.float64) for x in xs]
            mem, empty, array, address = HOST, numpy.empty, numpy.ndarray, _host_address
            called = all(x.size for x in xs)

        def new(shape, given=None):
            outs.append(empty(shape) if given is None else given)
            return outs[-1]
        args = body(mem, new, *xs)
        if called:
            pair = self._torch_enter() if mem == DEVICE else None
            self._check(fn(self._h, *[address(a) if isinstance(a, array) else a for a in args]))
            self._torch_leave(pair)
        return outs

    def kernel_eval(self, ln_ktheta):
        return self._run(self._L.chomp_kernel_eval, [ln_ktheta], _elementwise())[0]

    def kernel_raw(self, ln_ktheta):
        return self._run(self._L.chomp_kernel_raw, [ln_ktheta], _elementwise())[0]

    def window_eval(self, which, chi):
        return self._run(self._L.chomp_window_eval, [chi], _elementwise(int(which)))[0]

    def wtheta(self, which, epoch, k_min, k_max, D_z, theta):
        return self._run(self._L.chomp_wtheta, [theta], _elementwise(
            int(which), epoch, float(k_min), float(k_max), float(D_z)))[0]

    def wtheta_epochs(self, which, epoch0, n_epoch, k_min, k_max, D_z, theta):
        """w(theta) of the epochs epoch0 .. epoch0 + n_epoch - 1 in one call (chomp_wtheta_epochs):
        [n_epoch, theta.size], row e what wtheta(which, epoch0 + e, ...) returns, bit for bit."""
        return self._run(self._L.chomp_wtheta_epochs, [theta], _rows(
            n_epoch, int(which), int(epoch0), int(n_epoch), float(k_min), float(k_max),
            float(D_z)))[0]

    def wtheta_cell(self, which, epoch, k_min, k_max, D_z, theta, ell):
        """(w(theta), C_l) of one set-up in one call (chomp_wtheta_cell): with torch cuda
        tensors C_l is computed beside w(theta) on the context's side stream; same numbers as
        wtheta() and cell().  Torch outputs keep the inputs' shapes, numpy outputs are flat."""
        w, c = self._run(self._L.chomp_wtheta_cell, [theta, ell], lambda mem, new, th, el: (
            int(which), epoch, float(k_min), float(k_max), float(D_z), th, _numel(th),
            new(th.shape if mem == DEVICE else _numel(th)), el, _numel(el),
            new(el.shape if mem == DEVICE else _numel(el)), mem))
        return w, c

    def set_timing(self, on=True):
        self._check(self._L.chomp_set_timing(self._h, int(bool(on))))

    def get_timing(self):
        """Microseconds of (k_power_prep, k_power_stream, k_power_grid_lanes) of the last
        timed streaming power() call."""
        out = numpy.empty(3)
        self._check(self._L.chomp_get_timing(self._h, out.ctypes.data_as(c_double_p), 3))
        return out

    def covariance_table(self, which, epoch, D_z):
        """(ln_K, projected spectrum, Romberg levels), each [kernel_npoints]."""
        n = self.config.kernel_npoints
        ln_K, proj, lev = numpy.empty(n), numpy.empty(n), numpy.empty(n)
        self._check(self._L.chomp_covariance_table(
            self._h, int(which), epoch, float(D_z), ln_K.ctypes.data_as(c_double_p),
            proj.ctypes.data_as(c_double_p), lev.ctypes.data_as(c_double_p), n))
        return ln_K, proj, lev.astype(int)

    def covariance_gaussian(self, j0_limit, area, poisson_a, poisson_b, theta_a, theta_b):
        return self._run(self._L.chomp_covariance_gaussian, [_pairs(theta_a, theta_b)],
                         lambda mem, new, th: (float(j0_limit), float(area), float(poisson_a),
                                               float(poisson_b), th, th.size // 2,
                                               new(th.size // 2), mem))[0]

    def covariance_cross_stage(self, slot, src, which, epoch=0):
        """Snapshot of one side of a cross block into this context (slot 0: correlation a, 1: b):
        the projection set-up and spectrum `which` of halo epoch `epoch` of context `src`."""
        self._check(self._L.chomp_covariance_cross_stage(self._h, int(slot), src._h, int(which),
                                                         epoch))

    def covariance_table_cross(self, D_a, D_b):
        """(ln_K [kernel_npoints], the projected spectra a, b, ab, ba [4, kernel_npoints], their
        Romberg levels [4, kernel_npoints]) of the two staged sides."""
        n = self.config.kernel_npoints
        ln_K, tab, lev = numpy.empty(n), numpy.empty((4, n)), numpy.empty((4, n))
        self._check(self._L.chomp_covariance_table_cross(
            self._h, float(D_a), float(D_b), ln_K.ctypes.data_as(c_double_p),
            tab.ctypes.data_as(c_double_p), lev.ctypes.data_as(c_double_p), n))
        return ln_K, tab, lev.astype(int)

    def covariance_gaussian_cross(self, j0_limit, area, poisson, theta_a, theta_b=None):
        """covariance_G of a cross block for pairs of bin centres.  poisson: the four
        proj_power_poisson(window_pair = 0..3).  (theta_a, theta_b): host arrays of one length;
        or theta_a alone, a contiguous float64 torch cuda tensor holding theta_a[n] then
        theta_b[n], which stays on the device (so does the result)."""
        pairs = theta_a if theta_b is None else _pairs(theta_a, theta_b)
        p = [float(v) for v in poisson]
        assert len(p) == 4
        return self._run(self._L.chomp_covariance_gaussian_cross, [pairs],
                         lambda mem, new, th: (float(j0_limit), float(area), p[0], p[1], p[2],
                                               p[3], th, _numel(th) // 2,
                                               new(_numel(th) // 2), mem))[0]

    def covariance_blocks(self, which, epochs, j0_limit, area, poisson, theta_a, theta_b=None):
        """covariance_G of every block (i, j), i <= j, of len(epochs) correlations for the same
        pairs of bin centres (chomp_covariance_blocks): [n_blocks, n_pairs], the blocks in the
        row-major order of the upper triangle.  Correlation c is projection set c of the last
        kernel_setup_pairs and halo epoch epochs[c]; a diagonal block is what kernel_setup +
        covariance_table + covariance_gaussian return, a cross block what two
        covariance_cross_stage + covariance_table_cross + covariance_gaussian_cross do, bit for
        bit.  poisson [n_blocks, 4]: proj_power_poisson(window_pair = 0..3) of every block.
        (theta_a, theta_b): host arrays of one length; or theta_a alone, a contiguous float64
        torch cuda tensor holding theta_a[n] then theta_b[n], which stays on the device (so does
        the result; the Poisson terms are sent there)."""
        def args(n_blocks):
            p = numpy.ascontiguousarray(poisson, dtype=numpy.float64)
            if p.shape != (n_blocks, 4):
                raise ValueError("covariance_blocks: poisson must be [%d, 4]" % n_blocks)
            return (int(which),), (float(j0_limit), float(area)), [p]
        return self._blocks(self._L.chomp_covariance_blocks, epochs, theta_a, theta_b, args)

    def _blocks(self, fn, epochs, theta_a, theta_b, args, term=None):
        """A covariance_*_blocks call, fn(handle, *head, n_corr, epochs, *middle, *sent, pairs,
        n_pairs, out, mem): out [n_blocks, n_pairs].  args(n_blocks) checks the call's own arrays
        and returns (head, middle, sent), `sent` the host arrays that go where the pairs are.
        term: the pair count covariance_<term>_blocks_table sizes the k_b knots by, remembered
        after a successful call only -- a refused call leaves the last result readable, its k_b
        knots included (the C call gives its state up behind its last refusal only)."""
        ep = numpy.ascontiguousarray(epochs, dtype=numpy.uintp).ravel()
        n_blocks = ep.size * (ep.size + 1) // 2
        head, middle, sent = args(n_blocks)
        pairs = theta_a if theta_b is None else _pairs(theta_a, theta_b)
        if sent and _is_torch(pairs):
            import torch
            sent = [torch.as_tensor(x, device=pairs.device) for x in sent]
        out = self._run(fn, [pairs] + sent, lambda mem, new, th, *on: head + (
            ep.size, ep.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))) + middle + on + (
                th, _numel(th) // 2, new((n_blocks, _numel(th) // 2)), mem))[0]
        if term:
            setattr(self, "_%s_blocks_pairs" % term, _numel(pairs) // 2)
        return out

    def _blocks_table(self, fn, term, block, knots, minimum=False):
        """One block of the last covariance_<term>_blocks, fn(handle, block, info, table, levels,
        [table_min,] kb_knots, kb_levels): (info [7], table and Romberg levels [kernel_npoints,
        kernel_npoints] [, min(table)]); with `knots` also (k_b knots, Romberg levels), each
        [n_pairs, kernel_npoints]."""
        n = self.config.kernel_npoints
        info, tab, lev, mn = numpy.empty(7), numpy.empty((n, n)), numpy.empty((n, n)), numpy.empty(1)
        kb = kl = None
        if knots:
            n_pairs = getattr(self, "_%s_blocks_pairs" % term, None)
            if not n_pairs:
                raise ChompError("covariance_%s_blocks_table before covariance_%s_blocks" % (term, term))
            kb, kl = numpy.empty((int(n_pairs), n)), numpy.empty((int(n_pairs), n))
        self._check(fn(self._h, int(block), _ptr(info), _ptr(tab), _ptr(lev),
                       *([_ptr(mn)] if minimum else []), _ptr(kb), _ptr(kl)))
        out = (info, tab, lev.astype(int)) + ((numpy.float64(mn[0]),) if minimum else ())
        return out + (kb, kl.astype(int)) if knots else out

    def covariance_blocks_table(self, block):
        """(ln_K [kernel_npoints], the projected spectra a, b, ab, ba [4, kernel_npoints], their
        Romberg levels [4, kernel_npoints], scalars [8]) of one block of the last
        covariance_blocks; a diagonal block has row 0 alone (the others are zero)."""
        n = self.config.kernel_npoints
        ln_K, tab, lev, sc = numpy.empty(n), numpy.empty((4, n)), numpy.empty((4, n)), numpy.empty(8)
        self._check(self._L.chomp_covariance_blocks_table(
            self._h, int(block), ln_K.ctypes.data_as(c_double_p), tab.ctypes.data_as(c_double_p),
            lev.ctypes.data_as(c_double_p), sc.ctypes.data_as(c_double_p), n))
        return ln_K, tab, lev.astype(int), sc

    def covariance_cross_range(self):
        """(z_min, z_max, chi_min, chi_max) of the four windows in the two staged slots."""
        out = numpy.empty(4)
        self._check(self._L.chomp_covariance_cross_range(self._h, out.ctypes.data_as(c_double_p)))
        return tuple(float(v) for v in out)

    def kernel_ssc_setup(self, ln_ktheta_min, ln_ktheta_max, j0_ssc_limit, ln_chi, sigma2,
                         with_table=True, cross=False):
        """Super-sample kernel of the context's windows, or with `cross` of the four windows in
        the two staged slots of a cross block.  Returns (info[3] = z_bar_NG,
        chi(z_bar_NG), growth_factor(z_bar_NG); table and Romberg levels, each
        [kernel_npoints, kernel_npoints], or None without the table)."""
        n = self.config.kernel_npoints
        x = numpy.ascontiguousarray(ln_chi, dtype=numpy.float64)
        y = numpy.ascontiguousarray(sigma2, dtype=numpy.float64)
        assert x.size == y.size
        info = numpy.empty(3)
        tab, lev = (numpy.empty((n, n)), numpy.empty((n, n))) if with_table else (None, None)
        fn = self._L.chomp_kernel_ssc_setup_cross if cross else self._L.chomp_kernel_ssc_setup
        self._check(fn(
            self._h, float(ln_ktheta_min), float(ln_ktheta_max), float(j0_ssc_limit),
            _ptr(x), _ptr(y), x.size, int(bool(with_table)), _ptr(info), _ptr(tab), _ptr(lev)))
        return info, tab, (lev.astype(int) if with_table else None)

    def _pair_eval(self, fn, a, b):
        """One value per pair (a[i], b[i]) of ln(k theta): the four kernel_{ssc,ng}_{raw,eval}."""
        return self._run(fn, [_pairs(a, b)], lambda mem, new, x: (x, x.size // 2, new(x.size // 2)))[0]

    def _pair_knots(self, fn, pre, theta_a, theta_b, knots):
        """fn(handle, *pre, theta, n, out, k_b knots, levels) of covariance_ssc, _ssc_cross and
        _ng: the value per pair; with `knots` also (k_b knots, Romberg levels), each
        [n, kernel_npoints] (without, the C call gets no array for them)."""
        nk = self.config.kernel_npoints

        def body(mem, new, th):
            n = th.size // 2
            return pre + (th, n, new(n), new((n, nk)) if knots else None,
                          new((n, nk)) if knots else None)
        outs = self._run(fn, [_pairs(theta_a, theta_b)], body)
        if knots:
            return outs[0], outs[1], outs[2].astype(int)
        return outs[0]

    def kernel_ssc_raw(self, ln_ktheta_a, ln_ktheta_b):
        return self._pair_eval(self._L.chomp_kernel_ssc_raw, ln_ktheta_a, ln_ktheta_b)

    def kernel_ssc_eval(self, ln_ktheta_a, ln_ktheta_b):
        return self._pair_eval(self._L.chomp_kernel_ssc_eval, ln_ktheta_a, ln_ktheta_b)

    def covariance_ssc(self, epoch, area, theta_a, theta_b, knots=False):
        """covariance_ssc for each pair; with knots=True also (k_b knots, Romberg levels),
        each [n, kernel_npoints]."""
        return self._pair_knots(self._L.chomp_covariance_ssc, (epoch, float(area)), theta_a, theta_b,
                                knots)

    def covariance_ssc_cross(self, area, theta_a, theta_b, knots=False):
        """covariance_ssc of a cross block for each pair (halo_a's response at k_a, halo_b's at
        k_b, from the staged slots); with knots=True also (k_b knots, Romberg levels)."""
        return self._pair_knots(self._L.chomp_covariance_ssc_cross, (float(area),), theta_a, theta_b,
                                knots)

    def covariance_ssc_blocks_range(self, n_corr):
        """[n_blocks, 4] = (z_min, z_max, chi_min, chi_max) of the windows of every block (i, j),
        i <= j, of the n_corr projection sets of the last kernel_setup_pairs, in the row-major
        order of the upper triangle: a diagonal block's as kernel_info gives them, a cross block's
        as covariance_cross_range does.  One launch, one read-back."""
        n_corr = int(n_corr)
        out = numpy.empty((n_corr * (n_corr + 1) // 2, 4))
        self._check(self._L.chomp_covariance_ssc_blocks_range(self._h, n_corr,
                                                              out.ctypes.data_as(c_double_p)))
        return out

    def covariance_ssc_blocks(self, epochs, ln_ktheta_min, ln_ktheta_max, j0_ssc_limit, ln_chi,
                              sigma2, area, theta_a, theta_b=None):
        """covariance_ssc of every block (i, j), i <= j, of len(epochs) correlations for the same
        pairs of bin centres (chomp_covariance_ssc_blocks): [n_blocks, n_pairs], the blocks in the
        row-major order of the upper triangle.  Correlation c is projection set c of the last
        kernel_setup_pairs and halo epoch epochs[c]; a diagonal block is what kernel_setup +
        kernel_ssc_setup + covariance_ssc return, a cross block what two covariance_cross_stage +
        kernel_ssc_setup(cross=True) + covariance_ssc_cross do, bit for bit.  ln_chi, sigma2
        [n_blocks, corr_npoints]: every block's own sigma^2 knots (host arrays).
        (theta_a, theta_b): host arrays of one length; or theta_a alone, a contiguous float64
        torch cuda tensor holding theta_a[n] then theta_b[n], which stays on the device (so does
        the result)."""
        def args(n_blocks):
            x = numpy.ascontiguousarray(ln_chi, dtype=numpy.float64)
            y = numpy.ascontiguousarray(sigma2, dtype=numpy.float64)
            if x.ndim != 2 or x.shape[0] != n_blocks or y.shape != x.shape:
                raise ValueError("covariance_ssc_blocks: ln_chi and sigma2 must be [%d, n_sigma]"
                                 % n_blocks)
            return (), (float(ln_ktheta_min), float(ln_ktheta_max), float(j0_ssc_limit), _ptr(x),
                        _ptr(y), x.shape[1], float(area)), []
        return self._blocks(self._L.chomp_covariance_ssc_blocks, epochs, theta_a, theta_b, args, "ssc")

    def covariance_ssc_blocks_table(self, block, knots=False):
        """One block of the last covariance_ssc_blocks: (info[7] = z_bar_NG, chi(z_bar_NG),
        growth_factor(z_bar_NG), z_min, z_max, chi_min, chi_max; the kernel_ssc table and its
        Romberg levels, each [kernel_npoints, kernel_npoints]); with knots=True also (k_b knots,
        Romberg levels), each [n_pairs, kernel_npoints]."""
        return self._blocks_table(self._L.chomp_covariance_ssc_blocks_table, "ssc", block, knots)

    def covariance_fourier_zbar(self, z):
        """_calculate_zbar of the four window pairs a1a2, b1b2, a1b2, b1a2 in the two staged slots
        on the grid z: [4, 7] = z_min, z_max, z_bar, chi(z_bar), chi(z_min), chi(z_max),
        growth_factor(z_bar) per pair."""
        z = numpy.ascontiguousarray(z, dtype=numpy.float64)
        info = numpy.empty((4, 7))
        self._check(self._L.chomp_covariance_fourier_zbar(
            self._h, z.ctypes.data_as(c_double_p), z.size, info.ctypes.data_as(c_double_p)))
        return info

    def covariance_fourier_table(self, which, epochs, ln_l):
        """The four Limber tables of CovarianceFourier over the knots ln_l, pair X from spectrum
        `which` of halo epoch epochs[X]: (norms [4], tables [4, n] = integral / D(z_bar)^2, Romberg
        levels [4, n])."""
        x = numpy.ascontiguousarray(ln_l, dtype=numpy.float64)
        n = x.size
        ep = (ctypes.c_size_t * 4)(*[int(e) for e in epochs])
        norms, tab, lev = numpy.empty(4), numpy.empty((4, n)), numpy.empty((4, n))
        self._check(self._L.chomp_covariance_fourier_table(
            self._h, int(which), ep, x.ctypes.data_as(c_double_p), n,
            norms.ctypes.data_as(c_double_p), tab.ctypes.data_as(c_double_p),
            lev.ctypes.data_as(c_double_p)))
        return norms, tab, lev.astype(int)

    def covariance_fourier_gaussian(self, ln_l_and_l):
        """[5, n]: the four _pl_X and covariance_G at n multipoles; the argument holds ln l[n] then
        l[n] (a host array, or a contiguous float64 torch cuda tensor: the result stays on the
        device then)."""
        return self._run(self._L.chomp_covariance_fourier_gaussian, [ln_l_and_l],
                         lambda mem, new, x: (x, _numel(x) // 2, new((5, _numel(x) // 2)), mem))[0]

    def kernel_ng_setup(self, j0_limit, with_table=True):
        """Trispectrum kernel of the context's windows, after kernel_ssc_setup.  Returns (table,
        Romberg levels, min(table)), the first two [kernel_npoints, kernel_npoints]; (None, None,
        None) without the table."""
        if not with_table:
            self._check(self._L.chomp_kernel_ng_setup(self._h, float(j0_limit), 0, None, None,
                                                      None))
            return None, None, None
        n = self.config.kernel_npoints
        tab, lev, mn = numpy.empty((n, n)), numpy.empty((n, n)), numpy.empty(1)
        self._check(self._L.chomp_kernel_ng_setup(
            self._h, float(j0_limit), 1, tab.ctypes.data_as(c_double_p),
            lev.ctypes.data_as(c_double_p), mn.ctypes.data_as(c_double_p)))
        return tab, lev.astype(int), numpy.float64(mn[0])

    def warn_cov_ng_divmax(self, what, stacklevel=4):
        """ChompAccuracyWarning if ST_COV_NG_DIVMAX is set (on the context's first epoch)."""
        if self.n_epoch and self.status(0, 1)[0] & ST_COV_NG_DIVMAX:
            import warnings
            warnings.warn("%s: %s" % (what, "; ".join(describe_status(ST_COV_NG_DIVMAX))),
                          ChompAccuracyWarning, stacklevel=stacklevel)

    def kernel_ng_raw(self, ln_ktheta_a, ln_ktheta_b):
        return self._pair_eval(self._L.chomp_kernel_ng_raw, ln_ktheta_a, ln_ktheta_b)

    def kernel_ng_eval(self, ln_ktheta_a, ln_ktheta_b):
        return self._pair_eval(self._L.chomp_kernel_ng_eval, ln_ktheta_a, ln_ktheta_b)

    def covariance_ng(self, area, tri_table, tri_k_min, tri_k_max, theta_a, theta_b,
                      knots=False):
        """covariance_NG for each pair with the I_0^4 table tri_table [N, N] over
        linspace(ln tri_k_min, ln tri_k_max, N); with knots=True also (k_b knots, Romberg
        levels), each [n, kernel_npoints]."""
        tri = numpy.ascontiguousarray(tri_table, dtype=numpy.float64)
        if tri.ndim != 2 or tri.shape[0] != tri.shape[1]:
            raise ValueError("covariance_ng: the I_0^4 table must be square")
        return self._pair_knots(self._L.chomp_covariance_ng,
                                (float(area), tri, tri.shape[0], float(tri_k_min), float(tri_k_max)),
                                theta_a, theta_b, knots)

    def covariance_ng_blocks(self, epochs, ln_ktheta_min, ln_ktheta_max, j0_limit, area, tri_table,
                             tri_k_min, tri_k_max, theta_a, theta_b=None):
        """covariance_NG of every block (i, j), i <= j, of len(epochs) correlations for the same
        pairs of bin centres (chomp_covariance_ng_blocks): [n_blocks, n_pairs], the blocks in the
        row-major order of the upper triangle.  Correlation c is projection set c of the last
        kernel_setup_pairs; a diagonal block is what kernel_setup + kernel_ssc_setup(with_table=
        False) + kernel_ng_setup + covariance_ng return, a cross block what two
        covariance_cross_stage + kernel_ssc_setup(cross=True, with_table=False) + kernel_ng_setup
        + covariance_ng do, bit for bit.  The term reads no halo epoch: epochs[c] only names the
        status word ST_COV_NG_DIVMAX of a block (c, j) goes to.  tri_table [N, N]: the I_0^4 table
        over linspace(ln tri_k_min, ln tri_k_max, N) (a host array), one for all blocks.
        (theta_a, theta_b): host arrays of one length; or theta_a alone, a contiguous float64
        torch cuda tensor holding theta_a[n] then theta_b[n], which stays on the device (so does
        the result)."""
        def args(n_blocks):
            tri = numpy.ascontiguousarray(tri_table, dtype=numpy.float64)
            if tri.ndim != 2 or tri.shape[0] != tri.shape[1]:
                raise ValueError("covariance_ng_blocks: the I_0^4 table must be square")
            return (), (float(ln_ktheta_min), float(ln_ktheta_max), float(j0_limit), float(area),
                        _ptr(tri), tri.shape[0], float(tri_k_min), float(tri_k_max)), []
        return self._blocks(self._L.chomp_covariance_ng_blocks, epochs, theta_a, theta_b, args, "ng")

    def covariance_ng_blocks_table(self, block, knots=False):
        """One block of the last covariance_ng_blocks: (info[7] = z_bar_NG, chi(z_bar_NG),
        growth_factor(z_bar_NG), z_min, z_max, chi_min, chi_max; the kernel_NG table and its
        Romberg levels, each [kernel_npoints, kernel_npoints]; min(table)); with knots=True also
        (k_b knots, Romberg levels), each [n_pairs, kernel_npoints]."""
        return self._blocks_table(self._L.chomp_covariance_ng_blocks_table, "ng", block, knots, True)

    def hod_stats(self, epoch0=0, n=None):
        """[n, 3]: effective bias, effective halo mass, satellite fraction."""
        n = self.n_epoch - epoch0 if n is None else n
        out = numpy.empty((n, 3))
        self._check(self._L.chomp_hod_stats(self._h, epoch0, n, out.ctypes.data_as(c_double_p)))
        return out

    def xi3d(self, which, epoch, k_min, k_max, r):
        return self._run(self._L.chomp_xi3d, [r], _elementwise(
            int(which), epoch, float(k_min), float(k_max)))[0]

    def xi3d_epochs(self, which, epoch0, n_epoch, k_min, k_max, r):
        """xi(r) of the epochs epoch0 .. epoch0 + n_epoch - 1 in one call (chomp_xi3d_epochs):
        [n_epoch, r.size], row e what xi3d(which, epoch0 + e, ...) returns, bit for bit.  Needs no
        kernel set-up."""
        return self._run(self._L.chomp_xi3d_epochs, [r], _rows(
            n_epoch, int(which), int(epoch0), int(n_epoch), float(k_min), float(k_max)))[0]

    def spline_eval(self, xk, yk, x, deriv=0):
        """Not-a-knot cubic spline through (xk, yk) at x (FITPACK k=3, s=0); deriv=1: its
        first derivative."""
        xk = numpy.ascontiguousarray(xk, dtype=numpy.float64)
        yk = numpy.ascontiguousarray(yk, dtype=numpy.float64)
        return self._run(self._L.chomp_spline_eval, [numpy.atleast_1d(x)], lambda mem, new, x: (
            xk, yk, xk.size, x, x.size, int(deriv), new(x.size)))[0]

    def set_precision(self, mode):
        """Arithmetic of the w(theta) integral: PREC_F64 (default, the only mode held to
        the parity bar) or one of the narrowed modes of the configs[4] precision sweep."""
        self._check(self._L.chomp_set_precision(self._h, int(mode)))

    def cell(self, which, epoch, D_z, ell):
        return self._run(self._L.chomp_cell, [ell], _elementwise(int(which), epoch, float(D_z)))[0]

    def cell_epochs(self, which, epoch0, n_epoch, D_z, ell):
        """C_l of the epochs epoch0 .. epoch0 + n_epoch - 1 in one call (chomp_cell_epochs):
        [n_epoch, ell.size], row e what cell(which, epoch0 + e, D_z, ell) returns, bit for bit."""
        return self._run(self._L.chomp_cell_epochs, [ell], _rows(
            n_epoch, int(which), int(epoch0), int(n_epoch), float(D_z)))[0]
