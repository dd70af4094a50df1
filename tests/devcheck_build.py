"""Builds and loads the TEST-ONLY device harnesses under tests/devcheck, the device counterparts
of tests/hostcheck: libdevcheck.so (devcheck.hip: the fp64 primitives of chomp_math.h and the
wavefront Romberg of chomp_romberg.h), libdevphys.so (devphys.hip: the halo-model physics of
chomp_math.h, through the product's whole header chain from chomp_cov_kernels.h down) and
libdevproj.so (devproj.hip: the moment route of w(theta), the bicubic tables and HaloFit's
quintic derivatives of chomp_proj_kernels.h / chomp_cov_kernels.h) and libdevpower.so
(devpower.hip: the spectrum evaluator and the Stage E launch shapes of chomp_power_kernels.h,
the spectrum table and its stencil of chomp_proj_kernels.h) and libdevcell.so (devcell.hip: the
C_l route -- the node table, k_cell, k_cell4, the hand-over, k_cell_deep and their _epochs / _sets
forms with the Romberg levels as arguments -- the plan of its work buffer, and the parallel
not-a-knot spline build in the block shapes the product calls it in).  Each harness is
compiled with the product's compiler flags (imported from chomp_amd._lib, never copied) and
rebuilt only when the content of what IT is compiled from changes, as _lib.py does for the
product library: its own source, .so and content hash, the hash over every product header it
includes.  hipcc cross-compiles for gfx950 without a GPU."""
import ctypes
import hashlib
import os
import re
import subprocess

from chomp_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "devcheck")


def included_headers(src):
    """Every file that `src` includes with quotes, transitively (the product headers and the C
    header: whatever a change of can change the harness), in a fixed order."""
    seen, todo = [], [src]
    while todo:
        path = todo.pop()
        with open(path) as f:
            text = f.read()
        for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, re.M):
            inc = os.path.normpath(os.path.join(os.path.dirname(path), name))
            if inc not in seen and os.path.exists(inc):     # (not one found through -I)
                seen.append(inc)
                todo.append(inc)
    return sorted(seen)


class Harness:
    """One translation unit tests/devcheck/<name>.hip -> lib<name>.so (+ .srchash)."""

    def __init__(self, name):
        self.name = name
        self.src = os.path.join(DIR, name + ".hip")
        self.so = os.path.join(DIR, "lib" + name + ".so")
        self.hash = self.so + ".srchash"

    @property
    def headers(self):
        return included_headers(self.src)


HARNESSES = {"devcheck": Harness("devcheck"), "devphys": Harness("devphys"),
             "devproj": Harness("devproj"), "devpower": Harness("devpower"),
             "devcell": Harness("devcell")}
# the first harness under its earlier names
SRC = HARNESSES["devcheck"].src
SO = HARNESSES["devcheck"].so
HASH = HARNESSES["devcheck"].hash
HEADERS = HARNESSES["devcheck"].headers

c_double_p = ctypes.POINTER(ctypes.c_double)
_i, _p = ctypes.c_int, c_double_p
# every entry point the GPU tests use, with its argument types (all return the HIP error code,
# except the plain getters)
ENTRY_POINTS = {
    "dc_case_stride": [], "dc_out_stride": [], "dc_index_out_stride": [], "dc_fma_k_count": [],
    "dc_fma_k_constants": [_p], "dc_gl16": [_p],
    "dc_exp": [_p, _i, _p, _p],
    "dc_fast_log": [_p, _i, _p],
    "dc_sincos": [_p, _i, _p],
    "dc_sici": [_p, _p, _i, _p],
    "dc_bessel": [_i, _p, _i, _p],
    "dc_fma_k": [_p, _p, _i, _p, _p],
    "dc_spline": [_p, _p, _i, _p, _i, _p, _i],
    "dc_wave_sum": [_i, _p, _i, _p],
    "dc_group_sum": [_i, _p, _p, _i, _p, _p],
    "dc_quad": [_i, _p, _i, _p],
    "dc_resume": [_i, _p, _i, _p],
    "dc_index": [_i, _p, _i, _p],
    "dc_gauss": [_i, _p, _i, _p],
}
_v, _ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)
_d = ctypes.c_double
# the same for the second harness (devphys.hip)
PHYS_ENTRY_POINTS = {
    "dp_sizeof_epoch": [], "dp_epoch_inputs": [], "dp_power_fields": [], "dp_mf_fields": [],
    "dp_hod_fields": [], "dp_nfw_fields": [],
    "dp_epoch_field_names": [], "dp_epoch_offsets": [_ip],
    "dp_epoch": [_p, _v],
    "dp_scalars": [_v, _p, _p, _i, _p],
    "dp_power": [_v, _p, _i, _p],
    "dp_sigma": [_v, _d, _p, _i, _p, _p],
    "dp_mf": [_v, _p, _p, _i, _p],
    "dp_hod": [_v, _p, _i, _p],
    "dp_nfw": [_v, _p, _p, _i, _p],
    "dp_exclusion": [_p, _i, _p],
    "dp_e0_de": [_v, _p, _p, _i, _p, _i, _p, _p],
    "dp_linspace": [_p, _p, _p, _p, _i, _d, _d, _p],
}
# ... and for the third (devproj.hip)
PROJ_ENTRY_POINTS = {
    "dj_wth_items": [], "dj_wth_parts": [],
    "dj_wth_sizes": [_i, _i, _i, _p],
    "dj_moments": [_p, _i, _i, _d, _d, _i, _p],
    "dj_wtheta": [_p, _i, _i, _d, _d, _i, _i, _p, _d, _d, _p, _i, _ip, _i, _d, _d, _p, _p, _p],
    "dj_kernel_eval": [_i, _p, _d, _d, _p, _i, _p],
    "dj_ssc": [_i, _p, _p, _d, _d, _p, _p, _i, _p, _i, _p, _i, _p, _p, _p],
    "dj_ng": [_i, _p, _p, _d, _d, _p, _p, _i, _p, _p, _p],
    "dj_quintic_grid": [_i, _p],
    "dj_quintic": [_p, _i, _p, _i, _p],
}
# ... and for the fourth (devpower.hip); _S: the set-up every entry point starts with (n_epoch,
# ein, tab, NK, k_min, k_max)
_S = [_i, _p, _p, _i, _d, _d]
POWER_ENTRY_POINTS = {
    "dw_ptab_n": [], "dw_sizeof_epoch": [], "dw_epoch_inputs": [], "dw_wave_bits": [_ip],
    "dw_layout": [_i, _ip],
    "dw_logs": [_d, _d, _p],
    "dw_epochs": _S + [_v, _p],
    "dw_eval": _S + [_p, _i, _i, _p, _i, _p],
    "dw_at_ln": _S + [_p, _i, _i, _i, _p, _i, _p],
    "dw_grid": _S + [_p, _i, _i, _i, _i, _p, _i, _p],
    "dw_stream": _S + [_p, _i, _i, _i, _i, _p, _i, _i, _p, _ip, _ip],
    "dw_extrap": _S + [_i, _i, _p],
    "dw_ptab": _S[1:] + [_i, _p],
    "dw_stencil": _S[1:] + [_i, _p, _p, _p, _i, _p],
}
# ... and for the sixth (devcell.hip; the fifth, devaim.hip, is registered by its test module)
_ll, _llp, _u = ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong), ctypes.c_uint
CELL_ENTRY_POINTS = {
    "dl_romberg_dump": [], "dl_ptab_n": [], "dl_pd_inputs": [], "dl_constants": [_ip],
    "dl_proj_layout": [_i, _i, _i, _ip],
    "dl_plan": [_i, _i, _i, _i, _i, _ll, _ll, _i, _llp],
    "dl_nodes": [_i, _i, _p, _p, _d, _i, _i, _ll, _i, _p, _ip],
    "dl_nodes_sets": [_i, _i, _i, _p, _p, _p, _i, _i, _p],
    "dl_spline": [_i, _p, _p, _i, _i, _u, _i, _p],
    "dl_logs": [_p, _i, _p],
    "dl_cell": _S + [_i, _i, _i, _i, _i, _p, _p, _p, _p, _i, _d, _d, _i, _i, _i, _i, _i, _i, _i, _i,
                     _p, _p, _p, _p],
}
ALL_ENTRY_POINTS = {"devcheck": ENTRY_POINTS, "devphys": PHYS_ENTRY_POINTS,
                    "devproj": PROJ_ENTRY_POINTS, "devpower": POWER_ENTRY_POINTS,
                    "devcell": CELL_ENTRY_POINTS}
# dc_quad shapes
SHAPE = {"group1": 0, "group2": 1, "group4": 2, "group8": 3, "group16": 4,
         "group1_nf2": 5, "group4_nf2": 6, "group4_unroll4": 7, "group4_fast4": 8,
         "wave6": 9, "wave6_nf2": 10, "romberg1_1": 11, "romberg1_4": 12}


def flags():
    return list(_lib.HIPCC_FLAGS) + list(_lib.NO_LICM)


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def have_hipcc():
    return os.path.exists(hipcc())


def source_hash(harness="devcheck"):
    H = HARNESSES[harness]
    h = hashlib.sha256()
    h.update(repr(flags()).encode())
    for path in [H.src] + H.headers:
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def build(force=False, harness="devcheck"):
    """Compile one harness (no-op when it was built from exactly these sources and flags)."""
    H = HARNESSES[harness]
    want = source_hash(harness)
    if not force and os.path.exists(H.so):
        try:
            with open(H.hash) as f:
                if f.read().strip() == want:
                    return H.so
        except OSError:
            pass
    tmp = H.so + ".tmp%d" % os.getpid()
    subprocess.check_call([hipcc()] + flags() + ["-shared", "-o", tmp, H.src], cwd=DIR)
    os.replace(tmp, H.so)
    with open(H.hash, "w") as f:
        f.write(want + "\n")
    return H.so


VOID = {"devcheck": ("dc_fma_k_constants", "dc_gl16"), "devphys": ("dp_epoch_offsets",),
        "devproj": ("dj_quintic_grid",), "devpower": ("dw_wave_bits",),
        "devcell": ("dl_constants",)}


def load(harness="devcheck"):
    """Build if necessary and load one harness, on the process's one HIP runtime."""
    path = build(harness=harness)
    _lib._preload_hip_runtime()
    L = ctypes.CDLL(path)
    for name, argtypes in ALL_ENTRY_POINTS[harness].items():
        fn = getattr(L, name)           # AttributeError: the harness lacks an entry point
        fn.argtypes = argtypes
        fn.restype = None if name in VOID[harness] else ctypes.c_int
    if harness == "devphys":
        L.dp_epoch_field_names.restype = ctypes.c_char_p
    return L


def epoch_fields(L):
    """{field name: (byte offset, is_int)} of the Epoch fields the devphys harness lists."""
    names = L.dp_epoch_field_names().decode().strip(",").split(",")
    raw = (ctypes.c_int * (2 * len(names)))()
    L.dp_epoch_offsets(raw)
    return {nm: (raw[2 * j], bool(raw[2 * j + 1])) for j, nm in enumerate(names)}


def ptr(a):
    return a.ctypes.data_as(c_double_p)


_failed = None


def call(L, name, *args):
    """Run one entry point.  A HIP error ends the test, and nothing more is launched through the
    harness in this process after it (a faulted GPU is not handed further work)."""
    global _failed
    if _failed is not None:
        raise RuntimeError("not run: %s failed earlier in this process" % _failed)
    rc = getattr(L, name)(*args)
    if rc != 0:
        _failed = "%s (HIP error %d)" % (name, rc)
        raise RuntimeError(_failed)
