"""Builds and loads tests/devcheck/libdevcheck.so, the TEST-ONLY device harness of the fp64
primitives (chomp_math.h) and the wavefront Romberg (chomp_romberg.h): the device counterpart of
tests/hostcheck.  Compiled with the product's own compiler flags (imported from chomp_amd._lib,
never copied) and rebuilt only when the content of what it is compiled from changes, as _lib.py
does for the product library.  hipcc cross-compiles for gfx950 without a GPU."""
import ctypes
import hashlib
import os
import subprocess

from chomp_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "devcheck")
SRC = os.path.join(DIR, "devcheck.hip")
SO = os.path.join(DIR, "libdevcheck.so")
HASH = SO + ".srchash"
HEADERS = [os.path.join(_lib.CSRC, name)
           for name in ("chomp_math.h", "chomp_romberg.h", "special_tables.h")]

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


def source_hash():
    h = hashlib.sha256()
    h.update(repr(flags()).encode())
    for path in [SRC] + HEADERS:
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def build(force=False):
    """Compile the harness (no-op when it was built from exactly these sources and flags)."""
    want = source_hash()
    if not force and os.path.exists(SO):
        try:
            with open(HASH) as f:
                if f.read().strip() == want:
                    return SO
        except OSError:
            pass
    tmp = SO + ".tmp%d" % os.getpid()
    subprocess.check_call([hipcc()] + flags() + ["-shared", "-o", tmp, SRC], cwd=DIR)
    os.replace(tmp, SO)
    with open(HASH, "w") as f:
        f.write(want + "\n")
    return SO


def load():
    """Build if necessary and load the harness, on the process's one HIP runtime."""
    path = build()
    _lib._preload_hip_runtime()
    L = ctypes.CDLL(path)
    for name, argtypes in ENTRY_POINTS.items():
        fn = getattr(L, name)           # AttributeError: the harness lacks an entry point
        fn.argtypes = argtypes
        fn.restype = None if name in ("dc_fma_k_constants", "dc_gl16") else ctypes.c_int
    return L


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
