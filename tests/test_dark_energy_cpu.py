"""CPU tests of w0-wa dark energy (cosmology.py:96-104, 165-213): the host build of the device
code in chomp_math.h -- the pressure integrand, its knots, scipy's Romberg stopping rule over it,
the spline and E0 -- against the reference (G22), and how HaloGrid packs and opts in a batch that
mixes Lambda-CDM and w0-wa cosmologies."""
import ctypes
import os
import subprocess

import numpy
import pytest

from conftest import ROOT, load_golden
from params import c_dict

TAGS = ("a_", "b_", "c_")
HC = os.path.join(ROOT, "tests", "hostcheck")
dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def hc():
    so = os.path.join(HC, "libdecheck.so")
    src = os.path.join(HC, "decheck.cpp")
    deps = [src, os.path.join(ROOT, "chomp_amd", "csrc", "chomp_math.h"),
            os.path.join(ROOT, "include", "chomp_mi355x.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, deps)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.dc_knots.argtypes = [ctypes.c_double, ctypes.c_int, dp, dp]
    lib.dc_pressure.argtypes = [ctypes.c_double, ctypes.c_double, dp, ctypes.c_int,
                                ctypes.c_double, ctypes.c_double, ctypes.c_int, dp, ip, ip]
    lib.dc_e0.argtypes = [ctypes.c_double] * 3 + [dp, dp, ctypes.c_int, dp, ctypes.c_int, dp]
    return lib


@pytest.fixture(scope="module")
def g():
    return load_golden("g22_dark_energy")


def _p(a):
    return a.ctypes.data_as(dp)


def _prec():
    from chomp_amd import defaults
    return defaults.default_precision


def test_knots(hc, g):
    """numpy.logspace(log10(cosmo_precision), 0, cosmo_npoints): ln a and z = 1 / a - 1, with the
    C library's pow -- numpy's vectorised power may round a knot the other way (1 ulp)."""
    p = _prec()
    n = p["cosmo_npoints"]
    ln_a, z = numpy.empty(n), numpy.empty(n)
    hc.dc_knots(p["cosmo_precision"], n, _p(ln_a), _p(z))
    numpy.testing.assert_array_max_ulp(z, g["de_z"], maxulp=1)
    numpy.testing.assert_array_max_ulp(ln_a, g["de_ln_a"], maxulp=1)
    assert z[-1] == 0.0 and ln_a[-1] == 0.0


@pytest.mark.parametrize("tag", TAGS)
def test_pressure_romberg(hc, g, tag):
    """The pressure integrals with scipy's rule over chomp_math.h's integrand: the values within
    1e-11 and every knot's stopping level identical -- the not-converged ones included."""
    p = _prec()
    z = numpy.ascontiguousarray(g["de_z"])
    n = z.size
    val = numpy.empty(n)
    lev = numpy.empty(n, dtype=numpy.int32)
    conv = numpy.empty(n, dtype=numpy.int32)
    hc.dc_pressure(float(g[tag + "w0"]), float(g[tag + "wa"]), _p(z), n, p["global_precision"],
                   p["cosmo_precision"], p["divmax"], _p(val), lev.ctypes.data_as(ip),
                   conv.ctypes.data_as(ip))
    assert numpy.array_equal(lev, g[tag + "de_levels"])
    numpy.testing.assert_allclose(val, g[tag + "de_pressure"], rtol=1e-11, atol=0)
    assert val[-1] == 0.0 and lev[-1] == 1          # z = 0: a zero-width interval
    # the deep knots run out of divmax, as the reference's AccuracyWarnings say
    assert numpy.all(conv[lev < p["divmax"]] == 1)
    assert not numpy.all(conv == 1)


def test_levels_of_the_default_case(g):
    """With the default precision, (w0, wa) = (-0.9, 0.2): 22 knots at divmax = 20, then
    19 19 18 18 ... 6 6 5 and 1 for the last knot."""
    lev = g["a_de_levels"]
    assert lev.size == 50 and numpy.all(lev[:22] == 20) and lev[-1] == 1
    assert list(lev[22:26]) == [19, 19, 18, 18] and list(lev[-4:-1]) == [6, 6, 5]


@pytest.mark.parametrize("tag", TAGS)
def test_e0(hc, g, tag):
    """E0(z) = Omega_L0 exp(P(ln a)) + Omega_m0 / a^3 + Omega_r0 / a^4 from the reference's knots
    through the library's not-a-knot spline."""
    ln_a = numpy.ascontiguousarray(g["de_ln_a"])
    pr = numpy.ascontiguousarray(g[tag + "de_pressure"])
    z = numpy.ascontiguousarray(g["e0_z"])
    out = numpy.empty(z.size)
    hc.dc_e0(c_dict["omega_m0"], c_dict["omega_l0"], c_dict["omega_r0"], _p(ln_a), _p(pr),
             ln_a.size, _p(z), z.size, _p(out))
    numpy.testing.assert_allclose(out, g[tag + "e0"], rtol=1e-12)


def test_reference_table_of_numbers(g):
    """The reference's numbers quoted for c_dict with (w0, wa) = (-0.9, 0.2) at z = 0.5."""
    sc = g["a_scalars"][1]       # chi, growth, omega_m, omega_l, delta_c, delta_v, ...
    assert abs(sc[0] - 1295.905) < 1e-3
    assert abs(sc[2] - 0.55068) < 1e-5 and abs(sc[3] - 0.38082) < 1e-5
    assert abs(sc[5] - 366.21) < 1e-2
    assert abs(g["a_e0"][3] - 1.83812) < 1e-5


def test_de_kw():
    """Only a batch with some w0-wa cosmology opts in; Lambda-CDM calls stay as they were."""
    from chomp_amd import _lib, cosmology
    de = dict(c_dict, w0=-0.9, wa=0.2)
    wa_only = dict(c_dict, wa=0.3)
    assert cosmology._de_kw(c_dict) == {}
    assert cosmology._de_kw(de) == {"dark_energy": True}
    assert cosmology._de_kw([c_dict, c_dict]) == {}
    assert cosmology._de_kw([c_dict, wa_only]) == {"dark_energy": True}
    assert cosmology._de_kw(_lib.Context.pack_cosmo([c_dict, de], 2)) == {"dark_energy": True}
    assert cosmology._de_kw(_lib.Context.pack_cosmo(c_dict, 3)) == {}
    arr = numpy.array([[c_dict[k] for k in ("omega_m0", "omega_b0", "omega_l0", "omega_r0",
                                            "cmb_temp", "h", "sigma_8", "n_scalar", "w0", "wa")]] * 2)
    assert cosmology._de_kw(arr) == {}
    arr[1, 8] = -1.2
    assert cosmology._de_kw(arr) == {"dark_energy": True}


class _DeContext(object):
    """The part of _lib.Context HaloGrid uses, recording what reaches epochs_set."""

    def __init__(self):
        from chomp_amd import _lib
        self.pack_cosmo = _lib.Context.pack_cosmo
        self.pack_halo = _lib.Context.pack_halo
        self.pack_hod = _lib.Context.pack_hod
        self.calls = []

    def epochs_set(self, cosmo, z, with_bao=False, **kw):
        self.calls.append((bytes(cosmo), list(z), kw))

    def stage_k(self, *a):
        pass


def test_halo_grid_packs_and_opts_in(monkeypatch):
    from chomp_amd import _lib, cosmology, grid
    monkeypatch.setattr(cosmology, "_context", lambda stream=None, device=None: _DeContext())
    cosmos = [c_dict, dict(c_dict, w0=-0.9, wa=0.2), dict(c_dict, w0=-1.2), c_dict]
    hg = grid.HaloGrid([0.5] * 4, cosmo_dict=cosmos)
    hg.setup("power_mm")
    packed, z, kw = hg.ctx.calls[-1]
    assert kw == {"dark_energy": True} and z == [0.5] * 4
    assert packed == bytes(_lib.Context.pack_cosmo(cosmos, 4))
    rows = numpy.frombuffer(packed, dtype=numpy.float64).reshape(4, 10)
    assert list(rows[:, 8]) == [-1.0, -0.9, -1.2, -1.0] and list(rows[:, 9]) == [0.0, 0.2, 0.0, 0.0]
    # an all-Lambda-CDM batch is called exactly as before the opt-in existed
    hl = grid.HaloGrid([0.5] * 2, cosmo_dict=[c_dict, c_dict])
    hl.setup("power_mm")
    assert hl.ctx.calls[-1][2] == {}
    # set_parameters with a packed array carries the opt-in along
    hl.set_parameters(cosmo=_lib.Context.pack_cosmo([c_dict, dict(c_dict, wa=0.3)], 2))
    hl.setup("power_mm")
    assert hl.ctx.calls[-1][2] == {"dark_energy": True}
