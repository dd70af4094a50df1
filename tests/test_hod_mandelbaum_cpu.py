"""CPU tests of hod.HODMandelbaum (hod.py:232-299) and of the host side of its device path: the
moments against the reference's (G21), the reference's quirks, the tagged chomp_hod_model and
how HaloGrid / SimulationDesign pack a batch that mixes the two occupation models."""
import ctypes
import os
import subprocess

import numpy
import pytest

from conftest import ROOT, load_golden
from params import hod_dict, hod_dict_2

CASES = ("z000_", "z050_", "alt_", "low_")
HC = os.path.join(ROOT, "tests", "hostcheck")
dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def hc():
    so = os.path.join(HC, "libhodcheck.so")
    src = os.path.join(HC, "hodcheck.cpp")
    deps = [src, os.path.join(ROOT, "chomp_amd", "csrc", "chomp_math.h"),
            os.path.join(ROOT, "include", "chomp_mi355x.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, deps)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(dp)


@pytest.mark.parametrize("tag", CASES)
def test_moments_match_reference(tag):
    from chomp_amd import hod
    g = load_golden("g21_hod_mandelbaum")
    h = hod.HODMandelbaum({"log_M_0": float(g[tag + "log_M_0"]), "w": float(g[tag + "w"])})
    m = g[tag + "mass"]
    assert h.log_M_min == g[tag + "log_M_min"]
    for name, fn in (("first", h.first_moment), ("second", h.second_moment),
                     ("central", h.central_first_moment),
                     ("satellite", h.satellite_first_moment)):
        assert numpy.array_equal(fn(m, z=0.3), g[tag + name]), name
    assert numpy.array_equal(h.nth_moment(m, 2), g[tag + "second"])


@pytest.mark.parametrize("tag", CASES)
def test_host_build_of_device_moments(hc, tag):
    """chomp_math.h's Mandelbaum moments, compiled for the host, against the reference's
    (the grid includes both thresholds and their neighbouring doubles: the tie rule)."""
    g = load_golden("g21_hod_mandelbaum")
    m = numpy.ascontiguousarray(g[tag + "mass"])
    out = numpy.empty((m.size, 4))
    hc.hc_mandelbaum_moments(ctypes.c_double(float(g[tag + "log_M_0"])),
                             ctypes.c_double(float(g[tag + "w"])), _p(m), m.size, _p(out))
    for i, name in enumerate(("first", "second", "central", "satellite")):
        assert numpy.array_equal(out[:, i], g[tag + name]), name


def test_constants_bit_for_bit(hc):
    from chomp_amd import hod
    lm0 = numpy.concatenate([[12.14, 12.8, 6.0, 11.0, 13.5], numpy.linspace(9.0, 15.0, 601)])
    lmm, mmin = numpy.empty_like(lm0), numpy.empty_like(lm0)
    hc.hc_mandelbaum_constants(_p(lm0), lm0.size, _p(lmm), _p(mmin))
    ref_lmm = numpy.log10(3.0) + lm0
    assert numpy.array_equal(lmm, ref_lmm)
    assert numpy.array_equal(mmin, numpy.array([10 ** x for x in ref_lmm]))
    assert numpy.log10(3.0) == load_golden("g21_hod_mandelbaum")["log10_3"]
    for x in lm0[:5]:
        h = hod.HODMandelbaum({"log_M_0": float(x), "w": 1.0})
        assert h.log_M_min == numpy.log10(3.0) + x


def test_struct_layout_against_header(hc):
    from chomp_amd import _lib
    lay = (ctypes.c_size_t * 8)()
    hc.hc_hod_model_layout(lay)
    M = _lib.HodModel
    assert ctypes.sizeof(M) == lay[0] == 64
    assert [M.kind.offset, M.reserved.offset, M.zheng.offset, M.log_M_0.offset,
            M.w.offset] == list(lay[1:6])
    assert (_lib.HOD_ZHENG, _lib.HOD_MANDELBAUM) == (lay[6], lay[7])
    assert ctypes.sizeof(_lib.HodPar) == 40


def test_without_dictionary():
    """hod.py:248-259: no HOD.__init__ without a dictionary; a Halo on it fails at
    construction (halo.py:91); set_hod re-initialises the object."""
    from chomp_amd import halo, hod
    h = hod.HODMandelbaum()
    assert (h.log_M_0, h.w) == (12.14, 1.0)
    assert h.log_M_min == numpy.log10(3.0) + 12.14
    for name in ("hod_dict", "first_moment_zero", "second_moment_zero", "_safe_norm"):
        assert not hasattr(h, name), name
    with pytest.raises(AttributeError):
        halo.Halo(0.0, input_hod=h)
    h.set_hod({"log_M_0": 12.5, "w": 0.7})
    assert (h.log_M_0, h.w, h.get_hod()) == (12.5, 0.7, {"log_M_0": 12.5, "w": 0.7})
    assert h.log_M_min == numpy.log10(3.0) + 12.5
    assert (h.first_moment_zero, h.second_moment_zero, h._safe_norm) == (-1, -1, -1)
    m = numpy.logspace(10, 15, 11)
    assert numpy.array_equal(h.second_moment(m), (2 + h.satellite_first_moment(m)) *
                             h.satellite_first_moment(m))


def test_pack_hod_zheng_unchanged():
    from chomp_amd import _lib, hod
    for d in (hod_dict, hod_dict_2, None):
        z = hod.HODZheng(d)
        a = _lib.Context.pack_hod([z, z], 2)
        ref = _lib.hod_struct(z)
        for rec in a:
            assert rec.kind == _lib.HOD_ZHENG and rec.reserved == 0
            assert bytes(rec.zheng) == bytes(ref)
            assert (rec.log_M_0, rec.w) == (0.0, 0.0)
    m = hod.HODMandelbaum({"log_M_0": 12.8, "w": 0.5})
    rec = _lib.Context.pack_hod(m, 1)[0]
    assert (rec.kind, rec.log_M_0, rec.w) == (_lib.HOD_MANDELBAUM, 12.8, 0.5)
    with pytest.raises(AttributeError):           # any other HOD class: as before
        _lib.Context.pack_hod(hod.HOD({}), 1)


class _PackContext(object):
    """The part of _lib.Context HaloGrid packs with (the real static packers), recording what
    reaches stage_k."""
    pack_cosmo = staticmethod(lambda c, n: [c] * n if isinstance(c, dict) else list(c))
    pack_halo = pack_cosmo

    def __init__(self):
        from chomp_amd import _lib
        self.pack_hod = _lib.Context.pack_hod
        self.staged = []

    def epochs_set(self, cosmo, z, with_bao=False):
        pass

    def stage_k(self, mass_halo, mf_kind, profile, hods, tables):
        self.staged.append(hods)


def _kinds(arr):
    return [(r.kind, r.zheng.log_M_min, r.log_M_0, r.w) for r in arr]


def test_halo_grid_mixed_models(monkeypatch):
    from chomp_amd import _lib, cosmology, grid, hod
    monkeypatch.setattr(cosmology, "_context", lambda stream=None, device=None: _PackContext())
    Z, M = hod.HODZheng(hod_dict), hod.HODMandelbaum({"log_M_0": 12.14, "w": 1.0})
    hg = grid.HaloGrid([0.0, 0.5, 1.0, 1.5], hod_dict=[Z, M, Z, M])
    hg.setup("power_gm")
    got = _kinds(hg.ctx.staged[-1])
    assert [g[0] for g in got] == [_lib.HOD_ZHENG, _lib.HOD_MANDELBAUM] * 2
    assert got[0] == got[2] and got[1] == got[3]
    assert got[1][2:] == (12.14, 1.0)
    # dictionaries still mean HODZheng, exactly as before
    hd = grid.HaloGrid([0.0, 0.5], hod_dict=[hod_dict, hod_dict_2])
    hd.setup("power_gm")
    ref = _lib.Context.pack_hod([hod.HODZheng(hod_dict), hod.HODZheng(hod_dict_2)], 2)
    assert bytes(hd.ctx.staged[-1]) == bytes(ref)
    # set_parameters: objects, a single object, dicts
    hg.set_parameters(hod=[M, M, Z, Z])
    hg.setup("power_gm")
    assert [g[0] for g in _kinds(hg.ctx.staged[-1])] == [1, 1, 0, 0]
    hg.set_parameters(hod=M)
    hg.setup("power_gm")
    assert [g[0] for g in _kinds(hg.ctx.staged[-1])] == [1] * 4
    hg.set_parameters(hod=hod_dict)
    hg.setup("power_gm")
    assert bytes(hg.ctx.staged[-1]) == bytes(_lib.Context.pack_hod(hod.HODZheng(hod_dict), 4))


def test_simulation_design_packs_the_halos_model():
    from chomp_amd import hod, simulation_design as sd
    M = hod.HODMandelbaum({"log_M_0": 12.14, "w": 1.0})
    p = sd._point_hod(M, {"log_M_0": 12.5, "w": 0.8})
    assert type(p) is hod.HODMandelbaum and (p.log_M_0, p.w) == (12.5, 0.8)
    assert sd._point_hod(M, None) is M
    Z = hod.HODZheng(hod_dict)
    assert sd._point_hod(Z, dict(hod_dict_2)) == dict(hod_dict_2)
    assert sd._point_hod(Z, None) == dict(hod_dict)
