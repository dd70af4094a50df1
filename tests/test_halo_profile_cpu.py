"""CPU tests of the general-slope halo profile (halo_dict["alpha"] != -1, halo.py:491-559):

* chomp_math.h's profile mass integral, compiled for the host, against mpmath's 2F1 form;
* a NumPy restatement of _initialize_y_spline / y_general and of the knot integrals built on
  them -- on the oracle's mass tables and oracle/romberg.py -- against the reference's own
  numbers (G28), values and Romberg levels;
* the host-compiled y_general integrand against the restatement's;
* the host side of the opt-in: who accepts alpha != -1, who keeps refusing it, and that the flag
  travels with init_from_halo and copies.
"""
import copy
import ctypes
import os
import subprocess

import mpmath
import numpy
import pytest
from scipy import special
from scipy.interpolate import InterpolatedUnivariateSpline

from conftest import ROOT, load_golden
from params import c_dict_2, h_dict_2

HC = os.path.join(ROOT, "tests", "hostcheck")
dp = ctypes.POINTER(ctypes.c_double)
cd = ctypes.c_double

# (tag, redshift, alpha, c_dict_2 / h_dict_2 / Tinker instead of the defaults): G28's cases
CASES = (("a15_", 0.0, -1.5, False), ("a05_", 0.0, -0.5, False), ("alt_", 0.5, -1.2, True))
# The ln k knots the restatement's knot integrals run at: all 50.
KNOTS = tuple(range(50))


@pytest.fixture(scope="module")
def hc():
    so = os.path.join(HC, "libprofilecheck.so")
    src = os.path.join(HC, "profilecheck.cpp")
    deps = [src, os.path.join(ROOT, "chomp_amd", "csrc", "chomp_math.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(map(os.path.getmtime, deps)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    L.hc_y_general_norm.restype = cd
    L.hc_y_general_norm.argtypes = [cd, cd, cd, cd]
    L.hc_y_general_scale.restype = cd
    L.hc_y_general_scale.argtypes = [cd, cd, cd, cd]
    L.hc_y_general_integrand.argtypes = [cd, cd, cd, cd, cd, dp, ctypes.c_int, dp]
    L.hc_halo_normalization.argtypes = [cd, cd, cd, dp, ctypes.c_int, dp]
    L.hc_profile_mass_integral.argtypes = [dp, dp, ctypes.c_int, dp]
    return L


def _p(a):
    return a.ctypes.data_as(dp)


# -- the profile's mass integral ------------------------------------------------------------
ALPHAS = (-2.5, -2.0, -1.5, -1.0, -0.5, 0.0, 0.5)
CONS = (0.5, 3.0, 33.0, 1e3, 1e4)


def test_profile_mass_integral_against_mpmath(hc):
    """int_0^c x^(2 + alpha) (1 + x)^-(3 + alpha) dx = c^a / a 2F1(a, a; a + 1; -c), a = 3 + alpha
    (halo.py:893-895), to 1e-13 relative over the concentrations a mass table can reach."""
    mpmath.mp.dps = 40
    # (... and the two ends of the range the set-ups accept, (-3, 3.5])
    al, cc = [x.ravel() for x in numpy.meshgrid(ALPHAS + (-2.99, 3.5), CONS, indexing="ij")]
    got = numpy.empty(al.size)
    hc.hc_profile_mass_integral(_p(numpy.ascontiguousarray(al)), _p(numpy.ascontiguousarray(cc)),
                                al.size, _p(got))
    worst = 0.0
    for a_, c_, g in zip(al, cc, got):
        a = mpmath.mpf(3) + mpmath.mpf(float(a_))
        c = mpmath.mpf(float(c_))
        ref = c ** a / a * mpmath.hyp2f1(a, a, a + 1, -c)
        worst = max(worst, float(abs((mpmath.mpf(float(g)) - ref) / ref)))
    print("profile_mass_integral: worst relative error %.3g" % worst)
    assert worst <= 1e-13


def test_profile_mass_integral_nfw_closed_form(hc):
    c = numpy.array(CONS + (0.9, 1.0, 1.1, 7.0))
    got = numpy.empty(c.size)
    hc.hc_profile_mass_integral(_p(numpy.full(c.size, -1.0)), _p(c), c.size, _p(got))
    ref = numpy.log1p(c) - c / (1.0 + c)
    assert numpy.max(numpy.abs(got / ref - 1.0)) <= 1e-13


# -- the restatement ------------------------------------------------------------------------
def _table(z, alpha, alt, exclusion=False):
    """The oracle's epoch, mass table and halo splines of a G28 case (no knot table built)."""
    from oracle import chomp_oracle as o
    if alt:
        hd = dict(h_dict_2, alpha=alpha)
        e = o.epoch(c_dict_2, z)
        m = o.mass_table(e, hd, kind="tinker")
    else:
        hd = dict(o.default_halo_dict, alpha=alpha)
        e = o.epoch(None, z)
        m = o.mass_table(e, hd)
    t = o.halo_table(e, m, halo_dict=hd, families=(), exclusion=exclusion)
    t.alpha = alpha
    # halo.py:848-855, 880-897: the spline of ln(rho_s / rho_norm) over ln M
    con = t.c0 * (numpy.exp(m.ln_mass) / m.m_star) ** t.beta
    a = 3.0 + alpha
    rho_norm = con ** a * special.hyp2f1(a, a, a + 1.0, -con) / a
    t.ln_hn_spline = InterpolatedUnivariateSpline(
        m.ln_mass, numpy.log(t.rho_bar * t.delta_v * con * con * con / 3.0 / rho_norm))
    t.y_rows = {}
    return t


def _y_integrand(x, alpha, k, r_vir, c, norm):
    """halo.py:531-559."""
    r = x * r_vir / c
    return norm * x ** 2 * (x ** alpha / (1.0 + x) ** (3.0 + alpha)) * numpy.sinc(k * r / numpy.pi)


def _y_norm(alpha, k, r_vir, c):
    """halo.py:512-517."""
    if numpy.fabs(numpy.sinc(k * r_vir / (c * numpy.pi))) <= 1e-16:
        return 1.0 / _y_integrand(1.0 + numpy.pi / 4.0, alpha, k, r_vir, c, 1.0)
    return 1.0 / _y_integrand(1.0, alpha, k, r_vir, c, 1.0)


def _y_row(t, ln_k, alpha=None, ratios=None):
    """_initialize_y_spline at one ln k (halo.py:500-529): (y over the mass knots, levels).
    ratios: a list that receives err / (rtol |result|) of the row each integral stopped at."""
    from oracle.romberg import romberg
    alpha = t.alpha if alpha is None else alpha
    prec = t.e.prec
    k = numpy.exp(ln_k)
    y = numpy.empty_like(t.m.ln_mass)
    lev = numpy.empty(y.size, dtype=int)
    for i, lm in enumerate(t.m.ln_mass):
        mass = numpy.exp(lm)
        c = numpy.exp(t.ln_c_spline(numpy.log(mass)))
        r_vir = numpy.exp(t.ln_r_v_spline(numpy.log(mass)))
        norm = _y_norm(alpha, k, r_vir, c)
        val, lev[i] = romberg(_y_integrand, 1e-8, c, args=(alpha, k, r_vir, c, norm), vec_func=True,
                              tol=prec["global_precision"], rtol=prec["halo_precision"],
                              divmax=prec["divmax"], return_level=True)
        if ratios is not None and lev[i] > 0:
            below = romberg(_y_integrand, 1e-8, c, args=(alpha, k, r_vir, c, norm), vec_func=True,
                            tol=0.0, rtol=0.0, divmax=int(lev[i]) - 1)
            ratios.append(abs(val - below) / (prec["halo_precision"] * abs(val)))
        y[i] = (4.0 * numpy.pi * (val / norm) * (r_vir / c) ** 3 *
                numpy.exp(t.ln_hn_spline(numpy.log(mass))) / mass)
    return y, lev


def _y(t, ln_k, mass):
    """y_general (halo.py:491-498): the row's spline, 0 outside the mass table."""
    if ln_k not in t.y_rows:
        t.y_rows[ln_k] = InterpolatedUnivariateSpline(t.m.ln_mass, _y_row(t, ln_k)[0])
    lm = numpy.log(mass)
    return numpy.where(numpy.logical_and(lm >= t.m.ln_mass_min, lm <= t.m.ln_mass_max),
                       t.y_rows[ln_k](lm), 0.0)


def _h_m_integrand(ln_nu, t, ln_k, norm):                       # halo.py:922-927, 1208-1213
    from oracle import chomp_oracle as o
    nu = numpy.exp(ln_nu)
    mass = o.mass_of_nu(t.m, nu)
    return (norm * nu * o._mass_window(t, mass, ln_k) * o.f_nu(t.m, nu) * o.bias_nu(t.m, nu) *
            _y(t, ln_k, mass))


def _pp_mm_integrand(ln_nu, t, ln_k, norm):                     # :989-994
    from oracle import chomp_oracle as o
    nu = numpy.exp(ln_nu)
    mass = o.mass_of_nu(t.m, nu)
    y = _y(t, ln_k, mass)
    return norm * nu * o.f_nu(t.m, nu) * mass * y * y


def _h_g_integrand(ln_nu, t, ln_k, norm):                       # :964-969
    from oracle import chomp_oracle as o
    nu = numpy.exp(ln_nu)
    mass = o.mass_of_nu(t.m, nu)
    return (norm * nu * o._mass_window(t, mass, ln_k) * o.f_nu(t.m, nu) * o.bias_nu(t.m, nu) *
            _y(t, ln_k, mass) * o.zheng_first(t.hod, mass) / mass)


def _pp_gm_integrand(ln_nu, t, ln_k, norm):                     # :1078-1086
    from oracle import chomp_oracle as o
    nu = numpy.exp(ln_nu)
    mass = o.mass_of_nu(t.m, nu)
    y = _y(t, ln_k, mass)
    n_exp = o.zheng_first(t.hod, mass)
    return numpy.where(n_exp < 1, norm * nu * o.f_nu(t.m, nu) * n_exp * y,
                       norm * nu * o.f_nu(t.m, nu) * n_exp * y * y)


def _pp_gg_integrand(ln_nu, t, ln_k, norm):                     # :1032-1041
    from oracle import chomp_oracle as o
    nu = numpy.exp(ln_nu)
    mass = o.mass_of_nu(t.m, nu)
    y = _y(t, ln_k, mass)
    n_pair = o.zheng_second(t.hod, mass)
    return numpy.where(n_pair < 1, norm * nu * o.f_nu(t.m, nu) * n_pair * y / mass,
                       norm * nu * o.f_nu(t.m, nu) * n_pair * y * y / mass)


def _i_1_2_integrand(ln_nu, t, ln_k, norm):                     # :1194-1199
    from oracle import chomp_oracle as o
    nu = numpy.exp(ln_nu)
    mass = o.mass_of_nu(t.m, nu)
    y = _y(t, ln_k, mass)
    return nu * o.f_nu(t.m, nu) * o.bias_nu(t.m, nu) * y * y * mass * norm


def _knot_table(t, name, knots=KNOTS):
    """(values, levels) of one of the reference's knot tables at the ln k knots `knots`."""
    from oracle import chomp_oracle as o
    hod, m = t.hod, t.m
    lo_first = numpy.log(o._nu_lo(t, hod.first_moment_zero))
    lo_second = numpy.log(o._nu_lo(t, hod.second_moment_zero))
    integrand, lo, safe, scale = {
        "h_m": (_h_m_integrand, numpy.log(m.nu_min), None, 1.0),
        "pp_mm": (_pp_mm_integrand, numpy.log(m.nu_min), None, 1.0 / t.rho_bar),
        "i_1_2": (_i_1_2_integrand, numpy.log(m.nu_min), None, 1.0 / t.rho_bar),
        "h_g": (_h_g_integrand, lo_first, hod.safe_norm, 1.0 / t.n_bar_over_rho_bar),
        "pp_gm": (_pp_gm_integrand, lo_first, hod.safe_norm, 1.0 / t.n_bar),
        "pp_gg": (_pp_gg_integrand, lo_second, hod.safe_norm, t.rho_bar / (t.n_bar * t.n_bar)),
    }[name]
    sub = copy.copy(t)
    sub.ln_k = t.ln_k[list(knots)]
    sub.levels = {}
    val = o._knots(sub, integrand, lo, safe) * scale
    return val, numpy.array(sub.levels[integrand.__name__])


@pytest.fixture(scope="module")
def tables():
    return {tag: _table(z, alpha, alt) for tag, z, alpha, alt in CASES}


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_restatement_reproduces_y_table(tables, tag):
    g = load_golden("g28_halo_profile")
    t = tables[tag]
    assert numpy.max(numpy.abs(t.m.ln_mass - g[tag + "ln_mass"])) < 1e-10
    for ik in range(t.ln_k.size):
        y, lev = _y_row(t, t.ln_k[ik])
        assert numpy.array_equal(lev, g[tag + "y_level"][ik]), ik
        assert numpy.max(numpy.abs(y - g[tag + "y"][ik])) <= 1e-10, ik      # (y -> 1: scale 1)


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_restatement_reproduces_profile_lookups(tables, tag):
    g = load_golden("g28_halo_profile")
    t = tables[tag]
    lm = numpy.log(g[tag + "mass"])
    assert numpy.max(numpy.abs(numpy.exp(t.ln_c_spline(lm)) / g[tag + "concentration"] - 1)) < 1e-10
    assert numpy.max(numpy.abs(numpy.exp(t.ln_r_v_spline(lm)) / g[tag + "virial_radius"] - 1)) < 1e-10
    assert numpy.max(numpy.abs(numpy.exp(t.ln_hn_spline(lm)) / g[tag + "halo_normalization"] - 1)) < 1e-10
    for i, ln_k in enumerate(g["ln_k_off"]):
        assert numpy.max(numpy.abs(_y(t, float(ln_k), g[tag + "mass_y"]) - g[tag + "y_off"][i])) <= 1e-10


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
@pytest.mark.parametrize("name", ["h_m", "pp_mm", "h_g", "pp_gm", "pp_gg"])
def test_restatement_reproduces_knot_tables(tables, tag, name):
    g = load_golden("g28_halo_profile")
    val, lev = _knot_table(tables[tag], name)
    ref = g[tag + name]
    assert numpy.array_equal(lev, g[tag + name + "_level"][list(KNOTS)])
    assert numpy.max(numpy.abs(val - ref[list(KNOTS)])) <= 1e-10 * numpy.max(numpy.abs(ref))


def test_restatement_reproduces_ssc_and_exclusion(tables):
    g = load_golden("g28_halo_profile")
    val, lev = _knot_table(tables["a15_"], "i_1_2")
    ref = g["a15_i_1_2"]
    assert numpy.array_equal(lev, g["a15_i_1_2_level"][list(KNOTS)])
    assert numpy.max(numpy.abs(val - ref[list(KNOTS)])) <= 1e-10 * numpy.max(numpy.abs(ref))
    tx = _table(0.0, -1.5, False, exclusion=True)
    val, lev = _knot_table(tx, "h_m")
    ref = g["a15_excl_h_m"]
    assert numpy.array_equal(lev, g["a15_excl_h_m_level"][list(KNOTS)])
    assert numpy.max(numpy.abs(val - ref[list(KNOTS)])) <= 1e-10 * numpy.max(numpy.abs(ref))


def test_restatement_y_general_of_an_nfw_halo():
    """y_general called with alpha = -1 on a default halo: the Romberg value beside the closed
    form (G28 keeps both: their difference is the size of the Romberg truncation)."""
    g = load_golden("g28_halo_profile")
    t = _table(0.0, -1.0, False)
    for i, ln_k in enumerate(g["nfw_ln_k"]):
        y = _y(t, float(ln_k), g["nfw_mass"])
        assert numpy.max(numpy.abs(y - g["nfw_y_general"][i])) <= 1e-10


def test_host_build_of_y_general_integrand(hc, tables):
    """chomp_math.h's integrand, normalisation rule and table factor, compiled for the host,
    against the restatement's at 200 nodes of [1e-8, c]: within 4 ulp."""
    t = tables["a15_"]
    for im, ik in ((5, 10), (25, 30), (44, 49)):
        lm, ln_k = t.m.ln_mass[im], t.ln_k[ik]
        k = numpy.exp(ln_k)
        c = float(numpy.exp(t.ln_c_spline(lm)))
        r_vir = float(numpy.exp(t.ln_r_v_spline(lm)))
        norm = _y_norm(t.alpha, k, r_vir, c)
        got_norm = hc.hc_y_general_norm(t.alpha, k, r_vir, c)
        assert abs(got_norm - norm) <= 4 * numpy.spacing(abs(norm))
        x = numpy.linspace(1e-8, c, 200)
        ref = _y_integrand(x, t.alpha, k, r_vir, c, norm)
        got = numpy.empty(x.size)
        hc.hc_y_general_integrand(t.alpha, k, r_vir, c, norm, _p(x), x.size, _p(got))
        ulp = numpy.abs(got - ref) / numpy.spacing(numpy.abs(ref))
        print("y_general integrand (%d, %d): worst %.1f ulp" % (im, ik, ulp.max()))
        assert ulp.max() <= 4.0
        mass = numpy.exp(lm)
        hn = numpy.empty(1)
        hc.hc_halo_normalization(t.rho_bar, t.delta_v, t.alpha, _p(numpy.array([c])), 1, _p(hn))
        assert abs(hn[0] / numpy.exp(t.ln_hn_spline(lm)) - 1.0) < 1e-12
        scale = hc.hc_y_general_scale(r_vir, c, hn[0], mass)
        assert abs(scale / (4.0 * numpy.pi * (r_vir / c) ** 3 * hn[0] / mass) - 1.0) < 1e-14


# -- host logic -----------------------------------------------------------------------------
GENERAL = dict(stq=0.3, st_little_a=0.707, c0=9.0, beta=-0.13, alpha=-1.5, delta_v=-1.0)


def test_scope_errors_without_the_opt_in():
    from chomp_amd import _lib, halo
    for cls in (halo.Halo, halo.HaloExclusion, halo.HaloFit, halo.HaloSuperSampleCovariance):
        with pytest.raises(_lib.ChompScopeError):
            cls(0.0, halo_dict=GENERAL)
        with pytest.raises(_lib.ChompScopeError):
            cls(0.0, halo_dict=GENERAL, general_profile=False)


def test_opt_in_accepts_a_general_profile():
    from chomp_amd import halo
    # (HaloFit's constructor asks the device for omega_m: tests/test_gpu_halo_profile.py)
    for cls in (halo.Halo, halo.HaloExclusion, halo.HaloSuperSampleCovariance):
        h = cls(0.0, halo_dict=GENERAL, general_profile=True)
        assert h.alpha == -1.5 and h._general_profile is True
        assert h._profile()["alpha"] == -1.5
        for c in (copy.copy(h), copy.deepcopy(h)):       # (SimulationDesign's kind of copy)
            assert c._general_profile is True and c._profile()["alpha"] == -1.5
    # an NFW dictionary with the opt-in is an NFW halo
    h = halo.Halo(0.0, general_profile=True)
    assert h.alpha == -1.0 and h._general_profile is True
    for bad in (-3.0, 3.6):
        with pytest.raises(ValueError):
            halo.Halo(0.0, halo_dict=dict(GENERAL, alpha=bad), general_profile=True)


def test_set_halo_accepts_a_general_dictionary():
    """halo.py:220-235: only the mass function sees the dictionary, and the profile is NFW from
    there on."""
    from chomp_amd import halo
    h = halo.Halo(0.0, halo_dict=GENERAL, general_profile=True)
    h.set_halo(dict(GENERAL, alpha=-1.2, stq=0.31))
    assert h.alpha == -1.0 and h._profile()["alpha"] == -1.0
    assert h.mass.halo_dict["stq"] == 0.31


def test_init_from_halo_carries_the_flag():
    from chomp_amd import halo
    src = halo.Halo(0.0, halo_dict=GENERAL, general_profile=True)
    s = halo.HaloSuperSampleCovariance.init_from_halo(src, delta_b=0.01)
    assert s._general_profile is True and s.alpha == -1.5
    assert halo.HaloSuperSampleCovariance.init_from_halo(halo.Halo(0.0))._general_profile is False


def test_simulation_design_keeps_the_loop_for_a_general_profile():
    from chomp_amd import halo, simulation_design
    k = numpy.logspace(-2, 1, 4)
    params = {"sigma_8": [0.8, 0.7, 0.9]}
    nfw = simulation_design.SimulationDesign(halo.Halo(0.0), "power_mm", params, 2, k)
    gen = simulation_design.SimulationDesign(
        halo.Halo(0.0, halo_dict=GENERAL, general_profile=True), "power_mm", params, 2, k)
    assert nfw._batched() and not gen._batched()


def test_trispectrum_classes_still_refuse():
    from chomp_amd import _lib, halo_trispectrum, mass_function
    with pytest.raises(_lib.ChompScopeError):
        halo_trispectrum.HaloTrispectrumOneHalo(0.0, halo_dict=GENERAL)
    with pytest.raises(TypeError):
        halo_trispectrum.HaloTrispectrumOneHalo(0.0, halo_dict=GENERAL, general_profile=True)
    m2 = mass_function.MassFunctionSecondOrder(0.0)
    with pytest.raises(_lib.ChompScopeError):
        halo_trispectrum.HaloTrispectrum(0.0, mass_func_second=m2, halo_dict=GENERAL)
