"""HaloSuperSampleCovariance (halo.py:1089-1199) without a device: the reference's fixture
G19 against an oracle composition, and the host side of the mirror class."""
import numpy
import pytest

from conftest import load_golden, rel_err
from params import c_dict_2, h_dict_2

DELTA_B = 0.01


def i_1_2_integrand(ln_nu, t, ln_k, norm):
    """halo.py:1194-1199 from the oracle's pieces."""
    from oracle import chomp_oracle as o
    nu = numpy.exp(ln_nu)
    mass = o.mass_of_nu(t.m, nu)
    y = o.y_nfw(t, ln_k, mass)
    return nu * o.f_nu(t.m, nu) * o.bias_nu(t.m, nu) * y * y * mass * norm


def ssc_table(t):
    """halo.py:1176-1192 on an oracle halo table: the I_1^2 knots, their Romberg levels and
    the not-a-knot spline."""
    from scipy.interpolate import InterpolatedUnivariateSpline
    from oracle import chomp_oracle as o
    t.i_1_2 = o._knots(t, i_1_2_integrand, numpy.log(t.m.nu_min), None) / t.rho_bar
    t.i_1_2_levels = numpy.array(t.levels["i_1_2_integrand"], dtype=float)
    t.i_1_2_spline = InterpolatedUnivariateSpline(t.ln_k, t.i_1_2)
    return t


def ssc_response(t, k):
    """halo.py:1136-1156."""
    from oracle import chomp_oracle as o
    k = numpy.asarray(k, dtype=float)
    with numpy.errstate(all="ignore"):
        h = o._ranged(t, t.h_m_spline, k)
        num = 68.0 / 21.0 * h * h * o.linear_power(t.e, k) + o._ranged(t, t.i_1_2_spline, k)
        return numpy.where((k >= t.k_min) & (k <= t.k_max), num / o.halo_power(t, "mm", k), 0.0)


def ssc_mm(t, k, delta_b):
    """halo.py:1158-1169."""
    from oracle import chomp_oracle as o
    return o.halo_power(t, "mm", k) * (1.0 + ssc_response(t, k) * delta_b)


def oracle_case(tag):
    from oracle import chomp_oracle as o
    if tag == "alt_":
        e = o.epoch(c_dict_2, 0.3)
        t = o.halo_table(e, o.mass_table(e, h_dict_2, kind="tinker"), halo_dict=h_dict_2)
    else:
        z = {"z000_": 0.0, "z050_": 0.5, "from_": 0.2}[tag]
        e = o.epoch(None, z)
        t = o.halo_table(e, o.mass_table(e))
    return ssc_table(t)


@pytest.mark.parametrize("tag", ["z000_", "z050_", "alt_", "from_"])
def test_g19_against_oracle_composition(tag):
    g = load_golden("g19_halo_ssc")
    t = oracle_case(tag)
    assert numpy.array_equal(t.ln_k, g[tag + "ln_k"])
    assert rel_err(t.i_1_2, g[tag + "i_1_2"]) < 1e-12
    # the reference stops where pp_mm does: levels 6..10, inside the node tables
    assert t.i_1_2_levels.min() >= 5 and t.i_1_2_levels.max() <= 10
    k = g["k"]
    ref = g[tag + "resp"]
    got = ssc_response(t, k)
    inside = (k >= t.k_min) & (k <= t.k_max)
    assert numpy.all(ref[~inside] == 0.0) and numpy.all(got[~inside] == 0.0)
    assert rel_err(got[inside], ref[inside]) < 1e-10
    mm = ssc_mm(t, k, float(g["delta_b"]))
    nz = g[tag + "mm_ssc"] != 0.0
    assert numpy.array_equal(nz, mm != 0.0)
    assert rel_err(mm[nz], g[tag + "mm_ssc"][nz]) < 1e-10
    # below k_min it is power_mm itself, above k_max 0 (halo.py:1158-1169)
    assert numpy.array_equal(g[tag + "mm_ssc"][k < t.k_min], g[tag + "mm"][k < t.k_min])


def test_g19_fixture_quirks():
    g = load_golden("g19_halo_ssc")
    k = g["k"]
    # init_from_halo drops extrapolate: power_mm is 0 above k_max where the source extrapolates
    assert float(g["from_extrapolate"]) == 0.0 and float(g["from_k150_mm"][0]) == 0.0
    assert numpy.all(g["from_src_mm"][k > 100.0] > 0.0)
    # the stale sequence: after set_redshift(0.5) the I_1^2 knots are still those of z = 0
    assert numpy.array_equal(g["stale_i_1_2"], g["z000_i_1_2"])
    assert not numpy.allclose(g["stale_resp"], g["z050_resp"], rtol=1e-6)


def test_mirror_surface_without_device():
    from chomp_amd import _lib, halo
    h = halo.HaloSuperSampleCovariance(0.5, extrapolate=True, delta_b=0.02)
    assert h._extrapolate is False and h.get_extrapolation() is False
    assert h._delta_b == 0.02 and h._initialized_i_1_2 is False
    assert h.get_redshift() == 0.5
    for name in ("init_from_halo", "dln_power_ddelta_b", "power_mm_ssc", "_i_1_2",
                 "power_mm", "set_redshift", "set_cosmology", "set_halo", "set_hod"):
        assert callable(getattr(h, name))
    assert h._power_code(_lib.P_MM_SSC) == _lib.P_MM_SSC
    assert _lib.FAM_SSC == _lib.FAM_MM | _lib.T_I_1_2
    assert _lib.TAB["i_1_2"] == 9 and _lib.TAB["levels_i_1_2"] == 10
    assert any("i_1_2" in s for s in _lib.describe_status(_lib.ST_HALO_DIVMAX["i_1_2"]))
    src = halo.Halo(0.0, extrapolate=True)
    with pytest.raises(_lib.ChompError):      # no CPU fallback: a device context is needed
        halo.HaloSuperSampleCovariance(0.0).power_mm_ssc(numpy.array([1.0]))
    assert src.get_extrapolation() is True


def test_halo_grid_accepts_ssc_spectra():
    from chomp_amd import grid, _lib
    assert grid._WHICH["dln_power_ddelta_b"] == (_lib.P_SSC_RESPONSE, _lib.FAM_SSC)
    assert grid._WHICH["power_mm_ssc"] == (_lib.P_MM_SSC, _lib.FAM_SSC)
