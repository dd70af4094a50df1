"""MassFunctionSecondOrder on the MI355X (pytest -m gpu): bias_2_norm and its Romberg stopping
level, the sigma knots, bias_2_nu (inside and outside [nu_min, nu_max], where the sigma(nu) spline
extrapolates) and bias_2_mass against the reference's own numbers (G23,
tests/golden/make_golden_pt.py); the re-normalisation by the setters; the status bit; and a Halo
built on the subclass, whose tables, levels and spectra match the reference's Halo on it."""
import warnings

import numpy
import pytest

from conftest import load_golden, rel_err
from params import h_dict_2

pytestmark = pytest.mark.gpu

CASES = (("hdef_", None, 0.0), ("hdef_", None, 0.5), ("h2_", h_dict_2, 0.0), ("h2_", h_dict_2, 0.5))
TABLES = ("h_m", "pp_mm", "h_g", "pp_gm", "pp_gg")


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from chomp_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def g():
    return load_golden("g23_perturbation")


def _zt(tag, z):
    return "%sz%03d_" % (tag, int(round(100 * z)))


def _abs_err(a, b):
    a, b = numpy.asarray(a, dtype=float), numpy.asarray(b, dtype=float)
    return float(numpy.max(numpy.abs(a - b)) / numpy.max(numpy.abs(b)))


@pytest.mark.parametrize("tag,hd,z", CASES)
def test_second_order_against_reference(lib, g, tag, hd, z):
    from chomp_amd import cosmology, mass_function
    zt = _zt(tag, z)
    mf = mass_function.MassFunctionSecondOrder(z, cosmology.SingleEpoch(z), hd)
    assert abs(mf.bias_2_norm / float(g[zt + "bias_2_norm"]) - 1) < 1e-8
    assert mf._bias_2_level == int(g[zt + "norm_levels"][2])
    assert abs(mf.f_norm / float(g[zt + "f_norm"]) - 1) < 1e-8
    assert abs(mf.bias_norm / float(g[zt + "bias_norm"]) - 1) < 1e-8
    assert rel_err(mf._sigma_array, g[zt + "sigma_array"]) < 1e-7
    assert rel_err(mf._nu_array, g[zt + "nu_array"]) < 1e-7
    nu = g[zt + "probe_nu"]
    assert rel_err(mf._sigma_spline(nu), g[zt + "sigma_spline"]) < 1e-7
    assert _abs_err(mf.bias_2_nu(nu), g[zt + "bias_2_nu"]) < 1e-7
    assert _abs_err(mf.bias_2_mass(g["b2_masses"]), g[zt + "bias_2_mass"]) < 1e-7
    assert not mf._dev().status(0)[0] & lib.ST_B2_DIVMAX


def test_setters_renormalise(lib, g):
    from chomp_amd import cosmology, defaults, mass_function
    mf = mass_function.MassFunctionSecondOrder(0.0, cosmology.SingleEpoch(0.0))
    first = mf.bias_2_norm
    assert abs(first / float(g["hdef_z000_bias_2_norm"]) - 1) < 1e-8
    mf.set_halo(h_dict_2)
    assert abs(mf.bias_2_norm / float(g["h2_z000_bias_2_norm"]) - 1) < 1e-8
    mf.set_halo(defaults.default_halo_dict)
    assert mf.bias_2_norm == first
    mf.set_cosmology_object(cosmology.SingleEpoch(0.5))
    assert abs(mf.bias_2_norm / float(g["hdef_z050_bias_2_norm"]) - 1) < 1e-8


def test_plain_mass_function_is_unchanged(lib):
    """A Sheth-Tormen object gives the same nu table, f_norm and bias_norm bits, and has no b2."""
    from chomp_amd import cosmology, mass_function
    a = mass_function.MassFunction(0.5, cosmology.SingleEpoch(0.5))
    b = mass_function.MassFunctionSecondOrder(0.5, cosmology.SingleEpoch(0.5))
    assert numpy.array_equal(a._nu_array, b._nu_array)
    assert a.f_norm == b.f_norm and a.bias_norm == b.bias_norm
    nu = numpy.geomspace(0.2, 40.0, 9)
    assert numpy.array_equal(a.bias_nu(nu), b.bias_nu(nu))
    with pytest.raises(lib.ChompError):
        a._dev().second_order(0)


def test_divmax_status_bit(lib):
    from chomp_amd import cosmology, defaults, mass_function
    saved = defaults.default_precision["divmax"]
    defaults.default_precision["divmax"] = 6
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            mf = mass_function.MassFunctionSecondOrder(0.0, cosmology.SingleEpoch(0.0))
            mf.bias_2_norm
        assert mf._dev().status(0)[0] & lib.ST_B2_DIVMAX
        assert any(issubclass(x.category, lib.ChompAccuracyWarning) for x in w)
    finally:
        defaults.default_precision["divmax"] = saved


@pytest.mark.parametrize("z", (0.0, 0.5))
def test_halo_on_second_order(lib, g, z):
    from chomp_amd import cosmology, halo, mass_function
    zt = "halo_z%03d_" % int(round(100 * z))
    mf = mass_function.MassFunctionSecondOrder(z, cosmology.SingleEpoch(z))
    h = halo.Halo(z, None, cosmology.SingleEpoch(z), mf)
    k = g["k"]
    assert rel_err(h.power_mm(k), g[zt + "power_mm"]) < 1e-4
    assert rel_err(h.power_gm(k), g[zt + "power_gm"]) < 1e-4
    assert rel_err(h.power_gg(k), g[zt + "power_gg"]) < 1e-4
    ctx = h._sync(0)
    assert rel_err(ctx.table("nu"), g[zt + "nu_array"]) < 1e-12
    for name in TABLES:
        assert rel_err(ctx.table(name), g[zt + name]) < 1e-8, name
    lev = ctx.table("levels").reshape(5, -1)
    for row, name in enumerate(TABLES):
        ref = g[zt + "levels_" + name + "_integrand"]
        assert numpy.array_equal(lev[row], ref), (name, lev[row], ref)
    # the same set-up as on a plain MassFunction, bit for bit
    h0 = halo.Halo(z, None, cosmology.SingleEpoch(z), mass_function.MassFunction(z))
    assert numpy.array_equal(h.power_mm(k), h0.power_mm(k))
