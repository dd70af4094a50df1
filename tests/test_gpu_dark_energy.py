"""w0-wa dark energy on the MI355X (pytest -m gpu): the pressure tables and their Romberg
stopping levels, E0, the SingleEpoch scalars, the Halo knot tables with their levels, P(k), HaloFit,
the MultiEpoch tables, w(theta) and C_l against the reference's own numbers (G22,
tests/golden/make_golden_de.py); the status bit; batches that mix Lambda-CDM and w0-wa
cosmologies; and the entry points that still refuse w0 / wa without the opt-in."""
import warnings

import numpy
import pytest

from conftest import load_golden, rel_err
from params import c_dict

pytestmark = pytest.mark.gpu

RTOL_P = 1e-4
RTOL_KNOT = 1e-8
RTOL_PRESSURE = 1e-11
TAGS = {"a_": (-0.9, 0.2), "b_": (-1.0, 0.3), "c_": (-1.2, 0.0)}
HALOS = (("a_", 0.0), ("a_", 0.5), ("a_", 1.0), ("b_", 0.5), ("c_", 0.5))
TABLES = ("h_m", "pp_mm", "h_g", "pp_gm", "pp_gg")
SCALARS = ("chi", "growth", "omega_m", "omega_l", "delta_c", "delta_v", "rho_crit", "rho_bar",
           "sigma_norm")


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from chomp_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def g():
    return load_golden("g22_dark_energy")


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():           # (the deep pressure knots: ChompAccuracyWarning)
        warnings.simplefilter("ignore")
        yield


def _cosmo(tag):
    w0, wa = TAGS[tag]
    return dict(c_dict, w0=w0, wa=wa)


@pytest.mark.parametrize("tag", list(TAGS))
def test_pressure_table(lib, g, tag):
    from chomp_amd import cosmology
    e = cosmology.SingleEpoch(0.0, _cosmo(tag))
    t = e._dev().de_table("epoch", 0)
    numpy.testing.assert_array_max_ulp(t["ln_a"], g["de_ln_a"], maxulp=1)
    assert numpy.array_equal(t["levels"], g[tag + "de_levels"])
    ref = g[tag + "de_pressure"]
    assert rel_err(t["pressure"][:-1], ref[:-1]) < RTOL_PRESSURE and t["pressure"][-1] == 0.0
    assert numpy.array_equal(e._de_pressure_array, t["pressure"])
    assert numpy.array_equal(t["converged"], t["levels"] < 20) or not t["converged"].all()
    assert not t["converged"][0] and t["converged"][-1]
    assert rel_err(e.E0(g["e0_z"]), g[tag + "e0"]) < 1e-12


@pytest.mark.parametrize("tag", list(TAGS))
def test_single_epoch_scalars(lib, g, tag):
    from chomp_amd import cosmology
    for i, z in enumerate(g["redshifts"]):
        e = cosmology.SingleEpoch(float(z), _cosmo(tag))
        got = numpy.array([e._chi, e._growth, e.omega_m(), e.omega_l(), e.delta_c(), e.delta_v(),
                           e.rho_crit(), e.rho_bar(), e._sigma_norm])
        ref = g[tag + "scalars"][i]
        for name, a, b in zip(SCALARS, got, ref):
            if b == 0.0:
                assert a == 0.0, (z, name)
            else:
                assert abs(a / b - 1) < 1e-9, (z, name, a, b)


def test_status_bit(lib):
    from chomp_amd import _lib, cosmology
    e = cosmology.SingleEpoch(0.5, _cosmo("a_"))
    ctx = e._dev()
    assert int(ctx.status(0, 1)[0]) & _lib.ST_DE_DIVMAX
    with pytest.warns(_lib.ChompAccuracyWarning, match="dark-energy"):
        with warnings.catch_warnings():
            warnings.simplefilter("always")
            ctx.warn_status(0, 1)
    lcdm = cosmology.SingleEpoch(0.5, c_dict)
    assert not int(lcdm._dev().status(0, 1)[0]) & _lib.ST_DE_DIVMAX


@pytest.mark.parametrize("tag,z", HALOS)
def test_halo_tables_levels_and_spectra(lib, g, tag, z):
    from chomp_amd import cosmology, halo
    zt = "%sz%03d_" % (tag, int(round(100 * z)))
    h = halo.Halo(z, None, cosmology.SingleEpoch(z, _cosmo(tag)))
    k = g["k"]
    assert rel_err(h.power_mm(k), g[zt + "power_mm"]) < RTOL_P
    assert rel_err(h.power_gm(k), g[zt + "power_gm"]) < RTOL_P
    assert rel_err(h.power_gg(k), g[zt + "power_gg"]) < RTOL_P
    ctx = h._sync(0)
    for name in TABLES:
        assert rel_err(ctx.table(name), g[zt + name]) < RTOL_KNOT, name
    lev = ctx.table("levels").reshape(5, -1)
    for row, name in enumerate(TABLES):
        ref = g[zt + "levels_" + name + "_integrand"]
        assert numpy.array_equal(lev[row], ref), (name, lev[row], ref)
    assert abs(ctx.scalars(0)["n_bar"] / float(g[zt + "n_bar"]) - 1) < 2e-7


def test_halofit(lib, g):
    from chomp_amd import cosmology, halo
    hf = halo.HaloFit(0.5, None, cosmology.SingleEpoch(0.5, _cosmo("a_")))
    k = g["k"]
    inside = (k >= hf._k_min) & (k <= hf._k_max)
    assert rel_err(hf.power_mm(k)[inside], g["hf_z050_power_mm"][inside]) < RTOL_P


def test_multi_epoch(lib, g):
    from chomp_amd import cosmology
    me = cosmology.MultiEpoch(0.0, 5.0, _cosmo("a_"))
    assert rel_err(me._z_array, g["me_z"]) < 1e-14
    assert rel_err(me._chi_array[1:], g["me_chi"][1:]) < RTOL_KNOT and me._chi_array[0] == 0.0
    assert rel_err(me._growth_array, g["me_growth"]) < 1e-12
    zs = g["me_zs"]
    for name in ("omega_m", "omega_l", "rho_crit", "delta_c", "delta_v"):
        got = numpy.array([getattr(me, name)(float(z)) for z in zs])
        assert rel_err(got, g["me_" + name]) < 1e-10, name
    t = me._dev().de_table("proj")
    assert numpy.array_equal(t["levels"], g["a_de_levels"])


def _projection(cd, ggl):
    from chomp_amd import cosmology, kernel
    deg_to_rad = numpy.pi / 180.0
    cm = cosmology.MultiEpoch(0.0, 5.0, cd)
    wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    if ggl:
        wb = kernel.WindowFunctionConvergence(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2), cm)
        K = kernel.GalaxyGalaxyLensingKernel
    else:
        wb = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
        K = kernel.Kernel
    return K(1e-6 * deg_to_rad, 100.0 * deg_to_rad, wa, wb, cm)


def test_wtheta_cell_and_ggl(lib, g):
    from chomp_amd import cosmology, correlation, halo
    cd = _cosmo("a_")
    kern = _projection(cd, ggl=False)
    h = halo.Halo(0.0, None, cosmology.SingleEpoch(0.0, cd))
    corr = correlation.Correlation(0.001, 1.0, kern, input_halo=h, power_spec="power_gg")
    assert rel_err(corr.correlation(g["theta"]), g["w_gg"]) < RTOL_P
    assert abs(kern.z_bar / float(g["kernel_z_bar"]) - 1) < 1e-6
    assert rel_err(kern.window_function_a._wf_array, g["wa"]) < 1e-8
    cf = correlation.CorrelationFourier(10, 1e4, kern, input_halo=h, powSpec="power_gg")
    assert rel_err(cf.correlation(g["ell"]), g["cl_gg"]) < RTOL_P
    kern = _projection(cd, ggl=True)
    h = halo.Halo(0.0, None, cosmology.SingleEpoch(0.0, cd))
    corr = correlation.Correlation(0.001, 1.0, kern, input_halo=h, power_spec="power_gm")
    assert rel_err(corr.correlation(g["theta"]), g["w_ggl"]) < RTOL_P
    wb = numpy.asarray(kern.window_function_b._wf_array)
    ok = g["wb"] != 0.0
    assert rel_err(wb[ok], g["wb"][ok]) < 1e-8


def test_mixed_halo_grid(lib):
    """Each row of a batch that mixes Lambda-CDM and w0-wa cosmologies equals, bit for bit, the
    same cosmology set up alone; the Lambda-CDM rows equal an all-Lambda-CDM batch set up through
    the entry points without the opt-in."""
    from chomp_amd import grid
    k = numpy.logspace(-3, 2, 64)
    cosmos = [c_dict, _cosmo("a_"), _cosmo("b_"), dict(c_dict, sigma_8=0.85), _cosmo("c_")]
    z = [0.5, 0.5, 1.0, 0.5, 0.5]
    for which in ("power_mm", "power_gg"):
        mixed = grid.HaloGrid(z, cosmo_dict=cosmos).power(which, k)
        for i in range(len(cosmos)):
            alone = grid.HaloGrid([z[i]], cosmo_dict=[cosmos[i]]).power(which, k)
            assert numpy.array_equal(mixed[i], alone[0]), (which, i)
        lcdm = [0, 3]
        old = grid.HaloGrid([z[i] for i in lcdm], cosmo_dict=[cosmos[i] for i in lcdm])
        old.setup(which)
        assert numpy.array_equal(old.power(which, k), mixed[lcdm]), which


def test_lcdm_through_the_opt_in(lib):
    """A Lambda-CDM cosmology gives the same bits with the switch on."""
    from chomp_amd import cosmology, defaults, hod
    ctx = cosmology._context()
    k = numpy.logspace(-3, 2, 32)
    hd = defaults.default_halo_dict
    out = []
    for de in (False, True):
        ctx.epochs_set(c_dict, [0.3, 0.7], dark_energy=de)
        ctx.stage_k(hd, 0, hd, hod.HODZheng(), lib.FAM_MM)
        out.append((ctx.power(lib.P_MM, k), ctx.scalars(0), ctx.scalars(1)))
    assert numpy.array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1] and out[0][2] == out[1][2]


def test_old_entry_points_refuse(lib):
    from chomp_amd import _lib, cosmology, kernel
    de = _cosmo("a_")
    ctx = cosmology._context()
    with pytest.raises(_lib.ChompScopeError):
        ctx.epochs_set(de, [0.5])
    with pytest.raises(_lib.ChompScopeError):
        ctx.multi_epoch_setup(de, 0.0, 2.0)
    w = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0),
                                    cosmology.MultiEpoch(0.0, 2.0, de))
    with pytest.raises(_lib.ChompScopeError):
        ctx.kernel_setup(de, 0.0, 2.0, 1e-6, 1.0, w._struct(), w._struct(), 0)
    # the switch is per call: after an opted-in set-up the default refuses again
    ctx.epochs_set(de, [0.5], dark_energy=True)
    with pytest.raises(_lib.ChompScopeError):
        ctx.epochs_set(de, [0.5])
