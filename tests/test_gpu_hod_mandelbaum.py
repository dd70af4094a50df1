"""hod.HODMandelbaum on the MI355X (pytest -m gpu): the galaxy knot tables, their Romberg
stopping levels, n_bar, P_gm / P_gg, the HOD summary integrals, the CHOMP_EV_HOD_* lookups and
w(theta) against the reference's own numbers (G21, tests/golden/make_golden_hod.py), and batches
that mix the Zheng and Mandelbaum models."""
import numpy
import pytest

from conftest import load_golden, rel_err
from params import c_dict_2, h_dict_2, hod_dict

pytestmark = pytest.mark.gpu

RTOL_P = 1e-4
RTOL_KNOT = 1e-8
CASES = {"z000_": 0.0, "z050_": 0.5, "alt_": 0.3, "low_": 0.0}
TABLES = ("h_g", "pp_gm", "pp_gg")
LEVEL_ROWS = {"_h_g_integrand": 2, "_pp_gm_integrand": 3, "_pp_gg_integrand": 4}
M_DICT = {"log_M_0": 12.14, "w": 1.0}


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from chomp_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def g():
    return load_golden("g21_hod_mandelbaum")


def _halo(g, tag, cls=None, **kws):
    from chomp_amd import cosmology, halo, hod, mass_function
    cls = cls or halo.Halo
    z = CASES[tag]
    m = hod.HODMandelbaum({"log_M_0": float(g[tag + "log_M_0"]), "w": float(g[tag + "w"])})
    if tag == "alt_":
        cosmo = cosmology.SingleEpoch(z, c_dict_2)
        mass = mass_function.TinkerMassFunction(z, cosmo, h_dict_2)
        return cls(z, m, cosmo, mass, h_dict_2, **kws)
    return cls(z, m, **kws)


@pytest.mark.parametrize("tag", list(CASES))
def test_knots_levels_and_spectra(lib, g, tag):
    h = _halo(g, tag)
    k = g["k"]
    ctx0 = h._context()
    before = ctx0.deep_stats()
    assert rel_err(h.power_gm(k), g[tag + "pp_gm_k"]) < RTOL_P
    assert rel_err(h.power_gg(k), g[tag + "pp_gg_k"]) < RTOL_P
    ctx = h._sync(0)
    after = ctx.deep_stats()
    for name in TABLES:
        assert rel_err(ctx.table(name), g[tag + name]) < RTOL_KNOT, name
    lev = ctx.table("levels").reshape(5, -1)
    for name, row in LEVEL_ROWS.items():
        ref = g[tag + "levels" + name]
        assert numpy.array_equal(lev[row], ref), (name, lev[row], ref)
    assert abs(ctx.scalars(0)["n_bar"] / float(g[tag + "n_bar"]) - 1) < 2e-7
    # deep-level knots: how many the fast sums did and how many went to literal evaluation
    print("deep_stats %s: fast %d, literal %d, %r" % (tag, after[0] - before[0],
                                                     after[1] - before[1], ctx.deep_detail))


@pytest.mark.parametrize("tag", list(CASES))
def test_summary_integrals(lib, g, tag):
    h = _halo(g, tag)
    assert abs(h.calculate_bias() / float(g[tag + "bias"]) - 1) < 1e-6
    assert abs(h.calculate_m_eff() / float(g[tag + "m_eff"]) - 1) < 1e-6
    assert abs(h.calculate_f_sat() / float(g[tag + "f_sat"]) - 1) < 1e-6


@pytest.mark.parametrize("tag", list(CASES))
def test_moment_lookups(lib, g, tag):
    """CHOMP_EV_HOD_* of a Mandelbaum epoch, including the masses at and next to both
    thresholds (the device's log10 decides the steps)."""
    h = _halo(g, tag)
    h.power_gm(numpy.array([1.0]))
    ctx = h._sync(0)
    m = g[tag + "mass"]
    for what, name in (("hod_first", "first"), ("hod_second", "second"),
                       ("hod_central", "central"), ("hod_satellite", "satellite")):
        got = ctx.eval(what, m)
        assert numpy.allclose(got, g[tag + name], rtol=1e-15, atol=0.0), what
        # which branch: exactly the reference's
        assert numpy.array_equal(got > 0, g[tag + name] > 0), what


def test_wtheta(lib, g):
    from chomp_amd import correlation, cosmology, halo, hod, kernel
    d2r = numpy.pi / 180.0
    theta = g["theta"]
    for ps, ggl in (("power_gg", False), ("power_gm", True)):
        cm = cosmology.MultiEpoch(0.0, 5.0)
        wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
        if ggl:
            wb = kernel.WindowFunctionConvergence(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2), cm)
            K = kernel.GalaxyGalaxyLensingKernel
        else:
            wb = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
            K = kernel.Kernel
        kern = K(1e-6 * d2r, 100.0 * d2r, wa, wb, cm)
        h = halo.Halo(0.0, hod.HODMandelbaum(dict(M_DICT)))
        corr = correlation.Correlation(0.001, 1.0, kern, input_halo=h, power_spec=ps)
        assert rel_err(corr.correlation(theta), g["w_" + ps]) < RTOL_P, ps


def test_halofit_and_ssc_build_their_tables(lib, g):
    from chomp_amd import halo
    k = g["k"]
    plain = _halo(g, "z000_")
    p_gm, p_gg = plain.power_gm(k), plain.power_gg(k)
    hf = _halo(g, "z000_", cls=halo.HaloFit)
    hf_gm = hf.power_gm(k)
    inside = (k >= hf._k_min) & (k <= hf._k_max)      # (HaloFit is 0 outside the k range)
    assert numpy.all(numpy.isfinite(hf_gm)) and numpy.all(hf_gm[inside] > 0)
    hf.power_gg(k)
    ctx = hf._sync(0)
    for name in TABLES:
        assert rel_err(ctx.table(name), g["z000_" + name]) < RTOL_KNOT, name
    ssc = _halo(g, "z000_", cls=halo.HaloSuperSampleCovariance, delta_b=0.01)
    assert rel_err(ssc.power_gm(k), p_gm) < 1e-12
    assert rel_err(ssc.power_gg(k), p_gg) < 1e-12
    r = ssc.dln_power_ddelta_b(k)
    assert numpy.all(numpy.isfinite(r))
    ctx = ssc._sync(0)
    for name in TABLES:
        assert rel_err(ctx.table(name), g["z000_" + name]) < RTOL_KNOT, name
    cp = halo.HaloSuperSampleCovariance.init_from_halo(plain, delta_b=0.01)
    assert type(cp.get_hod_object()).__name__ == "HODMandelbaum"
    assert rel_err(cp.power_gm(k), p_gm) < 1e-12


def test_set_hod_and_set_hod_object(lib, g):
    from chomp_amd import halo, hod
    k = g["k"]
    h = halo.Halo(0.0, hod.HODZheng(hod_dict))
    h.power_gm(k)
    h.set_hod_object(hod.HODMandelbaum(dict(M_DICT)))
    assert rel_err(h.power_gm(k), g["z000_pp_gm_k"]) < RTOL_P
    h.set_hod({"log_M_0": 12.14, "w": 1.0})
    assert rel_err(h.power_gg(k), g["z000_pp_gg_k"]) < RTOL_P
    assert abs(h.calculate_f_sat() / float(g["z000_f_sat"]) - 1) < 1e-6


def test_mixed_batch_bit_for_bit(lib):
    """[Z, M, Z, M] equals [Z, Z, Z, Z] and [M, M, M, M] at the matching epochs, bit for bit:
    the model is decided per epoch and nothing of one epoch reaches another."""
    from chomp_amd import grid, hod
    z = [0.0, 0.5, 1.0, 0.3]
    k = numpy.logspace(-3, 2, 64)
    Z, M = hod.HODZheng(hod_dict), hod.HODMandelbaum(dict(M_DICT))
    out = {}
    for key, hods in (("mix", [Z, M, Z, M]), ("zzzz", [Z] * 4), ("mmmm", [M] * 4)):
        hg = grid.HaloGrid(z, hod_dict=hods)
        out[key] = (numpy.array(hg.power("power_gm", k)), numpy.array(hg.power("power_gg", k)))
    for w in (0, 1):
        assert numpy.array_equal(out["mix"][w][[0, 2]], out["zzzz"][w][[0, 2]])
        assert numpy.array_equal(out["mix"][w][[1, 3]], out["mmmm"][w][[1, 3]])
    # a list of dictionaries still means HODZheng
    hd = grid.HaloGrid(z, hod_dict=[hod_dict] * 4)
    assert numpy.array_equal(numpy.array(hd.power("power_gm", k)), out["zzzz"][0])


def test_simulation_design_batched_equals_loop(lib):
    from chomp_amd import halo, hod, simulation_design as sd
    numpy.random.seed(5)
    k = numpy.logspace(-3, 2, 24)
    params = {"log_M_0": [12.14, 11.8, 12.6], "w": [1.0, 0.5, 1.5]}
    dpd = dict(sd.default_parameter_dict, hod_dict=dict(M_DICT))

    def design():
        return sd.SimulationDesign(halo.Halo(0.3, hod.HODMandelbaum(dict(M_DICT))), "power_gm",
                                   params, n_design=5, independent_var=k,
                                   default_param_dict=dpd)
    des = design()
    batched = des.run_design()
    assert des._batched() and batched.shape == (24, 5)
    loop = design()
    loop._init_design_points()
    loop.points = des.points.copy()
    looped = loop.run_design(batched=False)
    assert rel_err(batched.values, looped.values) < 1e-12
