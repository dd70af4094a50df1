"""GPU tests of the general-slope halo profile (halo_dict["alpha"] != -1) against the reference's
own numbers (G28): the y(k, M) tables with the Romberg level of every integral, the profile
look-ups, the knot tables and spectra built on them, the mixed and the all-NFW set-ups."""
import numpy
import pytest

from conftest import load_golden
from params import c_dict_2, h_dict_2

pytestmark = pytest.mark.gpu

CASES = (("a15_", 0.0, -1.5, False), ("a05_", 0.0, -0.5, False), ("alt_", 0.5, -1.2, True))
TABLES = ("h_m", "pp_mm", "h_g", "pp_gm", "pp_gg")


def _build(cls, z, alpha, alt, **kws):
    from chomp_amd import cosmology, defaults, mass_function
    if alt:
        hd = dict(h_dict_2, alpha=alpha)
        cosmo = cosmology.SingleEpoch(z, c_dict_2)
        mass = mass_function.TinkerMassFunction(z, cosmo, hd)
        return cls(z, None, cosmo, mass, hd, general_profile=True, **kws)
    hd = dict(defaults.default_halo_dict, alpha=alpha)
    return cls(z, halo_dict=hd, general_profile=True, **kws)


@pytest.fixture(scope="module")
def g28():
    return load_golden("g28_halo_profile")


@pytest.fixture(scope="module")
def halos():
    """One Halo per G28 case with every knot table built (shared, left unchanged)."""
    import warnings
    from chomp_amd import _lib, halo
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", _lib.ChompAccuracyWarning)   # (pp_gm exhausts divmax, as G28's)
        for tag, z, alpha, alt in CASES:
            h = _build(halo.Halo, z, alpha, alt)
            h._sync(_lib.FAM_MM | _lib.FAM_GM | _lib.FAM_GG)
            out[tag] = h
    return out


def test_general_profile_is_served():
    from chomp_amd import _lib, cosmology, defaults, halo, hod
    hd = dict(defaults.default_halo_dict, alpha=-1.5)
    p = halo.Halo(0.0, halo_dict=hd, general_profile=True).power_mm(numpy.logspace(-2, 1, 7))
    assert numpy.all(numpy.isfinite(p)) and numpy.all(p > 0)
    ctx = cosmology._context()
    ctx.epochs_set(defaults.default_cosmo_dict, [0.0])
    ctx.mass_setup(hd, 0)
    ctx.halo_setup(hd, hod.HODZheng(), _lib.FAM_MM, general_profile=True)
    with pytest.raises(_lib.ChompScopeError):
        ctx.halo_setup(hd, hod.HODZheng(), _lib.FAM_MM)
    hf = halo.HaloFit(0.0, halo_dict=hd, general_profile=True)
    assert numpy.all(numpy.isfinite(hf.power_gm(numpy.logspace(-2, 1, 5))))


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_y_table(halos, g28, tag):
    """Every Romberg level the reference's; values within 1e-8 (y -> 1 as k -> 0: scale 1)."""
    y, lev = halos[tag]._ctx.y_general_table(0)
    ref, ref_lev = g28[tag + "y"], g28[tag + "y_level"]
    diff = numpy.abs(y - ref)
    print("%s y table: max |diff| %.3g, levels differing %d" %
          (tag, diff.max(), int(numpy.sum(lev != ref_lev))))
    assert numpy.array_equal(lev, ref_lev), numpy.argwhere(lev != ref_lev)
    assert diff.max() <= 1e-8


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_profile_lookups(halos, g28, tag):
    h = halos[tag]
    m = g28[tag + "mass"]
    for name in ("concentration", "virial_radius", "halo_normalization"):
        err = numpy.max(numpy.abs(getattr(h, name)(m) / g28[tag + name] - 1.0))
        print("%s %s: %.3g" % (tag, name, err))
        assert err <= 1e-7, name
    for i, ln_k in enumerate(g28["ln_k_off"]):
        got, ref = h.y(float(ln_k), g28[tag + "mass_y"]), g28[tag + "y_off"][i]
        assert numpy.array_equal(got[-2:], [0.0, 0.0])         # (outside the mass table)
        err = numpy.max(numpy.abs(got[:-2] / ref[:-2] - 1.0))
        print("%s y(ln k = %.3f): %.3g" % (tag, ln_k, err))
        assert err <= 1e-7


def _check_knots(got, lev, ref, ref_lev, what):
    diff = numpy.max(numpy.abs(got - ref)) / numpy.max(numpy.abs(ref))
    print("%s: max |diff| / scale %.3g, levels differing %d" % (what, diff, int(numpy.sum(lev != ref_lev))))
    assert numpy.array_equal(lev, ref_lev), (what, numpy.argwhere(lev != ref_lev))
    assert diff <= 1e-8, what


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_knot_tables_and_spectra(halos, g28, tag):
    h = halos[tag]
    ctx = h._ctx
    nk = ctx.config.halo_npoints
    levels = ctx.table("levels", 0).reshape(5, nk)
    for i, name in enumerate(TABLES):
        _check_knots(ctx.table(name, 0), levels[i], g28[tag + name], g28[tag + name + "_level"],
                     tag + name)
    k = g28["k"]
    for ps in ("mm", "gm", "gg"):
        got, ref = getattr(h, "power_" + ps)(k), g28[tag + "power_" + ps]
        assert numpy.array_equal(got == 0.0, ref == 0.0)       # (0 above k_max, as the fixture)
        ok = ref != 0.0
        err = numpy.max(numpy.abs(got[ok] / ref[ok] - 1.0))
        print("%spower_%s: %.3g" % (tag, ps, err))
        assert err <= 1e-7, ps


def test_ssc_and_exclusion(g28):
    from chomp_amd import _lib, halo
    s = _build(halo.HaloSuperSampleCovariance, 0.0, -1.5, False)
    k = g28["k"]
    got, ref = s.dln_power_ddelta_b(k), g28["a15_dln_power_ddelta_b"]
    assert numpy.array_equal(got == 0.0, ref == 0.0)           # (0 outside [k_min, k_max])
    ok = ref != 0.0
    err = numpy.max(numpy.abs(got[ok] / ref[ok] - 1.0))
    print("a15_dln_power_ddelta_b: %.3g" % err)
    assert err <= 1e-7
    ctx = s._ctx
    _check_knots(ctx.table("i_1_2", 0), ctx.table("levels_i_1_2", 0), g28["a15_i_1_2"],
                 g28["a15_i_1_2_level"], "a15_i_1_2")
    x = _build(halo.HaloExclusion, 0.0, -1.5, False)
    ctx = x._sync(_lib.T_H_M)
    nk = ctx.config.halo_npoints
    _check_knots(ctx.table("h_m", 0), ctx.table("levels", 0)[:nk], g28["a15_excl_h_m"],
                 g28["a15_excl_h_m_level"], "a15_excl_h_m")


def test_y_general_of_an_nfw_halo(g28):
    """Independent of the fixture's alpha != -1 cases: chomp_y_general with alpha = -1 against
    chomp_y_nfw.  The reference's own |y_general(alpha = -1) - y_nfw| is the size of the Romberg
    truncation; the bar is twice its largest."""
    from chomp_amd import halo
    h = halo.Halo(0.0)
    m = g28["nfw_mass"]
    bar = 2.0 * numpy.max(numpy.abs(g28["nfw_y_general"] - g28["nfw_y_nfw"]))
    worst = 0.0
    for ln_k in g28["nfw_ln_k"]:
        worst = max(worst, numpy.max(numpy.abs(h.y_general(float(ln_k), m) - h.y_nfw(float(ln_k), m))))
    print("y_general(alpha = -1) - y_nfw: %.3g (bar %.3g)" % (worst, bar))
    assert worst <= bar


def _setup(ctx, z, alphas, general_profile):
    from chomp_amd import _lib, defaults, hod
    ctx.epochs_set(defaults.default_cosmo_dict, z)
    hds = [dict(defaults.default_halo_dict, alpha=a) for a in alphas]
    ctx.stage_k(hds, 0, hds, hod.HODZheng(), _lib.FAM_MM | _lib.FAM_GM | _lib.FAM_GG,
                general_profile=general_profile)
    return [numpy.concatenate([ctx.table(name, e) for name in TABLES]) for e in range(len(z))]


def test_mixed_setup():
    import warnings
    from chomp_amd import _lib, cosmology
    ctx = cosmology._context()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", _lib.ChompAccuracyWarning)
        mixed = _setup(ctx, [0.0, 0.5, 1.0], [-1.0, -1.5, -1.0], True)
        single = _setup(ctx, [0.5], [-1.5], True)
        nfw_on = _setup(ctx, [0.0, 0.5, 1.0], [-1.0, -1.0, -1.0], True)
        nfw_off = _setup(ctx, [0.0, 0.5, 1.0], [-1.0, -1.0, -1.0], False)
    assert numpy.array_equal(mixed[1], single[0])
    for a, b in zip(nfw_on, nfw_off):
        assert numpy.array_equal(a, b)
    nk = ctx.config.halo_npoints
    for e in (0, 2):
        for i, name in enumerate(TABLES):
            a, b = mixed[e][i * nk:(i + 1) * nk], nfw_off[e][i * nk:(i + 1) * nk]
            diff = numpy.max(numpy.abs(a - b)) / numpy.max(numpy.abs(b))
            print("mixed epoch %d %s against the fast path: %.3g" % (e, name, diff))
            assert diff <= 1e-8, (e, name)


def test_alpha_at_the_divergence_is_refused():
    from chomp_amd import _lib, cosmology, defaults, halo, hod
    ctx = cosmology._context()
    ctx.epochs_set(defaults.default_cosmo_dict, [0.0])
    hd = dict(defaults.default_halo_dict, alpha=-3.0)
    ctx.mass_setup(hd, 0)
    with pytest.raises(ValueError):
        ctx.halo_setup(hd, hod.HODZheng(), _lib.FAM_MM, general_profile=True)
    with pytest.raises(ValueError):
        halo.Halo(0.0, halo_dict=hd, general_profile=True)
    with pytest.raises(ValueError):     # (beyond the validated range of the profile's mass integral)
        ctx.halo_setup(dict(hd, alpha=3.6), hod.HODZheng(), _lib.FAM_MM, general_profile=True)
    ok = dict(hd, alpha=-1.0)
    ctx.halo_setup(ok, hod.HODZheng(), _lib.FAM_MM, general_profile=True)
    assert numpy.all(numpy.isfinite(ctx.power(_lib.P_MM, numpy.logspace(-2, 1, 5), 0, 1)))
