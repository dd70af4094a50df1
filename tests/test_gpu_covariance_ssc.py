"""The super-sample covariance of w(theta) on the MI355X (pytest -m gpu):
Covariance(corr, corr, nongaussian_cov=False, ssc_cov=True) and KernelCovariance.kernel_ssc
against the reference's G20 and the oracle composition of test_covariance_ssc_cpu."""
import numpy
import pytest

from conftest import load_golden, rel_err
from test_covariance_ssc_cpu import KB_LEVELS, case_state, covariance_ssc as oracle_outer, \
    raw_kernel_ssc

pytestmark = pytest.mark.gpu

deg_to_rad = numpy.pi / 180.0
KWS = dict(bins_per_decade=2.0, survey_area_deg2=25.0, n_a=[1.0e10, 1.0e10],
           n_b=[1.0e10, 1.0e10], variance=1.0)
RTOL_COV = 1e-4          # the G12 bar, per element
RTOL_KERNEL = 1e-5       # kernel_precision 1.48e-6 of the integrals, relative to the table's scale


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from chomp_amd import _lib
    _lib.lib()
    return _lib


def correlation(tag, halo_obj=None):
    from chomp_amd import correlation as corr_mod, cosmology, halo, kernel
    cm = cosmology.MultiEpoch(0.0, 5.0)
    if tag == "zero":
        wa = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.5, 2.0, 1.0, 0.2), cm)
    else:
        wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    wb = wa if tag != "mag" else kernel.WindowFunctionConvergence(
        kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2), cm)
    kern = kernel.Kernel(1e-6 * deg_to_rad, 100.0 * deg_to_rad, wa, wb, cm)
    if halo_obj is None:
        halo_obj = halo.HaloFit(0.0) if tag == "fit" else halo.Halo(0.0)
    return corr_mod.Correlation(0.01, 1.0, kern, input_halo=halo_obj, power_spec="power_mm")


def covariance(tag, **kws):
    from chomp_amd import covariance as cov_mod
    corr = correlation(tag)
    return cov_mod.Covariance(corr, corr, nongaussian_cov=False, ssc_cov=True,
                              **dict(KWS, **kws))


def scaled_err(got, ref):
    scale = numpy.max(numpy.abs(ref))
    return float(numpy.max(numpy.abs(numpy.asarray(got) - ref)) / scale)


@pytest.mark.parametrize("tag", ["mag", "fit"])
def test_kernel_ssc_table_against_g20(lib, tag):
    g = load_golden("g20_covariance_ssc")
    cv = covariance(tag)
    kc = cv.kernel
    sc = g[tag + "_scalars"]
    assert kc.z_bar_NG == sc[0]                                  # the argmax index, exactly
    assert abs(cv.D_z_NG / sc[1] - 1.0) < 1e-10
    assert (kc._j0_ssc_limit, kc._j1_limit) == (sc[6], sc[7])
    assert numpy.array_equal(kc._ln_ktheta_array, g[tag + "_ln_ktheta"])
    # (chi_min, chi_max are device integrals: the ln chi knots agree to rounding)
    assert numpy.max(numpy.abs(kc._sigma2_ln_chi - g[tag + "_sigma2_ln_chi"])) < 1e-12
    assert rel_err(kc._sigma2_knots, g[tag + "_sigma2"]) < 1e-8
    tab = g[tag + "_kernel_ssc_array"]
    assert numpy.array_equal(kc._kernel_ssc_array, kc._kernel_ssc_array.T)
    assert scaled_err(kc._kernel_ssc_array, tab) < RTOL_KERNEL
    a, b = g[tag + "_probe_a"], g[tag + "_probe_b"]
    assert scaled_err(kc.raw_kernel_ssc(a, b), g[tag + "_raw"]) < RTOL_KERNEL
    spl = numpy.array([kc.kernel_ssc(x, y)[0][0] for x, y in zip(a, b)])
    assert scaled_err(spl, g[tag + "_spline"]) < RTOL_KERNEL
    assert numpy.all(spl[g[tag + "_spline"] == 0.0] == 0.0)      # the zero rule, exactly
    # grid-shaped like RectBivariateSpline: scalar x array -> [1, n]
    grid = kc.kernel_ssc(a[0], b[:5])
    assert grid.shape == (1, 5)
    # sigma^2 outside [chi_min, chi_max] is 0, negative arguments included
    s2 = kc._sigma2(numpy.array([-1.0, 0.5 * kc.chi_min, 2.0 * kc.chi_max]))
    assert numpy.array_equal(s2, numpy.zeros(3))


@pytest.mark.parametrize("tag", ["mag", "fit"])
def test_kernel_ssc_levels_equal_the_oracle(lib, tag):
    g = load_golden("g20_covariance_ssc")
    cv = covariance(tag)
    lev = cv.kernel._kernel_ssc_levels
    kt = case_state(tag, g)
    assert numpy.array_equal(lev, lev.T)
    for i in (0, 9, 24, 49):
        for j in (i, 37, 49):
            if j < i:
                continue
            v, level = raw_kernel_ssc(kt, kt.ssc_ln_kt[i], kt.ssc_ln_kt[j])
            assert lev[i, j] == level, (i, j, lev[i, j], level)


@pytest.mark.parametrize("tag", ["mag", "fit"])
def test_covariance_ssc_and_get_covariance_against_g20(lib, tag):
    g = load_golden("g20_covariance_ssc")
    cv = covariance(tag)
    c = numpy.array([b.center for b in cv.annular_bins])
    assert numpy.array_equal(c, g[tag + "_center"])
    cov = cv.get_covariance()
    assert rel_err(cov, g[tag + "_cov"]) < RTOL_COV
    nb = len(c)
    ia, ib = numpy.triu_indices(nb)
    ssc = cv.covariance_ssc(c[ia], c[ib])
    assert rel_err(ssc, g[tag + "_ssc"][ia, ib]) < RTOL_COV
    G = cv.covariance_G(c[ia], c[ib])
    assert rel_err(G, g[tag + "_G"][ia, ib]) < RTOL_COV       # G from the halo-model copy
    # one pair at a time: bit for bit the batched values
    for p in range(len(ia)):
        assert cv.covariance_ssc(c[ia[p]], c[ib[p]]) == ssc[p]
    # covariance() of one bin pair is G + SSC + P
    bins = cv.annular_bins
    assert cv.covariance(bins[0], bins[0]) == cov[0, 0] or \
        abs(cv.covariance(bins[0], bins[0]) / cov[0, 0] - 1.0) < 1e-15
    # the k_b knots of one pair and their levels
    out, knots, levels = cv.kernel._ssc().covariance_ssc(0, cv.area, c[:1], c[-1:], knots=True)
    ref = g[tag + "_kb_knots"]
    assert scaled_err(knots[0], ref) < 1e-5
    assert numpy.array_equal(levels[0], KB_LEVELS)              # the oracle's levels
    assert out[0] == ssc[nb - 1]
    # the k_a spline and the outer Romberg of the device's own knots, restated on the host
    assert abs(oracle_outer(g[tag + "_ln_k"], knots[0], cv.area, _prec()) / out[0] - 1) < 1e-10


def _prec():
    from chomp_amd import defaults
    return defaults.default_precision


def test_outer_step_at_the_largest_kernel_npoints(lib, monkeypatch):
    """kernel_npoints = 256, the largest chomp_kernel_ssc_setup takes: the k_a spline of
    k_ssc_outer (LDS sized for 256 knots and spline_build's work) against the host restatement
    of its own knots."""
    from chomp_amd import defaults
    monkeypatch.setitem(defaults.default_precision, "kernel_npoints", 256)
    cv = covariance("mag")
    c = numpy.array([b.center for b in cv.annular_bins])
    ctx = cv.kernel._ssc()
    assert ctx.config.kernel_npoints == 256 and cv.kernel._kernel_ssc_array.shape == (256, 256)
    cv.halo_a._sync(lib.FAM_SSC)
    out, knots, levels = ctx.covariance_ssc(0, cv.area, c[:1], c[-1:], knots=True)
    ln_k = numpy.linspace(numpy.log(0.001), numpy.log(100.0), 256)
    assert numpy.isfinite(out[0]) and numpy.any(knots[0] != 0.0)
    assert abs(oracle_outer(ln_k, knots[0], cv.area, _prec()) / out[0] - 1) < 1e-10


def test_halo_copies_have_the_same_response(lib):
    cv = covariance("mag")
    cv.get_covariance()
    k = numpy.logspace(-3.5, 2.5, 200)
    ra = cv.halo_a.dln_power_ddelta_b(k)
    rb = cv.halo_b.dln_power_ddelta_b(k)
    assert cv.halo_a is not cv.halo_b
    assert numpy.array_equal(ra, rb)


def test_all_zero_knots_give_nan(lib):
    g = load_golden("g20_covariance_ssc")
    cv = covariance("zero")
    assert numpy.all(cv.kernel._kernel_ssc_array == 0.0)
    c = numpy.array([b.center for b in cv.annular_bins])
    v = cv.covariance_ssc(c[0], c[-1])
    assert numpy.isnan(v) and numpy.isnan(g["zero_ssc"][0])


def test_refusals(lib):
    from chomp_amd import _lib, covariance as cov_mod, halo
    corr = correlation("mag")
    with pytest.raises(_lib.ChompScopeError):
        cov_mod.Covariance(corr, corr, ssc_cov=True)           # nongaussian_cov defaults to True
    cv = cov_mod.Covariance(corr, corr, nongaussian_cov=False, **KWS)
    with pytest.raises(AttributeError):
        cv.covariance_ssc(0.001, 0.002)                        # a plain Halo has no response
    for name in ("kernel", "kernel_NG", "raw_kernel", "raw_kernel_NG"):
        with pytest.raises(_lib.ChompScopeError):
            getattr(cv.kernel, name)(0.0, 0.0)
    with pytest.raises(_lib.ChompScopeError):
        cv.covariance_NG(0.001, 0.002)
    cv = covariance("mag")
    before = (cv.halo_a, cv.corr_a.kernel.cosmo.cosmo_dict)
    with pytest.raises(_lib.ChompScopeError):
        cv.set_cosmology(dict(cv.get_cosmology(), omega_m0=0.3))
    assert (cv.halo_a, cv.corr_a.kernel.cosmo.cosmo_dict) == before
    # a correlation whose halo already is a HaloSuperSampleCovariance works without ssc_cov
    corr = correlation("mag", halo.HaloSuperSampleCovariance(0.0))
    cv = cov_mod.Covariance(corr, corr, nongaussian_cov=False, **KWS)
    c = numpy.array([b.center for b in cv.annular_bins])
    assert numpy.isfinite(cv.covariance_ssc(c[0], c[1]))
