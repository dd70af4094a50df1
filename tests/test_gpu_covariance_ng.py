"""The one-halo trispectrum term of the covariance of w(theta) on the MI355X (pytest -m gpu):
Covariance(corr, corr, nongaussian_cov=True, input_halo_trispectrum=HaloTrispectrumOneHalo(...))
and KernelCovariance.kernel_NG against the reference's G25 and the NumPy restatement of
test_covariance_ng_cpu."""
import warnings

import numpy
import pytest

from conftest import load_golden, rel_err
from test_covariance_ng_cpu import ng_state, outer_step, raw_kernel_NG
from test_gpu_covariance_ssc import KWS, correlation, scaled_err

pytestmark = pytest.mark.gpu

RTOL_COV = 1e-4          # the G12 bar, per element
RTOL_KERNEL = 1e-5       # kernel_precision 1.48e-6 of the integrals, relative to the table's scale
CASES = {"mag": ("mag", 0.0, "power_mmmm"), "fit": ("fit", 0.0, "power_mmmm"),
         "ggmm": ("mag", 0.5, "power_ggmm")}


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from chomp_amd import _lib
    _lib.lib()
    return _lib


def covariance(tag, **kws):
    from chomp_amd import covariance as cov_mod, halo_trispectrum
    corr_tag, z_tri, power_spec = CASES[tag]
    corr = correlation(corr_tag)
    tri = halo_trispectrum.HaloTrispectrumOneHalo(z_tri, power_spec=power_spec)
    return cov_mod.Covariance(corr, corr, nongaussian_cov=True, input_halo_trispectrum=tri,
                              **dict(KWS, **kws))


def _prec():
    from chomp_amd import defaults
    return defaults.default_precision


@pytest.mark.parametrize("tag", ["mag", "fit"])
def test_kernel_NG_table_against_g25(lib, tag):
    g = load_golden("g25_covariance_ng")
    cv = covariance(tag)
    kc = cv.kernel
    sc = g[tag + "_scalars"]
    assert kc.z_bar_NG == sc[0]                                  # the argmax index, exactly
    assert abs(cv.D_z_NG / sc[1] - 1.0) < 1e-10
    assert kc._j0_limit == sc[6]
    assert numpy.array_equal(kc._ln_ktheta_array, g[tag + "_ln_ktheta"])
    tab = g[tag + "_kernel_array"]
    got = kc._kernel_array
    assert numpy.array_equal(got, got.T)
    print(tag, "table err / scale", scaled_err(got, tab), "min", kc._kernel_NG_min,
          g[tag + "_kernel_NG_min"][0])
    assert scaled_err(got, tab) < RTOL_KERNEL
    assert kc._kernel_NG_min == numpy.min(got)
    scale = numpy.max(numpy.abs(tab))
    assert abs(kc._kernel_NG_min - g[tag + "_kernel_NG_min"][0]) < RTOL_KERNEL * scale
    a, b = g[tag + "_probe_a"], g[tag + "_probe_b"]
    raw = kc.raw_kernel(a, b)
    assert numpy.array_equal(raw, kc.raw_kernel_NG(a, b))
    print(tag, "raw err / scale", float(numpy.max(numpy.abs(raw - g[tag + "_raw"])) / scale))
    assert numpy.max(numpy.abs(raw - g[tag + "_raw"])) < RTOL_KERNEL * scale
    spl = numpy.array([kc.kernel(x, y)[0][0] for x, y in zip(a, b)])
    print(tag, "spline err / scale", float(numpy.max(numpy.abs(spl - g[tag + "_spline"])) / scale))
    assert numpy.max(numpy.abs(spl - g[tag + "_spline"])) < RTOL_KERNEL * scale
    assert numpy.any(g[tag + "_spline"] == 0.0)
    assert numpy.array_equal(spl == 0.0, g[tag + "_spline"] == 0.0)   # the zero rule, exactly
    # strictly below the range is clamped: the value at the lower edge
    lo = kc.ln_ktheta_min
    assert kc.kernel_NG(lo - 2.0, lo - 3.0)[0][0] == kc.kernel_NG(lo, lo)[0][0]
    # grid-shaped like RectBivariateSpline: scalar x array -> [1, n]
    assert kc.kernel_NG(a[0], b[:5]).shape == (1, 5)
    # at the knots the spline interpolates the table
    x = kc._ln_ktheta_array
    at = kc.kernel_NG(x[::7], x[::7])
    assert numpy.max(numpy.abs(at - got[::7, ::7])) < 1e-9 * scale


@pytest.mark.parametrize("tag", ["mag", "fit"])
def test_kernel_NG_levels_equal_the_restatement(lib, tag):
    g = load_golden("g25_covariance_ng")
    cv = covariance(tag)
    lev = cv.kernel._kernel_levels
    kt = ng_state(tag, g)
    x = g[tag + "_ln_ktheta"]
    assert numpy.array_equal(lev, lev.T)
    for i in (0, 9, 24, 49):
        for j in (i, 37, 49):
            if j < i:
                continue
            v, level = raw_kernel_NG(kt, x[i], x[j])
            assert lev[i, j] == level, (i, j, lev[i, j], level)


@pytest.mark.parametrize("tag", ["mag", "fit", "ggmm"])
def test_covariance_NG_and_get_covariance_against_g25(lib, tag):
    g = load_golden("g25_covariance_ng")
    cv = covariance(tag)
    c = numpy.array([b.center for b in cv.annular_bins])
    assert numpy.array_equal(c, g[tag + "_center"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", lib.ChompAccuracyWarning)
        cov = cv.get_covariance()
        nb = len(c)
        ia, ib = numpy.triu_indices(nb)
        ng = cv.covariance_NG(c[ia], c[ib])
        print(tag, "NG rel err", rel_err(ng, g[tag + "_NG"][ia, ib]),
              "cov rel err", rel_err(cov, g[tag + "_cov"]))
        assert rel_err(ng, g[tag + "_NG"][ia, ib]) < RTOL_COV
        assert rel_err(cov, g[tag + "_cov"]) < RTOL_COV
        G = cv.covariance_G(c[ia], c[ib])
        assert rel_err(G, g[tag + "_G"][ia, ib]) < RTOL_COV
        # one pair at a time: bit for bit the batched values
        for p in range(len(ia)):
            assert cv.covariance_NG(c[ia[p]], c[ib[p]]) == ng[p]
        # covariance() of one bin pair is G + NG + P
        bins = cv.annular_bins
        one = cv.covariance(bins[0], bins[0])
        assert one == cov[0, 0] or abs(one / cov[0, 0] - 1.0) < 1e-15
        # the k_b knots of one pair and their levels
        out, knots, levels = cv._covariance_NG_pairs(c[:1], c[-1:], knots=True)
    ref = g[tag + "_kb_knots"]
    print(tag, "kb knots err / scale", scaled_err(knots[0], ref))
    assert scaled_err(knots[0], ref) < 1e-5
    assert knots[0][-1] == 0.0 and ref[-1] == 0.0               # the last k_a knot, exactly
    assert levels[0][-1] == 1
    assert out[0] == ng[nb - 1]
    # the trispectrum inside the integrand is the object's own table
    assert scaled_err(cv.halo_tri._i_0_4_array, g[tag + "_i_0_4"]) < 1e-6
    # the k_a spline and the outer Romberg of the device's own knots, restated on the host
    assert abs(outer_step(g[tag + "_ln_k"], knots[0], cv.area, _prec()) / out[0] - 1) < 1e-10


def test_get_covariance_with_the_super_sample_term(lib):
    g = load_golden("g25_covariance_ng")
    cv = covariance("mag", ssc_cov=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", lib.ChompAccuracyWarning)
        cov = cv.get_covariance()
    print("cov + ssc rel err", rel_err(cov, g["mag_cov_ssc"]))
    assert rel_err(cov, g["mag_cov_ssc"]) < RTOL_COV
    # both tables live side by side in the copy's context
    assert cv.kernel._kernel_array.shape == cv.kernel._kernel_ssc_array.shape == (50, 50)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", lib.ChompAccuracyWarning)
        assert numpy.array_equal(cv.get_covariance(), cov)


def test_largest_kernel_npoints(lib, monkeypatch):
    """kernel_npoints = 256, the largest the set-up takes: the LDS of k_ng_kb (a 256-knot
    kernel_NG row beside the trispectrum row) and the outer step against the host restatement of
    the device's own knots."""
    from chomp_amd import defaults
    monkeypatch.setitem(defaults.default_precision, "kernel_npoints", 256)
    cv = covariance("mag")
    c = numpy.array([b.center for b in cv.annular_bins])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", lib.ChompAccuracyWarning)
        ctx = cv.kernel._ng()
        assert ctx.config.kernel_npoints == 256 and cv.kernel._kernel_array.shape == (256, 256)
        tab = cv.kernel._kernel_array
        assert numpy.array_equal(tab, tab.T) and numpy.all(numpy.isfinite(tab))
        out, knots, levels = cv._covariance_NG_pairs(c[:1], c[-1:], knots=True)
    ln_k = numpy.linspace(numpy.log(0.001), numpy.log(100.0), 256)
    assert numpy.isfinite(out[0]) and numpy.any(knots[0] != 0.0) and knots[0][-1] == 0.0
    assert abs(outer_step(ln_k, knots[0], cv.area, _prec()) / out[0] - 1) < 1e-10


def test_set_cosmology_moves_the_trispectrum(lib):
    """covariance.py:244-271: halo_tri.set_cosmology(cosmo_dict, z_bar_NG) -- AttributeError with
    pert=None after the halo model has moved; with a PerturbationTheory the trispectrum goes to
    z_bar_NG and the kernel table and the k_b state are rebuilt."""
    from chomp_amd import covariance as cov_mod, halo_trispectrum, perturbation_spectra
    corr = correlation("mag")
    tri = halo_trispectrum.HaloTrispectrumOneHalo(0.0)
    cv = cov_mod.Covariance(corr, corr, nongaussian_cov=True, input_halo_trispectrum=tri, **KWS)
    c = numpy.array([b.center for b in cv.annular_bins])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", lib.ChompAccuracyWarning)
        before = cv.covariance_NG(c[1], c[1])
        tab = cv.kernel._kernel_array.copy()
        base = cv.get_cosmology()
        new = dict(base, omega_m0=0.31 - base["omega_r0"], omega_l0=0.69)
        with pytest.raises(AttributeError):
            cv.set_cosmology(new)
        assert tri._redshift == cv.kernel.z_bar_NG               # (the halo model has moved)
        tri.pert = perturbation_spectra.PerturbationTheory()
        cv.set_cosmology(new)
        assert tri._redshift == cv.kernel.z_bar_NG and not tri._initialized_i_0_4
        after = cv.covariance_NG(c[1], c[1])
        assert not numpy.array_equal(cv.kernel._kernel_array, tab)
    assert numpy.isfinite(after) and after != before


def test_refusals(lib):
    from chomp_amd import _lib, covariance as cov_mod, halo_trispectrum
    corr = correlation("mag")
    with pytest.raises(_lib.ChompScopeError):
        cov_mod.Covariance(corr, corr, nongaussian_cov=True, **KWS)
    with pytest.raises(_lib.ChompScopeError):
        cov_mod.Covariance(corr, corr, nongaussian_cov=True, input_halo_trispectrum=corr.halo,
                           **KWS)
    with pytest.raises(_lib.ChompScopeError):
        cov_mod.Covariance(corr, corr, nongaussian_cov=False,
                           input_halo_trispectrum=halo_trispectrum.HaloTrispectrumOneHalo(0.0),
                           **KWS)
    cv = cov_mod.Covariance(corr, corr, nongaussian_cov=False, **KWS)
    for name in ("kernel", "kernel_NG", "raw_kernel", "raw_kernel_NG"):
        with pytest.raises(_lib.ChompScopeError):
            getattr(cv.kernel, name)(0.0, 0.0)
    with pytest.raises(_lib.ChompScopeError):
        cv.covariance_NG(0.001, 0.002)
    # the C calls refuse to run out of order
    ctx = cv.kernel._ssc(table=False)
    with pytest.raises(_lib.ChompError):
        ctx.kernel_ng_eval(numpy.zeros(1), numpy.zeros(1))
    with pytest.raises(_lib.ChompError):
        ctx.covariance_ng(cv.area, numpy.ones((50, 50)), 0.001, 100.0, numpy.ones(1),
                          numpy.ones(1))
