"""The trispectrum and super-sample terms of a cross block without a device: the opt-in rules of
Covariance(corr_a, corr_b, cross_terms=True) / KernelCovariance(four_windows=True) /
CovarianceMulti(cross_terms=, ssc_cov=), the new entry points, and the reference's fixture G30
(tests/golden/make_golden_cov_cross_terms.py) against a NumPy restatement of KernelCovariance
with four different windows (kernel.py:893-972, 1035-1111, 1155-1206) and of _kb_ssc_integrand
with halo_a at k_a and halo_b at k_b (covariance.py:763-776), composed from the oracle and the
helpers of test_covariance_ssc_cpu / test_covariance_ng_cpu and held to those tests' bars."""
import os
import warnings

import numpy
import pytest
from scipy import special
from scipy.interpolate import InterpolatedUnivariateSpline

from conftest import ROOT, load_golden, rel_err
from test_covariance_ng_cpu import kernel_NG_spline, trispectrum_parallelogram
from test_covariance_ssc_cpu import covariance_ssc as outer_step, kernel_ssc_spline, \
    oracle_response

deg_to_rad = numpy.pi / 180.0
SWAPPED = ((3, 0), (2, 1))


# -- the restatement ------------------------------------------------------------------------
def windows(tag):
    """The oracle's tables of the fixture's four windows a1, a2, b1, b2."""
    from oracle import chomp_oracle as o
    gal = lambda *p: o.Table(kind="galaxy", dist=o.dndz_gaussian(*p))
    if tag == "gal":
        w1, w2 = gal(0.0, 2.0, 0.8, 0.2), gal(0.0, 2.0, 1.0, 0.2)
        return w1, w1, w2, w2
    wa = o.Table(kind="galaxy", dist=o.dndz_maglim(0.0, 2.0, 2.0, 0.3, 2.0))
    wb = o.Table(kind="convergence", dist=o.dndz_gaussian(0.0, 2.0, 1.0, 0.2))
    wc = gal(0.0, 1.5, 0.7, 0.2) if tag == "wide" else gal(0.5, 1.5, 1.0, 0.2)
    return wa, wb, wc, wc


class FourWindows(object):
    """kernel.py:893-972: the four windows on correlation a's MultiEpoch, their common range,
    z_bar_NG of a1 a2 b1 b2 D^4 / chi^2, the sigma^2 spline and the J0 limits."""

    def __init__(self, tag, ln_kt_min, ln_kt_max):
        from oracle import chomp_oracle as o
        me = o.multi_epoch(0.0, 5.0)
        a1, a2, b1, b2 = windows(tag)
        ka = o.kernel_table(1e-6 * deg_to_rad, 100.0 * deg_to_rad, a1, a2, me)
        kb = o.kernel_table(1e-6 * deg_to_rad, 100.0 * deg_to_rad, b1, b2, me)
        self.me, self.prec = ka.me, ka.prec
        self.w = (ka.wa, ka.wb, kb.wa, kb.wb)
        p = self.prec
        self.z_min, self.z_max = max(ka.z_min, kb.z_min), min(ka.z_max, kb.z_max)
        self.chi_min = max(p["window_precision"], float(o.me_chi(self.me, self.z_min)))
        self.chi_max = float(o.me_chi(self.me, self.z_max))
        z = numpy.linspace(self.z_min, self.z_max, p["kernel_npoints"])
        chi = o.me_chi(self.me, z)
        chi = numpy.where(chi > p["window_precision"], chi, p["window_precision"])
        self.z_bar_NG = z[numpy.argmax(self.ng_integrand(chi, 0.0, 0.0))]
        self.chi_peak_NG = float(o.me_chi(self.me, self.z_bar_NG))
        self.D_z_NG = float(o.me_growth(self.me, self.z_bar_NG))
        c = numpy.logspace(numpy.log10(self.chi_min), numpy.log10(self.chi_max),
                           p["corr_npoints"])
        sigma = numpy.array([o.sigma_r(self.me.e0, x) for x in c]) * o.me_growth(self.me, 0.0)
        self.sigma2_ln_chi, self.sigma2 = numpy.log(c), sigma * sigma
        self.sigma2_spline = InterpolatedUnivariateSpline(self.sigma2_ln_chi, self.sigma2)
        self.j0_limit = special.jn_zeros(0, p["kernel_bessel_limit"])[-1]
        self.j0_ssc_limit = special.jn_zeros(0, int(p["kernel_bessel_limit"] * 8))[-1]
        self.ln_kt = numpy.linspace(ln_kt_min, ln_kt_max, p["kernel_npoints"])

    def product(self, chi):
        """a1 a2 b1 b2, in the reference's order."""
        from oracle import chomp_oracle as o
        a1, a2, b1, b2 = (o.window(w, chi) for w in self.w)
        return a1 * a2 * b1 * b2

    def growth(self, chi):
        from oracle import chomp_oracle as o
        return o.me_growth(self.me, self.me.z_spline(chi))

    def ng_integrand(self, chi, kta, ktb, norm=1.0):
        """kernel.py:1103-1111."""
        D = self.growth(chi)
        return (norm * self.product(chi) * D * D * D * D / (chi * chi) * special.j0(kta * chi) *
                special.j0(ktb * chi))

    def ssc_integrand(self, x, kta, ktb, norm):
        """kernel.py:1197-1206, called with x = ln chi as chi."""
        with numpy.errstate(invalid="ignore", divide="ignore"):
            D = self.growth(x)
            s2 = numpy.where((x >= self.chi_min) & (x <= self.chi_max),
                             self.sigma2_spline(numpy.log(x)), 0.0)
            return (norm * self.product(x) * D * D * D * D * D * D * s2 / x *
                    special.j0(kta * x) * special.j0(ktb * x))

    def _raw(self, la, lb, limit, ssc):
        from oracle.romberg import AccuracyWarning, romberg
        p = self.prec
        kta, ktb = numpy.exp(la), numpy.exp(lb)
        chi_max = numpy.max([limit / kta, limit / ktb])
        if chi_max >= self.chi_max:
            chi_max = self.chi_max
        elif chi_max <= self.chi_min:
            return 0.0, 0
        inv = self.ng_integrand(self.chi_peak_NG, la, la)       # (the quirk: ln k theta_a)
        norm = 1.0 / inv if (inv > 1e-16 or inv < -1e-16) else 1.0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", AccuracyWarning)
            if ssc:
                v, level = romberg(self.ssc_integrand, numpy.log(self.chi_min),
                                   numpy.log(chi_max), args=(kta, ktb, norm), vec_func=True,
                                   tol=p["global_precision"], rtol=p["kernel_precision"],
                                   divmax=p["divmax"], return_level=True)
                return v * (16.0 * numpy.pi * numpy.pi / 9.0) / norm, level
            v, level = romberg(self.ng_integrand, self.chi_min, chi_max,
                               args=(kta, ktb, norm), vec_func=True, tol=p["global_precision"],
                               rtol=p["kernel_precision"], divmax=p["divmax"],
                               return_level=True)
        return v / norm, level

    def raw_kernel_NG(self, la, lb):
        """kernel.py:1035-1073 -> (value, Romberg level; 0 where the range is empty)."""
        return self._raw(la, lb, self.j0_limit, False)

    def raw_kernel_ssc(self, la, lb):
        """kernel.py:1155-1206 -> (value, Romberg level; 0 where the range is empty)."""
        return self._raw(la, lb, self.j0_ssc_limit, True)


_STATE = {}


def four_state(tag):
    if tag not in _STATE:
        sc = load_golden("g30_covariance_cross_terms")[tag + "_scalars"]
        _STATE[tag] = FourWindows(tag, sc[4], sc[5])
    return _STATE[tag]


KNOTS = (0, 13, 26, 38, 48, 49)      # the k_a knots the k_b integrals are restated at


def kb_knots(weight_a, weight_b, kernel, theta_a, theta_b, prec, k_min, k_max, at=KNOTS):
    """covariance.py:641-683 / 733-776 at the k_a knots `at`: the Romberg over ln k_b of
    k_b^2 weight(k_a, k_b) kernel(ln k_a theta_a, ln k_b theta_b), norm = 1, where the weight is
    T(k_a, k_b) for the trispectrum term (weight_b None) and R_a(k_a) R_b(k_b) -- halo_a's
    response at k_a, halo_b's at k_b -- for the super-sample term."""
    from oracle.romberg import AccuracyWarning, romberg
    ln_k = numpy.linspace(numpy.log(k_min), numpy.log(k_max), prec["kernel_npoints"])

    def integrand(ln_kb, ln_ka):
        ka, kb = numpy.exp(ln_ka), numpy.exp(ln_kb)
        w = weight_a(ka, kb)[0] if weight_b is None else weight_a(ka) * weight_b(kb)
        return (kb * 1.0 * kb * 1.0 * w *
                kernel(numpy.log(ka * theta_a), numpy.log(kb * theta_b))[0])
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", AccuracyWarning)
        for i in at:
            v = romberg(integrand, ln_k[0], ln_k[-1], args=(ln_k[i],), vec_func=True,
                        tol=prec["global_precision"], rtol=prec["corr_precision"],
                        divmax=prec["divmax"])
            out.append(float(numpy.ravel(v)[0]))
    return ln_k, numpy.array(out)


# -- G30 against the restatement --------------------------------------------------------------
@pytest.mark.parametrize("tag", ["wide", "gal", "far"])
def test_g30_four_window_state(tag):
    g = load_golden("g30_covariance_cross_terms")
    kt = four_state(tag)
    sc = g[tag + "_scalars"]
    assert kt.z_bar_NG == sc[0]
    assert abs(kt.D_z_NG / sc[1] - 1.0) < 1e-12
    assert abs(kt.chi_min / sc[2] - 1.0) < 1e-12 and abs(kt.chi_max / sc[3] - 1.0) < 1e-12
    assert (kt.j0_limit, kt.j0_ssc_limit) == (sc[6], sc[7])
    assert kt.z_min == sc[10] and kt.z_max == sc[11]
    assert numpy.array_equal(kt.ln_kt, g[tag + "_ln_ktheta"])
    assert numpy.array_equal(kt.sigma2_ln_chi, g[tag + "_sigma2_ln_chi"])
    assert rel_err(kt.sigma2, g[tag + "_sigma2"]) < 1e-10


@pytest.mark.parametrize("tag", ["wide", "gal"])
def test_g30_kernels_against_numpy_restatement(tag):
    g = load_golden("g30_covariance_cross_terms")
    kt = four_state(tag)
    ln_kt = g[tag + "_ln_ktheta"]
    a, b = g[tag + "_probe_a"], g[tag + "_probe_b"]
    assert numpy.any(a < ln_kt[0]) and numpy.any(b > ln_kt[-1])    # the clamp and zero edges
    for name, raw_fn, spline_fn, key in (
            ("ssc", kt.raw_kernel_ssc, kernel_ssc_spline, "_kernel_ssc_array"),
            ("ng", kt.raw_kernel_NG, kernel_NG_spline, "_kernel_array")):
        tab = g[tag + key]
        assert numpy.array_equal(tab, tab.T)
        scale = numpy.max(numpy.abs(tab))
        for i, j in ((0, 0), (0, 30), (17, 30), (17, 49), (49, 49)):
            v, _ = raw_fn(ln_kt[i], ln_kt[j])
            assert abs(v - tab[i, j]) <= 1e-10 * scale, (name, i, j)
        raw = numpy.array([raw_fn(x, y)[0] for x, y in zip(a, b)])
        assert numpy.max(numpy.abs(raw - g[tag + "_%s_raw" % name])) <= 1e-10 * scale, name
        spl = spline_fn(ln_kt, tab)
        got = numpy.array([spl(x, y)[0][0] for x, y in zip(a, b)])
        ref = g[tag + "_%s_spline" % name]
        assert numpy.max(numpy.abs(got - ref)) <= 1e-12 * scale, name
        assert numpy.array_equal(got == 0.0, ref == 0.0)            # the zero rule is exact
    assert numpy.min(g[tag + "_kernel_array"]) == g[tag + "_kernel_NG_min"][0]


@pytest.mark.parametrize("tag", ["wide", "gal"])
def test_g30_covariance_terms_against_numpy_restatement(tag):
    """The k_b integrals of the stored pair at a handful of k_a knots, and the outer step on the
    reference's own knots."""
    from oracle.chomp_oracle import default_precision as prec
    g = load_golden("g30_covariance_cross_terms")
    ln_kt, ln_k = g[tag + "_ln_ktheta"], g[tag + "_ln_k"]
    c, sc = g[tag + "_center"], g[tag + "_scalars"]
    pairs = [tuple(p) for p in g[tag + "_pairs"]]
    at = pairs.index((0, 3))
    idx = list(KNOTS)
    # the trispectrum term: / D(z_bar_NG)^4 (covariance.py:659)
    kernel = kernel_NG_spline(ln_kt, g[tag + "_kernel_array"])
    tri = trispectrum_parallelogram(ln_k, g[tag + "_i_0_4"], 0.001, 100.0)
    x, knots = kb_knots(tri, None, kernel, c[0], c[-1], prec, 0.001, 100.0)
    ref = g[tag + "_ng_kb_knots"]
    assert numpy.array_equal(x, ln_k)
    assert numpy.max(numpy.abs(knots / sc[1] ** 4 - ref[idx])) <= 1e-9 * numpy.max(numpy.abs(ref))
    assert ref[-1] == 0.0 and knots[-1] == 0.0 and ref[-2] != 0.0
    assert abs(outer_step(ln_k, ref, sc[9], prec) / g[tag + "_NG"][at] - 1.0) < 1e-8
    # the super-sample term: halo_a at z_bar_a answers at k_a, halo_b at z_bar_b at k_b
    kernel = kernel_ssc_spline(ln_kt, g[tag + "_kernel_ssc_array"])
    resp_a, resp_b = oracle_response(float(sc[12])), oracle_response(float(sc[13]))
    assert sc[12] != sc[13]
    _, knots = kb_knots(resp_a, resp_b, kernel, c[0], c[-1], prec, 0.001, 100.0)
    ref = g[tag + "_ssc_kb_knots"]
    assert numpy.max(numpy.abs(knots - ref[idx])) <= 1e-9 * numpy.max(numpy.abs(ref))
    assert ref[-1] == 0.0 and knots[-1] == 0.0
    assert abs(outer_step(ln_k, ref, sc[9], prec) / g[tag + "_ssc"][at] - 1.0) < 1e-8
    # ... and with the two halos interchanged the knots are others: a and b are not symmetric
    _, other = kb_knots(resp_b, resp_a, kernel, c[0], c[-1], prec, 0.001, 100.0, at=(13, 38))
    assert numpy.min(numpy.abs(other / ref[[13, 38]] - 1.0)) > 1e-4
    # get_covariance = G + NG + SSC on the upper triangle (no Poisson term on a cross block)
    nb = len(c)
    for p, (i, j) in enumerate(pairs[:nb * (nb + 1) // 2]):
        total = g[tag + "_G"][p] + g[tag + "_NG"][p] + g[tag + "_ssc"][p]
        assert abs(total / g[tag + "_cov"][i, j] - 1.0) < 1e-12
        assert g[tag + "_cov"][j, i] == g[tag + "_cov"][i, j]


@pytest.mark.parametrize("tag", ["wide", "gal"])
def test_g30_swapped_pairs_differ(tag):
    """covariance_NG(theta_a, theta_b) and covariance_ssc(theta_a, theta_b) of a cross block are
    not symmetric in their arguments; covariance_G is.  The two orders differ by more than twice
    the 1e-4 bar the device is held to per element, so a value within the bar of one order cannot
    pass for the other."""
    g = load_golden("g30_covariance_cross_terms")
    pairs = [tuple(p) for p in g[tag + "_pairs"]]
    for i, j in SWAPPED:
        p, q = pairs.index((i, j)), pairs.index((j, i))
        for name, least in (("NG", 2e-4), ("ssc", 2e-4)):
            v = g[tag + "_" + name]
            assert numpy.isfinite(v[p]) and numpy.isfinite(v[q])
            assert abs(v[p] / v[q] - 1.0) > least, (name, i, j, v[p], v[q])
        assert abs(g[tag + "_G"][p] / g[tag + "_G"][q] - 1.0) < 1e-12


def test_g30_far_zero_and_nan():
    """Windows that share z = 0.5-1.27 only: sigma^2(ln chi) is 0 over the whole range, so every
    kernel_ssc knot is 0, covariance_ssc is 0 * inf = NaN and so is the full matrix; the
    trispectrum term is finite."""
    from oracle.chomp_oracle import default_precision as prec
    g = load_golden("g30_covariance_cross_terms")
    assert numpy.all(g["far_kernel_ssc_array"] == 0.0)
    assert numpy.all(g["far_ssc_raw"] == 0.0) and numpy.all(g["far_ssc_spline"] == 0.0)
    assert numpy.all(numpy.isnan(g["far_ssc"])) and numpy.all(numpy.isnan(g["far_cov"]))
    ln_k = g["far_ln_k"]
    assert numpy.isnan(outer_step(ln_k, numpy.zeros_like(ln_k), 1.0, prec))
    kt = four_state("far")
    assert kt.raw_kernel_ssc(kt.ln_kt[3], kt.ln_kt[20])[0] == 0.0
    tab = g["far_kernel_array"]
    scale = numpy.max(numpy.abs(tab))
    for i, j in ((0, 0), (17, 30), (49, 49)):
        assert abs(kt.raw_kernel_NG(kt.ln_kt[i], kt.ln_kt[j])[0] - tab[i, j]) <= 1e-10 * scale
    a, b = g["far_probe_a"], g["far_probe_b"]
    raw = numpy.array([kt.raw_kernel_NG(x, y)[0] for x, y in zip(a, b)])
    assert numpy.max(numpy.abs(raw - g["far_ng_raw"])) <= 1e-10 * scale
    assert numpy.all(numpy.isfinite(g["far_NG"])) and numpy.all(g["far_NG"] > 0.0)


# -- the host-side surface, without a device ------------------------------------------------
def _corr(z0=1.0):
    from chomp_amd import correlation, cosmology, halo, kernel
    cm = cosmology.MultiEpoch(0.0, 5.0)
    w = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 2.0, z0, 0.2), cm)
    kern = kernel.Kernel(1e-6 * deg_to_rad, 100.0 * deg_to_rad, w, w, cm)
    c = correlation.Correlation.__new__(correlation.Correlation)
    c.log_theta_min, c.log_theta_max = numpy.log10(0.01 * deg_to_rad), numpy.log10(deg_to_rad)
    c.kernel, c.halo, c._power_name = kern, halo.Halo(0.0), "power_mm"
    return c


def _tri():
    from chomp_amd import halo_trispectrum
    return halo_trispectrum.HaloTrispectrumOneHalo.__new__(halo_trispectrum.HaloTrispectrumOneHalo)


def test_opt_in_rules():
    from chomp_amd import _lib, covariance, halo
    c1, c2, tri = _corr(0.8), _corr(1.0), _tri()
    # with the keyword a cross block takes either term, or both
    cv = covariance.Covariance(c1, c2, nongaussian_cov=True, input_halo_trispectrum=tri,
                               cross_terms=True)
    assert cv.matching_corrs is False and cv.nongaussian_cov is True and cv.ssc_cov is False
    assert cv.kernel._four_windows is True and cv.kernel._trispectrum_kernel is True
    assert cv.halo_a is c1.halo and cv.halo_b is c2.halo
    cv = covariance.Covariance(c1, c2, nongaussian_cov=False, ssc_cov=True, cross_terms=True)
    assert cv.kernel._four_windows is True and cv.kernel._trispectrum_kernel is False
    for h, src in ((cv.halo_a, c1.halo), (cv.halo_b, c2.halo)):
        assert isinstance(h, halo.HaloSuperSampleCovariance) and h is not src
    assert cv.halo_a is not cv.halo_b
    cv = covariance.Covariance(c1, c2, nongaussian_cov=True, input_halo_trispectrum=tri,
                               ssc_cov=True, cross_terms=True)
    assert cv.nongaussian_cov and cv.ssc_cov and cv.halo_tri is tri
    # without it: today's refusals, whose messages now also say how to opt in
    with pytest.raises(_lib.ChompScopeError, match="nongaussian_cov=False") as e:
        covariance.Covariance(c1, c2, nongaussian_cov=True, input_halo_trispectrum=tri)
    assert "cross_terms=True" in str(e.value)
    with pytest.raises(_lib.ChompScopeError, match="super-sample"):
        covariance.Covariance(c1, c2, nongaussian_cov=False, ssc_cov=True)
    with pytest.raises(_lib.ChompScopeError, match="super-sample"):
        covariance.Covariance(c1, c2, nongaussian_cov=False, ssc_cov=True, cross_terms=False)
    # the trispectrum object follows the matching path's rules
    with pytest.raises(_lib.ChompScopeError, match="input_halo_trispectrum"):
        covariance.Covariance(c1, c2, nongaussian_cov=True, cross_terms=True)
    with pytest.raises(_lib.ChompScopeError):
        covariance.Covariance(c1, c2, nongaussian_cov=True, input_halo_trispectrum=object(),
                              cross_terms=True)
    with pytest.raises(_lib.ChompScopeError):
        covariance.Covariance(c1, c2, nongaussian_cov=False, input_halo_trispectrum=tri,
                              cross_terms=True)
    # the other limits of a cross block stay
    c3 = _corr(1.0)
    c3._power_name = "power_gg"
    with pytest.raises(_lib.ChompScopeError, match="power_spec"):
        covariance.Covariance(c1, c3, nongaussian_cov=False, ssc_cov=True, cross_terms=True)
    c4 = _corr(1.0)
    c4.halo = object()
    with pytest.raises(_lib.ChompScopeError, match="halo.Halo"):
        covariance.Covariance(c1, c4, nongaussian_cov=False, ssc_cov=True, cross_terms=True)
    cv = covariance.Covariance(c1, c2, nongaussian_cov=False, ssc_cov=True, cross_terms=True)
    with pytest.raises(_lib.ChompScopeError, match="set_cosmology"):
        cv.set_cosmology({})
    # one correlation given twice: the keyword changes nothing
    cv = covariance.Covariance(c1, c1, nongaussian_cov=False, ssc_cov=True, cross_terms=True)
    assert cv.matching_corrs is True and cv.kernel._four_windows is False
    assert list(cv.equal_windows) == [False, False, False, False, True, True]


def test_four_windows_keyword():
    """KernelCovariance: four different windows are refused without the keyword, before any
    device call, and so are four windows with no redshift in common with it."""
    from chomp_amd import _lib, covariance, cosmology, kernel
    c1, c2 = _corr(0.8), _corr(1.0)
    k1, k2 = c1.kernel, c2.kernel
    args = (1e-8, 1.0, k1.window_function_a, k1.window_function_b, k2.window_function_a,
            k2.window_function_b, k1.cosmo)
    kc = covariance.KernelCovariance(*args)
    assert kc._four_windows is False
    for call in (lambda: kc.z_bar_NG, lambda: kc.raw_kernel_ssc(0.0, 0.0),
                 lambda: kc.kernel_ssc(0.0, 0.0)):
        with pytest.raises(_lib.ChompScopeError, match="four_windows=True"):
            call()
    kc = covariance.KernelCovariance(*args, four_windows=True)
    assert kc._four_windows is True and (kc.z_min, kc.z_max) == (k1.z_min, k1.z_max)
    with pytest.raises(_lib.ChompScopeError):            # the trispectrum kernel stays opt-in
        kc.kernel_NG(0.0, 0.0)
    cm = cosmology.MultiEpoch(0.0, 5.0)
    lo = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 0.5, 0.3, 0.1), cm)
    hi = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.5, 1.5, 1.0, 0.2), cm)
    kc = covariance.KernelCovariance(1e-8, 1.0, lo, lo, hi, hi, cm, four_windows=True)
    assert kc.z_min >= kc.z_max
    for call in (lambda: kc.z_bar_NG, lambda: kc.raw_kernel_ssc(0.0, 0.0)):
        with pytest.raises(_lib.ChompScopeError, match="no redshift in common"):
            call()


def test_covariance_multi_forwards_both_keywords():
    from chomp_amd import _lib, covariance
    c1, c2, tri = _corr(0.8), _corr(1.0), _tri()
    with pytest.raises(_lib.ChompScopeError):            # the reference's defaults: as before
        covariance.CovarianceMulti([c1, c2], input_halo_trispectrum=tri)
    with pytest.raises(_lib.ChompScopeError):
        covariance.CovarianceMulti([c1, c2], nongaussian_cov=False, ssc_cov=True)
    cm = covariance.CovarianceMulti([c1, c2], cross_terms=True, ssc_cov=True,
                                    input_halo_trispectrum=tri)
    assert [len(row) for row in cm.covariance_list] == [2, 1]
    for i, row in enumerate(cm.covariance_list):
        for j, cv in enumerate(row):
            assert cv.nongaussian_cov and cv.ssc_cov and cv.halo_tri is tri
            assert cv.matching_corrs is (j == 0) and cv.kernel._four_windows is (j != 0)
    cm = covariance.CovarianceMulti([c1, c2], nongaussian_cov=False)
    assert not any(cv.ssc_cov or cv.kernel._four_windows for row in cm.covariance_list
                   for cv in row)


def test_exports_and_declarations():
    from chomp_amd import _lib
    names = ("chomp_covariance_cross_range", "chomp_kernel_ssc_setup_cross",
             "chomp_covariance_ssc_cross")
    with open(os.path.join(ROOT, "include", "chomp_mi355x.h")) as f:
        header = f.read()
    for name in names:
        assert name in _lib.EXPORTS
        assert "int %s(chomp_ctx* ctx" % name in header
    assert "#define CHOMP_CROSS_WINDOWS (-1)" in header and _lib.CROSS_WINDOWS == -1
    for method in ("covariance_cross_range", "covariance_ssc_cross"):
        assert callable(getattr(_lib.Context, method))
