"""The super-sample covariance of w(theta) without a device: the reference's fixture G20
(Covariance(corr, corr, nongaussian_cov=False, ssc_cov=True), covariance.py:685-776, on
KernelCovariance.kernel_ssc, kernel.py:961-972, 1113-1231) against an oracle composition
that restates the reference's quirks: the Romberg over ln chi hands ln chi to the integrand
as chi, and the norm takes ln(k theta_a) for k theta_a."""
import warnings

import numpy
import pytest
from scipy import special
from scipy.interpolate import InterpolatedUnivariateSpline, RectBivariateSpline

from conftest import load_golden, rel_err

deg_to_rad = numpy.pi / 180.0
# Romberg levels of the k_b integrals of G20's stored pair, both cases (the oracle's)
KB_LEVELS = numpy.array([20] * 49 + [1])


def oracle_kernel(tag):
    """The windows of G20's case on an oracle MultiEpoch(0, 5)."""
    from oracle import chomp_oracle as o
    me = o.multi_epoch(0.0, 5.0)
    if tag == "zero":
        wa = o.Table(kind="galaxy", dist=o.dndz_gaussian(0.5, 2.0, 1.0, 0.2))
    else:
        wa = o.Table(kind="galaxy", dist=o.dndz_maglim(0.0, 2.0, 2.0, 0.3, 2.0))
    wb = wa if tag != "mag" else o.Table(kind="convergence",
                                         dist=o.dndz_gaussian(0.0, 2.0, 1.0, 0.2))
    return o.kernel_table(1e-6 * deg_to_rad, 100.0 * deg_to_rad, wa, wb, me)


def ng_integrand(kt, chi, kta, ktb):
    """kernel.py:1048-1056 with a1 = b1 = a, a2 = b2 = b."""
    from oracle import chomp_oracle as o
    D = o.me_growth(kt.me, kt.me.z_spline(chi))
    wa, wb = o.window(kt.wa, chi), o.window(kt.wb, chi)
    return wa * wb * wa * wb * D * D * D * D / (chi * chi) * special.j0(kta * chi) * \
        special.j0(ktb * chi)


def ssc_state(kt, ln_kt_min, ln_kt_max):
    """z_bar_NG (kernel.py:961-972), the sigma^2 spline (:1208-1222) and the J0 limit."""
    from oracle import chomp_oracle as o
    p = kt.prec
    z = numpy.linspace(kt.z_min, kt.z_max, p["kernel_npoints"])
    chi = o.me_chi(kt.me, z)
    chi = numpy.where(chi > p["window_precision"], chi, p["window_precision"])
    kt.z_bar_NG = z[numpy.argmax(ng_integrand(kt, chi, 0.0, 0.0))]
    kt.chi_peak_NG = float(o.me_chi(kt.me, kt.z_bar_NG))
    kt.D_z_NG = float(o.me_growth(kt.me, kt.z_bar_NG))
    c = numpy.logspace(numpy.log10(kt.chi_min), numpy.log10(kt.chi_max), p["corr_npoints"])
    sigma = numpy.array([o.sigma_r(kt.me.e0, x) for x in c]) * o.me_growth(kt.me, 0.0)
    kt.sigma2_ln_chi = numpy.log(c)
    kt.sigma2 = sigma * sigma
    kt.sigma2_spline = InterpolatedUnivariateSpline(kt.sigma2_ln_chi, kt.sigma2)
    kt.j0_ssc_limit = special.jn_zeros(0, int(p["kernel_bessel_limit"] * 8))[-1]
    kt.ssc_ln_kt = numpy.linspace(ln_kt_min, ln_kt_max, p["kernel_npoints"])
    return kt


def sigma2(kt, chi):
    with numpy.errstate(invalid="ignore", divide="ignore"):
        return numpy.where((chi >= kt.chi_min) & (chi <= kt.chi_max),
                           kt.sigma2_spline(numpy.log(chi)), 0.0)


def ssc_integrand(x, kt, kta, ktb, norm):
    """kernel.py:1208-1215, called with x = ln chi as chi."""
    from oracle import chomp_oracle as o
    with numpy.errstate(invalid="ignore", divide="ignore"):
        D = o.me_growth(kt.me, kt.me.z_spline(x))
        return (norm * o.window(kt.wa, x) * o.window(kt.wb, x) * o.window(kt.wa, x) *
                o.window(kt.wb, x) * D * D * D * D * D * D * sigma2(kt, x) / x *
                special.j0(kta * x) * special.j0(ktb * x))


def raw_kernel_ssc(kt, la, lb):
    """kernel.py:1155-1206 -> (value, Romberg level; level 0 where the range is empty)."""
    from oracle.romberg import AccuracyWarning, romberg
    p = kt.prec
    kta, ktb = numpy.exp(la), numpy.exp(lb)
    chi_max = numpy.max([kt.j0_ssc_limit / kta, kt.j0_ssc_limit / ktb])
    if chi_max >= kt.chi_max:
        chi_max = kt.chi_max
    elif chi_max <= kt.chi_min:
        return 0.0, 0
    inv = ng_integrand(kt, kt.chi_peak_NG, la, la)
    norm = 1.0 / inv if (inv > 1e-16 or inv < -1e-16) else 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", AccuracyWarning)
        v, level = romberg(ssc_integrand, numpy.log(kt.chi_min), numpy.log(chi_max),
                           args=(kt, kta, ktb, norm), vec_func=True,
                           tol=p["global_precision"], rtol=p["kernel_precision"],
                           divmax=p["divmax"], return_level=True)
    return v * (16.0 * numpy.pi * numpy.pi / 9.0) / norm, level


def kernel_ssc_spline(ln_kt, table):
    """kernel.py:1113-1153: RectBivariateSpline(s=0) with the clamp and zero rules."""
    spl = RectBivariateSpline(ln_kt, ln_kt, table)
    lo, hi = ln_kt[0], ln_kt[-1]

    def f(a, b):
        a = numpy.where(a <= lo, lo, a)
        b = numpy.where(b <= lo, lo, b)
        return numpy.where(numpy.logical_and(a <= hi, b <= hi), spl(a, b), 0.0)
    return f


def kb_knots(kernel, resp, theta_a, theta_b, prec, k_min, k_max):
    """covariance.py:723-776: the k_b integral at each k_a knot, norm = 1."""
    from oracle.romberg import romberg
    ln_k = numpy.linspace(numpy.log(k_min), numpy.log(k_max), prec["kernel_npoints"])

    def integrand(ln_kb, ln_ka):
        ka, kb = numpy.exp(ln_ka), numpy.exp(ln_kb)
        return (kb * 1.0 * kb * 1.0 * resp(ka) * resp(kb) *
                kernel(numpy.log(ka * theta_a), numpy.log(kb * theta_b))[0])
    out, lev = [], []
    for x in ln_k:
        v, level = romberg(integrand, ln_k[0], ln_k[-1], args=(x,), vec_func=True,
                           tol=prec["global_precision"], rtol=prec["corr_precision"],
                           divmax=prec["divmax"], return_level=True)
        out.append(float(numpy.ravel(v)[0]))
        lev.append(level)
    return ln_k, numpy.array(out), numpy.array(lev)


def covariance_ssc(ln_k, knots, area, prec):
    """covariance.py:694-721."""
    from oracle.romberg import AccuracyWarning, romberg
    spl = InterpolatedUnivariateSpline(ln_k, knots)

    def f(ln_ka, norm):
        ka = numpy.exp(ln_ka)
        return ka * 1.0 * ka * spl(ln_ka) * norm
    with numpy.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", AccuracyWarning)
        norm = 1.0 / f(0.0, 1.0)
        v = romberg(f, ln_k[0], ln_k[-1], args=(norm,), vec_func=True,
                    tol=prec["global_precision"], rtol=prec["corr_precision"],
                    divmax=prec["divmax"]) / (4.0 * numpy.pi * numpy.pi * norm * area)
    return float(numpy.ravel(v)[0])


def oracle_response(z):
    """dln_power_ddelta_b of a default HaloSuperSampleCovariance at z (halo.py:1136-1156)."""
    from oracle import chomp_oracle as o
    from test_ssc_cpu import ssc_response, ssc_table
    e = o.epoch(None, z)
    t = ssc_table(o.halo_table(e, o.mass_table(e)))
    return lambda k: ssc_response(t, k)


def case_state(tag, g):
    sc = g[tag + "_scalars"]
    return ssc_state(oracle_kernel(tag), sc[4], sc[5])


@pytest.mark.parametrize("tag", ["mag", "fit", "zero"])
def test_g20_kernel_against_oracle_composition(tag):
    g = load_golden("g20_covariance_ssc")
    kt = case_state(tag, g)
    sc = g[tag + "_scalars"]
    assert kt.z_bar_NG == sc[0]
    assert abs(kt.D_z_NG / sc[1] - 1.0) < 1e-12
    assert abs(kt.chi_min / sc[2] - 1.0) < 1e-12 and abs(kt.chi_max / sc[3] - 1.0) < 1e-12
    assert kt.j0_ssc_limit == sc[6]
    assert numpy.array_equal(kt.ssc_ln_kt, g[tag + "_ln_ktheta"])
    assert numpy.array_equal(kt.sigma2_ln_chi, g[tag + "_sigma2_ln_chi"])
    assert rel_err(kt.sigma2, g[tag + "_sigma2"]) < 1e-10
    tab = g[tag + "_kernel_ssc_array"]
    assert numpy.array_equal(tab, tab.T)
    if tag == "zero":
        # windows from z = 0.5: sigma^2(ln chi) is 0 over the whole range, every knot is 0
        assert numpy.all(tab == 0.0)
    scale = numpy.max(numpy.abs(tab)) if numpy.any(tab) else 1.0
    for i in (0, 17, 49):
        for j in (i, 30, 49):
            if j < i:
                continue
            v, _ = raw_kernel_ssc(kt, kt.ssc_ln_kt[i], kt.ssc_ln_kt[j])
            assert abs(v - tab[i, j]) <= 1e-10 * scale, (i, j)
    a, b = g[tag + "_probe_a"], g[tag + "_probe_b"]
    raw = numpy.array([raw_kernel_ssc(kt, x, y)[0] for x, y in zip(a, b)])
    assert numpy.max(numpy.abs(raw - g[tag + "_raw"])) <= 1e-10 * scale
    spl = kernel_ssc_spline(kt.ssc_ln_kt, tab)
    got = numpy.array([spl(x, y)[0][0] for x, y in zip(a, b)])
    assert numpy.max(numpy.abs(got - g[tag + "_spline"])) <= 1e-12 * scale
    # the clamp (<= min) and zero (> max) edges are among the probes
    assert numpy.any(a < kt.ssc_ln_kt[0]) and numpy.any(b > kt.ssc_ln_kt[-1])


@pytest.mark.parametrize("tag", ["mag", "fit"])
def test_g20_covariance_ssc_against_oracle_composition(tag):
    from oracle.chomp_oracle import default_precision as prec
    g = load_golden("g20_covariance_ssc")
    ln_kt = g[tag + "_ln_ktheta"]
    kernel = kernel_ssc_spline(ln_kt, g[tag + "_kernel_ssc_array"])
    resp = oracle_response(float(g[tag + "_z_bar_G"][0]))
    c = g[tag + "_center"]
    area = g[tag + "_scalars"][8]
    ln_k, knots, lev = kb_knots(kernel, resp, c[0], c[-1], prec, 0.001, 100.0)
    ref = g[tag + "_kb_knots"]
    assert numpy.array_equal(ln_k, g[tag + "_ln_k"])
    assert numpy.max(numpy.abs(knots - ref)) <= 1e-9 * numpy.max(numpy.abs(ref))
    # the k_b Romberg runs to divmax at every k_a knot but the last, where k_a = exp(ln k_max)
    # rounds above k_max: R(k_a) = 0, the integrand is 0 and the first row stops it
    assert numpy.array_equal(lev, KB_LEVELS)
    assert ref[-1] == 0.0 and knots[-1] == 0.0
    ssc = covariance_ssc(ln_k, knots, area, prec)
    assert abs(ssc / g[tag + "_ssc"][0, -1] - 1.0) < 1e-8
    # get_covariance = G + SSC (+ P on the diagonal)
    cov = g[tag + "_cov"]
    off = ~numpy.eye(len(c), dtype=bool)
    assert rel_err((g[tag + "_G"] + g[tag + "_ssc"])[off], cov[off]) < 1e-14


def test_g20_all_zero_knots_give_nan():
    """covariance.py:694-721 with every k_b knot 0: norm = 1/0 and the reference returns NaN."""
    from oracle.chomp_oracle import default_precision as prec
    g = load_golden("g20_covariance_ssc")
    assert numpy.all(g["zero_kb_knots"] == 0.0)
    assert numpy.isnan(g["zero_ssc"][0])
    ln_k = g["zero_ln_k"]
    assert numpy.isnan(covariance_ssc(ln_k, numpy.zeros_like(ln_k), 1.0, prec))
