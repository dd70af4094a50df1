#!/usr/bin/env python3
"""Generate tests/golden/g20_covariance_ssc.npz by RUNNING THE REFERENCE's super-sample
covariance of w(theta): Covariance(corr, corr, nongaussian_cov=False, ssc_cov=True)
(covariance.py:144-151, 276-335, 685-776) on KernelCovariance.kernel_ssc (kernel.py:961-972,
1113-1231).

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_cov_ssc.py
"""
import contextlib
import io
import os
import sys
import tempfile
import time
import warnings

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402
from make_golden import save  # noqa: E402

warnings.simplefilter("ignore")

deg_to_rad = numpy.pi / 180.0
KWS = dict(bins_per_decade=2.0, survey_area_deg2=25.0, n_a=[1.0e10, 1.0e10],
           n_b=[1.0e10, 1.0e10], variance=1.0)


def correlation(ns, tag):
    """"mag": G12's galaxy x convergence windows on Halo(0.0); "fit": one galaxy window
    used twice on HaloFit(0.0); "zero": one galaxy window that starts at z = 0.5."""
    cm = ns.cosmology.MultiEpoch(0.0, 5.0)
    if tag == "zero":
        wa = ns.kernel.WindowFunctionGalaxy(ns.kernel.dNdzGaussian(0.5, 2.0, 1.0, 0.2), cm)
    else:
        wa = ns.kernel.WindowFunctionGalaxy(ns.kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    wb = wa if tag != "mag" else ns.kernel.WindowFunctionConvergence(
        ns.kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2), cm)
    kern = ns.kernel.Kernel(1e-6 * deg_to_rad, 100.0 * deg_to_rad, wa, wb, cm)
    h = ns.halo.HaloFit(0.0) if tag == "fit" else ns.halo.Halo(0.0)
    return ns.correlation.Correlation(0.01, 1.0, kern, input_halo=h, power_spec="power_mm")


def probes(kc):
    """Off-knot ln(k theta) pairs, with the clamp (<= min) and zero (> max) edges."""
    lo, hi = kc.ln_ktheta_min, kc.ln_ktheta_max
    x = kc._ln_ktheta_array
    mid = 0.5 * (x[:-1] + x[1:])
    a = numpy.concatenate([mid[::7], [lo, lo - 1.0, hi, hi + 1e-9, mid[3], lo - 2.0]])
    b = numpy.concatenate([mid[::-7][:len(mid[::7])], [mid[5], mid[9], hi, mid[2], hi + 1.0,
                                                       lo - 3.0]])
    return a, b


def case(ns, out, tag):
    corr = correlation(ns, tag)
    with contextlib.redirect_stdout(io.StringIO()):
        cv = ns.covariance.Covariance(corr, corr, nongaussian_cov=False, ssc_cov=True, **KWS)
        kc = cv.kernel
        bins = cv.annular_bins
        centers = numpy.array([b.center for b in bins])
        out[tag + "_center"] = centers
        out[tag + "_scalars"] = numpy.array([kc.z_bar_NG, cv.D_z_NG, kc.chi_min, kc.chi_max,
                                             kc.ln_ktheta_min, kc.ln_ktheta_max,
                                             kc._j0_ssc_limit, kc._j1_limit, cv.area])
        t0 = time.time()
        kc._initialize_ssc_spline()
        print("  %s: kernel_ssc table %.1f s" % (tag, time.time() - t0))
        chi = numpy.logspace(numpy.log10(kc.chi_min), numpy.log10(kc.chi_max),
                             ns.defaults.default_precision["corr_npoints"])
        out[tag + "_sigma2_ln_chi"] = numpy.log(chi)
        out[tag + "_sigma2"] = kc._sigma2_spline(numpy.log(chi))
        out[tag + "_ln_ktheta"] = kc._ln_ktheta_array
        out[tag + "_kernel_ssc_array"] = numpy.asarray(kc._kernel_ssc_array, dtype=float)
        a, b = probes(kc)
        out[tag + "_probe_a"], out[tag + "_probe_b"] = a, b
        out[tag + "_raw"] = numpy.array([kc.raw_kernel_ssc(x, y) for x, y in zip(a, b)])
        out[tag + "_spline"] = numpy.array([kc.kernel_ssc(x, y)[0][0] for x, y in zip(a, b)])
        # one pair's k_b knots (covariance.py:723-736)
        cv._initialize_kb_ssc_spline(centers[0], centers[-1])
        out[tag + "_ln_k"] = cv._ln_k_array
        out[tag + "_kb_knots"] = numpy.asarray(cv._kb_ssc_spline(cv._ln_k_array), dtype=float)
        if tag == "zero":
            out[tag + "_ssc"] = numpy.array([cv.covariance_ssc(centers[0], centers[-1])])
            return
        nb = len(bins)
        ssc = numpy.zeros((nb, nb))
        G = numpy.zeros((nb, nb))
        t0 = time.time()
        for i in range(nb):
            for j in range(i, nb):
                ssc[i, j] = ssc[j, i] = cv.covariance_ssc(centers[i], centers[j])
                G[i, j] = G[j, i] = cv.covariance_G(centers[i], centers[j], bins[i].delta,
                                                    bins[j].delta)
        print("  %s: covariance_ssc + G %.1f s" % (tag, time.time() - t0))
        out[tag + "_ssc"] = ssc
        out[tag + "_G"] = G
        out[tag + "_z_bar_G"] = numpy.array([cv._z_bar_G_a, cv._D_z_a])
        out[tag + "_cov"] = numpy.asarray(cv.get_covariance(), dtype=float)


def g20(ns):
    out = {}
    for tag in ("mag", "fit", "zero"):
        case(ns, out, tag)
    save("g20_covariance_ssc", **out)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            t0 = time.time()
            g20(ns)
            print("  g20: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
