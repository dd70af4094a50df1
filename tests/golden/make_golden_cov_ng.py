#!/usr/bin/env python3
"""Generate tests/golden/g25_covariance_ng.npz by RUNNING THE REFERENCE's one-halo trispectrum
term of the covariance of w(theta): Covariance(corr, corr, nongaussian_cov=True,
input_halo_trispectrum=HaloTrispectrumOneHalo(...)) (covariance.py:593-683) on
KernelCovariance.kernel_NG (kernel.py:996-1073, 1103-1111).

Cases: "mag" and "fit" of make_golden_cov_ssc.py with HaloTrispectrumOneHalo(0.0), and "ggmm":
the "mag" correlation with HaloTrispectrumOneHalo(0.5, power_spec='power_ggmm').

Development-container only, like make_golden.py (whose helpers it imports; neither that file nor
make_golden_cov_ssc.py is changed).  Run from anywhere:  python tests/golden/make_golden_cov_ng.py
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
from make_golden_cov_ssc import KWS, correlation, probes  # noqa: E402

warnings.simplefilter("ignore")

CASES = {"mag": ("mag", 0.0, "power_mmmm"), "fit": ("fit", 0.0, "power_mmmm"),
         "ggmm": ("mag", 0.5, "power_ggmm")}


def case(ns, out, tag):
    corr_tag, z_tri, power_spec = CASES[tag]
    corr = correlation(ns, corr_tag)
    with contextlib.redirect_stdout(io.StringIO()):
        tri = ns.halo_trispectrum.HaloTrispectrumOneHalo(z_tri, power_spec=power_spec)
        cv = ns.covariance.Covariance(corr, corr, nongaussian_cov=True,
                                      input_halo_trispectrum=tri, **KWS)
        kc = cv.kernel
        bins = cv.annular_bins
        centers = numpy.array([b.center for b in bins])
        out[tag + "_center"] = centers
        out[tag + "_scalars"] = numpy.array([kc.z_bar_NG, cv.D_z_NG, kc.chi_min, kc.chi_max,
                                             kc.ln_ktheta_min, kc.ln_ktheta_max,
                                             kc._j0_limit, cv.area, z_tri])
        t0 = time.time()
        kc._initialize_NG_spline()
        print("  %s: kernel_NG table %.1f s" % (tag, time.time() - t0))
        out[tag + "_ln_ktheta"] = kc._ln_ktheta_array
        out[tag + "_kernel_array"] = numpy.asarray(kc._kernel_array, dtype=float)
        out[tag + "_kernel_NG_min"] = numpy.array([float(kc._kernel_NG_min)])
        a, b = probes(kc)
        out[tag + "_probe_a"], out[tag + "_probe_b"] = a, b
        out[tag + "_raw"] = numpy.array([float(kc.raw_kernel(x, y)) for x, y in zip(a, b)])
        out[tag + "_spline"] = numpy.array([float(kc.kernel(x, y)[0][0]) for x, y in zip(a, b)])
        t0 = time.time()
        tri._initialize_i_0_4()
        print("  %s: I_0^4 table %.1f s" % (tag, time.time() - t0))
        out[tag + "_i_0_4"] = numpy.asarray(tri._i_0_4_array, dtype=float)
        # one pair's k_b knots (covariance.py:624-639)
        cv._initialize_kb_spline(centers[0], centers[-1])
        out[tag + "_ln_k"] = cv._ln_k_array
        out[tag + "_kb_knots"] = numpy.asarray(cv._kb_spline(cv._ln_k_array), dtype=float)
        nb = len(bins)
        NG = numpy.zeros((nb, nb))
        G = numpy.zeros((nb, nb))
        t0 = time.time()
        for i in range(nb):
            for j in range(i, nb):
                NG[i, j] = NG[j, i] = cv.covariance_NG(centers[i], centers[j])
                G[i, j] = G[j, i] = cv.covariance_G(centers[i], centers[j], bins[i].delta,
                                                    bins[j].delta)
        print("  %s: covariance_NG + G %.1f s" % (tag, time.time() - t0))
        out[tag + "_NG"] = NG
        out[tag + "_G"] = G
        out[tag + "_cov"] = numpy.asarray(cv.get_covariance(), dtype=float)
        if tag == "mag":
            # G + NG + SSC + P: the same trispectrum object beside the super-sample term
            cs = ns.covariance.Covariance(corr, corr, nongaussian_cov=True,
                                          input_halo_trispectrum=tri, ssc_cov=True, **KWS)
            out[tag + "_cov_ssc"] = numpy.asarray(cs.get_covariance(), dtype=float)


def g25(ns):
    out = {}
    for tag in CASES:
        case(ns, out, tag)
    save("g25_covariance_ng", **out)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            t0 = time.time()
            g25(ns)
            print("  g25: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
