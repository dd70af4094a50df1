#!/usr/bin/env python3
"""Generate tests/golden/g29_covariance_cross.npz by RUNNING THE REFERENCE's cross-covariance of
two w(theta) measurements: Covariance(corr_a, corr_b, nongaussian_cov=False) with two different
correlation objects (the matching_corrs == False branch: covariance.py:422-453, 495-541) and
CovarianceMulti (covariance.py:796-871).

As shipped the reference cannot construct such a Covariance: its constructor compares the two
correlations with Correlation.__eq__ (correlation.py:119-131), a comparison of attribute
dictionaries that raises ValueError on the numpy arrays in them.  THIS SCRIPT REPLACES THAT ONE
METHOD WITH IDENTITY (``lambda s, o: s is o``) on the loaded class, in this process only -- for
two objects the comparison could return nothing but False -- and everything else runs as
shipped.

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_cov_cross.py
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


def correlations(ns, tag):
    """"gal": two galaxy windows, each used twice, each correlation on its own Halo(0.0);
    "mix": galaxy x convergence (G12's windows) and the auto-correlation of a galaxy window on
    z = 0.5-1.5, both on ONE Halo object."""
    cm = ns.cosmology.MultiEpoch(0.0, 5.0)
    K = ns.kernel

    def corr(wa, wb, h):
        kern = K.Kernel(1e-6 * deg_to_rad, 100.0 * deg_to_rad, wa, wb, cm)
        return ns.correlation.Correlation(0.01, 1.0, kern, input_halo=h, power_spec="power_mm")
    if tag == "gal":
        w1 = K.WindowFunctionGalaxy(K.dNdzGaussian(0.0, 2.0, 0.8, 0.2), cm)
        w2 = K.WindowFunctionGalaxy(K.dNdzGaussian(0.0, 2.0, 1.0, 0.2), cm)
        return corr(w1, w1, ns.halo.Halo(0.0)), corr(w2, w2, ns.halo.Halo(0.0))
    h = ns.halo.Halo(0.0)
    wa = K.WindowFunctionGalaxy(K.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    wb = K.WindowFunctionConvergence(K.dNdzGaussian(0.0, 2.0, 1.0, 0.2), cm)
    wc = K.WindowFunctionGalaxy(K.dNdzGaussian(0.5, 1.5, 1.0, 0.2), cm)
    return corr(wa, wb, h), corr(wc, wc, h)


def case(ns, out, tag, ca, cb):
    with contextlib.redirect_stdout(io.StringIO()):
        cv = ns.covariance.Covariance(ca, cb, nongaussian_cov=False, **KWS)
        assert cv.matching_corrs is False
        bins = cv.annular_bins
        out[tag + "_center"] = numpy.array([b.center for b in bins])
        out[tag + "_inner"] = numpy.array([b.inner for b in bins])
        out[tag + "_equal_windows"] = numpy.array(cv.equal_windows, dtype=bool)
        out[tag + "_cosmic_shear"] = numpy.array([bool(x) for x in cv.cosmic_shear])
        t0 = time.time()
        cv._initialize_halo_splines()
        dt = time.time() - t0
        x = cv._ln_K_array
        out[tag + "_ln_K"] = numpy.asarray(x, dtype=float)
        for name in ("a", "b", "ab", "ba"):
            out[tag + "_" + name] = numpy.asarray(
                getattr(cv, "_halo_%s_spline" % name)(x), dtype=float)
        cosmo = cv.kernel.cosmo
        # z_bar a, b; D a, b; chi_peak a, b; chi_min/max a; chi_min/max b; ln_K_min/max; j0; area
        out[tag + "_scalars"] = numpy.array([
            cv._z_bar_G_a, cv._z_bar_G_b, cv._D_z_a, cv._D_z_b,
            cosmo.comoving_distance(cv._D_z_a), cosmo.comoving_distance(cv._D_z_b),
            cv._chi_min_a, cv._chi_max_a, cv._chi_min_b, cv._chi_max_b,
            cv._ln_K_min, cv._ln_K_max, cv._j0_limit, cv.area], dtype=float)
        nb = len(bins)
        G = numpy.zeros((nb, nb))
        t1 = time.time()
        for i in range(nb):
            for j in range(i, nb):
                G[i, j] = G[j, i] = cv.covariance_G(bins[i].center, bins[j].center,
                                                    bins[i].delta, bins[j].delta)
        out[tag + "_G"] = G
        out[tag + "_cov"] = numpy.asarray(cv.get_covariance(), dtype=float)
    print("  %s: tables %.1f s, covariance_G %.1f s" % (tag, dt, time.time() - t1))


def multi(ns, out, ca, cb):
    with contextlib.redirect_stdout(io.StringIO()):
        cm = ns.covariance.CovarianceMulti([ca, cb], nongaussian_cov=False, **KWS)
        out["multi_wcovar"] = numpy.asarray(cm.get_covariance(), dtype=float)
        out["multi_theta_bins"] = numpy.array([cm.theta_bins])
        for i, row in enumerate(cm.covariance_list):
            for j, cv in enumerate(row):
                out["multi_block_%d_%d" % (i, i + j)] = numpy.asarray(cv.covar, dtype=float)


def g29(ns):
    ns.correlation.Correlation.__eq__ = lambda s, o: s is o
    out = {}
    ca, cb = correlations(ns, "gal")
    case(ns, out, "gal", ca, cb)
    t0 = time.time()
    multi(ns, out, ca, cb)
    print("  multi: %.1f s" % (time.time() - t0))
    ca, cb = correlations(ns, "mix")
    case(ns, out, "mix", ca, cb)
    save("g29_covariance_cross", **out)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            t0 = time.time()
            g29(ns)
            print("  g29: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
