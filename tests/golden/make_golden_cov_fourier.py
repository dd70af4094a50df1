#!/usr/bin/env python3
"""Generate tests/golden/g31_covariance_fourier.npz by RUNNING THE REFERENCE's
covariance.CovarianceFourier (covariance.py:874-1083): the Gaussian covariance of C_l.

Three cases, all on MultiEpoch(0, 5), KernelCovariance(1e-3, 1e2, ...), Halo(0.0), l from 10 to
1e4, at the defaults:

  auto   one convergence window four times                      as shipped
  mix    a1 = b1 a galaxy window, a2 = b2 that convergence one   as shipped
  tomo   a1 = a2 and b1 = b2 two different galaxy bins           WITH ``copy`` REPLACED

As shipped the four halo objects of a CovarianceFourier are ``copy(input_halo)`` (:917-920):
shallow copies that share one MassFunction, which every set_redshift moves (halo.py:159).  When
the four z_bar differ each halo integrates its tables with the mass function of the last redshift
set.  FOR THE CASE ``tomo`` ALONE THIS SCRIPT REPLACES THE NAME ``copy`` IN THE LOADED covariance
MODULE BY ``copy.deepcopy``, in this process only, so that the four halos are independent; the
as-shipped covariance_G of that case is stored beside it for the record (``tomo_G_shallow``).
Where the four z_bar coincide (auto, mix) the two variants agree bit for bit.  Everything else
runs as shipped.

The z_bar of every pair of every case must not hang on rounding: the largest value of the z_bar
function has to exceed the runner-up by 1e-6 relative, or the script stops.

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_cov_fourier.py
"""
import contextlib
import copy as copy_mod
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

PAIRS = ("a1a2", "b1b2", "a1b2", "b1a2")
L_MIN, L_MAX = 10.0, 1.0e4


def windows(ns, tag):
    """(a1, a2, b1, b2) of a case and its MultiEpoch."""
    cm = ns.cosmology.MultiEpoch(0.0, 5.0)
    K = ns.kernel
    conv = lambda: K.WindowFunctionConvergence(K.dNdzGaussian(0.0, 2.0, 1.0, 0.2), cm)
    if tag == "auto":
        w = conv()
        return (w, w, w, w), cm
    if tag == "mix":
        g = K.WindowFunctionGalaxy(K.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
        c = conv()
        return (g, c, g, c), cm
    a = K.WindowFunctionGalaxy(K.dNdzGaussian(0.5, 1.5, 1.0, 0.2), cm)
    b = K.WindowFunctionGalaxy(K.dNdzGaussian(0.2, 1.0, 0.6, 0.15), cm)
    return (a, a, b, b), cm


def multipoles(cf):
    """About 25 multipoles: log-spaced inside the range, both ends, one just outside each end."""
    inside = numpy.exp(numpy.linspace(cf._ln_l_min, cf._ln_l_max, 25)[1:-1])
    return numpy.concatenate([[L_MIN * (1.0 - 1e-9), L_MIN], inside,
                              [L_MAX, L_MAX * (1.0 + 1e-9)]])


def build(ns, tag):
    ws, cm = windows(ns, tag)
    kc = ns.kernel.KernelCovariance(1e-3, 1e2, ws[0], ws[1], ws[2], ws[3], cm)
    return ns.covariance.CovarianceFourier(L_MIN, L_MAX, input_kernel_covariance=kc,
                                           input_halo=ns.halo.Halo(0.0))


def check_zbar_margin(cf, tag):
    """The argmax of every pair's z_bar function is decided by more than rounding."""
    chi = cf.kernel.cosmo.comoving_distance(cf._z_array)
    wins = {"a1": cf.window_a1, "a2": cf.window_a2, "b1": cf.window_b1, "b2": cf.window_b2}
    for p in PAIRS:
        D = cf.kernel.cosmo.growth_factor(cf.kernel.cosmo.redshift(chi))
        f = wins[p[:2]](chi) * wins[p[2:]](chi) / (chi * chi) * D * D
        assert numpy.all(numpy.isfinite(f)), (tag, p)
        top = numpy.sort(f)[::-1]
        assert top[0] > 0.0 and top[0] - top[1] >= 1e-6 * top[0], (tag, p, top[:2])


def case(ns, out, tag):
    t0 = time.time()
    with contextlib.redirect_stdout(io.StringIO()):
        cf = build(ns, tag)
        check_zbar_margin(cf, tag)
        ell = multipoles(cf)
        G = numpy.asarray(cf.covariance_G(ell), dtype=float)
    assert cf.covariance(10.0, 10.0) is None
    out[tag + "_ln_l"] = numpy.asarray(cf._ln_l_array, dtype=float)
    out[tag + "_z_array"] = numpy.asarray(cf._z_array, dtype=float)
    out[tag + "_z_lim"] = numpy.array(
        [getattr(cf, "_z_min_" + p) for p in PAIRS] + [getattr(cf, "_z_max_" + p) for p in PAIRS],
        dtype=float)
    out[tag + "_z_bar"] = numpy.array([getattr(cf, "_z_bar_G_" + p) for p in PAIRS], dtype=float)
    out[tag + "_norm"] = numpy.array([getattr(cf, "_norm_G_" + p) for p in PAIRS], dtype=float)
    out[tag + "_D"] = numpy.array([cf.kernel.cosmo.growth_factor(z) for z in out[tag + "_z_bar"]],
                                  dtype=float)
    # the knot tables: the stored splines at their knots, exponentiated (integral / D^2)
    out[tag + "_tables"] = numpy.array(
        [numpy.exp(getattr(cf, "_%s_spline" % p)(cf._ln_l_array)) for p in PAIRS], dtype=float)
    out[tag + "_ell"] = ell
    out[tag + "_pl"] = numpy.array([getattr(cf, "_pl_" + p)(ell) for p in PAIRS], dtype=float)
    out[tag + "_G"] = G
    out[tag + "_halo_redshift"] = numpy.array([cf.halo_a1a2.get_redshift()], dtype=float)
    for k in ("_norm", "_D", "_tables", "_pl", "_G"):
        assert numpy.all(numpy.isfinite(out[tag + k])), (tag, k)
    print("  %s: %.1f s; z_bar %s" % (tag, time.time() - t0, out[tag + "_z_bar"]))
    return ell


def g31(ns):
    out = {}
    case(ns, out, "auto")
    case(ns, out, "mix")
    assert len(set(out["auto_z_bar"])) == 1 and len(set(out["mix_z_bar"])) == 1
    # tomo: four different z_bar.  First as shipped (shallow copies), for the record only ...
    with contextlib.redirect_stdout(io.StringIO()):
        cf = build(ns, "tomo")
        shallow = numpy.asarray(cf.covariance_G(multipoles(cf)), dtype=float)
    # ... then with four independent halos: THE ONE REPLACEMENT (see the module docstring)
    shipped = ns.covariance.copy
    ns.covariance.copy = copy_mod.deepcopy
    try:
        case(ns, out, "tomo")
    finally:
        ns.covariance.copy = shipped
    out["tomo_G_shallow"] = shallow
    inside = out["tomo_G"] != 0.0
    dev = numpy.abs(shallow[inside] / out["tomo_G"][inside] - 1.0)
    print("  tomo: shallow / deep copies differ by up to %.3g (at l = %.4g)"
          % (dev.max(), out["tomo_ell"][inside][numpy.argmax(dev)]))
    save("g31_covariance_fourier", **out)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            t0 = time.time()
            g31(ns)
            print("  g31: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
