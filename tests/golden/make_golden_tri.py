#!/usr/bin/env python3
"""Generate tests/golden/g26_trispectrum.npz by RUNNING THE REFERENCE's
halo_trispectrum.HaloTrispectrum (halo_trispectrum.py:153-837).

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_tri.py

Three cases:

  a_  z = 0, the defaults, MassFunctionSecondOrder, PerturbationTheory();
  b_  z = 0.5, the default PerturbationTheory() left at its own cosmology and redshift
      (the constructor never aligns it: the PT terms are those of z = 0);
  c_  h_dict_2 at z = 0.3, then set_cosmology(c_dict_2), which realigns the PT object.

Per case: the five mass-integral tables (upper triangles, row-major, i <= j; _i_2_1 whole),
the Romberg level of every one of their integrals (make_golden_hod.LevelLog), rho_bar, the
four terms at the (k1, k2, z) configurations, tri_spec_proj_integral at the pairs with its
levels, and i_1_3 at a few triples.  The points where the reference raises ZeroDivisionError
(k1 = k2 with z = +1) are not among the configurations.
"""
import os
import sys
import tempfile
import time
import warnings

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_loader  # noqa: E402
from make_golden import save  # noqa: E402
from make_golden_hod import LevelLog  # noqa: E402
from params import c_dict_2, h_dict_2  # noqa: E402

warnings.simplefilter("ignore")

TABLES = ("i_0_4", "i_1_2", "i_1_3", "i_2_1", "i_2_2")


def configurations(k_min, k_max):
    """(k1, k2, z): inside the range, below k_min, above k_max, at the range ends, z = 0,
    z = +-0.999, k1 = k2 with |z| < 1, and (1, 1, -1)."""
    c = [(0.1, 1.0, 0.3), (1.0, 0.1, 0.3), (0.01, 10.0, -0.5), (10.0, 0.01, 0.7),
         (0.5, 2.0, 0.0), (2.0, 0.5, 0.0), (0.05, 0.2, 0.999), (0.05, 0.2, -0.999),
         (3.0, 30.0, 0.999), (3.0, 30.0, -0.999), (0.02, 0.03, 0.25), (7.0, 0.3, -0.8),
         (0.3, 0.3, 0.5), (1.0, 1.0, 0.0), (1.0, 1.0, -0.4), (5.0, 5.0, 0.9),
         (0.01, 0.01, -0.999), (1.0, 1.0, -1.0), (0.2, 0.2, 0.999),
         (5e-4, 1.0, 0.3), (1.0, 5e-4, -0.3), (5e-4, 2e-4, 0.1), (150.0, 1.0, 0.3),
         (1.0, 150.0, -0.3), (150.0, 200.0, 0.2), (5e-4, 150.0, 0.6),
         (k_min, 1.0, 0.3), (k_min * (1 - 1e-9), 1.0, 0.3), (k_min * (1 + 1e-9), 1.0, 0.3),
         (1.0, k_max, 0.3), (1.0, k_max * (1 - 1e-9), 0.3), (1.0, k_max * (1 + 1e-9), 0.3),
         (k_min, k_max, -0.2), (k_max, k_min, 0.2), (k_min, k_min, 0.5), (k_max, k_max, -0.5),
         (0.1, 1.0, 1.0), (0.1, 1.0, -1.0), (20.0, 0.7, 1.0), (0.004, 0.06, -1.0),
         (50.0, 80.0, 0.45), (0.0015, 90.0, -0.95)]
    return numpy.array(c)


def proj_pairs():
    """tri_spec_proj_integral: k1 != k2 (finite) and, last, two with k1 = k2 (NaN)."""
    p = [(0.1, 1.0), (1.0, 0.1), (0.01, 10.0), (0.5, 2.0), (0.02, 0.03), (3.0, 30.0),
         (0.05, 0.2), (7.0, 0.3), (5e-4, 1.0), (1.0, 150.0), (0.001, 100.0), (0.3, 0.31),
         (1.0, 1.0), (0.05, 0.05)]
    return numpy.array(p)


def triples():
    return numpy.array([(0.1, 0.1, 1.0), (0.1, 1.0, 0.1), (0.02, 0.5, 7.0), (1.0, 1.0, 1.0),
                        (30.0, 0.3, 0.3), (0.001, 0.001, 100.0)])


def f0(x):
    return float(numpy.ravel(x)[0])


def triu(a):
    return a[numpy.triu_indices(a.shape[0])]


class TableLog(object):
    """Records the array each _initialize_* hands to its spline constructor (the reference keeps
    the tables in local variables)."""

    def __init__(self, module):
        self.module, self.arrays = module, []
        self.orig = (module.RectBivariateSpline, module.InterpolatedUnivariateSpline)

    def __enter__(self):
        rect, uni = self.orig

        def rect_logged(x, y, z, *a, **k):
            self.arrays.append(numpy.array(z))
            return rect(x, y, z, *a, **k)

        def uni_logged(x, y, *a, **k):
            self.arrays.append(numpy.array(y))
            return uni(x, y, *a, **k)
        self.module.RectBivariateSpline = rect_logged
        self.module.InterpolatedUnivariateSpline = uni_logged
        return self

    def __exit__(self, *exc):
        self.module.RectBivariateSpline, self.module.InterpolatedUnivariateSpline = self.orig


def grab(ns, out, tag, h, cfg, pairs, trip):
    with LevelLog(ns.halo_trispectrum.integrate) as log:
        t0 = time.time()
        with TableLog(ns.halo_trispectrum) as tl:
            h._initialize_i_0_4()
            h._initialize_i_1_2()
            h._initialize_i_1_3()
            h._initialize_i_2_1()
            h._initialize_i_2_2()
        print("  %s tables: %.1f s" % (tag, time.time() - t0))
        for name, a in zip(TABLES, tl.arrays):
            out[tag + name] = triu(a) if a.ndim == 2 else a
            lev = numpy.array(log.levels["_%s_integrand" % name])
            assert lev.size == out[tag + name].size
            out[tag + name + "_levels"] = lev
        terms = numpy.empty((cfg.shape[0], 4))
        for n, (k1, k2, z) in enumerate(cfg):
            k1, k2, z = numpy.float64(k1), numpy.float64(k2), numpy.float64(z)
            terms[n] = (f0(h.t_1_h(k1, k2)), f0(h.t_2_h(k1, k2, z)), f0(h.t_3_h(k1, k2, z)),
                        f0(h.t_4_h(k1, k2, z)))
        out[tag + "terms"] = terms
        out[tag + "t_pt"] = numpy.array([f0(h.t_PT(*[numpy.float64(x) for x in c])) for c in cfg])
        out[tag + "h_m"] = numpy.array([f0(h._h_m(numpy.float64(k))) for k in cfg[:, 0]])
        out[tag + "p_lin"] = numpy.array([f0(h.linear_power(numpy.float64(k))) for k in cfg[:, 0]])
        out[tag + "lookups"] = numpy.array(
            [[f0(v) for v in (h.i_1_2(a, b), h.i_1_3_parallelogram(a, b),
                              h.i_1_3_parallelogram(b, a), h.i_2_2(a, b), h.i_2_1(a), h.i_2_1(b))]
             for a, b in cfg[:, :2]])
        log.levels["_i_1_3_integrand"] = []
        out[tag + "i_1_3_triples"] = numpy.array([f0(h.i_1_3(*t)) for t in trip])
        out[tag + "i_1_3_triples_levels"] = numpy.array(log.levels["_i_1_3_integrand"])
        t0 = time.time()
        log.levels["_trispectrum_parallelogram_wrap"] = []
        out[tag + "proj"] = numpy.array(
            [f0(h.tri_spec_proj_integral(numpy.float64(a), numpy.float64(b))) for a, b in pairs])
        out[tag + "proj_levels"] = numpy.array(log.levels["_trispectrum_parallelogram_wrap"])
        print("  %s proj: %.1f s" % (tag, time.time() - t0))
    out[tag + "rho_bar"] = h.rho_bar
    out[tag + "redshift"] = h._redshift
    out[tag + "pert_redshift"] = h.pert._redshift


def g26(ns):
    d = ns.defaults
    k_min, k_max = d.default_limits["k_min"], d.default_limits["k_max"]
    cfg, pairs, trip = configurations(k_min, k_max), proj_pairs(), triples()
    out = {"configs": cfg, "pairs": pairs, "triples": trip}
    HT = ns.halo_trispectrum.HaloTrispectrum
    MF = ns.mass_function.MassFunctionSecondOrder
    for tag, z in (("a_", 0.0), ("b_", 0.5)):
        cosmo = ns.cosmology.SingleEpoch(z)
        h = HT(z, cosmo, MF(z, cosmo))
        grab(ns, out, tag, h, cfg, pairs, trip)
        out[tag + "ln_k"] = h._ln_k_array
    z = 0.3
    cosmo = ns.cosmology.SingleEpoch(z)
    h = HT(z, cosmo, MF(z, cosmo, h_dict_2), None, h_dict_2)
    h.t_1_h(1.0, 1.0)
    h.set_cosmology(c_dict_2)
    out["c_flags_after_set"] = numpy.array(
        [int(getattr(h, "_initialized_%s" % n)) for n in TABLES])
    grab(ns, out, "c_", h, cfg, pairs, trip)
    save("g26_trispectrum", **out)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            t0 = time.time()
            g26(ns)
            print("  g26: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
