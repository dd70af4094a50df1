#!/usr/bin/env python3
"""Generate tests/golden/g21_hod_mandelbaum.npz by RUNNING THE REFERENCE's
hod.HODMandelbaum (hod.py:232-299) through halo.Halo and correlation.Correlation.

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_hod.py

Besides the tables, every Romberg call of the halo integrals is wrapped to record its
stopping level (nodes = 2**level + 1, oracle/romberg.py's numbering), per knot.
"""
import os
import sys
import tempfile
import time
import warnings

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402
from make_golden import _projection, deg_to_rad, save  # noqa: E402
from params import c_dict_2, h_dict_2  # noqa: E402

warnings.simplefilter("ignore")

# (log_M_0 = 6 lies below the mass function's mass_min at z = 0: the central term is always on)
CASES = (("z000_", 0.0, {"log_M_0": 12.14, "w": 1.0}, False),
         ("z050_", 0.5, {"log_M_0": 12.14, "w": 1.0}, False),
         ("alt_", 0.3, {"log_M_0": 12.8, "w": 0.5}, True),
         ("low_", 0.0, {"log_M_0": 6.0, "w": 1.0}, False))
INTEGRANDS = ("_nbar_integrand", "_h_g_integrand", "_pp_gm_integrand", "_pp_gg_integrand")


class LevelLog(object):
    """Wraps integrate.romberg as the reference's halo module sees it: the level of every call,
    by integrand name."""

    def __init__(self, integrate):
        from oracle.romberg import romberg
        self.integrate, self.romberg, self.orig = integrate, romberg, integrate.romberg
        self.levels = {}

    def __enter__(self):
        def wrapped(function, a, b, **kws):
            val, level = self.romberg(function, a, b, return_level=True, **kws)
            self.levels.setdefault(function.__name__, []).append(level)
            return val
        self.integrate.romberg = wrapped
        return self

    def __exit__(self, *exc):
        self.integrate.romberg = self.orig


def k_samples(k_min, k_max):
    """k = logspace(-4, 3, 64) plus the range ends and their neighbours at 1e-9."""
    edges = [k_min * (1 - 1e-9), k_min, k_min * (1 + 1e-9),
             k_max * (1 - 1e-9), k_max, k_max * (1 + 1e-9)]
    return numpy.concatenate([numpy.logspace(-4, 3, 64), edges])


def mass_grid(hod):
    """The moments' masses: a log grid and the two thresholds with their neighbours."""
    edges = []
    for lm in (hod.log_M_0, hod.log_M_min):
        m = 10.0 ** lm
        edges += [numpy.nextafter(m, 0.0), m, numpy.nextafter(m, numpy.inf)]
    return numpy.concatenate([numpy.logspace(5, 17, 121), edges])


def g21(ns):
    d = ns.defaults
    k = k_samples(d.default_limits["k_min"], d.default_limits["k_max"])
    out = {"k": k, "log10_3": numpy.log10(3.0)}
    for tag, z, hd, alt in CASES:
        hod = ns.hod.HODMandelbaum(dict(hd))
        with LevelLog(ns.halo.integrate) as log:
            if alt:
                cosmo = ns.cosmology.SingleEpoch(z, c_dict_2)
                mass = ns.mass_function.TinkerMassFunction(z, cosmo, h_dict_2)
                h = ns.halo.Halo(z, hod, cosmo, mass, h_dict_2)
            else:
                h = ns.halo.Halo(z, hod)
            lk = h._ln_k_array
            out[tag + "pp_gm_k"] = h.power_gm(k)
            out[tag + "pp_gg_k"] = h.power_gg(k)
            out[tag + "h_g"] = h._h_g_spline(lk)
            out[tag + "pp_gm"] = h._pp_gm_spline(lk)
            out[tag + "pp_gg"] = h._pp_gg_spline(lk)
            out[tag + "n_bar"] = h.n_bar
            h.calculate_bias()
            h.calculate_m_eff()
            h.calculate_f_sat()
            out[tag + "bias"], out[tag + "m_eff"], out[tag + "f_sat"] = h.bias, h.m_eff, h.f_sat
        for name in INTEGRANDS:
            out[tag + "levels" + name] = numpy.array(log.levels[name])
        out[tag + "ln_k"] = lk
        out[tag + "mass_min"] = numpy.exp(h.mass.ln_mass_min)
        out[tag + "log_M_0"] = hod.log_M_0
        out[tag + "log_M_min"] = hod.log_M_min
        out[tag + "w"] = hod.w
        m = mass_grid(hod)
        out[tag + "mass"] = m
        out[tag + "first"] = hod.first_moment(m, z)
        out[tag + "second"] = hod.second_moment(m, z)
        out[tag + "central"] = hod.central_first_moment(m, z)
        out[tag + "satellite"] = hod.satellite_first_moment(m, z)
    assert out["low_mass_min"] > 10.0 ** out["low_log_M_0"]
    # w(theta) over the first case's HOD: galaxy x galaxy (power_gg) and GGL (power_gm)
    theta = numpy.logspace(-3, 0, 33) * deg_to_rad
    out["theta"] = theta
    for ps, ggl in (("power_gg", False), ("power_gm", True)):
        cm, kern = _projection(ns, ggl=ggl)
        h = ns.halo.Halo(0.0, ns.hod.HODMandelbaum({"log_M_0": 12.14, "w": 1.0}))
        corr = ns.correlation.Correlation(0.001, 1.0, kern, input_halo=h, power_spec=ps)
        out["w_" + ps] = corr.correlation(theta)
    save("g21_hod_mandelbaum", **out)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            t0 = time.time()
            g21(ns)
            print("  g21: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
