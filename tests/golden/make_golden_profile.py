#!/usr/bin/env python3
"""Generate tests/golden/g28_halo_profile.npz by RUNNING THE REFERENCE's halo model with a
general inner slope, halo_dict["alpha"] != -1 (y_general, halo.py:491-559).

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_profile.py

Per case: the 50 x 50 table y[k][M] the reference builds one ln k at a time
(_initialize_y_spline) with the Romberg stopping level of each of its integrals, the profile
look-ups at the knots and off them, the five knot tables with their levels, and the spectra.
Numbers only; takes a few minutes.
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
from make_golden import save  # noqa: E402
from make_golden_hod import LevelLog  # noqa: E402
from params import c_dict_2, h_dict_2  # noqa: E402

warnings.simplefilter("ignore")

# (tag, redshift, alpha, c_dict_2 / h_dict_2 / Tinker instead of the defaults)
CASES = (("a15_", 0.0, -1.5, False),
         ("a05_", 0.0, -0.5, False),
         ("alt_", 0.5, -1.2, True))
TABLES = ("h_m", "pp_mm", "h_g", "pp_gm", "pp_gg")
LN_K_OFF = numpy.log(numpy.array([0.0123, 0.77, 31.0]))
K_POWER = numpy.array([5e-4, 1e-3, 3.3e-3, 0.02, 0.1, 0.45, 1.0, 3.0, 10.0, 42.0, 99.0, 250.0])


def y_table(h, log):
    """The table of _initialize_y_spline at every ln k knot, and each integral's level."""
    lk, nm = h._ln_k_array, h.mass._ln_mass_array.size
    y = numpy.empty((lk.size, nm))
    lev = numpy.empty((lk.size, nm), dtype=numpy.int64)
    for i, ln_k in enumerate(lk):
        log.levels["_y_integrand"] = []
        h._initialize_y_spline(ln_k)
        y[i] = h._y_array
        lev[i] = log.levels["_y_integrand"]
    return y, lev


def build(ns, z, alpha, alt, cls, **kws):
    if alt:
        hd = dict(h_dict_2, alpha=alpha)
        cosmo = ns.cosmology.SingleEpoch(z, c_dict_2)
        mass = ns.mass_function.TinkerMassFunction(z, cosmo, hd)
        return cls(z, None, cosmo, mass, hd, **kws), hd
    hd = dict(ns.defaults.default_halo_dict, alpha=alpha)
    return cls(z, halo_dict=hd, **kws), hd


def g28(ns):
    out = {"k": K_POWER, "ln_k_off": LN_K_OFF}
    first = None
    for tag, z, alpha, alt in CASES:
        t0 = time.time()
        with LevelLog(ns.halo.integrate) as log:
            h, hd = build(ns, z, alpha, alt, ns.halo.Halo)
            lk, lm = h._ln_k_array, h.mass._ln_mass_array
            out[tag + "y"], out[tag + "y_level"] = y_table(h, log)
            for name in TABLES:
                log.levels["_%s_integrand" % name] = []
                getattr(h, "_initialize_" + name)()
                out[tag + name] = getattr(h, "_%s_spline" % name)(lk)
                out[tag + name + "_level"] = numpy.array(log.levels["_%s_integrand" % name])
            for ps in ("mm", "gm", "gg"):
                out[tag + "power_" + ps] = getattr(h, "power_" + ps)(K_POWER)
        out[tag + "z"], out[tag + "alpha"] = z, alpha
        out[tag + "ln_k"], out[tag + "ln_mass"] = lk, lm
        out[tag + "ln_mass_min"], out[tag + "ln_mass_max"] = h.mass.ln_mass_min, h.mass.ln_mass_max
        out[tag + "n_bar"], out[tag + "rho_bar"], out[tag + "delta_v"] = h.n_bar, h.rho_bar, h.delta_v
        # eight masses between the knots, and two outside the mass table (y is 0 there)
        m_off = numpy.exp(lm[2:47:6][:8] + 0.37 * (lm[1] - lm[0]))
        m_all = numpy.concatenate([numpy.exp(lm), m_off])
        out[tag + "mass"] = m_all
        out[tag + "concentration"] = h.concentration(m_all)
        out[tag + "virial_radius"] = h.virial_radius(m_all)
        out[tag + "halo_normalization"] = h.halo_normalization(m_all)
        m_y = numpy.concatenate([m_off, [numpy.exp(lm[0]) * 0.5, numpy.exp(lm[-1]) * 2.0]])
        out[tag + "mass_y"] = m_y
        out[tag + "y_off"] = numpy.array([h.y(ln_k, m_y) for ln_k in LN_K_OFF])
        if first is None:
            first = (h, z, alpha, alt)
        print("  %s %.1f s" % (tag, time.time() - t0), flush=True)

    # the first case's I_1^2 and response (the matter tables copied by init_from_halo), and
    # HaloExclusion's h_m
    h, z, alpha, alt = first
    with LevelLog(ns.halo.integrate) as log:
        s = ns.halo.HaloSuperSampleCovariance.init_from_halo(h)
        out["a15_dln_power_ddelta_b"] = s.dln_power_ddelta_b(K_POWER)
        out["a15_i_1_2"] = s._i_1_2_spline(s._ln_k_array)
        out["a15_i_1_2_level"] = numpy.array(log.levels["_i_1_2_integrand"])
        x, _ = build(ns, z, alpha, alt, ns.halo.HaloExclusion)
        x._initialize_h_m()
        out["a15_excl_h_m"] = x._h_m_spline(x._ln_k_array)
        out["a15_excl_h_m_level"] = numpy.array(log.levels["_h_m_integrand"])

    # y_general called directly on a default (NFW) halo: the size of the Romberg truncation
    h = ns.halo.Halo(0.0)
    m = numpy.exp(h.mass._ln_mass_array)
    out["nfw_ln_k"] = LN_K_OFF
    out["nfw_mass"] = m
    out["nfw_y_general"] = numpy.array([h.y_general(ln_k, m) for ln_k in LN_K_OFF])
    out["nfw_y_nfw"] = numpy.array([h.y_nfw(ln_k, m) for ln_k in LN_K_OFF])
    save("g28_halo_profile", **out)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            t0 = time.time()
            g28(ns)
            print("  g28: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
