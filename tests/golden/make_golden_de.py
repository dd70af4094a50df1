#!/usr/bin/env python3
"""Generate tests/golden/g22_dark_energy.npz by RUNNING THE REFERENCE with w0-wa dark energy
(cosmology.py:96-104, 165-213) through SingleEpoch, MultiEpoch, Halo, HaloFit, Correlation and
CorrelationFourier.

Development-container only, like make_golden.py (whose helpers it imports; that file is not
changed).  Run from anywhere:  python tests/golden/make_golden_de.py

Every Romberg call of the cosmology and halo modules is wrapped (make_golden_hod.LevelLog) to
record its stopping level: the pressure integrals' per knot, the halo integrals' per knot.
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
from make_golden import deg_to_rad, save  # noqa: E402
from make_golden_hod import LevelLog, k_samples  # noqa: E402
from params import c_dict  # noqa: E402

warnings.simplefilter("ignore")

# (tag, w0, wa): both branches of the reference's test (w0 != -1; w0 == -1 with wa != 0)
COSMOLOGIES = (("a_", -0.9, 0.2), ("b_", -1.0, 0.3), ("c_", -1.2, 0.0))
REDSHIFTS = (0.0, 0.5, 1.0)
HALO_Z = {"a_": (0.0, 0.5, 1.0), "b_": (0.5,), "c_": (0.5,)}
E0_Z = numpy.array([0.0, 0.01, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 100.0, 1e4])
HALO_INTEGRANDS = ("_h_m_integrand", "_pp_mm_integrand", "_h_g_integrand", "_pp_gm_integrand",
                   "_pp_gg_integrand")
SCALARS = ("chi", "growth", "omega_m", "omega_l", "delta_c", "delta_v", "rho_crit", "rho_bar",
           "sigma_norm")


def cosmo(w0, wa):
    return dict(c_dict, w0=w0, wa=wa)


def scalars(e):
    return numpy.array([e._chi, e._growth, e.omega_m(), e.omega_l(), e.delta_c(), e.delta_v(),
                        e.rho_crit(), e.rho_bar(), e._sigma_norm])


def projection(ns, cd, ggl):
    cm = ns.cosmology.MultiEpoch(0.0, 5.0, cd)
    lens = ns.kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0)
    wa = ns.kernel.WindowFunctionGalaxy(lens, cm)
    if ggl:
        wb = ns.kernel.WindowFunctionConvergence(ns.kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2), cm)
        K = ns.kernel.GalaxyGalaxyLensingKernel
    else:
        wb = ns.kernel.WindowFunctionGalaxy(ns.kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
        K = ns.kernel.Kernel
    return cm, K(1e-6 * deg_to_rad, 100.0 * deg_to_rad, wa, wb, cm)


def g22(ns):
    d = ns.defaults
    prec = d.default_precision
    k = k_samples(d.default_limits["k_min"], d.default_limits["k_max"])
    a_knots = numpy.logspace(numpy.log10(prec["cosmo_precision"]), 0, prec["cosmo_npoints"])
    out = {"k": k, "redshifts": numpy.array(REDSHIFTS), "e0_z": E0_Z,
           "de_ln_a": numpy.log(a_knots), "de_z": 1 / a_knots - 1.0}
    for tag, w0, wa in COSMOLOGIES:
        cd = cosmo(w0, wa)
        out[tag + "w0"], out[tag + "wa"] = w0, wa
        e = ns.cosmology.SingleEpoch(0.0, cd)
        with LevelLog(ns.cosmology.integrate) as log:      # (the table again, levels recorded)
            again = e._de_pressure(1 / a_knots - 1.0)
        out[tag + "de_levels"] = numpy.array(log.levels["<lambda>"])
        out[tag + "de_pressure"] = e._de_pressure_array
        assert numpy.array_equal(again, e._de_pressure_array) and again.size == a_knots.size
        out[tag + "e0"] = e.E0(E0_Z)
        out[tag + "scalars"] = numpy.array([scalars(ns.cosmology.SingleEpoch(z, cd))
                                            for z in REDSHIFTS])
        for z in HALO_Z[tag]:
            zt = "%sz%03d_" % (tag, int(round(100 * z)))
            with LevelLog(ns.halo.integrate) as hl:
                h = ns.halo.Halo(z, None, ns.cosmology.SingleEpoch(z, cd))
                lk = h._ln_k_array
                out[zt + "power_mm"] = h.power_mm(k)
                out[zt + "power_gm"] = h.power_gm(k)
                out[zt + "power_gg"] = h.power_gg(k)
                for name in ("h_m", "pp_mm", "h_g", "pp_gm", "pp_gg"):
                    out[zt + name] = getattr(h, "_%s_spline" % name)(lk)
            for name in HALO_INTEGRANDS:
                out[zt + "levels" + name] = numpy.array(hl.levels[name])
            out[zt + "n_bar"] = h.n_bar
    # HaloFit and the projections: the first cosmology
    cd = cosmo(-0.9, 0.2)
    hf = ns.halo.HaloFit(0.5, None, ns.cosmology.SingleEpoch(0.5, cd))
    out["hf_z050_power_mm"] = hf.power_mm(k)
    me = ns.cosmology.MultiEpoch(0.0, 5.0, cd)
    out["me_z"], out["me_chi"], out["me_growth"] = me._z_array, me._chi_array, me._growth_array
    zs = numpy.array([0.0, 0.3, 0.5, 1.0, 2.0, 4.5])
    out["me_zs"] = zs
    out["me_omega_m"] = numpy.array([me.omega_m(z) for z in zs])
    out["me_omega_l"] = numpy.array([me.omega_l(z) for z in zs])
    out["me_rho_crit"] = numpy.array([me.rho_crit(z) for z in zs])
    out["me_delta_c"] = numpy.array([me.delta_c(z) for z in zs])
    out["me_delta_v"] = numpy.array([me.delta_v(z) for z in zs])
    theta = numpy.logspace(-3, 0, 17) * deg_to_rad
    ell = numpy.logspace(1, 4, 17)
    out["theta"], out["ell"] = theta, ell
    _, kern = projection(ns, cd, ggl=False)
    h = ns.halo.Halo(0.0, None, ns.cosmology.SingleEpoch(0.0, cd))
    corr = ns.correlation.Correlation(0.001, 1.0, kern, input_halo=h, power_spec="power_gg")
    out["w_gg"] = corr.correlation(theta)
    out["w_gg_D_z"] = corr.D_z
    cf = ns.correlation.CorrelationFourier(10, 1e4, kern, input_halo=h, powSpec="power_gg")
    out["cl_gg"] = cf.correlation(ell)
    out["kernel_z_bar"], out["kernel_chi_min"], out["kernel_chi_max"] = (
        kern.z_bar, kern.chi_min, kern.chi_max)
    out["wa_chi"] = kern.window_function_a._chi_array
    out["wa"] = numpy.asarray(kern.window_function_a._wf_array, dtype=float)
    _, kern = projection(ns, cd, ggl=True)
    h = ns.halo.Halo(0.0, None, ns.cosmology.SingleEpoch(0.0, cd))
    corr = ns.correlation.Correlation(0.001, 1.0, kern, input_halo=h, power_spec="power_gm")
    out["w_ggl"] = corr.correlation(theta)
    out["wb_chi"] = kern.window_function_b._chi_array
    out["wb"] = numpy.asarray(kern.window_function_b._wf_array, dtype=float)
    save("g22_dark_energy", **out)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            t0 = time.time()
            g22(ns)
            print("  g22: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
