#!/usr/bin/env python3
"""Generate tests/golden/g19_halo_ssc.npz by RUNNING THE REFERENCE's
halo.HaloSuperSampleCovariance (halo.py:1089-1199).

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_ssc.py
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
from params import c_dict_2, h_dict_2  # noqa: E402

warnings.simplefilter("ignore")

DELTA_B = 0.01


def k_samples(k_min, k_max):
    """k = logspace(-4, 3, 64) plus the range ends and their neighbours at 1e-9."""
    edges = [k_min * (1 - 1e-9), k_min, k_min * (1 + 1e-9),
             k_max * (1 - 1e-9), k_max, k_max * (1 + 1e-9)]
    return numpy.concatenate([numpy.logspace(-4, 3, 64), edges])


def grab(out, tag, h, k):
    out[tag + "ln_k"] = h._ln_k_array
    out[tag + "resp"] = h.dln_power_ddelta_b(k)
    out[tag + "i_1_2"] = h._i_1_2_spline(h._ln_k_array)
    out[tag + "mm_ssc"] = h.power_mm_ssc(k)
    out[tag + "mm"] = h.power_mm(k)


def g19(ns):
    d = ns.defaults
    k = k_samples(d.default_limits["k_min"], d.default_limits["k_max"])
    out = {"k": k, "delta_b": DELTA_B}
    # default set-up at z = 0 and z = 0.5
    for z in (0.0, 0.5):
        h = ns.halo.HaloSuperSampleCovariance(z, delta_b=DELTA_B)
        grab(out, "z%03d_" % round(100 * z), h, k)
    # c_dict_2 / Tinker / h_dict_2 at z = 0.3
    z = 0.3
    cosmo = ns.cosmology.SingleEpoch(z, c_dict_2)
    mass = ns.mass_function.TinkerMassFunction(z, cosmo, h_dict_2)
    h = ns.halo.HaloSuperSampleCovariance(z, None, cosmo, mass, h_dict_2, delta_b=DELTA_B)
    grab(out, "alt_", h, k)
    # init_from_halo of a Halo(extrapolate=True) that has built its tables: the copy never
    # extrapolates (halo.py:1102-1108, 1110-1134)
    src = ns.halo.Halo(0.2, extrapolate=True)
    out["from_src_mm"] = src.power_mm(k)
    h = ns.halo.HaloSuperSampleCovariance.init_from_halo(src, delta_b=DELTA_B)
    grab(out, "from_", h, k)
    out["from_extrapolate"] = float(h._extrapolate)
    out["from_k150_mm"] = h.power_mm(numpy.array([150.0]))
    # the stale sequence: the I_1^2 knots of the first build survive set_redshift (halo.py:135-235)
    h = ns.halo.HaloSuperSampleCovariance(0.0, delta_b=DELTA_B)
    out["stale_resp0"] = h.dln_power_ddelta_b(k)
    h.set_redshift(0.5)
    grab(out, "stale_", h, k)
    save("g19_halo_ssc", **out)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            t0 = time.time()
            g19(ns)
            print("  g19: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
