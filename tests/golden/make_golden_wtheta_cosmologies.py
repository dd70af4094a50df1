#!/usr/bin/env python3
"""Generate tests/golden/g34_wtheta_cosmologies.npz by RUNNING THE REFERENCE's loop over
cosmologies (simulation_design.py:116-155 over Correlation.set_cosmology, correlation.py:161-171):
one correlation.Correlation on the G6 projection (galaxy x galaxy windows, Kernel) per spectrum,
then set_cosmology and correlation(theta) per cosmology, for power_gg and power_mm.

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_wtheta_cosmologies.py

The three cosmologies: params.c_dict; c_dict with omega_m0 raised by 0.05 and omega_l0 lowered
to keep the universe flat (omega_l0 = 1 - omega_m0 - omega_r0: a SimulationDesignFlatUniverse
point); c_dict with sigma_8 = 0.9 and h = 0.65.  All three leave the mass-limit search of the
halo set-up unsaturated at their z_bar (status word 0 on the device: the GPU test asserts it), so
no milder point had to be chosen.

The file holds arrays only: theta [9] (the 9 theta of g32), cosmo [3, 10] in the field order of
chomp_cosmo (omega_m0, omega_b0, omega_l0, omega_r0, cmb_temp, h, sigma_8, n_scalar, w0, wa),
z_bar [3] and D_z [3] as Correlation holds them after set_cosmology, and w_<spectrum> [3, 9].
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
from params import c_dict  # noqa: E402

warnings.simplefilter("ignore")

COSMO_KEYS = ("omega_m0", "omega_b0", "omega_l0", "omega_r0", "cmb_temp", "h", "sigma_8",
              "n_scalar", "w0", "wa")


def _flat(omega_m0):
    c = dict(c_dict, omega_m0=omega_m0)
    c["omega_l0"] = 1.0 - c["omega_m0"] - c["omega_r0"]
    return c


COSMOS = (dict(c_dict), _flat(c_dict["omega_m0"] + 0.05), dict(c_dict, sigma_8=0.9, h=0.65))


def g34(ns):
    theta = numpy.logspace(-3, 0, 9) * deg_to_rad
    out = {"theta": theta,
           "cosmo": numpy.array([[c[key] for key in COSMO_KEYS] for c in COSMOS])}
    for ps in ("power_gg", "power_mm"):
        _, kern = _projection(ns, ggl=False)
        corr = ns.correlation.Correlation(0.001, 1.0, kern, input_halo=ns.halo.Halo(0.0),
                                          power_spec=ps)
        rows, z_bar, D_z = [], [], []
        for c in COSMOS:
            corr.set_cosmology(dict(c))
            rows.append(corr.correlation(theta))
            z_bar.append(corr.kernel.z_bar)
            D_z.append(corr.D_z)
        out["w_" + ps] = numpy.array(rows)
        out["z_bar"] = numpy.array(z_bar)
        out["D_z"] = numpy.array(D_z)
    save("g34_wtheta_cosmologies", **out)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)          # the reference's Kernel.__init__ writes files to CWD
        try:
            t0 = time.time()
            g34(ns)
            print("  g34: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
