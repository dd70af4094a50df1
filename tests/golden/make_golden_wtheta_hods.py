#!/usr/bin/env python3
"""Generate tests/golden/g32_wtheta_hods.npz by RUNNING THE REFERENCE's loop over HODs
(examples/example_script.py:141-143): one correlation.Correlation on the G6 projection (galaxy x
galaxy windows, Kernel), then set_hod / set_hod_object and correlation(theta) per HOD, for
power_gg and power_gm.

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_wtheta_hods.py

The file holds arrays only: theta [9], the HODs' parameters (zheng [3, 5] in the order log_M_min,
sigma, log_M_0, log_M_1p, alpha; mandelbaum [2]: log_M_0, w), and w_<spectrum> [4, 9] with the
rows in the order of HODS below (the three Zheng HODs, then the Mandelbaum one).
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

warnings.simplefilter("ignore")

ZHENG_KEYS = ("log_M_min", "sigma", "log_M_0", "log_M_1p", "alpha")
# the example script's Zehavi values; a sharp cutoff; a steep satellite slope with a high M_1'
ZHENG = ({"log_M_min": 12.14, "sigma": 0.15, "log_M_0": 12.14, "log_M_1p": 13.43, "alpha": 1.0},
         {"log_M_min": 12.14, "sigma": 0.05, "log_M_0": 12.14, "log_M_1p": 13.43, "alpha": 1.0},
         {"log_M_min": 12.14, "sigma": 0.15, "log_M_0": 12.14, "log_M_1p": 13.8, "alpha": 1.3})
MANDELBAUM = {"log_M_0": 12.8, "w": 0.5}


def g32(ns):
    # 9 theta spanning the binned range of Correlation(0.001, 1.0 deg)
    theta = numpy.logspace(-3, 0, 9) * deg_to_rad
    out = {"theta": theta,
           "zheng": numpy.array([[d[key] for key in ZHENG_KEYS] for d in ZHENG]),
           "mandelbaum": numpy.array([MANDELBAUM["log_M_0"], MANDELBAUM["w"]])}
    cm, kern = _projection(ns, ggl=False)
    out["z_bar"] = numpy.array(kern.z_bar)
    for ps in ("power_gg", "power_gm"):
        corr = ns.correlation.Correlation(0.001, 1.0, kern, input_halo=ns.halo.Halo(0.0),
                                          power_spec=ps)
        rows = []
        for d in ZHENG:
            corr.set_hod(dict(d))
            rows.append(corr.correlation(theta))
        corr.set_hod_object(ns.hod.HODMandelbaum(dict(MANDELBAUM)))
        rows.append(corr.correlation(theta))
        out["w_" + ps] = numpy.array(rows)
        out["D_z"] = numpy.array(corr.D_z)
    save("g32_wtheta_hods", **out)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)          # the reference's Kernel.__init__ writes files to CWD
        try:
            t0 = time.time()
            g32(ns)
            print("  g32: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
