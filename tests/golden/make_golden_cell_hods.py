#!/usr/bin/env python3
"""Generate tests/golden/g33_cell_hods.npz by RUNNING THE REFERENCE's loop over HODs on the Limber
C_l: one correlation.CorrelationFourier on the G6 projection (galaxy x galaxy windows, Kernel), then
set_hod / set_hod_object and correlation(ell) per HOD, for power_gg and power_gm.  The HODs are
those of G32 (make_golden_wtheta_hods.py).

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_cell_hods.py

The file holds arrays only: ell [22] (logspace(1, 4, 19), then 8000, 9000, 9500: multipoles whose
Romberg integrals stop at the levels of all three routes of the device's C_l kernels, and whose set
of deep ones differs from HOD to HOD), the HODs' parameters (zheng [3, 5] in the order log_M_min,
sigma, log_M_0, log_M_1p, alpha; mandelbaum [2]: log_M_0, w), z_bar, D_z and cl_<spectrum> [4, 22]
with the rows in the order of the HODs (the three Zheng HODs, then the Mandelbaum one).

The oracle's agreement with cl_power_gg of the three Zheng rows and its Romberg levels are printed
(tests/test_cell_hods_cpu.py asserts both).
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
from make_golden_wtheta_hods import MANDELBAUM, ZHENG, ZHENG_KEYS  # noqa: E402

warnings.simplefilter("ignore")

ELL = numpy.concatenate([numpy.logspace(1, 4, 19), [8000., 9000., 9500.]])


def g33(ns):
    out = {"ell": ELL,
           "zheng": numpy.array([[d[key] for key in ZHENG_KEYS] for d in ZHENG]),
           "mandelbaum": numpy.array([MANDELBAUM["log_M_0"], MANDELBAUM["w"]])}
    cm, kern = _projection(ns, ggl=False)
    out["z_bar"] = numpy.array(kern.z_bar)
    for ps in ("power_gg", "power_gm"):
        corr = ns.correlation.CorrelationFourier(10, 1e4, kern, input_halo=ns.halo.Halo(0.0),
                                                 powSpec=ps)
        rows = []
        for d in ZHENG:
            corr.set_hod(dict(d))
            rows.append(corr.correlation(ELL))
        corr.set_hod_object(ns.hod.HODMandelbaum(dict(MANDELBAUM)))
        rows.append(corr.correlation(ELL))
        out["cl_" + ps] = numpy.array(rows)
        out["D_z"] = numpy.array(corr.D_z)
    save("g33_cell_hods", **out)
    return out


def oracle_check(out):
    """The oracle against the three Zheng rows of cl_power_gg, with its stopping levels."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import chomp_oracle as o
    d2r = numpy.pi / 180.0
    me = o.multi_epoch(0.0, 5.0)
    ow = o.window_table("galaxy", o.dndz_maglim(0.0, 2.0, 2.0, 0.3, 2.0), me)
    kt = o.kernel_table(1e-6 * d2r, 100 * d2r, ow, ow, me)
    e = o.epoch(None, kt.z_bar)
    m = o.mass_table(e)
    for i, d in enumerate(ZHENG):
        t = o.halo_table(e, m, o.zheng(dict(d)), families=("gg",))
        lev = []
        cl = o.cell(kt, lambda k: o.halo_power(t, "gg", k), ELL, float(out["D_z"]), levels=lev)
        err = numpy.max(numpy.abs(numpy.asarray(cl) / out["cl_power_gg"][i] - 1))
        print("  oracle against the reference, power_gg HOD %d: %.2e; levels %s"
              % (i, err, [int(x) for x in lev]))


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)          # the reference's Kernel.__init__ writes files to CWD
        try:
            t0 = time.time()
            out = g33(ns)
            print("  g33: %.1f s" % (time.time() - t0))
            oracle_check(out)
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
