#!/usr/bin/env python3
"""Generate tests/golden/g35_xi_batch.npz by RUNNING THE REFERENCE's loops behind the xi(r)
batches: correlation.Correlation3d.raw_correlation(r) per HOD (set_hod / set_hod_object on one
object) and per cosmology (a fresh halo and object per point).

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_xi_batch.py

The file holds arrays only: r [7]; k_ranges [2, 2] ((1e-3, 100): the halo's own range, the
object built without k_min / k_max; (1e-3, 10)), tagged "full" and "cut" in the names below;
  HOD part (z = 0, the HODs of G32): zheng [3, 5], mandelbaum [2] as in g32, and
    xi_<spectrum>_<range> [4, 7] for power_gg and power_gm, the rows in the order of the HODs
    (the three Zheng HODs, then the Mandelbaum one);
  cosmology part (z_cosmo = 0.5, the cosmologies of G34): cosmo [3, 10] as in g34, and
    xic_<spectrum>_<range> [3, 7] for power_mm and power_gg with the default HOD.

The oracle's agreement with the Zheng and the cosmology rows and its Romberg levels are printed
(tests/test_xi_batch_cpu.py asserts them for a subset).
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
from make_golden_wtheta_cosmologies import COSMO_KEYS, COSMOS  # noqa: E402
from make_golden_wtheta_hods import MANDELBAUM, ZHENG, ZHENG_KEYS  # noqa: E402

warnings.simplefilter("ignore")

R = numpy.array([0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0])
RANGES = (("full", (1e-3, 100.0)), ("cut", (1e-3, 10.0)))
Z_COSMO = 0.5


def _range_kw(tag, lim):
    # ("full" is the halo's own range: the object is built without limits, as a user would)
    return {} if tag == "full" else dict(k_min=lim[0], k_max=lim[1])


def g35(ns):
    out = {"r": R, "k_ranges": numpy.array([lim for _, lim in RANGES]),
           "zheng": numpy.array([[d[key] for key in ZHENG_KEYS] for d in ZHENG]),
           "mandelbaum": numpy.array([MANDELBAUM["log_M_0"], MANDELBAUM["w"]]),
           "z_cosmo": numpy.array(Z_COSMO),
           "cosmo": numpy.array([[c[key] for key in COSMO_KEYS] for c in COSMOS])}
    for tag, lim in RANGES:
        for ps in ("power_gg", "power_gm"):
            c3 = ns.correlation.Correlation3d(0.1, 100.0, redshift=0.0,
                                              input_halo=ns.halo.Halo(0.0), powSpec=ps,
                                              **_range_kw(tag, lim))
            rows = []
            for d in ZHENG:
                c3.set_hod(dict(d))
                rows.append(c3.raw_correlation(R))
            c3.set_hod_object(ns.hod.HODMandelbaum(dict(MANDELBAUM)))
            rows.append(c3.raw_correlation(R))
            assert not c3.halo.get_extrapolation()
            out["xi_%s_%s" % (ps, tag)] = numpy.array(rows)
        for ps in ("power_mm", "power_gg"):
            rows = []
            for c in COSMOS:
                h = ns.halo.Halo(Z_COSMO, None, ns.cosmology.SingleEpoch(Z_COSMO, dict(c)))
                c3 = ns.correlation.Correlation3d(0.1, 100.0, redshift=Z_COSMO, input_halo=h,
                                                  powSpec=ps, **_range_kw(tag, lim))
                rows.append(c3.raw_correlation(R))
            out["xic_%s_%s" % (ps, tag)] = numpy.array(rows)
    save("g35_xi_batch", **out)
    return out


def oracle_check(out):
    """The oracle against the Zheng rows and the cosmology rows, with its stopping levels."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import chomp_oracle as o
    e = o.epoch(None, 0.0)
    m = o.mass_table(e)
    for tag, lim in RANGES:
        for i, d in enumerate(ZHENG):
            t = o.halo_table(e, m, o.zheng(dict(d)), families=("gm", "gg"))
            for ps in ("gg", "gm"):
                lev = []
                xi = o.xi3d_raw(lambda k: o.halo_power(t, ps, k), R, lim[0], lim[1], levels=lev)
                err = numpy.max(numpy.abs(xi / out["xi_power_%s_%s" % (ps, tag)][i] - 1))
                print("  oracle against the reference, power_%s %s HOD %d: %.2e; levels %s"
                      % (ps, tag, i, err, [int(x) for x in lev]))
        for i, c in enumerate(COSMOS):
            ec = o.epoch(dict(c), Z_COSMO)
            t = o.halo_table(ec, o.mass_table(ec), families=("mm", "gg"))
            for ps in ("mm", "gg"):
                lev = []
                xi = o.xi3d_raw(lambda k: o.halo_power(t, ps, k), R, lim[0], lim[1], levels=lev)
                err = numpy.max(numpy.abs(xi / out["xic_power_%s_%s" % (ps, tag)][i] - 1))
                print("  oracle against the reference, power_%s %s cosmology %d: %.2e; levels %s"
                      % (ps, tag, i, err, [int(x) for x in lev]))


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            t0 = time.time()
            out = g35(ns)
            print("  g35: %.1f s" % (time.time() - t0))
            oracle_check(out)
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
