#!/usr/bin/env python3
"""Generate tests/golden/g37_kernels_tabulated.npz by RUNNING THE REFERENCE once per kernel of a
tomographic analysis whose bins are tables and whose cosmology may have w0-wa dark energy: per row
a fresh kernel.Kernel / GalaxyGalaxyLensingKernel on that row's windows and cosmology, a fresh
halo.Halo of that cosmology, and correlation.Correlation (w(theta)) / correlation.CorrelationFourier
(C_l, correlation(l) per multipole) on them -- the loop that
Correlation.correlation_kernels(..., tabulated=True, dark_energy=True) runs as one batch.

Development-container only, like make_golden_kernels.py (after which it is made; that file is not
changed).  Run from anywhere:  python tests/golden/make_golden_kernels_tab.py

Tables (17 points each, photometric-style bins with a ripple; dNdzInterpolation of the points):
T0 a lens bin around z = 0.3 on [0.05, 0.65], T1 a lens bin around z = 0.5 on [0.2, 0.9] (both
order 2 through the points), T2 a source bin around z = 1 on [0.4, 1.6] (order 3, smoothing 1e-4),
T3 a lens bin around z = 0.32 on [0.07, 0.67] (order 2).
ML = dNdzMagLim(0, 2, 2, 0.3, 2).  Cosmologies: c0 and c1 are G34's first two points, cw is c0 with
(w0, wa) = (-0.9, 0.2).  The HOD is G32's first Zheng row everywhere; every MultiEpoch is (0, 5).

  J0 (Kernel, power_gg; w(theta) and C_l)            windows        cosmology
    0  a tabulated auto-correlation                   T0 x T0        c0
    1  a tabulated cross-bin pair                     T0 x T1        c0
    2  analytic x tabulated                           ML x T1        c1
    3  an analytic pair with dark energy              ML x ML        cw
  J2 (GalaxyGalaxyLensingKernel, power_gm; w(theta))
    0  galaxy table x convergence table         gal T3 x conv T2     c0

The lens bin of the J2 row was to be T0 (z_bar 0.307).  There the device's halo set-up for power_gm
reports a status word ("pp_gm: Romberg exhausted divmax at some knots") -- reported, not matched,
so such a row cannot be held to the reference, as with G36's J2 rows -- and the milder T3 (z_bar
0.327, status word 0) replaces it.  The J0 rows are as planned and unflagged on the device, but for
the bit that every w0-wa cosmology carries: row 3's pressure table exhausts divmax at its deepest
knots in the reference and on the device alike, and the device says so (ST_DE_DIVMAX).

The file holds arrays only.  Shared: theta [9] (logspace(-3, 0, 9) deg in radians), ell [6] (six of
G33's multipoles), t_z / t_p [4, 17] (the tables' points), t_order [4], t_smoothing [4] (0: the
spline goes through the points).  Per group g in (j0, j2), one row per kernel: g_wkind [n, 2] (0
galaxy, 1 convergence), g_tab [n, 2] (the window's table, -1 for ML), g_cosmo [n, 10] (the field
order of chomp_cosmo), g_z_bar [n] and g_D_z [n] as the reference's Correlation holds them, g_w [n,
9], and for j0 j0_cl [4, 6].
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
from make_golden import deg_to_rad, save  # noqa: E402
from make_golden_cell_hods import ELL  # noqa: E402
from make_golden_wtheta_cosmologies import COSMO_KEYS, COSMOS  # noqa: E402
from make_golden_wtheta_hods import ZHENG  # noqa: E402

warnings.simplefilter("ignore")

GAL, CONV = 0, 1
ML = -1
C0, C1 = COSMOS[0], COSMOS[1]
CW = dict(C0, w0=-0.9, wa=0.2)
KTHETA = (1e-6 * deg_to_rad, 100.0 * deg_to_rad)
ELL_PICK = (0, 5, 9, 13, 17, 21)


def _bin(z_lo, z_hi, z0, sigma, ripple):
    z = numpy.linspace(z_lo, z_hi, 17)
    p = numpy.exp(-0.5 * ((z - z0) / sigma) ** 2) * (1.0 + 0.2 * numpy.sin(ripple * z)) + 0.01
    return z, p


TABLES = (_bin(0.05, 0.65, 0.3, 0.1, 25.0), _bin(0.2, 0.9, 0.5, 0.12, 19.0),
          _bin(0.4, 1.6, 1.0, 0.2, 11.0), _bin(0.07, 0.67, 0.32, 0.1, 25.0))
T_ORDER = (2, 2, 3, 2)
T_SMOOTHING = (0.0, 0.0, 1e-4, 0.0)

# (window a, window b, cosmology): window = (kind, table or ML)
J0 = (((GAL, 0), (GAL, 0), C0),
      ((GAL, 0), (GAL, 1), C0),
      ((GAL, ML), (GAL, 1), C1),
      ((GAL, ML), (GAL, ML), CW))
J2 = (((GAL, 3), (CONV, 2), C0),)


def _window(ns, spec, me):
    kind, t = spec
    if t == ML:
        dist = ns.kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0)
    elif T_SMOOTHING[t]:
        dist = ns.kernel.dNdzInterpolation(TABLES[t][0], TABLES[t][1],
                                           interpolation_order=T_ORDER[t],
                                           smoothing=T_SMOOTHING[t])
    else:
        dist = ns.kernel.dNdzInterpolation(TABLES[t][0], TABLES[t][1],
                                           interpolation_order=T_ORDER[t])
    cls = ns.kernel.WindowFunctionGalaxy if kind == GAL else ns.kernel.WindowFunctionConvergence
    return cls(dist, me)


def _row(ns, row, ggl, fourier):
    """A fresh kernel, halo and correlation object of one row, as the reference builds them."""
    wa, wb, cosmo = row
    me = ns.cosmology.MultiEpoch(0.0, 5.0, dict(cosmo))
    K = ns.kernel.GalaxyGalaxyLensingKernel if ggl else ns.kernel.Kernel
    kern = K(KTHETA[0], KTHETA[1], _window(ns, wa, me), _window(ns, wb, me), me)
    h = ns.halo.Halo(0.0, ns.hod.HODZheng(dict(ZHENG[0])),
                     ns.cosmology.SingleEpoch(0.0, dict(cosmo)))
    ps = "power_gm" if ggl else "power_gg"
    if fourier:
        return ns.correlation.CorrelationFourier(10, 1e4, kern, input_halo=h, powSpec=ps)
    return ns.correlation.Correlation(0.001, 1.0, kern, input_halo=h, power_spec=ps)


def g37(ns):
    theta = numpy.logspace(-3, 0, 9) * deg_to_rad
    ell = numpy.ascontiguousarray(numpy.asarray(ELL, dtype=float)[list(ELL_PICK)])
    out = {"theta": theta, "ell": ell,
           "t_z": numpy.array([t[0] for t in TABLES]), "t_p": numpy.array([t[1] for t in TABLES]),
           "t_order": numpy.array(T_ORDER, dtype=float),
           "t_smoothing": numpy.array(T_SMOOTHING, dtype=float)}
    for tag, rows, ggl in (("j0", J0, False), ("j2", J2, True)):
        out[tag + "_wkind"] = numpy.array([[r[0][0], r[1][0]] for r in rows], dtype=float)
        out[tag + "_tab"] = numpy.array([[r[0][1], r[1][1]] for r in rows], dtype=float)
        out[tag + "_cosmo"] = numpy.array([[r[2][key] for key in COSMO_KEYS] for r in rows])
        w, z_bar, D_z, cl = [], [], [], []
        for i, row in enumerate(rows):
            t0 = time.time()
            corr = _row(ns, row, ggl, False)
            w.append(corr.correlation(theta))
            z_bar.append(corr.kernel.z_bar)
            D_z.append(corr.D_z)
            if not ggl:
                four = _row(ns, row, ggl, True)
                cl.append([float(four.correlation(l)) for l in ell])
            print("  %s row %d: z_bar %.4f, %.1f s" % (tag, i, z_bar[-1], time.time() - t0))
        out[tag + "_w"] = numpy.array(w, dtype=float)
        out[tag + "_z_bar"] = numpy.array(z_bar, dtype=float)
        out[tag + "_D_z"] = numpy.array(D_z, dtype=float)
        if cl:
            out[tag + "_cl"] = numpy.array(cl, dtype=float)
    save("g37_kernels_tabulated", **out)
    return out


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)          # the reference's Kernel.__init__ writes files to CWD
        try:
            t0 = time.time()
            g37(ns)
            print("  g37: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
