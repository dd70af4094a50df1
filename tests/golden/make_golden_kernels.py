#!/usr/bin/env python3
"""Generate tests/golden/g36_kernels.npz by RUNNING THE REFERENCE once per kernel of a tomographic
analysis: per row a fresh kernel.Kernel / GalaxyGalaxyLensingKernel on that row's windows,
MultiEpoch range and cosmology, a fresh halo.Halo of that cosmology and HOD, and
correlation.Correlation (w(theta)) / correlation.CorrelationFourier (C_l, correlation(l) per
multipole) on them -- the loop that Correlation.correlation_kernels runs as one batch.

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_kernels.py

Windows: ML = dNdzMagLim(0, 2, 2, 0.3, 2), ML4 = dNdzMagLim(0, 2, 2, 0.4, 2), G4 =
dNdzGaussian(0, 1, 0.4, 0.1), G3 = dNdzGaussian(0, 1, 0.3, 0.1), S1 = dNdzGaussian(0, 2, 1.0, 0.2).  Cosmologies: c0 = params.c_dict,
c1 = c0 with omega_m0 raised by 0.05 and omega_l0 lowered to keep the universe flat (G34's second
point).  HODs: G32's Zheng rows (the first is the example script's Zehavi values).

  J0 (Kernel, power_gg; w(theta) and C_l)          windows   cosmology  MultiEpoch  HOD
    0  the G6 projection                            ML x ML   c0         (0, 5)      Zheng 0
    1  a lens-bin auto-correlation                  G4 x G4   c0         (0, 2)      Zheng 0
    2  a cross-bin pair                             ML x G4   c0         (0, 5)      Zheng 0
    3  another cosmology                            ML x ML   c1         (0, 5)      Zheng 0
    4  another HOD                                  ML x ML4  c0         (0, 5)      Zheng 1
  J2 (GalaxyGalaxyLensingKernel, power_gm; w(theta))
    0  G7                                gal ML x conv S1     c0         (0, 5)      Zheng 0
    1                                    gal G3 x conv S1     c0         (0, 5)      Zheng 0
    2                                    gal G3 x conv S1     c1         (0, 5)      Zheng 0

The lens bin of J2 rows 1 and 2 was to be G4 (z_bar 0.408).  There the device's halo set-up for
power_gm reports a status word ("pp_gm: Romberg exhausted divmax at some knots") in both
cosmologies -- reported, not matched, so such a row cannot be held to the reference -- and the
milder G3 (z_bar 0.306, status word 0 in c0 and c1) replaces it.  The J0 rows, which carry the
route conditions of C_l, are as planned; all of them are unflagged on the device.

The file holds arrays only.  Shared: theta [9] (logspace(-3, 0, 9) deg in radians), ell [22] (G33's
multipoles).  Per group g in (j0, j2), one row per kernel: g_wkind [n, 2] (0 galaxy, 1
convergence), g_dkind [n, 2] (0 dNdzMagLim: parameters a, z0, b; 1 dNdzGaussian: z0, sigma_z),
g_dz [n, 2, 2] (z_min, z_max as given to the distribution), g_dpar [n, 2, 3], g_me [n, 2]
(MultiEpoch range), g_cosmo [n, 10] (the field order of chomp_cosmo), g_zheng [n, 5] (log_M_min,
sigma, log_M_0, log_M_1p, alpha), g_z_bar [n] and g_D_z [n] as the reference's Correlation holds
them, g_w [n, 9], and for j0 j0_cl [5, 22].

The oracle's agreement with every row and its C_l stopping levels are printed
(tests/test_kernels_batch_cpu.py asserts both).
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
from make_golden_wtheta_hods import ZHENG, ZHENG_KEYS  # noqa: E402

warnings.simplefilter("ignore")

GAL, CONV = 0, 1
ML = (0, 0.0, 2.0, (2.0, 0.3, 2.0))
ML4 = (0, 0.0, 2.0, (2.0, 0.4, 2.0))
G4 = (1, 0.0, 1.0, (0.4, 0.1))
G3 = (1, 0.0, 1.0, (0.3, 0.1))
S1 = (1, 0.0, 2.0, (1.0, 0.2))
C0, C1 = COSMOS[0], COSMOS[1]
KTHETA = (1e-6 * deg_to_rad, 100.0 * deg_to_rad)

# (window a, window b, cosmology, MultiEpoch range, HOD): window = (kind, distribution)
J0 = (((GAL, ML), (GAL, ML), C0, (0.0, 5.0), ZHENG[0]),
      ((GAL, G4), (GAL, G4), C0, (0.0, 2.0), ZHENG[0]),
      ((GAL, ML), (GAL, G4), C0, (0.0, 5.0), ZHENG[0]),
      ((GAL, ML), (GAL, ML), C1, (0.0, 5.0), ZHENG[0]),
      ((GAL, ML), (GAL, ML4), C0, (0.0, 5.0), ZHENG[1]))
J2 = (((GAL, ML), (CONV, S1), C0, (0.0, 5.0), ZHENG[0]),
      ((GAL, G3), (CONV, S1), C0, (0.0, 5.0), ZHENG[0]),
      ((GAL, G3), (CONV, S1), C1, (0.0, 5.0), ZHENG[0]))


def _window(ns, spec, me):
    kind, (dkind, z_min, z_max, par) = spec
    dist = (ns.kernel.dNdzMagLim if dkind == 0 else ns.kernel.dNdzGaussian)(z_min, z_max, *par)
    cls = ns.kernel.WindowFunctionGalaxy if kind == GAL else ns.kernel.WindowFunctionConvergence
    return cls(dist, me)


def _row(ns, row, ggl, fourier):
    """A fresh kernel, halo and correlation object of one row, as the reference builds them."""
    wa, wb, cosmo, me_range, hod = row
    me = ns.cosmology.MultiEpoch(me_range[0], me_range[1], dict(cosmo))
    K = ns.kernel.GalaxyGalaxyLensingKernel if ggl else ns.kernel.Kernel
    kern = K(KTHETA[0], KTHETA[1], _window(ns, wa, me), _window(ns, wb, me), me)
    h = ns.halo.Halo(0.0, ns.hod.HODZheng(dict(hod)), ns.cosmology.SingleEpoch(0.0, dict(cosmo)))
    ps = "power_gm" if ggl else "power_gg"
    if fourier:
        return ns.correlation.CorrelationFourier(10, 1e4, kern, input_halo=h, powSpec=ps)
    return ns.correlation.Correlation(0.001, 1.0, kern, input_halo=h, power_spec=ps)


def _describe(tag, rows):
    out = {tag + "_wkind": numpy.array([[r[0][0], r[1][0]] for r in rows], dtype=float),
           tag + "_dkind": numpy.array([[r[0][1][0], r[1][1][0]] for r in rows], dtype=float),
           tag + "_dz": numpy.array([[[w[1][1], w[1][2]] for w in r[:2]] for r in rows]),
           tag + "_dpar": numpy.array([[list(w[1][3]) + [0.0] * (3 - len(w[1][3])) for w in r[:2]]
                                       for r in rows]),
           tag + "_me": numpy.array([list(r[3]) for r in rows]),
           tag + "_cosmo": numpy.array([[r[2][key] for key in COSMO_KEYS] for r in rows]),
           tag + "_zheng": numpy.array([[r[4][key] for key in ZHENG_KEYS] for r in rows])}
    return out


def g36(ns):
    theta = numpy.logspace(-3, 0, 9) * deg_to_rad
    out = {"theta": theta, "ell": ELL}
    for tag, rows, ggl in (("j0", J0, False), ("j2", J2, True)):
        out.update(_describe(tag, rows))
        w, z_bar, D_z, cl = [], [], [], []
        for i, row in enumerate(rows):
            t0 = time.time()
            corr = _row(ns, row, ggl, False)
            w.append(corr.correlation(theta))
            z_bar.append(corr.kernel.z_bar)
            D_z.append(corr.D_z)
            if not ggl:
                four = _row(ns, row, ggl, True)
                cl.append([float(four.correlation(l)) for l in ELL])
            print("  %s row %d: z_bar %.4f, %.1f s" % (tag, i, z_bar[-1], time.time() - t0))
        out[tag + "_w"] = numpy.array(w, dtype=float)
        out[tag + "_z_bar"] = numpy.array(z_bar, dtype=float)
        out[tag + "_D_z"] = numpy.array(D_z, dtype=float)
        if cl:
            out[tag + "_cl"] = numpy.array(cl, dtype=float)
    save("g36_kernels", **out)
    return out


def oracle_check(out):
    """The oracle against every row, by the recipe the CPU test asserts with."""
    sys.path.insert(0, os.path.dirname(HERE))
    from test_kernels_batch_cpu import oracle_of_fixture
    for tag in ("j0", "j2"):
        w, cl, levels = oracle_of_fixture(out, tag)
        for i in range(w.shape[0]):
            msg = "  oracle against the reference, %s row %d: w %.2e" % (
                tag, i, numpy.max(numpy.abs(w[i] / out[tag + "_w"][i] - 1)))
            if cl is not None:
                msg += "; C_l %.2e; levels %s" % (
                    numpy.max(numpy.abs(cl[i] / out[tag + "_cl"][i] - 1)), levels[i])
            print(msg)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)          # the reference's Kernel.__init__ writes files to CWD
        try:
            t0 = time.time()
            out = g36(ns)
            print("  g36: %.1f s" % (time.time() - t0))
            oracle_check(out)
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
