#!/usr/bin/env python3
"""Generate tests/golden/g24_trispectrum_one_halo.npz by RUNNING THE REFERENCE's
halo_trispectrum.HaloTrispectrumOneHalo (halo_trispectrum.py:13-151).

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_tri1h.py

The 50 x 50 tables are stored as their upper triangle (row-major, i <= j): the reference
fills the lower one by mirroring (halo_trispectrum.py:112-123).
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

MANDELBAUM = {"log_M_0": 12.14, "w": 1.0}


def scalars(k_min, k_max):
    """Scalar arguments of trispectrum_parallelogram: the range ends and their neighbours at
    1e-9, one point below k_min, one above k_max and a few inside."""
    return numpy.array([k_min * (1 - 1e-9), k_min, k_min * (1 + 1e-9),
                        k_max * (1 - 1e-9), k_max, k_max * (1 + 1e-9),
                        5e-4, 150.0, 0.01, 0.1, 0.5, 1.0, 2.0, 30.0])


def scalar_pairs(k_min, k_max):
    s = scalars(k_min, k_max)
    pairs = [(a, 1.0) for a in s] + [(1.0, b) for b in s] + [(a, a) for a in s]
    pairs += [(0.5, 2.0), (2.0, 0.5), (5e-4, 150.0), (150.0, 5e-4)]
    return numpy.array(pairs)


def quadruples(k_min, k_max):
    """32 (k1, k2, k3, k4): log-spaced in [1e-3, 1e2], equal pairs, points outside the range."""
    rng = numpy.random.RandomState(24)
    q = numpy.exp(rng.uniform(numpy.log(1e-3), numpy.log(1e2), size=(20, 4)))
    for i in range(6):                       # (a, a, b, b) and (a, b, a, b)
        q[i, 1] = q[i, 0]
        q[i, 3] = q[i, 2]
    for i in range(6, 9):
        q[i, 2] = q[i, 0]
        q[i, 3] = q[i, 1]
    extra = numpy.array([[0.1, 0.1, 1.0, 1.0], [0.5, 0.5, 2.0, 2.0], [1e-4, 1e-4, 1.0, 1.0],
                         [5e-4, 0.3, 150.0, 2.0], [150.0, 150.0, 150.0, 150.0],
                         [k_min, k_min, k_max, k_max], [k_min * (1 - 1e-9), 1.0, 1.0, 1.0],
                         [k_max * (1 + 1e-9), 1.0, 1.0, 1.0], [1e-3, 1e-3, 1e-3, 1e-3],
                         [3.0, 3.0, 3.0, 3.0], [0.02, 0.05, 0.2, 7.0], [200.0, 0.01, 0.01, 0.01]])
    return numpy.concatenate([q, extra])


def triu(a):
    return a[numpy.triu_indices(a.shape[0])]


def grab(out, tag, h, pairs, quads, with_scal=True):
    if with_scal:
        out[tag + "scal"] = numpy.array(
            [numpy.asarray(h.trispectrum_parallelogram(a, b)).ravel()[0] for a, b in pairs])
    else:
        h.trispectrum_parallelogram(1.0, 1.0)
    out[tag + "table"] = triu(h._i_0_4_array)
    out[tag + "quad"] = numpy.array([h.i_0_4(*q) for q in quads])
    out[tag + "rho_bar"] = h.rho_bar


def g24(ns):
    d = ns.defaults
    k_min, k_max = d.default_limits["k_min"], d.default_limits["k_max"]
    pairs = scalar_pairs(k_min, k_max)
    quads = quadruples(k_min, k_max)
    out = {"pairs": pairs, "quads": quads}
    HT = ns.halo_trispectrum.HaloTrispectrumOneHalo
    # the default set-up at z = 0 and z = 0.5
    for z in (0.0, 0.5):
        h = HT(z)
        tag = "z%03d_" % round(100 * z)
        grab(out, tag, h, pairs, quads)
        out[tag + "ln_k"] = h._ln_k_array
        out[tag + "default_0_1"] = h.i_0_4(0.1, 0.1, 1.0, 1.0)
        if z == 0.0:
            # 1-D array calls: the k_max mask broadcasts along the last axis of the grid
            a = numpy.array([5e-4, 0.5, 200.0])
            b = numpy.array([0.01, 1.0, 2.0])
            for name, x, y in (("arr_", a, b), ("arr_col_", a, 1.0), ("arr_row_", 1.0, b),
                               ("arr_rev_", b, a)):
                r = numpy.asarray(h.trispectrum_parallelogram(x, y))
                out[name + "a"] = numpy.atleast_1d(x)
                out[name + "b"] = numpy.atleast_1d(y)
                out[name + "out"] = r
                out[name + "shape"] = numpy.array(r.shape)
    # the four HOD moments with HODZheng at z = 0.3
    z = 0.3
    for spec in ("power_gmmm", "power_ggmm", "power_gggm", "power_gggg"):
        h = HT(z, power_spec=spec, input_hod=ns.hod.HODZheng())
        grab(out, spec[-4:] + "_", h, pairs, quads, with_scal=(spec == "power_gggg"))
    # HODMandelbaum through the moment formula
    h = HT(z, power_spec="power_gggg", input_hod=ns.hod.HODMandelbaum(dict(MANDELBAUM)))
    grab(out, "mand_", h, pairs, quads, with_scal=False)
    out["mand_hod"] = numpy.array([MANDELBAUM["log_M_0"], MANDELBAUM["w"]])
    # c_dict_2 / Tinker / h_dict_2 at z = 0.3
    cosmo = ns.cosmology.SingleEpoch(z, c_dict_2)
    mass = ns.mass_function.TinkerMassFunction(z, cosmo, h_dict_2)
    h = HT(z, cosmo, mass, None, h_dict_2)
    grab(out, "alt_", h, pairs, quads)
    # MassFunctionSecondOrder at z = 0.2
    z = 0.2
    cosmo = ns.cosmology.SingleEpoch(z)
    mass = ns.mass_function.MassFunctionSecondOrder(z, cosmo)
    h = HT(z, cosmo, mass)
    grab(out, "mso_", h, pairs, quads, with_scal=False)
    # the stale sequence: pert = None, set_redshift raises after the halo has moved; the flag
    # stays True and the z = 0 table is served
    h = HT(0.0)
    h.trispectrum_parallelogram(0.5, 2.0)
    raised = 0
    try:
        h.set_redshift(0.5)
    except AttributeError:
        raised = 1
    out["stale_raised"] = raised
    out["stale_redshift"] = h._redshift
    out["stale_flag"] = int(h._initialized_i_0_4)
    out["stale_scal"] = numpy.array(
        [numpy.asarray(h.trispectrum_parallelogram(a, b)).ravel()[0] for a, b in pairs])
    out["stale_quad"] = numpy.array([h.i_0_4(*q) for q in quads[:8]])
    # the rebuilt sequence: with a PerturbationTheory the flag resets
    pert = ns.perturbation_spectra.PerturbationTheory(0.0)
    h = HT(0.0, perturbation=pert)
    h.trispectrum_parallelogram(0.5, 2.0)
    h.set_redshift(0.5)
    out["rebuilt_flag"] = int(h._initialized_i_0_4)
    out["rebuilt_scal"] = numpy.array(
        [numpy.asarray(h.trispectrum_parallelogram(a, b)).ravel()[0] for a, b in pairs])
    save("g24_trispectrum_one_halo", **out)


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            t0 = time.time()
            g24(ns)
            print("  g24: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
