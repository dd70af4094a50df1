#!/usr/bin/env python3
"""Generate tests/golden/g30_covariance_cross_terms.npz by RUNNING THE REFERENCE's trispectrum and
super-sample terms of a cross block: Covariance(corr_a, corr_b, nongaussian_cov=True, ssc_cov=True,
input_halo_trispectrum=HaloTrispectrumOneHalo(0.5)) with two different correlation objects --
KernelCovariance with four different windows (kernel.py:893-972, 1035-1111, 1155-1206) and
_kb_ssc_integrand with halo_a at k_a and halo_b at k_b (covariance.py:763-776).

As make_golden_cov_cross.py documents, the reference cannot construct such a Covariance as
shipped; THIS SCRIPT REPLACES Correlation.__eq__ WITH IDENTITY (``lambda s, o: s is o``) on the
loaded class, in this process only, and everything else runs as shipped.

Cases: "wide" -- a = MagLim galaxy window x convergence, b = galaxy Gaussian(0.0, 1.5, 0.7, 0.2)
used twice, each correlation on its own Halo(0.0); "gal" -- g29's "gal" pair; "far" -- g29's
"mix" windows on two separate Halo(0.0): its common range starts at z = 0.5, where kernel_ssc is
identically 0 and covariance_ssc NaN.

Every covariance_* value is taken after _initialize_halo_splines, which is where the reference
moves halo_a / halo_b to z_bar_a / z_bar_b (covariance.py:465-466), as its own get_covariance
does (covariance_G comes first there).

The work is cut into parts that run side by side, one process each (a covariance_ssc pair
takes about a minute of CPU, a kernel_NG table some minutes); each part writes a partial file
and the last step merges them.  "far" records its kernel_NG table only when that finishes within
FAR_NG_BUDGET seconds; without it the case has the raw probes alone for the trispectrum term
(covariance_NG needs the table).

Development-container only, like make_golden.py (whose helpers it imports; that file is
not changed).  Run from anywhere:  python tests/golden/make_golden_cov_cross_terms.py
  --part TAG:PART --out FILE   run one part;   --merge DIR   merge the parts found in DIR
"""
import contextlib
import io
import os
import signal
import subprocess
import sys
import tempfile
import time
import warnings

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402
from make_golden import save  # noqa: E402
from make_golden_cov_cross import KWS, correlations  # noqa: E402
from make_golden_cov_ssc import probes  # noqa: E402

warnings.simplefilter("ignore")

deg_to_rad = numpy.pi / 180.0
Z_TRI = 0.5
SWAPPED = ((3, 0), (2, 1))
FAR_NG_BUDGET = 1800
PARTS = ("wide:main", "wide:ssc0", "wide:ssc1", "wide:ssc2", "wide:cov",
         "gal:main", "gal:ssc0", "gal:ssc1", "gal:ssc2", "gal:cov",
         "far:main", "far:ng", "far:cov")


def pair_of(ns, tag):
    if tag == "gal":
        return correlations(ns, "gal")
    cm = ns.cosmology.MultiEpoch(0.0, 5.0)
    K = ns.kernel

    def corr(wa, wb):
        kern = K.Kernel(1e-6 * deg_to_rad, 100.0 * deg_to_rad, wa, wb, cm)
        return ns.correlation.Correlation(0.01, 1.0, kern, input_halo=ns.halo.Halo(0.0),
                                          power_spec="power_mm")
    wa = K.WindowFunctionGalaxy(K.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    wb = K.WindowFunctionConvergence(K.dNdzGaussian(0.0, 2.0, 1.0, 0.2), cm)
    if tag == "wide":
        wc = K.WindowFunctionGalaxy(K.dNdzGaussian(0.0, 1.5, 0.7, 0.2), cm)
    else:
        wc = K.WindowFunctionGalaxy(K.dNdzGaussian(0.5, 1.5, 1.0, 0.2), cm)
    return corr(wa, wb), corr(wc, wc)


def build(ns, tag, ng, ssc):
    ca, cb = pair_of(ns, tag)
    tri = ns.halo_trispectrum.HaloTrispectrumOneHalo(Z_TRI) if ng else None
    cv = ns.covariance.Covariance(ca, cb, nongaussian_cov=ng, ssc_cov=ssc,
                                  input_halo_trispectrum=tri, **KWS)
    assert cv.matching_corrs is False
    cv._initialize_halo_splines()
    return cv, numpy.array([b.center for b in cv.annular_bins])


def all_pairs(nb):
    return [(i, j) for i in range(nb) for j in range(i, nb)] + list(SWAPPED)


def scalars(cv):
    kc = cv.kernel
    return numpy.array([kc.z_bar_NG, cv.D_z_NG, kc.chi_min, kc.chi_max, kc.ln_ktheta_min,
                        kc.ln_ktheta_max, kc._j0_limit, kc._j0_ssc_limit, kc._j1_limit, cv.area,
                        kc.z_min, kc.z_max, cv._z_bar_G_a, cv._z_bar_G_b, cv._D_z_a, cv._D_z_b,
                        Z_TRI])


def ssc_table(ns, cv, out, tag):
    kc = cv.kernel
    kc._initialize_ssc_spline()
    chi = numpy.logspace(numpy.log10(kc.chi_min), numpy.log10(kc.chi_max),
                         ns.defaults.default_precision["corr_npoints"])
    out[tag + "_sigma2_ln_chi"] = numpy.log(chi)
    out[tag + "_sigma2"] = kc._sigma2_spline(numpy.log(chi))
    out[tag + "_ln_ktheta"] = kc._ln_ktheta_array
    out[tag + "_kernel_ssc_array"] = numpy.asarray(kc._kernel_ssc_array, dtype=float)
    a, b = probes(kc)
    out[tag + "_probe_a"], out[tag + "_probe_b"] = a, b
    out[tag + "_ssc_raw"] = numpy.array([kc.raw_kernel_ssc(x, y) for x, y in zip(a, b)],
                                        dtype=float)
    out[tag + "_ssc_spline"] = numpy.array([kc.kernel_ssc(x, y)[0][0] for x, y in zip(a, b)],
                                           dtype=float)


def ng_raw(cv, out, tag):
    kc = cv.kernel
    a, b = probes(kc)
    out[tag + "_ng_raw"] = numpy.array([float(kc.raw_kernel(x, y)) for x, y in zip(a, b)])


def ng_table(cv, out, tag):
    kc = cv.kernel
    t0 = time.time()
    kc._initialize_NG_spline()
    print("  %s: kernel_NG table %.1f s" % (tag, time.time() - t0), file=sys.stderr)
    out[tag + "_kernel_array"] = numpy.asarray(kc._kernel_array, dtype=float)
    out[tag + "_kernel_NG_min"] = numpy.array([float(kc._kernel_NG_min)])
    a, b = probes(kc)
    out[tag + "_ng_spline"] = numpy.array([float(kc.kernel(x, y)[0][0]) for x, y in zip(a, b)])


def ng_pairs(cv, centers, out, tag, pairs):
    tri = cv.halo_tri
    tri._initialize_i_0_4()
    out[tag + "_i_0_4"] = numpy.asarray(tri._i_0_4_array, dtype=float)
    cv._initialize_kb_spline(centers[0], centers[-1])
    out[tag + "_ln_k"] = cv._ln_k_array
    out[tag + "_ng_kb_knots"] = numpy.asarray(cv._kb_spline(cv._ln_k_array), dtype=float)
    out[tag + "_ng_pairs"] = numpy.array(pairs)
    out[tag + "_NG"] = numpy.array([float(cv.covariance_NG(centers[i], centers[j]))
                                    for i, j in pairs])


def g_pairs(cv, centers, out, tag, pairs):
    bins = cv.annular_bins
    out[tag + "_G"] = numpy.array([float(cv.covariance_G(centers[i], centers[j], bins[i].delta,
                                                         bins[j].delta)) for i, j in pairs])


def part(ns, tag, name, fn):
    out = {}

    def flush():
        numpy.savez_compressed(fn, **out)

    with contextlib.redirect_stdout(io.StringIO()):
        if name == "main":
            cv, centers = build(ns, tag, True, True)
            pairs = all_pairs(len(centers))
            out[tag + "_center"] = centers
            out[tag + "_scalars"] = scalars(cv)
            out[tag + "_pairs"] = numpy.array(pairs)
            ssc_table(ns, cv, out, tag)
            ng_raw(cv, out, tag)
            g_pairs(cv, centers, out, tag, pairs)
            flush()
            if tag == "far":
                # the zero table gives 0 * inf in the outer norm: NaN (as G20 "zero")
                out[tag + "_ssc_pairs"] = numpy.array([(0, len(centers) - 1)])
                out[tag + "_ssc"] = numpy.array(
                    [float(cv.covariance_ssc(centers[0], centers[-1]))])
                flush()
                return
            ng_table(cv, out, tag)
            flush()
            ng_pairs(cv, centers, out, tag, pairs)
            flush()
            cv._initialize_kb_ssc_spline(centers[0], centers[-1])
            out[tag + "_ssc_kb_knots"] = numpy.asarray(cv._kb_ssc_spline(cv._ln_k_array),
                                                       dtype=float)
        elif name == "ng":                                   # "far" only
            cv, centers = build(ns, tag, True, False)
            signal.signal(signal.SIGALRM, lambda *a: sys.exit(3))
            signal.alarm(FAR_NG_BUDGET)
            ng_table(cv, out, tag)
            signal.alarm(0)
            flush()
            nb = len(centers)
            ng_pairs(cv, centers, out, tag, [(0, 0), (0, nb - 1), (1, 2), (nb - 1, 0)])
        elif name.startswith("ssc"):
            cv, centers = build(ns, tag, False, True)
            pairs = all_pairs(len(centers))[int(name[3:])::3]
            vals = []
            for i, j in pairs:
                vals.append(float(cv.covariance_ssc(centers[i], centers[j])))
                out[tag + "_ssc_pairs_" + name[3:]] = numpy.array(pairs[:len(vals)])
                out[tag + "_ssc_" + name[3:]] = numpy.array(vals)
                flush()
        elif name == "cov":
            # "far": the super-sample term beside the Gaussian one (the NaN pattern)
            cv, centers = build(ns, tag, tag != "far", True)
            out[tag + "_cov"] = numpy.asarray(cv.get_covariance(), dtype=float)
    flush()


def merge(tmp):
    out = {}
    for p in PARTS:
        fn = os.path.join(tmp, p.replace(":", "_") + ".npz")
        if not os.path.exists(fn):
            print("  missing part", p)
            continue
        with numpy.load(fn) as z:
            out.update({k: z[k] for k in z.files})
    for tag in ("wide", "gal"):
        if tag + "_pairs" not in out:
            continue
        order = [tuple(p) for p in out[tag + "_pairs"]]
        got = {}
        for n in "012":
            for p, v in zip(out.pop(tag + "_ssc_pairs_" + n, []), out.pop(tag + "_ssc_" + n, [])):
                got[tuple(p)] = v
        out[tag + "_ssc"] = numpy.array([got.get(p, numpy.inf) for p in order])   # inf: missing
    save("g30_covariance_cross_terms", **out)


def main():
    args = sys.argv[1:]
    if args[:1] == ["--merge"]:
        return merge(args[1])
    if args[:1] == ["--part"]:
        ns = ref_loader.load()
        ns.correlation.Correlation.__eq__ = lambda s, o: s is o
        tag, name = args[1].split(":")
        fn = os.path.abspath(args[3])
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                t0 = time.time()
                part(ns, tag, name, fn)
                print("  %s: %.1f s" % (args[1], time.time() - t0))
            finally:
                os.chdir(cwd)
        return
    with tempfile.TemporaryDirectory() as tmp:
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--part", p, "--out",
                                   os.path.join(tmp, p.replace(":", "_") + ".npz")])
                 for p in PARTS]
        for p in procs:
            p.wait()
        merge(tmp)


if __name__ == "__main__":
    main()
