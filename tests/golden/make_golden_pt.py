#!/usr/bin/env python3
"""Generate tests/golden/g23_perturbation.npz by RUNNING THE REFERENCE's PerturbationTheory
(perturbation_spectra.py:36-345) and MassFunctionSecondOrder (mass_function.py:365-434), and a
Halo built on the latter.

Development-container only, like make_golden.py (whose helpers it imports; that file is not
changed).  Run from anywhere:  python tests/golden/make_golden_pt.py

The configurations are seeded: a few hundred random ones per form, then the edge cases (a zero
vector, k1 = -k2, |k| < 1e-8, k < 1e-16, collinear vectors; for the scalar forms lengths below
the thresholds and mu = +-1).  The Romberg stopping levels of the mass function's three
normalisations and of the Halo's knot integrals are recorded (make_golden_hod.LevelLog).
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
from make_golden import save  # noqa: E402
from make_golden_hod import LevelLog, k_samples  # noqa: E402
from params import c_dict_2, h_dict_2  # noqa: E402

warnings.simplefilter("ignore")

N_RANDOM = 256
REDSHIFTS = (0.0, 0.5)
VECTOR_FORMS = {"Fs2": 2, "Fs3": 3, "F3": 3, "Fs3_BCGS": 3, "bispectrum": 3, "trispectrum": 4}
SCALAR_FORMS = {"Fs2_len": 3, "Fs2_kdiff": 3, "Fs3_parallelogram": 3, "bispectrum_len": 6,
                "trispectrum_parallelogram": 3}
HALO_INTEGRANDS = ("_h_m_integrand", "_pp_mm_integrand", "_h_g_integrand", "_pp_gm_integrand",
                   "_pp_gg_integrand")


def random_vectors(rng, n):
    """n wavevectors: lengths log-uniform in [1e-3, 10] h/Mpc, isotropic directions."""
    length = 10.0 ** rng.uniform(-3.0, 1.0, n)
    d = rng.normal(size=(n, 3))
    d /= numpy.sqrt((d * d).sum(axis=1))[:, None]
    return d * length[:, None]


def vector_configs(rng, nvec):
    """[N, nvec, 3]: random configurations, then the edge cases."""
    out = [random_vectors(rng, N_RANDOM * nvec).reshape(N_RANDOM, nvec, 3)]
    base = random_vectors(rng, 6 * nvec).reshape(6, nvec, 3)
    edges = []
    for j in range(nvec):                        # a zero vector in each slot
        c = base[0].copy()
        c[j] = 0.0
        edges.append(c)
    c = base[1].copy()
    c[1] = -c[0]                                 # k1 = -k2
    edges.append(c)
    if nvec >= 3:
        c = base[1].copy()
        c[2] = -c[1]                             # k2 = -k3
        edges.append(c)
    c = base[2].copy()
    c[0] *= 5e-9 / numpy.sqrt(c[0] @ c[0])       # |k1| < 1e-8
    edges.append(c)
    c = base[3].copy()
    c[1] *= 1e-17 / numpy.sqrt(c[1] @ c[1])      # |k2| < 1e-16 (P_lin = 1e-16)
    edges.append(c)
    c = base[4].copy()
    for j in range(1, nvec):                     # collinear
        c[j] = (j + 1.5) * c[0]
    edges.append(c)
    c = base[5].copy()
    c[-1] = -c[:-1].sum(axis=0)                  # a closed polygon (k1 + ... + kn = 0)
    edges.append(c)
    c = numpy.zeros((nvec, 3))                   # every vector zero
    edges.append(c)
    return numpy.concatenate([out[0], numpy.array(edges)])


def scalar_configs(rng, form):
    k = 10.0 ** rng.uniform(-3.0, 1.0, (N_RANDOM, 3))
    mu = rng.uniform(-1.0, 1.0, (N_RANDOM, 3))
    if form == "bispectrum_len":
        rand = numpy.concatenate([k, mu], axis=1)
        edges = [[5e-9, 0.1, 0.2, 0.3, -0.2, 0.5], [0.1, 5e-9, 0.2, 0.3, -0.2, 0.5],
                 [1e-17, 0.1, 0.2, 0.3, -0.2, 0.5], [0.1, 0.2, 0.0, 1.0, -1.0, 1.0],
                 [0.1, 0.1, 0.1, 1.0, 1.0, -1.0]]
    else:
        rand = numpy.stack([k[:, 0], k[:, 1], mu[:, 0]], axis=1)
        edges = [[5e-9, 0.1, 0.3], [0.1, 5e-9, 0.3], [1e-17, 0.1, 0.3], [0.1, 1e-17, -0.3],
                 [0.1, 0.2, 1.0], [0.1, 0.2, -1.0], [0.2, 0.1, 1.0], [0.1, 0.1, 1.0],
                 [0.1, 0.1, -1.0], [0.0, 0.1, 0.5], [0.1, 0.0, 0.5]]
    return numpy.concatenate([rand, numpy.array(edges, dtype=float)])


def g23_pt(ns, out):
    rng = numpy.random.default_rng(23)
    cfg = {}
    for form, nvec in VECTOR_FORMS.items():
        cfg[form] = vector_configs(rng, nvec)
    for form in SCALAR_FORMS:
        cfg[form] = scalar_configs(rng, form)
    for form, a in cfg.items():
        out["pt_args_" + form] = a.reshape(a.shape[0], -1)
    cosmos = (("def_", ns.defaults.default_cosmo_dict), ("c2_", c_dict_2))
    for tag, cd in cosmos:
        for z in REDSHIFTS:
            pt = ns.perturbation_spectra.PerturbationTheory(z, ns.cosmology.SingleEpoch(z, cd))
            zt = "%sz%03d_" % (tag, int(round(100 * z)))
            for form in VECTOR_FORMS:
                fn = getattr(pt, form)
                out[zt + form] = numpy.array([fn(*[numpy.array(v) for v in c]) for c in cfg[form]],
                                             dtype=float)
            for form in SCALAR_FORMS:
                fn = getattr(pt, form)
                a = cfg[form]
                out[zt + form] = numpy.array([fn(*[numpy.float64(x) for x in row]) for row in a],
                                             dtype=float)
    # the quirks
    e = ns.cosmology.SingleEpoch(0.0)
    pt = ns.perturbation_spectra.PerturbationTheory(0.5, e)
    out["quirk_moved_redshift"] = e._redshift
    try:
        pt.set_redshift(1.0)
        out["quirk_set_redshift_raises"] = 0
    except AttributeError as exc:
        out["quirk_set_redshift_raises"] = 1
        out["quirk_set_redshift_message"] = str(exc)
    out["quirk_redshift_after"] = pt._redshift


def g23_mass(ns, out):
    d = ns.defaults
    k = k_samples(d.default_limits["k_min"], d.default_limits["k_max"])
    out["k"] = k
    halos = (("hdef_", d.default_halo_dict), ("h2_", h_dict_2))
    masses = numpy.logspace(9.0, 16.0, 29)
    out["b2_masses"] = masses
    for tag, hd in halos:
        for z in REDSHIFTS:
            zt = "%sz%03d_" % (tag, int(round(100 * z)))
            with LevelLog(ns.mass_function.integrate) as log:
                mf = ns.mass_function.MassFunctionSecondOrder(z, ns.cosmology.SingleEpoch(z), hd)
            out[zt + "norm_levels"] = numpy.array(log.levels["f_nu"] + log.levels["<lambda>"])
            out[zt + "bias_2_norm"] = mf.bias_2_norm
            out[zt + "f_norm"], out[zt + "bias_norm"] = mf.f_norm, mf.bias_norm
            out[zt + "nu_min"], out[zt + "nu_max"] = mf.nu_min, mf.nu_max
            out[zt + "sigma_array"] = mf._sigma_array
            out[zt + "nu_array"] = mf._nu_array
            out[zt + "ln_mass_array"] = mf._ln_mass_array
            nu = numpy.concatenate([[0.02, 0.05, 0.09], numpy.geomspace(mf.nu_min, mf.nu_max, 25),
                                    [60.0, 100.0]])
            out[zt + "probe_nu"] = nu
            out[zt + "bias_2_nu"] = mf.bias_2_nu(nu)
            out[zt + "sigma_spline"] = mf._sigma_spline(nu)
            out[zt + "bias_2_mass"] = numpy.array([mf.bias_2_mass(m) for m in masses])
    # a Halo on the subclass (what HaloTrispectrum builds)
    for z in REDSHIFTS:
        zt = "halo_z%03d_" % int(round(100 * z))
        with LevelLog(ns.halo.integrate) as hl:
            mf = ns.mass_function.MassFunctionSecondOrder(z, ns.cosmology.SingleEpoch(z))
            h = ns.halo.Halo(z, None, ns.cosmology.SingleEpoch(z), mf)
            lk = h._ln_k_array
            out[zt + "power_mm"] = h.power_mm(k)
            out[zt + "power_gm"] = h.power_gm(k)
            out[zt + "power_gg"] = h.power_gg(k)
            for name in ("h_m", "pp_mm", "h_g", "pp_gm", "pp_gg"):
                out[zt + name] = getattr(h, "_%s_spline" % name)(lk)
        for name in HALO_INTEGRANDS:
            out[zt + "levels" + name] = numpy.array(hl.levels[name])
        out[zt + "nu_array"] = mf._nu_array
        out[zt + "n_bar"] = h.n_bar


def main():
    ns = ref_loader.load()
    cwd = os.getcwd()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            t0 = time.time()
            g23_pt(ns, out)
            print("  pt: %.1f s" % (time.time() - t0))
            t0 = time.time()
            g23_mass(ns, out)
            print("  mass: %.1f s" % (time.time() - t0))
        finally:
            os.chdir(cwd)
    save("g23_perturbation", **out)


if __name__ == "__main__":
    main()
