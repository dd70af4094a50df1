"""HaloTrispectrum (halo_trispectrum.py:153-837) without a device: a NumPy restatement of the five
mass integrals, their tables and Romberg levels, the four terms and tri_spec_proj_integral on the
oracle's halo tables, checked against the reference's fixture G26; the scope pins, the host-side
argument rules and the ABI constants.  oracle_g26(tag) also gives the GPU test the restatement's
Romberg levels and the terms' cancellation scales (the sums of the absolute values of their
addends), which therefore do not depend on the code under test.
"""
import functools
import os
import warnings

import numpy
import pytest

from conftest import load_golden, rel_err
from params import c_dict_2, h_dict_2
from test_perturbation_cpu import r_bispectrum_len, r_fs2_len, r_trispectrum_par

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("a_", "b_", "c_")
TABLES = ("i_0_4", "i_1_2", "i_1_3", "i_2_1", "i_2_2")
N = 50


def full(tri):
    a = numpy.zeros((N, N))
    iu = numpy.triu_indices(N)
    a[iu] = tri
    a.T[iu] = tri
    return a


class _Restated(object):
    """The reference's HaloTrispectrum on an oracle halo table t (its MassFunctionSecondOrder
    restated here: the sigma(nu) spline and bias_2_norm, mass_function.py:365-434) and the linear
    spectrum P_pt of the PerturbationTheory object's epoch."""

    def __init__(self, t, e_pt):
        from oracle import chomp_oracle as o
        from scipy.interpolate import InterpolatedUnivariateSpline
        self.o, self.t, self.m, self.e_pt = o, t, t.m, e_pt
        m = t.m
        self.sigma_spline = InterpolatedUnivariateSpline(m.nu_arr, m.delta_c / numpy.sqrt(m.nu_arr))
        self.b2norm = 0.0
        self.b2norm = -o._rom(lambda x: o.f_nu(m, x) * self.bias_2(x), m.nu_min, m.nu_max,
                              t.e.prec["mass_precision"], t.e.prec)
        self._y = {}
        self.tab, self.lev = {}, {}

    def bias_2(self, nu):
        m, o = self.m, self.o
        sigma = self.sigma_spline(nu)
        nu_prime = nu * m.st_a
        return self.b2norm + (
            8.0 / 21.0 * (o.bias_nu(m, nu) - 1.0) + (nu - 3.0) / (sigma * sigma) +
            2.0 * m.stq / (m.delta_c ** 2 * (1.0 + nu_prime ** m.stq)) *
            (2.0 * m.stq + 2 * nu_prime - 1.0))

    def y(self, ln_k, ln_nu):
        key = (float(ln_k), ln_nu.tobytes())
        if key not in self._y:
            self._y[key] = self.o.y_nfw(self.t, ln_k, self.o.mass_of_nu(self.m, numpy.exp(ln_nu)))
        return self._y[key]

    # -- the five integrands (:615-623, 682-688, 737-745, 779-784, 830-836) -----------------
    def integrand(self, ln_nu, name, lks, norm):
        o, m = self.o, self.m
        ln_nu = numpy.atleast_1d(numpy.asarray(ln_nu, dtype=float))
        nu = numpy.exp(ln_nu)
        mass = o.mass_of_nu(m, nu)
        ys = [self.y(lk, ln_nu) for lk in lks]
        nf = nu * o.f_nu(m, nu)
        if name == "i_0_4":
            return nf * ys[0] * ys[1] * ys[2] * ys[3] * mass * mass * mass * norm
        if name == "i_1_2":
            return nf * o.bias_nu(m, nu) * ys[0] * ys[1] * mass * norm
        if name == "i_1_3":
            return nf * o.bias_nu(m, nu) * ys[0] * ys[1] * ys[2] * mass * mass * norm
        if name == "i_2_1":
            return nf * self.bias_2(nu) * ys[0] * norm
        return nf * self.bias_2(nu) * ys[0] * ys[1] * mass * norm          # i_2_2

    def romberg(self, name, lks, norm):
        from oracle.romberg import romberg
        prec = self.t.e.prec
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            val, level = romberg(self.integrand, numpy.log(self.m.nu_min), numpy.log(self.m.nu_max),
                                 args=(name, lks, norm), vec_func=True,
                                 tol=prec["global_precision"], rtol=prec["halo_precision"],
                                 divmax=prec["divmax"], return_level=True)
        return float(numpy.ravel(val)[0]), level

    def entry(self, name, i, j):
        """One table entry as its _initialize_* loop forms it, quirks included."""
        lk, rb = self.t.ln_k, self.t.rho_bar
        a, b = lk[i], lk[j]
        if name == "i_0_4":                                   # :592-613, 566-583
            ka, kb = numpy.log(numpy.exp(a)), numpy.log(numpy.exp(b))
            args = (ka, ka, kb, kb)
            norm = 1.0 / self.integrand(0.0, name, args, 1.0)[0]
            v, lv = self.romberg(name, args, norm)
            return v / (rb * rb * rb * norm), lv
        if name == "i_1_2":                                   # :655-680
            norm = 1.0 / self.integrand(0.0, name, (a, b), 1.0)[0]
            v, lv = self.romberg(name, (a, b), norm)
            return v / rb / norm, lv
        if name == "i_1_3":                                   # :714-735, 690-705: I(k_i, k_i, k_j)
            ka, kb = numpy.log(numpy.exp(a)), numpy.log(numpy.exp(b))
            norm = 1.0 / self.integrand(0.0, name, (ka, ka, kb), 1.0)[0]
            v, lv = self.romberg(name, (ka, ka, kb), norm)
            return v / (rb * rb * norm), lv
        if name == "i_2_1":                                   # :761-777: the raw integrand, / norm
            norm = 1.0 / self.integrand(0.0, name, (a,), 1.0)[0]
            v, lv = self.romberg(name, (a,), 1.0)
            return v / norm, lv
        norm = 1.0 / self.integrand(0.0, name, (a, b), 1.0)[0]     # :802-828: norm of (k_i, k_j),
        v, lv = self.romberg(name, (b, b), norm)                    # integrand of (k_j, k_j)
        return v / rb / norm, lv

    def build(self):
        from scipy.interpolate import InterpolatedUnivariateSpline, RectBivariateSpline
        lk = self.t.ln_k
        for name in TABLES:
            if name == "i_2_1":
                r = [self.entry(name, i, i) for i in range(N)]
                self.tab[name] = numpy.array([v for v, _ in r])
                self.lev[name] = numpy.array([lv for _, lv in r])
                continue
            tab, lev = numpy.empty((N, N)), numpy.empty((N, N))
            for i in range(N):
                for j in range(i, N):
                    tab[i, j], lev[i, j] = self.entry(name, i, j)
                    tab[j, i], lev[j, i] = tab[i, j], lev[i, j]
            self.tab[name], self.lev[name] = tab, lev
        self.sp = {n: RectBivariateSpline(lk, lk, self.tab[n]) for n in TABLES if n != "i_2_1"}
        self.sp1 = InterpolatedUnivariateSpline(lk, self.tab["i_2_1"])
        return self

    # -- look-ups (:585-590, 649-653, 707-712, 757-759, 796-800) --------------------------------
    def look(self, name, k1, k2):
        t = self.t
        k1 = max(k1, t.k_min)
        k2 = max(k2, t.k_min)
        if not (k1 <= t.k_max and k2 <= t.k_max):
            return 0.0
        return float(self.sp[name](numpy.log(k1), numpy.log(k2))[0, 0])

    def i_2_1(self, k):
        k = max(k, self.t.k_min)
        return float(self.sp1(numpy.log(k))) if k <= self.t.k_max else 0.0

    def h_m(self, k):
        return float(self.o._ranged(self.t, self.t.h_m_spline, k))

    def p_h(self, k):
        with numpy.errstate(all="ignore"):
            return self.o.linear_power(self.t.e, k)

    def p_pt(self, k):
        with numpy.errstate(all="ignore"):
            return self.o.linear_power(self.e_pt, k)

    # -- the terms (:320-512): values and the sums of |addend| ------------------------------
    def terms(self, k1, k2, z):
        """t_1_h .. t_4_h at scalars k1, k2 and z (scalar or array): ([4, ...], [4, ...])."""
        A = numpy.abs
        z = numpy.asarray(z, dtype=float)
        k1, k2 = numpy.float64(k1), numpy.float64(k2)
        h1, h2, P1, P2 = self.h_m(k1), self.h_m(k2), self.p_h(k1), self.p_h(k2)
        i12 = self.look("i_1_2", k1, k2)
        i13_112, i13_221 = self.look("i_1_3", k1, k2), self.look("i_1_3", k2, k1)
        i22_1, i22_2 = self.look("i_2_2", k1, k1), self.look("i_2_2", k2, k2)
        i22_12 = self.look("i_2_2", k1, k2)
        one = numpy.ones(z.shape)
        t1 = self.look("i_0_4", k1, k2) * one
        with numpy.errstate(all="ignore"):
            a31 = (2.0 * (P1 * i13_221 * h1), 2.0 * (P2 * i13_112 * h2))
            pm = self.p_h(numpy.sqrt(k1 * k1 + k2 * k2 - 2.0 * k1 * k2 * z))
            pp = self.p_h(numpy.sqrt(k1 * k1 + k2 * k2 + 2.0 * k1 * k2 * z))
            t22 = (2.0 * i12 * i12 * pm, 2.0 * i12 * i12 * pp)
            t2 = a31[0] + a31[1] + (t22[0] + t22[1])
            s2 = (A(a31[0]) + A(a31[1])) * one + A(t22[0]) + A(t22[1])
            lenplus = numpy.sqrt(k1 * k1 + 2.0 * k1 * k2 * z + k2 * k2)
            lenminus = numpy.sqrt(k1 * k1 - 2.0 * k1 * k2 * z + k2 * k2)
            z1p = numpy.where(lenplus > 0.0, (k1 * k1 + k1 * k2 * z) / (k1 * lenplus), 0.0)
            z2p = numpy.where(lenplus > 0.0, (k2 * k2 + k1 * k2 * z) / (k2 * lenplus), 0.0)
            z1m = numpy.where(lenminus > 0.0, (k1 * k1 - k1 * k2 * z) / (k1 * lenminus), 0.0)
            z2m = numpy.where(lenminus > 0.0, (k2 * k2 - k1 * k2 * z) / (k2 * lenminus), 0.0)
            perm_1 = P1 * P1 * i22_2 * h1 * h1
            perm_2 = P2 * P2 * i22_1 * h2 * h2
            bl = r_bispectrum_len(self.p_pt, k1 * one, k2 * one, lenplus, z, -z1p, -z2p)
            f2 = r_fs2_len(k1 * one, k2 * one, z)
            bp = numpy.where(lenplus > 1e-8, bl[0], 2.0 * (f2[0] * P1 * P2))
            bps = numpy.where(lenplus > 1e-8, bl[1], 2.0 * (f2[1] * P1 * P2))
            bm = r_bispectrum_len(self.p_pt, k1 * one, k2 * one, lenminus, -z, -z1m, -z2m)
            two = P1 * P2 * i22_12 * h1 * h2
            w = i12 * h1 * h2
            t3 = perm_1 + perm_2 + 2.0 * ((bp * w + two) + (bm[0] * w + two))      # perm_4: unguarded
            s3 = (A(perm_1) + A(perm_2)) * one + 2.0 * (bps * A(w) + bm[1] * A(w) + 2.0 * A(two))
            tp = r_trispectrum_par(self.p_pt, k1 * one, k2 * one, z)
            c1 = self.i_2_1(k1) * P1 * P2 * P2
            c2 = self.i_2_1(k2) * P2 * P1 * P1
            hh = h1 * h1 * h2 * h2
            t4 = hh * (tp[0] + 2.0 * (c1 + c2))
            s4 = hh * (tp[1] + 2.0 * (A(c1) + A(c2)))
        return numpy.array([t1, t2, t3, t4]), numpy.array([A(t1), s2, s3, s4])

    def proj(self, k1, k2):
        """tri_spec_proj_integral (:267-278): (value, level, scale).  The scale is |t_1_h| +
        2 / pi times the trapezoid sum of the three terms' addend scales over the nodes the
        Romberg stopped on: the quantity whose cancellation the quadrature's own sum carries."""
        from oracle.romberg import romberg
        prec = self.t.e.prec

        def wrap(theta, norm):
            v = self.terms(k1, k2, numpy.cos(theta))[0]
            return (v[1] + v[2] + v[3]) * norm
        with numpy.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            norm = 1.0 / wrap(numpy.pi / 2.0, 1.0)
            val, level = romberg(wrap, 0.0, numpy.pi, args=(norm,), vec_func=True,
                                 rtol=prec["halo_precision"], tol=prec["global_precision"],
                                 divmax=prec["divmax"], return_level=True)
            t1 = self.look("i_0_4", k1, k2)
            value = t1 + 2.0 * float(val) / (norm * numpy.pi)
            if not numpy.isfinite(value):
                return numpy.nan, level, numpy.nan
            th = numpy.linspace(0.0, numpy.pi, 2 ** level + 1)
            s = self.terms(k1, k2, numpy.cos(th))[1][1:].sum(axis=0)
            w = numpy.full(th.size, th[1] - th[0])
            w[0] = w[-1] = 0.5 * (th[1] - th[0])
        return value, level, abs(t1) + 2.0 / numpy.pi * float(numpy.sum(w * s))


@functools.lru_cache(maxsize=None)
def oracle_g26(tag):
    """The restatement of case `tag` of G26: a dictionary with the built _Restated object "r",
    "terms" and "scales" [n, 4] at the fixture's configurations, and "proj", "proj_levels",
    "proj_scales" at its pairs."""
    from oracle import chomp_oracle as o
    g = load_golden("g26_trispectrum")
    if tag == "c_":
        e = o.epoch(c_dict_2, 0.3)
        t = o.halo_table(e, o.mass_table(e, h_dict_2), halo_dict=h_dict_2)
        e_pt = e                                            # (set_cosmology realigned pert)
    else:
        e = o.epoch(None, 0.0 if tag == "a_" else 0.5)
        t = o.halo_table(e, o.mass_table(e))
        e_pt = o.epoch(None, 0.0)                           # (PerturbationTheory(): z = 0)
    r = _Restated(t, e_pt).build()
    tv = [r.terms(*c) for c in g["configs"]]
    pj = [r.proj(a, b) for a, b in g["pairs"]]
    return {"r": r, "terms": numpy.array([v for v, _ in tv]), "scales": numpy.array([s for _, s in tv]),
            "proj": numpy.array([p[0] for p in pj]), "proj_levels": numpy.array([p[1] for p in pj]),
            "proj_scales": numpy.array([p[2] for p in pj])}


@pytest.fixture(scope="module")
def g():
    return numpy.load(os.path.join(HERE, "golden", "g26_trispectrum.npz"))


@pytest.mark.parametrize("tag", CASES)
def test_g26_tables_against_restatement(g, tag):
    r = oracle_g26(tag)["r"]
    assert abs(r.t.rho_bar / float(g[tag + "rho_bar"]) - 1) < 1e-12
    for name in TABLES:
        tab = r.tab[name] if name == "i_2_1" else r.tab[name][numpy.triu_indices(N)]
        lev = r.lev[name] if name == "i_2_1" else r.lev[name][numpy.triu_indices(N)]
        ref = g[tag + name]
        err = numpy.max(numpy.abs(tab - ref)) / numpy.max(numpy.abs(ref))
        print("%s%s: %.3e of scale, %d levels differ" % (tag, name, err,
                                                       int(numpy.sum(lev != g[tag + name + "_levels"]))))
        assert err < 1e-10
        assert numpy.array_equal(lev, g[tag + name + "_levels"])


@pytest.mark.parametrize("tag", CASES)
def test_g26_terms_against_restatement(g, tag):
    d = oracle_g26(tag)
    ref = g[tag + "terms"]
    with numpy.errstate(all="ignore"):
        rel = numpy.where(d["scales"] > 0, numpy.abs(d["terms"] - ref) / d["scales"],
                          numpy.abs(d["terms"] - ref))
    assert numpy.all(numpy.isfinite(rel))
    print("%sterms: %s" % (tag, rel.max(axis=0)))
    assert rel.max() < 1e-9
    fin = numpy.isfinite(g[tag + "proj"])
    assert numpy.array_equal(numpy.isfinite(d["proj"]), fin)
    assert numpy.array_equal(d["proj_levels"], g[tag + "proj_levels"])
    prel = numpy.abs(d["proj"][fin] - g[tag + "proj"][fin]) / d["proj_scales"][fin]
    print("%sproj: %s" % (tag, prel))
    assert prel.max() < 1e-9


def _build(z=0.0):
    from chomp_amd import cosmology, halo_trispectrum, mass_function
    cosmo = cosmology.SingleEpoch(z)
    return halo_trispectrum.HaloTrispectrum(z, cosmo,
                                            mass_function.MassFunctionSecondOrder(z, cosmo))


def test_constructs_with_second_order_mass_function():
    from chomp_amd import perturbation_spectra
    h = _build(0.5)
    assert isinstance(h.pert, perturbation_spectra.PerturbationTheory)
    assert h.pert._redshift == 0.0 and h._redshift == 0.5      # (never aligned by the constructor)
    for name in TABLES:
        assert getattr(h, "_initialized_" + name) is False
    assert h._initialzied_PT_averaged is False and h._initialized_tri_proj is False
    for name in ("t_1_h", "t_2_h", "t_3_h", "t_4_h", "t_PT", "trispectrum_parallelogram",
                 "tri_spec_proj_integral", "i_0_4", "i_0_4_parallelogram", "i_1_1", "i_1_2",
                 "i_1_3", "i_1_3_parallelogram", "i_2_1", "i_2_2", "set_cosmology", "set_redshift",
                 "terms_many", "tri_spec_proj_integral_many"):
        assert callable(getattr(h, name))


def test_scope_pins():
    from chomp_amd import _lib, cosmology, halo_trispectrum, mass_function
    with pytest.raises(_lib.ChompScopeError) as exc:
        halo_trispectrum.HaloTrispectrum(0.0)
    assert "MassFunctionSecondOrder" in str(exc.value)
    cosmo = cosmology.SingleEpoch(0.0)
    with pytest.raises(_lib.ChompScopeError):
        halo_trispectrum.HaloTrispectrum(0.0, cosmo, mass_function.MassFunction(0.0, cosmo))
    h = _build()
    for call in (lambda: h.trispectrum_projected(0.1, 1.0), h._initialize_tri_proj,
                 lambda: h.t_PT_averaged(0.1, 1.0), h._initialize_PT_averaged):
        with pytest.raises(_lib.ChompScopeError) as exc:
            call()
        assert "NaN" in str(exc.value)


def test_different_transfer_functions_are_refused():
    """One device context has one transfer function: a halo model and a PerturbationTheory object
    that differ in with_bao are outside the scope (the refusal comes before any device work)."""
    from chomp_amd import _lib, cosmology, halo_trispectrum, mass_function, perturbation_spectra
    cosmo = cosmology.SingleEpoch(0.0)
    pert = perturbation_spectra.PerturbationTheory(0.0, cosmology.SingleEpoch(0.0, with_bao=True))
    h = halo_trispectrum.HaloTrispectrum(
        0.0, cosmo, mass_function.MassFunctionSecondOrder(0.0, cosmo), pert)
    with pytest.raises(_lib.ChompScopeError):
        h.t_2_h(0.1, 1.0, 0.3)


def test_set_cosmology_resets_flags_and_realigns_pert():
    h = _build()
    for name in TABLES:
        setattr(h, "_initialized_" + name, True)
    h._tables_built = True
    h.set_cosmology(c_dict_2, 0.3)
    assert not any(getattr(h, "_initialized_" + n) for n in TABLES)
    assert h._tables_built is False
    assert h.pert.cosmo is h.cosmo and h.pert._redshift == 0.3
    h._initialized_i_1_2 = True
    h.set_redshift(0.3)                    # (unlike Halo.set_redshift: always through set_cosmology)
    assert h._initialized_i_1_2 is False


def test_many_argument_validation():
    h = _build()
    for bad in (numpy.ones(3), numpy.ones((4, 2)), numpy.ones((2, 3, 1))):
        with pytest.raises(ValueError):
            h.terms_many(bad)
    for bad in (numpy.ones(2), numpy.ones((4, 3))):
        with pytest.raises(ValueError):
            h.tri_spec_proj_integral_many(bad)
    with pytest.raises(ValueError):
        h.i_1_3_many(numpy.ones((4, 4)))


def test_abi_constants():
    from chomp_amd import _lib
    for name in ("chomp_tri_setup", "chomp_tri_table_eval", "chomp_tri_terms", "chomp_tri_proj",
                 "chomp_tri_triple"):
        assert name in _lib.EXPORTS
    assert _lib.ST_TRI_DIVMAX == 0x4000
    assert any("tri_spec_proj_integral" in s for s in _lib.describe_status(_lib.ST_TRI_DIVMAX))
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include",
                            "chomp_mi355x.h")).read()
    assert "#define CHOMP_ST_TRI_DIVMAX 0x4000u" in hdr
    for name, code in _lib.TRI_TAB.items():
        assert "#define CHOMP_TRI_TAB_%s %d" % (name.upper(), code) in hdr


def test_fixture_shape(g):
    cfg, pairs = g["configs"], g["pairs"]
    assert cfg.shape[1] == 3 and cfg.shape[0] >= 40
    same = cfg[:, 0] == cfg[:, 1]
    assert not numpy.any(same & (cfg[:, 2] == 1.0))       # (the reference raises there)
    assert numpy.any(same & (numpy.abs(cfg[:, 2]) < 1)) and numpy.any(numpy.all(cfg == [1, 1, -1], axis=1))
    for tag in CASES:
        for name in TABLES:
            n = 50 if name == "i_2_1" else 1275
            assert g[tag + name].shape == (n,) and g[tag + name + "_levels"].shape == (n,)
            assert g[tag + name + "_levels"].max() < 20      # (no divmax)
        assert numpy.all(numpy.isfinite(g[tag + "terms"]))
        proj = g[tag + "proj"]
        # NaN for k1 = k2 (the theta = 0 end point) and where a k lies above k_max (the integrand
        # is 0 there and norm = 1 / 0)
        assert numpy.array_equal(numpy.isnan(proj),
                                 (pairs[:, 0] == pairs[:, 1]) | (pairs.max(axis=1) > 100.0))
        assert numpy.all(g[tag + "proj_levels"][numpy.isnan(proj)] == 20)
    assert g["b_pert_redshift"] == 0.0 and g["b_redshift"] == 0.5
    assert g["c_pert_redshift"] == 0.3
    assert not numpy.any(g["c_flags_after_set"])


@pytest.mark.parametrize("tag", CASES)
def test_range_rules_in_fixture(g, tag):
    """k > k_max gives exact zeros; k < k_min the value at k_min."""
    cfg, look, hm = g["configs"], g[tag + "lookups"], g[tag + "h_m"]
    k1, k2 = cfg[:, 0], cfg[:, 1]
    above = (k1 > 100.0) | (k2 > 100.0)
    assert numpy.all(look[above][:, :4] == 0.0) and numpy.all(look[~above][:, :4] != 0.0)
    assert numpy.all(look[k1 > 100.0, 4] == 0.0) and numpy.all(look[k2 > 100.0, 5] == 0.0)
    assert numpy.all(hm[(k1 < 0.001) | (k1 > 100.0)] == 0.0)
    i = numpy.where(numpy.all(cfg == [0.001, 1.0, 0.3], axis=1))[0][0]
    j = numpy.where(numpy.all(cfg == [5e-4, 1.0, 0.3], axis=1))[0][0]
    assert numpy.array_equal(look[i], look[j])
    # t_1_h is symmetric, t_4_h vanishes where _h_m does
    t = g[tag + "terms"]
    assert numpy.all(t[(k1 < 0.001) | (k1 > 100.0) | (k2 < 0.001) | (k2 > 100.0), 3] == 0.0)
