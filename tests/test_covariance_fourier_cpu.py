"""CovarianceFourier (covariance.py:874-1083) without a device: a NumPy restatement of the
algorithm -- z_bar of the four window pairs, the norms with their quirks, the 4 x corr_npoints
Romberg integrals, the splines of their logarithms, _pl_X and covariance_G -- built on
oracle/romberg.py and the oracle's MultiEpoch, windows and halo model, against the reference's
fixture G31 (tests/golden/make_golden_cov_fourier.py); the constructor, the scope errors and the
new entry points of the class itself.

Bar: 1e-6 relative, the project's bar for intermediates; z_bar exactly.
"""
import functools
import os
import re

import numpy
import pytest
from scipy.interpolate import InterpolatedUnivariateSpline

from conftest import ROOT, load_golden

RTOL = 1e-6
PAIRS = ("a1a2", "b1b2", "a1b2", "b1a2")
CASES = ("auto", "mix", "tomo")
L_MIN, L_MAX = 10.0, 1.0e4
NAMES = ("chomp_covariance_fourier_zbar", "chomp_covariance_fourier_table",
         "chomp_covariance_fourier_gaussian")


# -- the restatement ------------------------------------------------------------------------
def windows(tag, me):
    """The oracle's tables of the fixture's four windows a1, a2, b1, b2 on the MultiEpoch."""
    from oracle import chomp_oracle as o
    conv = lambda: o.window_table("convergence", o.dndz_gaussian(0.0, 2.0, 1.0, 0.2), me)
    if tag == "auto":
        w = conv()
        return w, w, w, w
    if tag == "mix":
        g, c = o.window_table("galaxy", o.dndz_maglim(0.0, 2.0, 2.0, 0.3, 2.0), me), conv()
        return g, c, g, c
    a = o.window_table("galaxy", o.dndz_gaussian(0.5, 1.5, 1.0, 0.2), me)
    b = o.window_table("galaxy", o.dndz_gaussian(0.2, 1.0, 0.6, 0.15), me)
    return a, a, b, b


@functools.lru_cache(maxsize=None)
def halo_at(z, with_bao=False):
    """The oracle's halo model (P_mm tables) at redshift z: one independent object per z_bar."""
    from oracle import chomp_oracle as o
    return o.halo_table(e=o.epoch(redshift=z, with_bao=with_bao), families=("mm",))


class Restatement(object):
    """covariance.py:874-1083 with four independent halos.  The first two keywords switch single
    quirks off, for the test that pins them; `extrapolate` is Halo(extrapolate=True), `with_bao` a
    halo on SingleEpoch(with_bao=True) that stands at z_bar already (set_redshift would drop it)."""

    def __init__(self, tag, norm_windows_of_pair=False, norm_halo_of_pair=False,
                 extrapolate=False, with_bao=False):
        from oracle import chomp_oracle as o
        self.o = o
        self.extrapolate = extrapolate
        self.me = me = o.multi_epoch(0.0, 5.0)
        self.prec = p = me.prec
        self.w = dict(zip(("a1", "a2", "b1", "b2"), windows(tag, me)))
        self.ln_l_min, self.ln_l_max = numpy.log(L_MIN), numpy.log(L_MAX)
        self.ln_l = numpy.linspace(self.ln_l_min, self.ln_l_max, p["corr_npoints"])
        self.z_min = {x: max(self.w[x[:2]].z_min, self.w[x[2:]].z_min) for x in PAIRS}
        self.z_max = {x: min(self.w[x[:2]].z_max, self.w[x[2:]].z_max) for x in PAIRS}
        self.z_array = numpy.linspace(min(self.z_min.values()), max(self.z_max.values()),
                                      p["kernel_npoints"])
        # _calculate_zbar (:1067-1075): the first argmax
        chi = o.me_chi(me, self.z_array)
        self.z_bar = {}
        for x in PAIRS:
            D = self.growth(chi)
            f = o.window(self.w[x[:2]], chi) * o.window(self.w[x[2:]], chi) / (chi * chi) * D * D
            self.z_bar[x] = float(self.z_array[numpy.argmax(f)])
        self.halo = {x: halo_at(self.z_bar[x], with_bao) for x in PAIRS}
        self.D_bar = {x: float(o.me_growth(me, self.z_bar[x])) for x in PAIRS}
        # the norms (:987-1006): a1 and a2 whatever the pair; halo_a1a2 for a1b2
        self.norm = {}
        for x in PAIRS:
            c = float(o.me_chi(me, self.z_bar[x]))
            h = self.halo[x if (x != "a1b2" or norm_halo_of_pair) else "a1a2"]
            w1, w2 = (x[:2], x[2:]) if norm_windows_of_pair else ("a1", "a2")
            self.norm[x] = 1.0 / float(self.integrand(c, numpy.log(c), h, w1, w2, 1.0))
        self._tables = None

    def growth(self, chi):
        return self.o.me_growth(self.me, self.me.z_spline(chi))

    def integrand(self, chi, ln_l, h, w1, w2, norm):
        """_pl_integrand (:1077-1083)."""
        o = self.o
        k = numpy.exp(ln_l) / chi
        D = self.growth(chi)
        return (norm * o.window(self.w[w1], chi) * o.window(self.w[w2], chi) * D * D /
                (chi * chi) * o.halo_power(h, "mm", k, extrapolate=self.extrapolate))

    def tables(self):
        """(integral / D(z_bar)^2 [4, N], Romberg levels [4, N]): _initialize_pl (:1008-1063)."""
        if self._tables is None:
            from oracle.romberg import romberg
            o, p = self.o, self.prec
            tab = numpy.empty((4, self.ln_l.size))
            lev = numpy.empty((4, self.ln_l.size), dtype=int)
            for i, x in enumerate(PAIRS):
                lo = float(o.me_chi(self.me, self.z_min[x]))
                hi = float(o.me_chi(self.me, self.z_max[x]))
                for j, ln_l in enumerate(self.ln_l):
                    v, lev[i, j] = romberg(
                        self.integrand, lo, hi,
                        args=(ln_l, self.halo[x], x[:2], x[2:], self.norm[x]), vec_func=True,
                        tol=p["global_precision"], rtol=p["corr_precision"], divmax=p["divmax"],
                        return_level=True)
                    tab[i, j] = v / self.D_bar[x] ** 2
            self._tables = tab, lev
        return self._tables

    def pl(self, x, ell):
        i = PAIRS.index(x)
        spline = InterpolatedUnivariateSpline(self.ln_l, numpy.log(self.tables()[0][i]))
        ln_l = numpy.log(ell)
        return numpy.where(numpy.logical_and(ln_l >= self.ln_l_min, ln_l <= self.ln_l_max),
                           numpy.exp(spline(ln_l)) / self.norm[x], 0.0)

    def covariance_G(self, ell):
        return 1.0 / (2.0 * ell + 1.0) * (self.pl("a1a2", ell) * self.pl("b1b2", ell) +
                                          self.pl("a1b2", ell) * self.pl("b1a2", ell))


@functools.lru_cache(maxsize=None)
def restatement(tag, **kw):
    """One per case, shared by the tests (and by the GPU tests that compare with it)."""
    return Restatement(tag, **kw)


def rel(got, ref):
    got, ref = numpy.asarray(got, dtype=float), numpy.asarray(ref, dtype=float)
    zero = ref == 0.0
    assert numpy.array_equal(got[zero], ref[zero])
    return float(numpy.max(numpy.abs(got[~zero] / ref[~zero] - 1.0)))


# -- the fixture ----------------------------------------------------------------------------
def test_fixture_is_self_consistent():
    g = load_golden("g31_covariance_fourier")
    for tag in CASES:
        ell = g[tag + "_ell"]
        assert 20 <= ell.size <= 30 and ell[1] == L_MIN and ell[-2] == L_MAX
        assert ell[0] < L_MIN and ell[-1] > L_MAX
        pl, G = g[tag + "_pl"], g[tag + "_G"]
        assert pl.shape == (4, ell.size) and g[tag + "_tables"].shape == (4, 50)
        assert numpy.all(pl[:, [0, -1]] == 0.0) and numpy.all(pl[:, 1:-1] > 0.0)
        assert rel(1.0 / (2.0 * ell + 1.0) * (pl[0] * pl[1] + pl[2] * pl[3]), G) < 1e-14
        for k in ("_norm", "_D", "_tables", "_z_bar"):
            assert numpy.all(numpy.isfinite(g[tag + k]))
        assert g[tag + "_halo_redshift"][0] == g[tag + "_z_bar"][0]
        assert numpy.array_equal(g[tag + "_ln_l"], numpy.linspace(numpy.log(L_MIN),
                                                                   numpy.log(L_MAX), 50))
    # windows that reach down to window_precision: z_bar at the first grid point (1 / chi^2)
    assert numpy.all(g["auto_z_bar"] == 1.48e-6) and numpy.all(g["auto_z_bar"] == g["auto_z_array"][0])
    assert len(set(g["mix_z_bar"])) == 1 and abs(g["mix_z_bar"][0] - 0.18197) < 1e-5
    assert numpy.allclose(g["tomo_z_bar"], [0.9694, 0.5714, 0.7041, 0.7041], atol=5e-5)
    # the as-shipped shallow copies of tomo are on record, and differ by percents
    inside = g["tomo_G"] != 0.0
    dev = numpy.abs(g["tomo_G_shallow"][inside] / g["tomo_G"][inside] - 1.0)
    assert 0.05 < dev.max() < 0.3


# -- the restatement against the reference --------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_g31(tag):
    g = load_golden("g31_covariance_fourier")
    r = restatement(tag)
    assert numpy.array_equal(r.ln_l, g[tag + "_ln_l"])
    assert numpy.array_equal(r.z_array, g[tag + "_z_array"])
    assert [r.z_min[x] for x in PAIRS] + [r.z_max[x] for x in PAIRS] == list(g[tag + "_z_lim"])
    assert [r.z_bar[x] for x in PAIRS] == list(g[tag + "_z_bar"])           # exactly
    errs = {"D": rel([r.D_bar[x] for x in PAIRS], g[tag + "_D"]),
            "norm": rel([r.norm[x] for x in PAIRS], g[tag + "_norm"]),
            "tables": rel(r.tables()[0], g[tag + "_tables"])}
    ell = g[tag + "_ell"]
    for i, x in enumerate(PAIRS):
        errs["pl_" + x] = rel(r.pl(x, ell), g[tag + "_pl"][i])
    errs["G"] = rel(r.covariance_G(ell), g[tag + "_G"])
    print(tag, {k: "%.3g" % v for k, v in errs.items()})
    assert max(errs.values()) < RTOL, errs


def test_quirks_are_pinned():
    """Each quirk, switched off, misses the fixture: the a1 a2 windows of every norm, the
    halo_a1a2 spectrum of a1b2's norm, and D(z_bar)^2 in the tables."""
    g = load_golden("g31_covariance_fourier")
    r = restatement("tomo")
    ref = g["tomo_norm"]
    own = Restatement("tomo", norm_windows_of_pair=True)
    got = numpy.array([own.norm[x] for x in PAIRS])
    assert abs(got[0] / ref[0] - 1) < RTOL                      # (a1a2: the same windows)
    assert numpy.all(numpy.abs(got[1:] / ref[1:] - 1) > 1e-2)
    own = Restatement("tomo", norm_halo_of_pair=True)
    got = numpy.array([own.norm[x] for x in PAIRS])
    assert numpy.all(numpy.abs(got[[0, 1, 3]] / ref[[0, 1, 3]] - 1) < RTOL)
    assert abs(got[2] / ref[2] - 1) > 1e-2
    # D(z_bar)^2: the tables with one power of D less, or none, are off by D, D^2 (D < 0.8)
    tab = r.tables()[0]
    D = numpy.array([r.D_bar[x] for x in PAIRS])[:, None]
    assert numpy.all(D < 0.8)
    assert rel(tab, g["tomo_tables"]) < RTOL
    assert numpy.min(numpy.abs(tab * D / g["tomo_tables"] - 1)) > 0.2
    assert numpy.min(numpy.abs(tab * D * D / g["tomo_tables"] - 1)) > 0.2
    # and the tables carry the norm: _pl divides it out again
    i = PAIRS.index("b1b2")
    assert rel(r.pl("b1b2", numpy.exp(r.ln_l[[3, 20, 44]])) * r.norm["b1b2"],
               g["tomo_tables"][i][[3, 20, 44]]) < RTOL


# -- the class, without a device -------------------------------------------------------------
def build(tag, halo_obj=None, four_windows=False):
    from chomp_amd import cosmology, covariance, halo, kernel
    cm = cosmology.MultiEpoch(0.0, 5.0)
    conv = lambda: kernel.WindowFunctionConvergence(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2), cm)
    if tag == "auto":
        w = conv()
        ws = (w, w, w, w)
    elif tag == "mix":
        g = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
        c = conv()
        ws = (g, c, g, c)
    elif tag == "tomo":
        a = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.5, 1.5, 1.0, 0.2), cm)
        b = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.2, 1.0, 0.6, 0.15), cm)
        ws = (a, a, b, b)
    else:                                                    # "apart": a and b share no redshift
        a = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(1.2, 1.5, 1.3, 0.05), cm)
        b = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.2, 1.0, 0.6, 0.15), cm)
        ws = (a, a, b, b)
    kc = covariance.KernelCovariance(1e-3, 1e2, ws[0], ws[1], ws[2], ws[3], cm,
                                     four_windows=four_windows)
    h = halo.Halo(0.0) if halo_obj is None else halo_obj
    return covariance.CovarianceFourier(L_MIN, L_MAX, input_kernel_covariance=kc, input_halo=h)


@pytest.mark.parametrize("tag", CASES)
def test_constructor_attributes(tag):
    g = load_golden("g31_covariance_fourier")
    cf = build(tag, four_windows=(tag == "tomo"))
    assert cf._ln_l_min == numpy.log(L_MIN) and cf._ln_l_max == numpy.log(L_MAX)
    assert numpy.array_equal(cf._ln_l_array, g[tag + "_ln_l"])
    assert numpy.array_equal(cf._z_array, g[tag + "_z_array"])
    lim = [getattr(cf, "_z_min_" + p) for p in PAIRS] + [getattr(cf, "_z_max_" + p) for p in PAIRS]
    assert lim == list(g[tag + "_z_lim"])
    assert cf._initialized_pl is False and cf.halo_tri is None
    assert cf.halo_a1a2.get_redshift() == 0.0                 # (moved by _initialize_pl only)
    assert cf.covariance(100.0, 100.0) is None
    for name in ("_initialize_pl", "_calculate_zbar", "_pl_a1a2", "_pl_b1b2", "_pl_a1b2",
                 "_pl_b1a2", "covariance_G", "covariance"):
        assert callable(getattr(cf, name))
    # only the windows and the MultiEpoch of the KernelCovariance are read
    assert cf.kernel._ssc_table is False and cf.kernel._ng_table is False
    assert cf.kernel._ssc_key is None


def test_halo_trispectrum_is_stored():
    from chomp_amd import covariance, halo
    marker = object()
    cf = build("mix")
    cf2 = covariance.CovarianceFourier(L_MIN, L_MAX, cf.kernel, halo.Halo(0.0), marker)
    assert cf2.halo_tri is marker


def test_scope_errors():
    from chomp_amd import _lib, covariance, halo
    kc = build("mix").kernel
    with pytest.raises(_lib.ChompScopeError, match="KernelCovariance"):
        covariance.CovarianceFourier(L_MIN, L_MAX, None, halo.Halo(0.0))
    # (HaloFit's constructor asks the device for omega_m: a bare instance shows its type)
    for bad in (None, halo.HaloFit.__new__(halo.HaloFit), halo.HaloExclusion(0.0),
                halo.HaloSuperSampleCovariance(0.0), object()):
        with pytest.raises(_lib.ChompScopeError, match="halo.Halo"):
            covariance.CovarianceFourier(L_MIN, L_MAX, kc, bad)
    from chomp_amd import defaults
    general = halo.Halo(0.0, halo_dict=dict(defaults.default_halo_dict, alpha=-1.5),
                        general_profile=True)
    with pytest.raises(_lib.ChompScopeError, match="general_profile"):
        covariance.CovarianceFourier(L_MIN, L_MAX, kc, general)
    with pytest.raises(_lib.ChompScopeError, match="a1b2.*no redshift in common"):
        build("apart")


def test_no_device_without_a_gpu():
    """The tables are the device's: without one the first evaluation raises, it does not compute."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from chomp_amd import _lib
    with pytest.raises(_lib.ChompError):
        build("mix").covariance_G(100.0)


# -- the boundary ---------------------------------------------------------------------------
def test_exports_and_declarations():
    import ctypes
    from chomp_amd import _lib
    _lib.build()                                             # (the library compiles for gfx950)
    L = _lib.lib()
    with open(os.path.join(ROOT, "include", "chomp_mi355x.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    flat = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert ("int chomp_covariance_fourier_zbar(chomp_ctx* ctx, const double* z, size_t n_z, "
            "double* info);") in flat
    assert ("int chomp_covariance_fourier_table(chomp_ctx* ctx, int which, const size_t epoch[4], "
            "const double* ln_l, size_t n, double* norms, double* tables, double* levels);") in flat
    assert ("int chomp_covariance_fourier_gaussian(chomp_ctx* ctx, const double* l, size_t n, "
            "double* out, int mem);") in flat
    vp, sz, i, dp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, _lib.c_double_p
    assert L.chomp_covariance_fourier_zbar.argtypes == [vp, dp, sz, dp]
    assert L.chomp_covariance_fourier_table.argtypes == [vp, i, ctypes.POINTER(sz), dp, sz, dp,
                                                         dp, dp]
    assert L.chomp_covariance_fourier_gaussian.argtypes == [vp, vp, sz, vp, i]
    for name in NAMES:
        assert getattr(L, name).restype is i
    for method in ("covariance_fourier_zbar", "covariance_fourier_table",
                   "covariance_fourier_gaussian"):
        assert callable(getattr(_lib.Context, method))
