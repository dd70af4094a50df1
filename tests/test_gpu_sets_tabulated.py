"""Tabulated redshift distributions and w0-wa cosmologies on the projection set axis:
chomp_kernel_setup_pairs / chomp_kernel_setup_sets behind chomp_set_sets_scope, bit for bit
against chomp_kernel_setup of the same kernel on the same context (kernel_info and the tables
tests/test_gpu_kernels_batch.py compares), the sets' arena across calls, and the three batches on
top -- Correlation.correlation_kernels (w(theta), C_l, galaxy-galaxy lensing),
correlation_cosmologies and CovarianceMulti.get_covariance_batched -- against the project's own
loops (bit for bit) and against the reference's loop over kernels (G37)."""
import warnings

import numpy
import pytest

from conftest import load_golden, rel_err
from test_gpu_kernels_batch import PROJ_RTOL, TABLES
from test_kernels_batch_cpu import COSMO_KEYS, KTHETA, ZEHAVI

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g37():
    import torch
    assert torch.cuda.is_available()
    return load_golden("g37_kernels_tabulated")


def _dist(g, t):
    from chomp_amd import kernel
    t = int(t)
    if t < 0:
        return kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0)
    z, p, order = g["t_z"][t], g["t_p"][t], int(g["t_order"][t])
    if g["t_smoothing"][t]:
        return kernel.dNdzInterpolation(z, p, interpolation_order=order,
                                        smoothing=float(g["t_smoothing"][t]))
    return kernel.dNdzInterpolation(z, p, interpolation_order=order)


def fixture_cosmo(g, tag, i):
    return dict(zip(COSMO_KEYS, (float(v) for v in g[tag + "_cosmo"][i])))


def fixture_kernels(g, tag, shared=True):
    """The rows of group `tag` of G37 as fresh kernels, each with its own MultiEpoch.  shared: a
    table that several windows use is one distribution object, as the bins of an analysis are."""
    from chomp_amd import cosmology, kernel
    bins = {}
    out = []
    for i in range(g[tag + "_w"].shape[0]):
        me = cosmology.MultiEpoch(0.0, 5.0, fixture_cosmo(g, tag, i))
        win = []
        for w in range(2):
            t = int(g[tag + "_tab"][i, w])
            dist = bins.get(t) if shared and t >= 0 else None
            if dist is None:
                dist = bins[t] = _dist(g, t)
            cls = (kernel.WindowFunctionGalaxy if g[tag + "_wkind"][i, w] == 0
                   else kernel.WindowFunctionConvergence)
            win.append(cls(dist, me))
        K = kernel.Kernel if tag == "j0" else kernel.GalaxyGalaxyLensingKernel
        out.append(K(KTHETA[0], KTHETA[1], win[0], win[1], me))
    return out


def _single(ctx, kern, dark_energy=None):
    """(kernel_info, tables) of chomp_kernel_setup of one kernel's own inputs."""
    from chomp_amd import cosmology
    kw = cosmology._de_kw(kern.cosmo.cosmo_dict) if dark_energy is None else dict(
        dark_energy=dark_energy)
    ctx.kernel_setup(kern.cosmo.cosmo_dict, kern.cosmo.z_min, kern.cosmo.z_max, kern._ktheta[0],
                     kern._ktheta[1], kern.window_function_a._struct(),
                     kern.window_function_b._struct(), kern._order, **kw)
    return ctx.kernel_info(), {t: ctx.kernel_table(t) for t in TABLES}


def _sets(ctx, n):
    """(kernel_info, tables) of every set of the last set-up of sets."""
    info = ctx.kernel_info_sets()
    return [({name: info[name][s] for name in info},
             {t: ctx.kernel_table_set(s, t) for t in TABLES}) for s in range(n)]


def _same(got, want, what):
    (info, tabs), (one, ref) = got, want
    for name, value in one.items():
        assert numpy.array_equal(info[name], value), (what, name, info[name], value)
    for t in TABLES:
        assert numpy.all(numpy.isfinite(ref[t])), (what, t)
        assert numpy.array_equal(tabs[t], ref[t]), (what, t, rel_err(tabs[t], ref[t]))


def _galaxy(dist, me):
    from chomp_amd import kernel
    return kernel.WindowFunctionGalaxy(dist, me)


def _four_kernels():
    """Analytic x 17-point order-2 table; that table in both windows (at two host addresses);
    analytic x convergence over a smoothing spline of order 3 (the lensing-efficiency integrand
    reads the table); an analytic pair beside them."""
    from chomp_amd import cosmology, kernel
    z = numpy.linspace(0.05, 1.45, 17)
    p = z ** 2 * numpy.exp(-(z / 0.5) ** 1.5) * (1.0 + 0.3 * numpy.sin(9.0 * z)) + 0.02
    ml = kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0)
    me = [cosmology.MultiEpoch(0.0, 5.0) for _ in range(4)]
    smooth = kernel.dNdzInterpolation(z, p, interpolation_order=3, smoothing=1e-4)
    # (FITPACK puts the knots of an order-2 spline between the points: 15 pieces)
    assert smooth._coef.shape[1] == 4 and kernel.dNdzInterpolation(z, p)._coef.shape == (15, 3)
    pairs = [(_galaxy(ml, me[0]), _galaxy(kernel.dNdzInterpolation(z, p), me[0])),
             (_galaxy(kernel.dNdzInterpolation(z, p), me[1]),
              _galaxy(kernel.dNdzInterpolation(z, p), me[1])),
             (_galaxy(ml, me[2]), kernel.WindowFunctionConvergence(smooth, me[2])),
             (_galaxy(ml, me[3]), _galaxy(kernel.dNdzGaussian(0.0, 1.0, 0.4, 0.1), me[3]))]
    return [kernel.Kernel(KTHETA[0], KTHETA[1], a, b, m) for (a, b), m in zip(pairs, me)]


@pytest.fixture(scope="module")
def four():
    """(context, the four kernels, their single set-ups), the singles computed once."""
    from chomp_amd import cosmology
    ctx = cosmology._context()
    kernels = _four_kernels()
    singles = [_single(ctx, k) for k in kernels]
    for one, tabs in singles:
        for t in tabs.values():
            t.setflags(write=False)
    return ctx, kernels, singles


def test_pairs_with_tables_bit_for_bit(four):
    from chomp_amd import _lib, kernel
    ctx, kernels, singles = four
    last = ctx.kernel_info()
    assert kernel.Kernel._setup_pairs_on(ctx, kernels) is ctx
    for s, got in enumerate(_sets(ctx, 4)):
        _same(got, singles[s], "set %d" % s)
    assert kernels[2].window_function_b._struct().kind == _lib.WINDOW_CONVERGENCE
    for s in range(4):
        for r in range(s):
            assert not numpy.array_equal(singles[s][1]["kernel"], singles[r][1]["kernel"]), (s, r)
    # the single set-up, its table behind it included, is as it was
    after = ctx.kernel_info()
    assert all(numpy.array_equal(after[name], last[name]) for name in last)
    assert numpy.array_equal(ctx.kernel_table("kernel"), singles[3][1]["kernel"])
    _same(_single(ctx, kernels[1]), singles[1], "single again")
    assert all(k._done == {} and k._info is None for k in kernels)


def test_one_set_with_a_one_piece_table():
    """Three points of order 2 are one piece: the search for the piece has nothing to halve."""
    from chomp_amd import cosmology, kernel
    me = cosmology.MultiEpoch(0.0, 5.0)
    dist = kernel.dNdzInterpolation(numpy.array([0.2, 0.5, 0.8]), numpy.array([0.1, 1.0, 0.1]))
    assert dist._struct().pp_n == 1 and dist._struct().pp_order == 2
    kern = kernel.Kernel(KTHETA[0], KTHETA[1], _galaxy(dist, me),
                         _galaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), me), me)
    ctx = cosmology._context()
    want = _single(ctx, kern)
    kernel.Kernel._setup_pairs_on(ctx, [kern])
    got, = _sets(ctx, 1)
    _same(got, want, "one piece")
    assert numpy.max(want[1]["wa"]) > 0.0


def test_the_arena_grows_and_is_reused(four):
    """Small tables, then a dNdChiGaussian (a cubic through 4097 points, over 4000 pieces: the
    arena grows and moves), then the small tables again: what the first call gave."""
    from chomp_amd import cosmology, kernel
    ctx, kernels, singles = four
    kernel.Kernel._setup_pairs_on(ctx, kernels)
    first = _sets(ctx, 4)
    me = cosmology.MultiEpoch(0.0, 5.0)
    chi = kernel.dNdChiGaussian(600.0, 1800.0, 1200.0, 150.0, me)
    assert chi._struct().pp_n > 4000 and chi._struct().pp_order == 3
    big = kernel.Kernel(KTHETA[0], KTHETA[1], _galaxy(chi, me),
                        kernel.WindowFunctionConvergence(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2), me),
                        me)
    want = _single(ctx, big)
    kernel.Kernel._setup_pairs_on(ctx, [kernels[0], big])
    got = _sets(ctx, 2)
    _same(got[0], singles[0], "small beside big")
    _same(got[1], want, "big")
    kernel.Kernel._setup_pairs_on(ctx, kernels)
    for s, (again, before) in enumerate(zip(_sets(ctx, 4), first)):
        _same(again, before, "again, set %d" % s)
        _same(again, singles[s], "again, set %d against the single set-up" % s)


def _lensing_kernel(dist_a=None, cosmo=None):
    from chomp_amd import cosmology, kernel
    me = cosmology.MultiEpoch(0.0, 5.0, cosmo)
    wa = _galaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0) if dist_a is None else dist_a, me)
    wb = kernel.WindowFunctionConvergence(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2), me)
    return kernel.Kernel(KTHETA[0], KTHETA[1], wa, wb, me)


def _de_cosmos():
    """Lambda-CDM; (w0, wa) = (-0.9, 0.2); the same pair with another Omega_m (one pressure
    table serves both); (-1.1, 0)."""
    from chomp_amd import defaults
    c = dict(defaults.default_cosmo_dict)
    other = dict(c, omega_m0=c["omega_m0"] + 0.05)
    other["omega_l0"] = 1.0 - other["omega_m0"] - other["omega_r0"]
    return [c, dict(c, w0=-0.9, wa=0.2), dict(other, w0=-0.9, wa=0.2), dict(c, w0=-1.1, wa=0.0)], other


def test_setup_sets_with_dark_energy():
    from chomp_amd import cosmology
    cosmos, other = _de_cosmos()
    kern = _lensing_kernel()
    ctx = cosmology._context()
    a, b = kern.window_function_a._struct(), kern.window_function_b._struct()
    singles = []
    for c in cosmos:
        ctx.kernel_setup(c, 0.0, 5.0, KTHETA[0], KTHETA[1], a, b, 0, dark_energy=True)
        singles.append((ctx.kernel_info(), {t: ctx.kernel_table(t) for t in TABLES}))
    assert kern._setup_sets_on(ctx, cosmos) is ctx
    mixed = _sets(ctx, 4)
    for s in range(4):
        _same(mixed[s], singles[s], "cosmology %d" % s)
    # dark energy moves the tables, Omega_m moves them again
    for s, r in ((1, 0), (2, 1), (3, 0), (3, 1)):
        assert not numpy.array_equal(singles[s][1]["me_chi"], singles[r][1]["me_chi"]), (s, r)
        assert not numpy.array_equal(singles[s][1]["wb"], singles[r][1]["wb"]), (s, r)
    # the Lambda-CDM set is what it is in a batch without dark energy
    kern._setup_sets_on(ctx, [cosmos[0], other])
    pure = _sets(ctx, 2)
    _same(mixed[0], pure[0], "Lambda-CDM, mixed against pure")
    ctx.kernel_setup(cosmos[0], 0.0, 5.0, KTHETA[0], KTHETA[1], a, b, 0)
    _same(pure[0], (ctx.kernel_info(), {t: ctx.kernel_table(t) for t in TABLES}), "pure")


def test_pairs_mixing_a_table_and_dark_energy_then_no_keywords(four):
    """One call with a table in set 0 and a w0-wa cosmology in set 1 (and both in set 2); a call
    without the keywords after it is refused with the words it always was."""
    from chomp_amd import _lib, kernel
    ctx, kernels, singles = four
    cosmos, _ = _de_cosmos()
    z = numpy.linspace(0.05, 1.45, 17)
    tab = kernel.dNdzInterpolation(z, z * z * numpy.exp(-z / 0.3))
    mix = [kernels[0], _lensing_kernel(cosmo=cosmos[1]), _lensing_kernel(tab, cosmos[3]),
           kernels[3]]
    want = [singles[0], _single(ctx, mix[1]), _single(ctx, mix[2]), singles[3]]
    kernel.Kernel._setup_pairs_on(ctx, mix)
    for s, got in enumerate(_sets(ctx, 4)):
        _same(got, want[s], "mixed set %d" % s)
    args = ([k.cosmo.cosmo_dict for k in mix], [0.0] * 4, [5.0] * 4, KTHETA[0], KTHETA[1],
            [k.window_function_a._struct() for k in mix],
            [k.window_function_b._struct() for k in mix], 0)
    with pytest.raises(_lib.ChompScopeError, match="kernel_setup_pairs: set 0: a tabulated"):
        ctx.kernel_setup_pairs(*args, dark_energy=True)
    with pytest.raises(_lib.ChompScopeError, match="kernel_setup_pairs: set 1: a w0/wa"):
        ctx.kernel_setup_pairs(*args, tabulated=True)
    with pytest.raises(_lib.ChompScopeError, match="kernel_setup_pairs: set 0: a tabulated"):
        ctx.kernel_setup_pairs(*args)
    plain = [a[1:2] if isinstance(a, list) else a for a in args]
    with pytest.raises(_lib.ChompScopeError, match="kernel_setup_pairs: set 0: a w0/wa"):
        ctx.kernel_setup_pairs(*plain)
    a, b = mix[2].window_function_a._struct(), mix[2].window_function_b._struct()
    with pytest.raises(_lib.ChompScopeError, match="kernel_setup_sets: a tabulated"):
        ctx.kernel_setup_sets(cosmos[:1], 0.0, 5.0, KTHETA[0], KTHETA[1], a, b, 0)
    with pytest.raises(_lib.ChompScopeError, match="kernel_setup_sets: a w0/wa"):
        ctx.kernel_setup_sets(cosmos[:2], 0.0, 5.0, KTHETA[0], KTHETA[1], b, b, 0)
    for s, got in enumerate(_sets(ctx, 4)):              # (a refusal leaves the last sets alone)
        _same(got, want[s], "mixed set %d, after the refusals" % s)
    kernel.Kernel._setup_pairs_on(ctx, kernels[3:])
    ctx.kernel_setup_pairs(*args, tabulated=True, dark_energy=True)
    for s, got in enumerate(_sets(ctx, 4)):
        _same(got, want[s], "mixed set %d, through the binding" % s)


# -- the user level ----------------------------------------------------------------------------
def _words(g, tag):
    """The status word every row is to carry: 0, but for a row with a w0-wa cosmology
    ST_DE_DIVMAX and nothing else.  That bit is the pressure table's: at the default precision
    the reference's own Romberg of P(a) exhausts divmax at the deepest knots and keeps its last
    row, the device does the same and says so (tests/test_gpu_dark_energy.py asserts the bit on the
    single set-up), so no w0-wa row is without it and it does not keep a row from the reference."""
    from chomp_amd import _lib, cosmology
    return numpy.array([_lib.ST_DE_DIVMAX if cosmology.has_dark_energy(fixture_cosmo(g, tag, i))
                        else 0 for i in range(g[tag + "_w"].shape[0])], dtype=numpy.uint32)


def _fresh(g, tag, i, fourier):
    """A fresh Correlation / CorrelationFourier of row i, as correlation_kernels' contract has it."""
    from chomp_amd import correlation, cosmology, halo, hod as hod_mod
    kern = fixture_kernels(g, tag, shared=False)[i]
    h = halo.Halo(0.0, hod_mod.HODZheng(dict(ZEHAVI)),
                  cosmology.SingleEpoch(0.0, fixture_cosmo(g, tag, i)))
    ps = "power_gg" if tag == "j0" else "power_gm"
    if fourier:
        return correlation.CorrelationFourier(10, 1e4, kern, input_halo=h, powSpec=ps)
    return correlation.Correlation(0.001, 1.0, kern, input_halo=h, power_spec=ps)


@pytest.fixture(scope="module", params=[("j0", False), ("j0", True), ("j2", False)],
                ids=["J0-w", "J0-cl", "J2-w"])
def batch(request, g37):
    """(tag, fourier, x, the object the batch is called on, its rows, status, fixture rows)."""
    from chomp_amd import _lib
    tag, fourier = request.param
    x = numpy.ascontiguousarray(g37["ell"] if fourier else g37["theta"])
    corr = _fresh(g37, tag, 0, fourier)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got, words = corr.correlation_kernels(x, fixture_kernels(g37, tag), with_status=True,
                                              tabulated=True, dark_energy=True)
    flagged = [str(w.message) for w in caught
               if issubclass(w.category, (_lib.ChompAccuracyWarning, _lib.ChompParityWarning))]
    # (a flagged row warns "kernel i: ..."; the w0-wa row's pressure table does, see _words)
    assert flagged == ["kernel %d: a Romberg of the dark-energy pressure table exhausted divmax" % i
                       for i in numpy.nonzero(_words(g37, tag))[0]], flagged
    want = g37["j0_cl"] if fourier else g37[tag + "_w"]
    return tag, fourier, x, corr, got, words, want


def test_against_the_reference(batch, g37):
    tag, fourier, x, corr, got, words, want = batch
    assert got.shape == want.shape and words.dtype == numpy.uint32
    assert numpy.array_equal(words, _words(g37, tag)) and words is corr.kernels_status
    assert numpy.array_equal(corr.kernels_z_bar, g37[tag + "_z_bar"])
    assert rel_err(corr.kernels_D_z, g37[tag + "_D_z"]) < PROJ_RTOL
    for i in range(got.shape[0]):
        err = rel_err(got[i], want[i])
        print("%s %s row %d against G37: %.2e" % (tag, "C_l" if fourier else "w", i, err))
    for i in range(got.shape[0]):
        assert rel_err(got[i], want[i]) < PROJ_RTOL, (tag, fourier, i)


def test_against_the_loop(batch, g37):
    """Fresh objects, one per kernel, equal the batch rows; this object is not touched."""
    tag, fourier, x, corr, got, words, want = batch
    for i in range(got.shape[0]):
        one = _fresh(g37, tag, i, fourier).correlation(x)
        assert numpy.array_equal(one, got[i]), (tag, fourier, i, rel_err(got[i], one))
    assert numpy.array_equal(corr.correlation(x), got[0])
    assert corr.kernel._done and corr.kernel._z_bar_override is None


def test_the_keywords_are_needed(g37):
    from chomp_amd import _lib
    corr = _fresh(g37, "j0", 3, False)
    kernels = fixture_kernels(g37, "j0")
    theta = numpy.ascontiguousarray(g37["theta"][:2])
    with pytest.raises(_lib.ChompScopeError, match="kernel 0: window_function_a has a tabulated"):
        corr.correlation_kernels(theta, kernels)
    with pytest.raises(_lib.ChompScopeError, match="kernel 3 has a w0-wa cosmology"):
        corr.correlation_kernels(theta, kernels, tabulated=True)
    assert not hasattr(corr, "_kernels_grid")


def test_cosmologies_with_a_dark_energy_point(g37):
    """One w0-wa point among Lambda-CDM ones, over a tabulated lens bin: every row is what
    set_cosmology + correlation gives on a fresh object, and the Lambda-CDM rows are what a batch
    without the dark-energy point gives."""
    from chomp_amd import _lib, correlation, cosmology, halo, kernel
    theta = numpy.ascontiguousarray(g37["theta"][[0, 3, 5, 8]])
    c0, c1 = fixture_cosmo(g37, "j0", 0), fixture_cosmo(g37, "j0", 2)
    cosmos = [c0, dict(c0, w0=-0.9, wa=0.2), c1]

    def fresh():
        me = cosmology.MultiEpoch(0.0, 5.0)
        kern = kernel.Kernel(KTHETA[0], KTHETA[1], _galaxy(_dist(g37, 0), me),
                             _galaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), me), me)
        return correlation.Correlation(0.001, 1.0, kern, input_halo=halo.Halo(0.0),
                                       power_spec="power_gg")
    corr = fresh()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        rows, words = corr.correlation_cosmologies(theta, cosmos, with_status=True, tabulated=True,
                                                   dark_energy=True)
    # (the w0-wa point's pressure table reports its exhausted divmax, as in the loop: see _words)
    assert rows.shape == (3, 4) and numpy.array_equal(words, [0, _lib.ST_DE_DIVMAX, 0])
    assert [str(w.message) for w in caught if issubclass(w.category, _lib.ChompAccuracyWarning)] == [
        "cosmology 1: a Romberg of the dark-energy pressure table exhausted divmax"]
    for i, c in enumerate(cosmos):
        loop = fresh()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", _lib.ChompAccuracyWarning)   # (the same bit, per call)
            loop.set_cosmology(c)
            one = loop.correlation(theta)
        assert loop.kernel.z_bar == corr.cosmologies_z_bar[i]
        assert numpy.array_equal(one, rows[i]), (i, rel_err(rows[i], one))
    assert rel_err(rows[1], rows[0]) > 1e-3
    pure = corr.correlation_cosmologies(theta, [c0, c1], tabulated=True)
    assert numpy.array_equal(pure, rows[[0, 2]])


def test_covariance_batched_over_tabulated_bins(g37):
    """Three correlations over two tabulated bins (two auto-correlations and the cross pair),
    Gaussian term: get_covariance_batched(tabulated=True) is get_covariance()."""
    from chomp_amd import _lib, correlation, cosmology, covariance, halo, kernel
    from test_gpu_covariance_cross import D2R, KWS

    def three():
        cm = cosmology.MultiEpoch(0.0, 5.0)
        bins = [_galaxy(_dist(g37, 0), cm), _galaxy(_dist(g37, 1), cm)]

        def corr(wa, wb):
            kern = kernel.Kernel(1e-6 * D2R, 100.0 * D2R, wa, wb, cm)
            return correlation.Correlation(0.01, 1.0, kern, input_halo=halo.Halo(0.0),
                                           power_spec="power_mm")
        return [corr(bins[0], bins[0]), corr(bins[1], bins[1]), corr(bins[0], bins[1])]
    cl = covariance.CovarianceMulti(three(), nongaussian_cov=False, **KWS)
    cl.get_covariance()
    cb = covariance.CovarianceMulti(three(), nongaussian_cov=False, **KWS)
    with pytest.raises(_lib.ChompScopeError, match="correlation 0: window_function_a has a tabulated"):
        cb.get_covariance_batched()
    out, words = cb.get_covariance_batched(with_status=True, tabulated=True)
    assert out is cb.wcovar and out.shape == (12, 12) and not words.any()
    assert numpy.array_equal(out, out.T)
    assert numpy.array_equal(out, cl.wcovar), rel_err(out, cl.wcovar)
    for row_l, row_b in zip(cl.covariance_list, cb.covariance_list):
        for cov_l, cov_b in zip(row_l, row_b):
            assert numpy.array_equal(cov_b.covar, cov_l.covar)
    assert numpy.array_equal(cb.blocks_z_bar, [row[0].corr_a.kernel.z_bar
                                               for row in cl.covariance_list])
