"""Host side of tabulated redshift distributions and w0-wa cosmologies on the projection set axis:
the C declaration of chomp_set_sets_scope and its binding, the opt-ins of
Correlation.correlation_cosmologies / correlation_kernels and
CovarianceMulti.get_covariance_batched (what they let through, what they still refuse, what they
say without the keywords), the keywords Kernel._setup_sets_on / _setup_pairs_on forward, and the
binding's taking the opt-in back after a call that raised.  No device."""
import ctypes
import os
import re

import numpy
import pytest

import test_covariance_blocks_cpu as cov_cpu
import test_kernels_batch_cpu as kernels_cpu
import test_wtheta_cosmologies_cpu as cosmo_cpu
from conftest import ROOT
from test_kernels_batch_cpu import KTHETA, THETA, no_device  # noqa: F401

TABULATED = "has a tabulated redshift distribution"
DARK = ("has w0-wa", "has a w0-wa cosmology")
ASKED = "a device context was asked for"


def _table(n=17):
    from chomp_amd import kernel
    z = numpy.linspace(0.0, 2.0, n)
    return kernel.dNdzInterpolation(z, z * z * numpy.exp(-z / 0.3))


def _de_cosmo():
    from chomp_amd import defaults
    return dict(defaults.default_cosmo_dict, w0=-0.9, wa=0.2)


def test_header_and_binding_agree():
    from chomp_amd import _lib, correlation, covariance
    with open(os.path.join(ROOT, "include", "chomp_mi355x.h")) as f:
        header = f.read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert "int chomp_set_sets_scope(chomp_ctx* ctx, unsigned flags);" in flat
    for name, value in (("TABULATED", 1), ("DARK_ENERGY", 2)):
        m = re.search(r"#define CHOMP_SETS_%s (\d+)u?\b" % name, header)
        assert m and int(m.group(1)) == value == getattr(_lib, "SETS_" + name)
    assert "chomp_set_sets_scope" in _lib.EXPORTS
    L = _lib.lib()
    assert L.chomp_set_sets_scope.argtypes == [ctypes.c_void_p, ctypes.c_uint]
    assert L.chomp_set_sets_scope(None, 0) == _lib.ERR_ARG      # (no context: nothing to set)
    # the planner is a header of its own with nothing of HIP in it
    with open(os.path.join(ROOT, "chomp_amd", "csrc", "chomp_pp_plan.h")) as f:
        plan = f.read()
    assert "hip" not in re.sub(r"//.*", "", plan).lower()
    import inspect
    for fn, names in ((_lib.Context.kernel_setup_sets, ("tabulated", "dark_energy")),
                      (_lib.Context.kernel_setup_pairs, ("tabulated", "dark_energy")),
                      (correlation.Correlation.correlation_cosmologies, ("tabulated", "dark_energy")),
                      (correlation.Correlation.correlation_kernels, ("tabulated", "dark_energy")),
                      (covariance.CovarianceMulti.get_covariance_batched, ("tabulated",))):
        par = inspect.signature(fn).parameters
        for name in names:
            assert par[name].default is False, (fn, name)
    assert "dark_energy" not in inspect.signature(
        covariance.CovarianceMulti.get_covariance_batched).parameters
    assert (correlation.CorrelationFourier.correlation_kernels
            is correlation.Correlation.correlation_kernels)


# -- what the keywords let through: as far as the first device call ---------------------------
@pytest.mark.parametrize("fourier", [False, True], ids=["w", "cl"])
def test_correlation_kernels_takes_tables_and_dark_energy(no_device, fourier):  # noqa: F811
    from chomp_amd import _lib, correlation, halo
    _kernel, _bare = kernels_cpu._kernel, kernels_cpu._bare
    cls = correlation.CorrelationFourier if fourier else correlation.Correlation
    tab = [_kernel(), _kernel(dist_b=_table())]
    de = [_kernel(), _kernel(cosmo=_de_cosmo())]
    both = [_kernel(dist_b=_table()), _kernel(cosmo=_de_cosmo())]
    for kernels, kw in ((tab, dict(tabulated=True)), (de, dict(dark_energy=True)),
                        (both, dict(tabulated=True, dark_energy=True))):
        corr = _bare(halo.Halo(0.0), cls=cls)
        with pytest.raises(AssertionError, match=ASKED):
            corr.correlation_kernels(THETA, kernels, **kw)
    # one keyword does not let the other input in, and False is the default
    with pytest.raises(_lib.ChompScopeError, match="kernel 1 has a w0-wa cosmology"):
        _bare(halo.Halo(0.0), cls=cls).correlation_kernels(THETA, both, tabulated=True)
    with pytest.raises(_lib.ChompScopeError, match="kernel 0: window_function_b " + TABULATED):
        _bare(halo.Halo(0.0), cls=cls).correlation_kernels(THETA, both, dark_energy=True)
    with pytest.raises(_lib.ChompScopeError, match="kernel 1: window_function_b " + TABULATED):
        _bare(halo.Halo(0.0), cls=cls).correlation_kernels(THETA, tab, tabulated=False,
                                                           dark_energy=False)


def test_correlation_cosmologies_takes_tables_and_dark_energy(no_device):  # noqa: F811
    from chomp_amd import _lib, halo, kernel
    _bare, _Kernel = cosmo_cpu._bare, cosmo_cpu._Kernel
    two = cosmo_cpu._cosmos()
    de = [two[0], dict(two[1], w0=-0.9, wa=0.2)]
    chi = kernel.dNdChiGaussian.__new__(kernel.dNdChiGaussian)     # (its constructor tabulates chi(z))
    for dist, cosmos, kw in ((_table(), two, dict(tabulated=True)),
                             (chi, two, dict(tabulated=True)),
                             (None, de, dict(dark_energy=True)),
                             (_table(), de, dict(tabulated=True, dark_energy=True))):
        corr = _bare(halo.Halo(0.0), kern=_Kernel(dist))
        with pytest.raises(AssertionError, match=ASKED):
            corr.correlation_cosmologies(THETA, cosmos, **kw)
    with pytest.raises(_lib.ChompScopeError, match="cosmology 1 has w0-wa dark energy"):
        _bare(halo.Halo(0.0), kern=_Kernel(_table())).correlation_cosmologies(
            THETA, de, tabulated=True)
    with pytest.raises(_lib.ChompScopeError, match="window_function_b " + TABULATED):
        _bare(halo.Halo(0.0), kern=_Kernel(_table())).correlation_cosmologies(
            THETA, de, dark_energy=True)


def test_get_covariance_batched_takes_tables(no_device):  # noqa: F811
    from chomp_amd import _lib
    bare, multi, _kernel = cov_cpu.bare, cov_cpu.multi, kernels_cpu._kernel
    cm = multi([bare(), bare(kern=_kernel(dist_b=_table()))])
    with pytest.raises(AssertionError, match=ASKED):
        cm.get_covariance_batched(tabulated=True)
    with pytest.raises(_lib.ChompScopeError, match="correlation 1: window_function_b " + TABULATED):
        cm.get_covariance_batched(tabulated=False)
    # w0-wa stays out of the covariance batch, whatever the keyword
    cm = multi([bare(kern=_kernel(cosmo=_de_cosmo()))])
    with pytest.raises(_lib.ChompScopeError, match="the kernel of correlation 0 has a w0-wa"):
        cm.get_covariance_batched(tabulated=True)


# -- every other refusal stands, with its text --------------------------------------------------
def _others(cases):
    kept = [c for c in cases if TABULATED not in c[0] and not any(d in c[0] for d in DARK)]
    assert len(kept) == len(cases) - 2          # (the two cases the keywords are about)
    return kept


@pytest.mark.parametrize("fourier", [False, True], ids=["w", "cl"])
def test_correlation_kernels_still_refuses_the_rest(no_device, fourier):  # noqa: F811
    from chomp_amd import _lib, correlation
    for label, corr, kernels, hods in _others(kernels_cpu._out_of_scope()):
        if fourier:
            corr.__class__ = correlation.CorrelationFourier
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)) as info:
            corr.correlation_kernels(THETA, kernels, hods=hods, tabulated=True, dark_energy=True)
        assert str(info.value).startswith("correlation_kernels: ")
        assert str(info.value).endswith(
            "use the loop fresh Correlation objects, one per kernel, + correlation")


def test_correlation_cosmologies_still_refuses_the_rest(no_device):  # noqa: F811
    from chomp_amd import _lib, correlation, halo
    for label, corr, cosmos, hods in _others(cosmo_cpu._out_of_scope()):
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)) as info:
            corr.correlation_cosmologies(THETA, cosmos, hods=hods, tabulated=True,
                                         dark_energy=True)
        assert str(info.value).startswith("correlation_cosmologies: ")
        assert "set_cosmology" in str(info.value)
    # C_l over cosmologies keeps its pinned refusal and takes no keyword
    corr = kernels_cpu._bare(halo.Halo(0.0), cls=correlation.CorrelationFourier)
    with pytest.raises(_lib.ChompScopeError, match="chomp_cell_epochs"):
        corr.correlation_cosmologies(numpy.array([10.0, 100.0]), cosmo_cpu._cosmos())
    with pytest.raises(TypeError):
        corr.correlation_cosmologies(numpy.array([10.0, 100.0]), cosmo_cpu._cosmos(),
                                     dark_energy=True)


def test_get_covariance_batched_still_refuses_the_rest(no_device):  # noqa: F811
    from chomp_amd import _lib
    cases = [c for c in cov_cpu._out_of_scope() if TABULATED not in c[0]]
    assert len(cases) == 19
    for label, cm in cases:
        kw = dict(tabulated=True)
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)) as info:
            cm.get_covariance_batched(**kw)
        assert str(info.value).startswith("get_covariance_batched: "), label
        assert str(info.value).endswith("; use get_covariance"), label
        assert not hasattr(cm, "_blocks_grid"), label


# -- the keywords travel only when something needs them ---------------------------------------
class _Recorder(object):
    def __init__(self):
        self.calls = []

    def kernel_setup_pairs(self, *args, **kw):
        self.calls.append(("pairs", args, kw))

    def kernel_setup_sets(self, *args, **kw):
        self.calls.append(("sets", args, kw))


def test_setup_on_forwards_keywords_only_when_needed(no_device):  # noqa: F811
    from chomp_amd import _lib, defaults, kernel
    _kernel = kernels_cpu._kernel
    plain, tab, de = _kernel(), _kernel(dist_b=_table()), _kernel(cosmo=_de_cosmo())
    lens = _kernel(kernel.GalaxyGalaxyLensingKernel, dist_b=_table())
    ctx = _Recorder()
    for kernels, want in (([plain, plain], {}),
                          ([plain, tab], {"tabulated": True}),
                          ([de, plain], {"dark_energy": True}),
                          ([tab, plain, de], {"tabulated": True, "dark_energy": True}),
                          ([lens], {"tabulated": True})):
        del ctx.calls[:]
        assert kernel.Kernel._setup_pairs_on(ctx, kernels) is ctx
        (name, args, kw), = ctx.calls
        assert name == "pairs" and len(args) == 8 and kw == want, (kw, want)
        assert [w.dist.kind == _lib.DNDZ_PPOLY for w in args[6]] == [k is tab or k is lens
                                                                     for k in kernels]
    lcdm = dict(defaults.default_cosmo_dict)
    for kern, cosmos, want in ((plain, [lcdm, dict(lcdm, sigma_8=0.9)], {}),
                               (tab, [lcdm, lcdm], {"tabulated": True}),
                               (plain, [lcdm, _de_cosmo()], {"dark_energy": True}),
                               (tab, [_de_cosmo()], {"tabulated": True, "dark_energy": True}),
                               (plain, _lib.Context.pack_cosmo([lcdm, _de_cosmo()], 2),
                                {"dark_energy": True}),
                               (plain, _lib.Context.pack_cosmo([lcdm, lcdm], 2), {})):
        del ctx.calls[:]
        assert kern._setup_sets_on(ctx, cosmos) is ctx
        (name, args, kw), = ctx.calls
        assert name == "sets" and len(args) == 8 and kw == want, (kw, want)
    assert all(k._done == {} and k._info is None for k in (plain, tab, de, lens))


# -- the binding: the opt-in goes before the call and is taken back after it ------------------
class _FakeLib(object):
    """The three C calls the two set-ups of sets make, recorded; `rc` is what the set-up returns."""

    def __init__(self, rc):
        self.rc, self.calls = rc, []

    def chomp_set_sets_scope(self, h, flags):
        self.calls.append(("scope", flags))
        return 0

    def chomp_kernel_setup_pairs(self, *args):
        self.calls.append(("pairs", len(args)))
        return self.rc

    def chomp_kernel_setup_sets(self, *args):
        self.calls.append(("sets", len(args)))
        return self.rc

    def chomp_last_error(self, h):
        return b"kernel_setup_pairs: set 1: refused"


def _fake_context(rc):
    from chomp_amd import _lib
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._L, ctx._h = _FakeLib(rc), None
    return ctx


def _pairs_args(n=2):
    from chomp_amd import defaults
    w = kernels_cpu._kernel().window_function_a._struct()
    c = dict(defaults.default_cosmo_dict)
    return ([c] * n, [0.0] * n, [5.0] * n, KTHETA[0], KTHETA[1], [w] * n, [w] * n, 0)


@pytest.mark.parametrize("rc", ["ok", "scope", "arg", "hip"])
def test_binding_sets_and_clears_the_flags(no_device, rc):  # noqa: F811
    from chomp_amd import _lib
    code = {"ok": _lib.OK, "scope": _lib.ERR_SCOPE, "arg": _lib.ERR_ARG, "hip": _lib.ERR_HIP}[rc]
    error = {"ok": None, "scope": _lib.ChompScopeError, "arg": ValueError, "hip": _lib.ChompError}[rc]
    pairs, one = _pairs_args(), _pairs_args()
    sets = (one[0], 0.0, 5.0, one[3], one[4], one[5][0], one[6][0], 0)
    for name, args, n_args in (("kernel_setup_pairs", pairs, 10), ("kernel_setup_sets", sets, 10)):
        short = name[len("kernel_setup_"):]
        for kw, flags in (({}, None), (dict(tabulated=False, dark_energy=False), None),
                          (dict(tabulated=True), 1), (dict(dark_energy=True), 2),
                          (dict(tabulated=True, dark_energy=True), 3)):
            ctx = _fake_context(code)
            if error is None:
                getattr(ctx, name)(*args, **kw)
                assert ctx._n_sets == 2
            else:
                with pytest.raises(error, match="set 1: refused"):
                    getattr(ctx, name)(*args, **kw)
                assert not hasattr(ctx, "_n_sets")
            want = [(short, n_args)]
            if flags is not None:        # (taken back on the way out, also of a call that raised)
                want = [("scope", flags)] + want + [("scope", 0)]
            assert ctx._L.calls == want, (name, kw, ctx._L.calls)


def test_fixture_is_well_formed():
    """G37: arrays only, under 100 KB, the rows the generator's docstring lists."""
    from conftest import load_golden
    path = os.path.join(ROOT, "tests", "golden", "g37_kernels_tabulated.npz")
    assert os.path.getsize(path) < 100 * 1024
    g = load_golden("g37_kernels_tabulated")
    for name in g.files:
        assert g[name].dtype == numpy.float64 and numpy.all(numpy.isfinite(g[name])), name
    D2R = numpy.pi / 180.0
    assert numpy.array_equal(g["theta"], numpy.logspace(-3, 0, 9) * D2R)
    ell = load_golden("g33_cell_hods")["ell"]
    assert g["ell"].shape == (6,) and all(l in ell for l in g["ell"])
    assert g["t_z"].shape == g["t_p"].shape == (4, 17)
    assert numpy.array_equal(g["t_order"], [2, 2, 3, 2])
    assert numpy.array_equal(g["t_smoothing"] > 0, [False, False, True, False])
    assert g["j0_w"].shape == (4, 9) and g["j0_cl"].shape == (4, 6) and g["j2_w"].shape == (1, 9)
    assert numpy.array_equal(g["j0_tab"], [[0, 0], [0, 1], [-1, 1], [-1, -1]])
    assert numpy.array_equal(g["j2_tab"], [[3, 2]]) and numpy.array_equal(g["j2_wkind"], [[0, 1]])
    g34 = load_golden("g34_wtheta_cosmologies")
    for i in (0, 1):
        assert numpy.array_equal(g["j0_cosmo"][i], g34["cosmo"][0])
    assert numpy.array_equal(g["j0_cosmo"][2], g34["cosmo"][1])
    assert numpy.array_equal(g["j0_cosmo"][3, :8], g34["cosmo"][0][:8])
    assert numpy.array_equal(g["j0_cosmo"][3, 8:], [-0.9, 0.2])
    assert numpy.array_equal(g["j2_cosmo"][0], g34["cosmo"][0])
    for r in (g["j0_w"], g["j0_cl"]):
        for i in range(4):
            for j in range(i):
                assert numpy.max(numpy.abs(r[i] / r[j] - 1)) > 1e-3, (i, j)
