"""Host side of the batch over kernels (window pairs, MultiEpoch ranges, cosmologies): the C
declarations of chomp_kernel_setup_pairs / chomp_cell_sets and their bindings, the scope of
Correlation.correlation_kernels, the G36 fixture, the oracle against it and the routes its C_l
rows take.  No device."""
import os
import re

import numpy
import pytest

from conftest import ROOT, load_golden

D2R = numpy.pi / 180.0
THETA = numpy.logspace(-3, 0, 5) * D2R
KTHETA = (1e-6 * D2R, 100.0 * D2R)
COSMO_KEYS = ("omega_m0", "omega_b0", "omega_l0", "omega_r0", "cmb_temp", "h", "sigma_8",
              "n_scalar", "w0", "wa")
ZHENG_KEYS = ("log_M_min", "sigma", "log_M_0", "log_M_1p", "alpha")
ZEHAVI = {"log_M_min": 12.14, "sigma": 0.15, "log_M_0": 12.14, "log_M_1p": 13.43, "alpha": 1.0}


# -- the fixture's rows as this package's objects (tests/test_gpu_kernels_batch.py shares them) ----
def fixture_cosmo(g, tag, i):
    return dict(zip(COSMO_KEYS, (float(v) for v in g[tag + "_cosmo"][i])))


def fixture_hod(g, tag, i):
    return dict(zip(ZHENG_KEYS, (float(v) for v in g[tag + "_zheng"][i])))


def fixture_kernel(g, tag, i):
    """Row i of group `tag` ("j0": Kernel, "j2": GalaxyGalaxyLensingKernel) of G36 as a fresh kernel
    with its own MultiEpoch."""
    from chomp_amd import cosmology, kernel
    me = cosmology.MultiEpoch(float(g[tag + "_me"][i, 0]), float(g[tag + "_me"][i, 1]),
                              fixture_cosmo(g, tag, i))
    win = []
    for w in range(2):
        z0, z1 = (float(v) for v in g[tag + "_dz"][i, w])
        p = [float(v) for v in g[tag + "_dpar"][i, w]]
        dist = (kernel.dNdzMagLim(z0, z1, p[0], p[1], p[2]) if g[tag + "_dkind"][i, w] == 0
                else kernel.dNdzGaussian(z0, z1, p[0], p[1]))
        cls = (kernel.WindowFunctionGalaxy if g[tag + "_wkind"][i, w] == 0
               else kernel.WindowFunctionConvergence)
        win.append(cls(dist, me))
    K = kernel.Kernel if tag == "j0" else kernel.GalaxyGalaxyLensingKernel
    return K(KTHETA[0], KTHETA[1], win[0], win[1], me)


def fixture_kernels(g, tag):
    return [fixture_kernel(g, tag, i) for i in range(g[tag + "_w"].shape[0])]


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to create a device context fails the test."""
    from chomp_amd import cosmology

    def boom(*a, **k):
        raise AssertionError("a device context was asked for")
    monkeypatch.setattr(cosmology, "_context", boom)


def _kernel(cls=None, dist_b=None, ktheta=KTHETA, cosmo=None):
    from chomp_amd import cosmology, kernel
    me = cosmology.MultiEpoch(0.0, 5.0, cosmo)
    wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), me)
    wb = kernel.WindowFunctionGalaxy(
        kernel.dNdzGaussian(0.0, 1.0, 0.4, 0.1) if dist_b is None else dist_b, me)
    return (kernel.Kernel if cls is None else cls)(ktheta[0], ktheta[1], wa, wb, me)


def _bare(h, power_name="power_gg", cls=None, kern=None):
    """A Correlation without its constructor's device work."""
    from chomp_amd import correlation
    cls = correlation.Correlation if cls is None else cls
    corr = cls.__new__(cls)
    corr.kernel = _kernel() if kern is None else kern
    corr.halo = h
    corr.D_z = 1.0
    corr._k_lim = (h._k_min, h._k_max)
    corr._power_name = power_name
    return corr


def test_header_declares_the_entry_points():
    from chomp_amd import _lib
    with open(os.path.join(ROOT, "include", "chomp_mi355x.h")) as f:
        header = f.read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    for decl in (
            "int chomp_kernel_setup_pairs(chomp_ctx* ctx, size_t n_set, const chomp_cosmo* cosmo , "
            "const double* me_z_min , const double* me_z_max , double ktheta_min, double ktheta_max, "
            "const chomp_window* a , const chomp_window* b , int bessel_order);",
            "int chomp_cell_sets(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, "
            "const double* D_z , const double* ell, size_t n, double* out, int mem);"):
        assert decl in flat, decl
    # (the prototypes as the issue states them, comments included)
    assert ("const double* me_z_min /*[n_set]*/, const double* me_z_max /*[n_set]*/,"
            in re.sub(r"\s+", " ", header))
    assert "const double* D_z /*[n_epoch], host*/, const double* ell, size_t n," in re.sub(
        r"\s+", " ", header)
    m = re.search(r"#define CHOMP_TUNE_COUNT (\d+)\b", header)
    assert m and int(m.group(1)) == 12
    assert "C_l has no such call" not in header
    for name in ("kernel_setup_pairs", "cell_sets"):
        assert "chomp_" + name in _lib.EXPORTS
        assert callable(getattr(_lib.Context, name))
    from chomp_amd import correlation, kernel
    assert callable(kernel.Kernel._setup_pairs_on)
    assert callable(correlation.Correlation.correlation_kernels)
    assert (correlation.CorrelationFourier.correlation_kernels
            is correlation.Correlation.correlation_kernels)
    assert (correlation.CorrelationFourier._kernels_evaluate
            is not correlation.Correlation._kernels_evaluate)


def _out_of_scope():
    """(label, Correlation, kernels, hods) of every case correlation_kernels refuses."""
    from chomp_amd import cosmology, halo, hod, kernel
    fit = halo.HaloFit.__new__(halo.HaloFit)
    fit.__dict__.update(halo.Halo(0.0).__dict__)
    two = [_kernel(), _kernel()]
    cases = [("HaloFit", _bare(fit), two, None),
             ("HaloExclusion", _bare(halo.HaloExclusion(0.0)), two, None),
             ("general_profile", _bare(halo.Halo(0.0, general_profile=True)), two, None),
             ("extrapolat", _bare(halo.Halo(0.0, extrapolate=True)), two, None)]
    h = halo.Halo(0.0, cosmo_single_epoch=cosmology.SingleEpoch(0.0, with_bao=True))
    cases.append(("with_bao", _bare(h), two, None))
    h = halo.Halo(0.0)
    h.set_halo(dict(h.get_halo(), c0=7.5))
    cases.append(("set_halo", _bare(h), two, None))
    cases.append(("hods[1]", _bare(halo.Halo(0.0)), two, [ZEHAVI, hod.HOD(dict(ZEHAVI))]))
    # what the kernel axis adds
    cases.append(("kernel 1 is a GalaxyGalaxyLensingKernel, this object's kernel a Kernel",
                  _bare(halo.Halo(0.0)), [_kernel(), _kernel(kernel.GalaxyGalaxyLensingKernel)],
                  None))
    cases.append(("kernel 0 is a Kernel, this object's kernel a GalaxyGalaxyLensingKernel",
                  _bare(halo.Halo(0.0), kern=_kernel(kernel.GalaxyGalaxyLensingKernel)), two, None))

    class Other(kernel.Kernel):
        pass
    cases.append(("kernel 1 is a Other", _bare(halo.Halo(0.0)), [_kernel(), _kernel(Other)], None))
    cases.append(("this object's kernel is a Other", _bare(halo.Halo(0.0), kern=_kernel(Other)),
                  [_kernel(Other)], None))
    cases.append(("kernel 1 has another k theta range", _bare(halo.Halo(0.0)),
                  [_kernel(), _kernel(ktheta=(KTHETA[0], 2.0 * KTHETA[1]))], None))
    moved = _kernel()
    moved.z_bar = 0.4
    cases.append(("kernel 1 has an assigned z_bar", _bare(halo.Halo(0.0)), [_kernel(), moved], None))
    z = numpy.linspace(0.0, 2.0, 17)
    tab = kernel.dNdzInterpolation(z, z * z * numpy.exp(-z / 0.3))
    cases.append(("kernel 1: window_function_b has a tabulated redshift distribution "
                  "(dNdzInterpolation)", _bare(halo.Halo(0.0)), [_kernel(), _kernel(dist_b=tab)],
                  None))
    from chomp_amd import defaults
    de = dict(defaults.default_cosmo_dict, w0=-0.9, wa=0.1)
    cases.append(("kernel 1 has a w0-wa cosmology", _bare(halo.Halo(0.0)),
                  [_kernel(), _kernel(cosmo=de)], None))
    return cases


@pytest.mark.parametrize("fourier", [False, True], ids=["w", "cl"])
def test_correlation_kernels_refuses_what_it_does_not_serve(no_device, fourier):
    from chomp_amd import _lib, correlation
    for label, corr, kernels, hods in _out_of_scope():
        if fourier:
            corr.__class__ = correlation.CorrelationFourier
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)) as info:
            corr.correlation_kernels(THETA, kernels, hods=hods)
        assert str(info.value).startswith("correlation_kernels: ")
        assert str(info.value).endswith(
            "use the loop fresh Correlation objects, one per kernel, + correlation")


def test_hods_must_match_the_kernels(no_device):
    from chomp_amd import halo
    with pytest.raises(ValueError, match="1 hods for 2 kernels"):
        _bare(halo.Halo(0.0)).correlation_kernels(THETA, [_kernel(), _kernel()], hods=[ZEHAVI])


def test_empty_inputs_need_no_device(no_device):
    from chomp_amd import correlation, halo
    for cls in (correlation.Correlation, correlation.CorrelationFourier):
        corr = _bare(halo.Halo(0.0), cls=cls)
        out, words = corr.correlation_kernels(THETA, [], with_status=True)
        assert out.shape == (0, 5) and words.shape == (0,) and words.dtype == numpy.uint32
        assert corr.correlation_kernels(THETA[:0], [_kernel(), _kernel()]).shape == (2, 0)
        assert corr.kernels_z_bar.shape == (2,) and corr.kernels_D_z.shape == (2,)
        assert corr.kernels_status.shape == (2,)


def test_correlation3d_has_no_kernels(no_device):
    from chomp_amd import _lib, correlation, halo
    corr = correlation.Correlation3d.__new__(correlation.Correlation3d)
    corr.halo = halo.Halo(0.0)
    with pytest.raises(_lib.ChompScopeError, match="Correlation3d.correlation_kernels"):
        corr.correlation_kernels(numpy.array([1.0]), [])


def test_fourier_over_cosmologies_is_still_refused(no_device):
    """The pinned refusal: its message names chomp_cell_epochs as before."""
    from chomp_amd import _lib, correlation, defaults, halo
    corr = _bare(halo.Halo(0.0), cls=correlation.CorrelationFourier)
    c = dict(defaults.default_cosmo_dict)
    with pytest.raises(_lib.ChompScopeError, match="chomp_cell_epochs"):
        corr.correlation_cosmologies(numpy.array([10.0, 100.0]), [c, dict(c, sigma_8=0.9)])


def test_setup_pairs_reads_every_kernel(no_device):
    """Kernel._setup_pairs_on hands Context.kernel_setup_pairs each kernel's own cosmology, range
    and windows, and the shared k theta range and order; the kernels' own state is not touched."""
    from chomp_amd import _lib, kernel
    g = load_golden("g36_kernels")
    kernels = fixture_kernels(g, "j2")
    calls = []

    class Ctx(object):
        def kernel_setup_pairs(self, *args):
            calls.append(args)
    ctx = Ctx()
    assert kernel.Kernel._setup_pairs_on(ctx, kernels) is ctx
    (cosmos, z0, z1, kt0, kt1, wa, wb, order), = calls
    assert order == 2 and (kt0, kt1) == KTHETA
    assert cosmos == [fixture_cosmo(g, "j2", i) for i in range(3)]
    assert list(z0) == [0.0] * 3 and list(z1) == [5.0] * 3
    assert [w.kind for w in wa] == [_lib.WINDOW_GALAXY] * 3
    assert [w.kind for w in wb] == [_lib.WINDOW_CONVERGENCE] * 3
    assert [w.dist.kind for w in wa] == [_lib.DNDZ_MAGLIM, _lib.DNDZ_GAUSSIAN, _lib.DNDZ_GAUSSIAN]
    assert all(k._done == {} and k._info is None for k in kernels)


def test_fixture_is_well_formed():
    g = load_golden("g36_kernels")
    assert numpy.array_equal(g["theta"], numpy.logspace(-3, 0, 9) * D2R)
    assert numpy.array_equal(g["ell"], load_golden("g33_cell_hods")["ell"]) and g["ell"].shape == (22,)
    for name in g.files:
        assert g[name].dtype == numpy.float64, name
        assert numpy.all(numpy.isfinite(g[name])), name
    for tag, n in (("j0", 5), ("j2", 3)):
        assert g[tag + "_w"].shape == (n, 9)
        assert g[tag + "_wkind"].shape == (n, 2) and g[tag + "_dkind"].shape == (n, 2)
        assert g[tag + "_dz"].shape == (n, 2, 2) and g[tag + "_dpar"].shape == (n, 2, 3)
        assert g[tag + "_me"].shape == (n, 2) and g[tag + "_cosmo"].shape == (n, 10)
        assert g[tag + "_zheng"].shape == (n, 5)
        assert g[tag + "_z_bar"].shape == (n,) and g[tag + "_D_z"].shape == (n,)
        rows = [g[tag + "_w"]] + ([g["j0_cl"]] if tag == "j0" else [])
        for r in rows:
            for i in range(n):
                for j in range(i):
                    assert numpy.max(numpy.abs(r[i] / r[j] - 1)) > 1e-3, (tag, i, j)
    assert g["j0_cl"].shape == (5, 22)
    # what the rows are: the windows of the G6 / G7 projections first (rows 0 and 3 of J0 are G34's
    # first two points), the lens-bin auto-correlation on its own MultiEpoch range, the second
    # cosmology where the issue puts it, the other HOD in J0 row 4
    g34 = load_golden("g34_wtheta_cosmologies")
    assert numpy.array_equal(g["j0_z_bar"][[0, 3]], g34["z_bar"][:2])
    assert numpy.array_equal(g["j0_D_z"][[0, 3]], g34["D_z"][:2])
    assert numpy.array_equal(g["j0_me"][:, 1], [5.0, 2.0, 5.0, 5.0, 5.0])
    assert numpy.array_equal(g["j0_cosmo"][3], g34["cosmo"][1])
    assert numpy.array_equal(g["j2_cosmo"][2], g34["cosmo"][1])
    for tag, rows in (("j0", (0, 1, 2, 4)), ("j2", (0, 1))):
        for i in rows:
            assert numpy.array_equal(g[tag + "_cosmo"][i], g34["cosmo"][0])
    zheng = load_golden("g32_wtheta_hods")["zheng"]
    assert all(numpy.array_equal(g["j0_zheng"][i], zheng[0]) for i in range(4))
    assert numpy.array_equal(g["j0_zheng"][4], zheng[1])
    assert numpy.allclose(g["j0_z_bar"], [0.286, 0.408, 0.367, 0.286, 0.338], atol=6e-4)


def oracle_of_fixture(g, tag):
    """The oracle's w(theta) (and, for j0, C_l with its stopping levels) of every row of group
    `tag` of the fixture `g`, from nothing but the fixture's arrays: (w [n, 9], cl [n, 22] or
    None, levels [n][22] or None)."""
    from oracle import chomp_oracle as o
    fam, order = ("gg", 0) if tag == "j0" else ("gm", 2)
    ws, cls, levels = [], [], []
    for i in range(g[tag + "_w"].shape[0]):
        cosmo = fixture_cosmo(g, tag, i)
        me = o.multi_epoch(float(g[tag + "_me"][i, 0]), float(g[tag + "_me"][i, 1]), cosmo)
        win = []
        for w in range(2):
            z0, z1 = (float(x) for x in g[tag + "_dz"][i, w])
            p = [float(x) for x in g[tag + "_dpar"][i, w]]
            dist = (o.dndz_maglim(z0, z1, p[0], p[1], p[2]) if g[tag + "_dkind"][i, w] == 0
                    else o.dndz_gaussian(z0, z1, p[0], p[1]))
            win.append(o.window_table("galaxy" if g[tag + "_wkind"][i, w] == 0 else "convergence",
                                      dist, me))
        kt = o.kernel_table(KTHETA[0], KTHETA[1], win[0], win[1], me, bessel_order=order)
        e = o.epoch(cosmo, kt.z_bar)
        t = o.halo_table(e, o.mass_table(e), o.zheng(fixture_hod(g, tag, i)), families=(fam,))

        def power(k, t=t):
            return o.halo_power(t, fam, k)
        D_z = float(g[tag + "_D_z"][i])
        ws.append(o.wtheta(kt, power, g["theta"], e.k_min, e.k_max, D_z))
        if tag == "j0":
            lev = []
            cls.append(o.cell(kt, power, g["ell"], D_z, levels=lev))
            levels.append([int(x) for x in lev])
    if tag != "j0":
        return numpy.array(ws), None, None
    return numpy.array(ws), numpy.array(cls), levels


@pytest.fixture(scope="module")
def oracle_rows():
    g = load_golden("g36_kernels")
    return g, oracle_of_fixture(g, "j0"), oracle_of_fixture(g, "j2")


def test_oracle_reproduces_the_fixture(oracle_rows):
    """The bar tests/test_cell_hods_cpu.py and tests/test_gpu_projection.py use, 1e-9."""
    g, (w0, cl0, _), (w2, _, _) = oracle_rows
    assert w0.shape == (5, 9) and cl0.shape == (5, 22) and w2.shape == (3, 9)
    for name, got, want in (("J0 w", w0, g["j0_w"]), ("J0 C_l", cl0, g["j0_cl"]),
                            ("J2 w", w2, g["j2_w"])):
        for i in range(got.shape[0]):
            err = numpy.max(numpy.abs(got[i] / want[i] - 1))
            print("oracle against G36, %s row %d: %.2e" % (name, i, err))
            assert err < 1e-9, (name, i, err)


def test_fixture_covers_every_route(oracle_rows):
    """The levels at which the integrals stop decide the route of a multipole on the device: up to
    8 a wavefront's own levels, 9..11 the block's cooperative walk, 12 and beyond the deep kernel
    and its per-row lists.  All three occur; row 1 lists nothing for the deep kernel, rows 0 and 3
    list different multipoles: a kernel that read another row's list or node table cannot pass."""
    _, (_, _, levels), _ = oracle_rows
    levels = numpy.array(levels)
    print("levels:\n%s" % levels)
    assert levels.shape == (5, 22)
    assert numpy.any(levels <= 8)
    assert numpy.any((levels >= 9) & (levels <= 11))
    assert numpy.any(levels >= 12)
    deep = [frozenset(numpy.nonzero(row >= 12)[0]) for row in levels]
    assert not deep[1]
    assert deep[0] and deep[3] and deep[0] != deep[3], deep
