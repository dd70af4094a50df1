"""w(theta) over cosmologies: the set axis of the projection set-up (chomp_kernel_setup_sets,
chomp_kernel_info_sets, chomp_kernel_table_set), chomp_wtheta_sets and their Python routes
(Correlation.correlation_cosmologies, SimulationDesign.run_design(batched="cosmology")): bit for
bit against the single set-up and the single call on the same context, against the reference's loop
over cosmologies (G34) and against the project's own loop."""
import copy
import warnings

import numpy
import pytest

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
# the bar tests/test_gpu_projection.py holds the single call to (measured 4e-11 there)
PROJ_RTOL = 1e-9
D2R = numpy.pi / 180.0
COSMO_KEYS = ("omega_m0", "omega_b0", "omega_l0", "omega_r0", "cmb_temp", "h", "sigma_8",
              "n_scalar", "w0", "wa")
TABLES = ("kernel", "levels", "wa", "wb", "wa_chi", "me_chi", "me_growth")


@pytest.fixture(scope="module")
def g34():
    import torch
    assert torch.cuda.is_available()
    return load_golden("g34_wtheta_cosmologies")


def _cosmos(g):
    return [dict(zip(COSMO_KEYS, (float(v) for v in row))) for row in g["cosmo"]]


def _kernel(ggl=False):
    """The G6 projection (galaxy x galaxy, J0) or the G7 one (galaxy x convergence, J2)."""
    from chomp_amd import cosmology, kernel
    cm = cosmology.MultiEpoch(0.0, 5.0)
    wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    if ggl:
        wb = kernel.WindowFunctionConvergence(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2), cm)
        return kernel.GalaxyGalaxyLensingKernel(1e-6 * D2R, 100.0 * D2R, wa, wb, cm)
    wb = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    return kernel.Kernel(1e-6 * D2R, 100.0 * D2R, wa, wb, cm)


def _single_setup(ctx, kern, cosmo, wa=None, wb=None):
    """chomp_kernel_setup of `kern`'s windows with another cosmology."""
    ctx.kernel_setup(cosmo, kern.cosmo.z_min, kern.cosmo.z_max, kern._ktheta[0], kern._ktheta[1],
                     kern.window_function_a._struct() if wa is None else wa,
                     kern.window_function_b._struct() if wb is None else wb, kern._order)


@pytest.mark.parametrize("ggl", [False, True], ids=["galaxy-galaxy-J0", "galaxy-convergence-J2"])
def test_setup_sets_bit_for_bit(g34, ggl):
    from chomp_amd import cosmology
    cosmos = _cosmos(g34)
    kern = _kernel(ggl)
    ctx = cosmology._context()
    single = []
    for c in cosmos:
        _single_setup(ctx, kern, c)
        single.append((ctx.kernel_info(), {t: ctx.kernel_table(t) for t in TABLES}))
    last = ctx.kernel_info()
    kern._setup_sets_on(ctx, cosmos)
    info = ctx.kernel_info_sets()
    for s, (one, tabs) in enumerate(single):
        for name, value in one.items():
            assert numpy.array_equal(info[name][s], value), (s, name, info[name][s], value)
        for t in TABLES:
            assert numpy.array_equal(ctx.kernel_table_set(s, t), tabs[t]), (s, t)
    # the sets differ from one another (0 and 2 share their densities, hence chi(z) in Mpc/h and
    # the normalised growth: the projection of 2 is that of 0), and the single set-up is as it was
    assert info["chi_max"][0] != info["chi_max"][1] and info["chi_max"][1] != info["chi_max"][2]
    assert not numpy.array_equal(single[0][1]["kernel"], single[1][1]["kernel"])
    assert not numpy.array_equal(ctx.kernel_table_set(1, "wa"), ctx.kernel_table_set(2, "wa"))
    after = ctx.kernel_info()
    assert all(numpy.array_equal(after[name], last[name]) for name in last)
    assert numpy.array_equal(ctx.kernel_table("kernel"), single[2][1]["kernel"])
    with pytest.raises(ValueError):
        ctx.kernel_table_set(3, "kernel")


class _Grid(object):
    """A HaloGrid of one epoch per cosmology at that cosmology's z_bar, with the sets staged on its
    context: what chomp_wtheta_sets and chomp_kernel_setup + chomp_wtheta are compared on."""

    def __init__(self, cosmos, spectrum):
        from chomp_amd import correlation, defaults, grid
        self.cosmos = cosmos
        self.kern = _kernel()
        self.hg = grid.HaloGrid(numpy.zeros(len(cosmos)), cosmo_dict=list(cosmos))
        self.ctx = self.hg.ctx
        info = self.stage()
        self.z_bar, self.D = info["z_bar"], info["D_zbar"]
        self.hg.set_parameters(z=self.z_bar)
        self.hg.setup(spectrum)
        self.code = correlation._POWER[spectrum][0]
        self.k = (defaults.default_limits["k_min"], defaults.default_limits["k_max"])

    def stage(self, first=0, n=None):
        n = len(self.cosmos) - first if n is None else n
        self.kern._setup_sets_on(self.ctx, self.cosmos[first:first + n])
        return self.ctx.kernel_info_sets()

    def batch(self, theta):
        return self.ctx.wtheta_sets(self.code, 0, len(self.cosmos), *self.k, self.D, theta)

    def single(self, theta):
        rows = []
        for e, c in enumerate(self.cosmos):
            _single_setup(self.ctx, self.kern, c)
            assert self.ctx.kernel_info()["D_zbar"] == self.D[e]
            rows.append(self.ctx.wtheta(self.code, e, *self.k, self.D[e], theta))
        return numpy.array(rows)


@pytest.fixture(scope="module", params=["power_gg", "power_mm"])
def three(request, g34):
    """Three epochs (the fixture's cosmologies at their z_bar) and their single-call rows."""
    G = _Grid(_cosmos(g34), request.param)
    theta = numpy.ascontiguousarray(g34["theta"])
    ref = G.single(theta)
    ref.setflags(write=False)
    return G, theta, ref


def test_wtheta_sets_bit_for_bit(three, g34):
    from chomp_amd import _lib
    G, theta, ref = three
    assert ref.shape == (3, 9) and numpy.all(numpy.isfinite(ref))
    assert numpy.max(numpy.abs(ref[1] / ref[0] - 1)) > 1e-3      # (the cosmologies do differ)
    assert numpy.array_equal(G.z_bar, g34["z_bar"])
    assert not G.hg.status().any()                               # (the fixture's condition)
    got = G.batch(theta)
    assert got.shape == (3, 9) and numpy.array_equal(got, ref)
    try:                                                         # (a seam inside three epochs)
        G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, 2)
        seam = G.batch(theta)
    finally:
        G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, -1)
    assert numpy.array_equal(seam, ref)
    one = G.batch(theta[4:5])
    assert one.shape == (3, 1) and numpy.array_equal(one[:, 0], ref[:, 4])


def test_wtheta_sets_single_epoch(three):
    """n_epoch = 1: one set, any epoch of the context."""
    G, theta, ref = three
    try:
        info = G.stage(1, 1)
        assert numpy.array_equal(info["D_zbar"], G.D[1:2])
        got = G.ctx.wtheta_sets(G.code, 1, 1, *G.k, G.D[1:2], theta)
    finally:
        G.stage()
    assert got.shape == (1, 9) and numpy.array_equal(got, ref[1:2])
    assert numpy.array_equal(G.batch(theta), ref)


@pytest.mark.parametrize("over", [dict(divmax=8), dict(kernel_npoints=72), "direct"])
def test_other_routes(g34, over):
    """A shallow node table (divmax 8), more kernel knots than a wavefront has lanes (72: the
    node-by-node kernel) and CHOMP_TUNE_WTHETA_DIRECT: each equal to the per-epoch calls on that
    context.  (divmax = 22, the node-by-node kernel beyond the table, takes the same kernel as the
    other two and tens of seconds: left to tests/test_gpu_wtheta_hods.py.)"""
    from chomp_amd import _lib, defaults
    saved = copy.deepcopy(defaults.default_precision)
    theta = numpy.ascontiguousarray(g34["theta"][[0, 3, 5, 7, 8]])
    try:
        if over != "direct":
            defaults.default_precision.update(over)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")              # (divmax warnings of the shallow set-up)
            G = _Grid(_cosmos(g34), "power_gg")
            try:
                if over == "direct":
                    G.ctx.set_tuning(_lib.TUNE_WTHETA_DIRECT, 1)
                ref = G.single(theta)
                got = G.batch(theta)
                try:
                    G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, 2)
                    seam = G.batch(theta)
                finally:
                    G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, -1)
            finally:
                G.ctx.set_tuning(_lib.TUNE_WTHETA_DIRECT, -1)
    finally:
        defaults.default_precision.clear()
        defaults.default_precision.update(saved)
    assert ref.shape == (3, 5) and numpy.all(numpy.isfinite(ref))
    assert numpy.array_equal(got, ref) and numpy.array_equal(seam, ref)


def test_refusals(three):
    """CHOMP_ERR_SCOPE: a HaloFit code, a tabulated distribution, a w0-wa cosmology; CHOMP_ERR_ARG:
    n_epoch that is not the number of sets, more sets than the bound; CHOMP_ERR_STATE: wtheta_sets
    before any set-up."""
    from chomp_amd import _lib, cosmology, kernel
    G, theta, ref = three
    with pytest.raises(_lib.ChompScopeError, match="HaloFit"):
        G.ctx.wtheta_sets(G.code | _lib.P_HALOFIT, 0, 3, *G.k, G.D, theta)
    with pytest.raises(ValueError, match="number of sets"):
        G.ctx.wtheta_sets(G.code, 0, 2, *G.k, G.D[:2], theta)
    fresh = cosmology._context()
    with pytest.raises(_lib.ChompError, match="before kernel_setup_sets"):
        fresh.wtheta_sets(G.code, 0, 3, *G.k, G.D, theta)
    with pytest.raises(_lib.ChompError, match="before kernel_setup_sets"):
        fresh.kernel_info_sets()
    z = numpy.linspace(0.0, 2.0, 33)
    tab = kernel.WindowFunctionGalaxy(kernel.dNdzInterpolation(z, z * z * numpy.exp(-z / 0.3)),
                                      G.kern.cosmo)
    kern = G.kern
    args = (kern.cosmo.z_min, kern.cosmo.z_max, kern._ktheta[0], kern._ktheta[1])
    wa = kern.window_function_a._struct()
    with pytest.raises(_lib.ChompScopeError, match="tabulated"):
        fresh.kernel_setup_sets(G.cosmos, *args, wa, tab._struct(), 0)
    with pytest.raises(_lib.ChompScopeError, match="w0/wa"):
        fresh.kernel_setup_sets([G.cosmos[0], dict(G.cosmos[1], w0=-0.9)], *args, wa, wa, 0)
    with pytest.raises(ValueError, match="sets in one call"):
        fresh.kernel_setup_sets([G.cosmos[0]] * (_lib.KERNEL_SETS_MAX + 1), *args, wa, wa, 0)
    with pytest.raises(_lib.ChompError, match="before kernel_setup_sets"):   # (nothing was staged)
        fresh.kernel_info_sets()
    assert numpy.array_equal(G.batch(theta), ref)


def test_refuses_the_wiggle_transfer_function(g34):
    """A context with the wiggle transfer function is out of scope, as for chomp_wtheta_epochs (a
    grid of its own: the switch drops the context's tables)."""
    from chomp_amd import _lib
    G = _Grid(_cosmos(g34)[:2], "power_gg")
    theta = numpy.ascontiguousarray(g34["theta"][:3])
    assert G.batch(theta).shape == (2, 3)
    G.ctx.set_transfer(True)
    with pytest.raises(_lib.ChompScopeError, match="wiggle"):
        G.batch(theta)


@pytest.fixture(scope="module")
def corrs(g34):
    """Per spectrum: (Correlation, its correlation_cosmologies rows over the fixture's points)."""
    from chomp_amd import correlation, halo
    theta = numpy.ascontiguousarray(g34["theta"])
    out = {}
    for ps in ("power_gg", "power_mm"):
        corr = correlation.Correlation(0.001, 1.0, _kernel(), input_halo=halo.Halo(0.0),
                                       power_spec=ps)
        before = (dict(corr.get_cosmology()), dict(corr.halo.cosmo.cosmo_dict),
                  corr.halo.get_redshift(), corr.kernel._signature(), corr.halo.local_hod)
        rows, words = corr.correlation_cosmologies(theta, _cosmos(g34), with_status=True)
        # the Correlation's own kernel, halo, cosmology and HOD are untouched
        assert (dict(corr.get_cosmology()), dict(corr.halo.cosmo.cosmo_dict),
                corr.halo.get_redshift(), corr.kernel._signature(), corr.halo.local_hod) == before
        assert words.shape == (3,) and not words.any() and words is corr.cosmologies_status
        rows.setflags(write=False)
        out[ps] = (corr, rows)
    return out


@pytest.mark.parametrize("ps", ["power_gg", "power_mm"])
def test_against_the_reference(g34, corrs, ps):
    """The batch against the reference's loop (G34) at the bar of the single call, and the
    project's existing loop (set_cosmology + correlation, unchanged code) against the same rows,
    printed first: what the bar means at the two cosmologies nobody had measured.  Measured on the
    MI355X, loop and batch alike: power_gg 4.4e-11 / 3.6e-11 / 3.6e-11, power_mm 5.2e-11 / 4.3e-11
    / 4.2e-11 -- the loop meets 1e-9 at all three points, so no point's bar is widened."""
    from chomp_amd import correlation, halo
    corr, rows = corrs[ps]
    theta = numpy.ascontiguousarray(g34["theta"])
    assert rows.shape == (3, 9)
    assert numpy.array_equal(corr.cosmologies_z_bar, g34["z_bar"])
    loop = correlation.Correlation(0.001, 1.0, _kernel(), input_halo=halo.Halo(0.0), power_spec=ps)
    for i, c in enumerate(_cosmos(g34)):
        loop.set_cosmology(c)
        print("G34 %s cosmology %d: loop %.2e" % (ps, i, rel_err(loop.correlation(theta),
                                                                  g34["w_" + ps][i])))
    for i in range(3):
        err = rel_err(rows[i], g34["w_" + ps][i])
        print("G34 %s cosmology %d: batch %.2e" % (ps, i, err))
        assert err < PROJ_RTOL, (ps, i, err)


@pytest.mark.parametrize("ps", ["power_gg", "power_mm"])
def test_against_the_loop(g34, corrs, ps):
    """The loop set_cosmology + correlation on a second Correlation; a second call with the points
    reversed reuses the grid."""
    from chomp_amd import correlation, halo
    corr, rows = corrs[ps]
    theta = numpy.ascontiguousarray(g34["theta"])
    cosmos = _cosmos(g34)
    loop = correlation.Correlation(0.001, 1.0, _kernel(), input_halo=halo.Halo(0.0), power_spec=ps)
    for i, c in enumerate(cosmos):
        loop.set_cosmology(c)
        err = rel_err(rows[i], loop.correlation(theta))
        print("loop %s cosmology %d: %.2e" % (ps, i, err))
        assert err < 2 * PROJ_RTOL, (ps, i, err)
        assert loop.kernel.z_bar == corr.cosmologies_z_bar[i]
    hg = corr._cosmologies_grid[1]
    again = corr.correlation_cosmologies(theta, cosmos[::-1])
    assert corr._cosmologies_grid[1] is hg
    assert numpy.array_equal(again, rows[::-1])
    assert numpy.array_equal(corr.cosmologies_z_bar, g34["z_bar"][::-1])
    assert corr.correlation_cosmologies(theta[:0], cosmos).shape == (3, 0)
    assert corr.correlation_cosmologies(theta, []).shape == (0, 9)
    assert corr.cosmologies_status.shape == (0,)


def test_hods_move_the_rows(g34, corrs):
    from chomp_amd import correlation, halo, hod
    corr, rows = corrs["power_gg"]
    theta = numpy.ascontiguousarray(g34["theta"][[1, 4, 7]])
    cosmos = _cosmos(g34)[:2]
    hods = [{"log_M_min": 12.14, "sigma": 0.05, "log_M_0": 12.14, "log_M_1p": 13.43, "alpha": 1.0},
            hod.HODMandelbaum({"log_M_0": 12.8, "w": 0.5})]
    got = corr.correlation_cosmologies(theta, cosmos, hods=hods)
    assert got.shape == (2, 3)
    for i in range(2):
        assert rel_err(got[i], rows[i][[1, 4, 7]]) > 1e-3
    loop = correlation.Correlation(0.001, 1.0, _kernel(), input_halo=halo.Halo(0.0),
                                   power_spec="power_gg")
    loop.set_cosmology(cosmos[1])
    loop.set_hod_object(hods[1])
    assert rel_err(got[1], loop.correlation(theta)) < 2 * PROJ_RTOL
    with pytest.raises(ValueError):
        corr.correlation_cosmologies(theta, cosmos, hods=hods[:1])


def test_device_buffers(g34, corrs):
    import torch
    corr, rows = corrs["power_gg"]
    theta = torch.as_tensor(g34["theta"], device="cuda")
    got, words = corr.correlation_cosmologies(theta, _cosmos(g34), with_status=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == (3, 9)
    assert numpy.array_equal(got.cpu().numpy(), rows)
    assert words.shape == (3,) and not words.any()


def test_design_matches_the_loop(g34):
    from chomp_amd import correlation, halo, simulation_design
    theta = numpy.ascontiguousarray(g34["theta"][[0, 2, 4, 6, 8]])
    params = {"omega_m0": [0.3, 0.27, 0.33], "sigma_8": [0.8, 0.75, 0.85]}
    corr = correlation.Correlation(0.001, 1.0, _kernel(), input_halo=halo.Halo(0.0),
                                   power_spec="power_gg")
    numpy.random.seed(11)
    des = simulation_design.SimulationDesignFlatUniverse(
        corr, "correlation", params, n_design=4, independent_var=theta)
    assert not des._batched()                    # (None and True never pick the cosmology route)
    frame, status = des.run_design(batched="cosmology", with_status=True)
    assert frame.shape == (5, 4) and list(frame.columns) == list(des.points.index)
    assert list(status.index) == list(des.points.index) and not status.any()
    assert status is des.design_status
    loop = des.run_design(batched=False)
    assert des.design_status is None and loop.shape == (5, 4)
    for col in frame.columns:
        err = rel_err(frame[col].values, loop[col].values)
        print("design point %s: %.2e" % (col, err))
        assert err < 2 * PROJ_RTOL, (col, err)
    assert rel_err(frame[0].values, frame[1].values) > 1e-3     # (the points do differ)
