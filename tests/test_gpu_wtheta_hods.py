"""w(theta) with an epoch axis (chomp_wtheta_epochs) and its Python routes
(Correlation.correlation_hods, SimulationDesign over HOD parameters of Correlation.correlation):
bit for bit against the single-epoch call on the same context, against the reference's loop over
HODs (G32) and against the project's own loop."""
import copy
import warnings

import numpy
import pytest

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
# the bar tests/test_gpu_projection.py holds the single call to (measured 4e-11 there)
PROJ_RTOL = 1e-9
D2R = numpy.pi / 180.0
STATUS_DIVMAX = 16
ZHENG_KEYS = ("log_M_min", "sigma", "log_M_0", "log_M_1p", "alpha")


@pytest.fixture(scope="module")
def g32():
    import torch
    assert torch.cuda.is_available()
    return load_golden("g32_wtheta_hods")


def _kernel():
    """The G6 projection: galaxy x galaxy windows."""
    from chomp_amd import cosmology, kernel
    cm = cosmology.MultiEpoch(0.0, 5.0)
    wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    wb = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    return kernel.Kernel(1e-6 * D2R, 100.0 * D2R, wa, wb, cm)


def _hods(g, with_default=False):
    """The fixture's HODs in its row order: three Zheng dictionaries, one Mandelbaum object."""
    from chomp_amd import defaults, hod
    out = [dict(zip(ZHENG_KEYS, (float(v) for v in row))) for row in g["zheng"]]
    out.append(hod.HODMandelbaum({"log_M_0": float(g["mandelbaum"][0]), "w": float(g["mandelbaum"][1])}))
    if with_default:
        out.append(dict(defaults.default_hod_dict))
    return out


class _Grid(object):
    """A HaloGrid of one epoch per HOD at the kernel's z_bar with the kernel staged on its context:
    what chomp_wtheta_epochs and chomp_wtheta are compared on."""

    def __init__(self, hods, spectrum):
        from chomp_amd import correlation, defaults, grid
        self.kern = _kernel()
        self.hg = grid.HaloGrid(numpy.full(len(hods), self.kern.z_bar), hod_dict=list(hods))
        self.ctx = self.kern._setup_on(self.hg.ctx)
        self.hg.setup(spectrum)
        self.code = correlation._POWER[spectrum][0]
        self.args = (defaults.default_limits["k_min"], defaults.default_limits["k_max"],
                     self.kern._get("D_zbar"))

    def batch(self, theta, epoch0=0, n=None):
        n = len(self.hg.idx) - epoch0 if n is None else n
        return self.ctx.wtheta_epochs(self.code, epoch0, n, *self.args, theta)

    def single(self, theta, epoch0=0, n=None):
        n = len(self.hg.idx) - epoch0 if n is None else n
        return numpy.array([self.ctx.wtheta(self.code, e, *self.args, theta)
                            for e in range(epoch0, epoch0 + n)])


@pytest.fixture(scope="module", params=["power_gg", "power_gm"])
def five(request, g32):
    """Five epochs (the fixture's HODs and the default one) and their single-epoch rows."""
    G = _Grid(_hods(g32, with_default=True), request.param)
    theta = numpy.ascontiguousarray(g32["theta"])
    ref = G.single(theta)
    ref.setflags(write=False)
    return G, theta, ref


def test_same_context_bit_for_bit(five):
    G, theta, ref = five
    assert ref.shape == (5, 9) and numpy.all(numpy.isfinite(ref))
    assert numpy.max(numpy.abs(ref[1] / ref[0] - 1)) > 1e-3      # (the epochs do differ)
    got = G.batch(theta)
    assert got.shape == (5, 9) and numpy.array_equal(got, ref)
    assert numpy.array_equal(G.batch(theta, 2, 2), ref[2:4])


def test_chunk_seam(five):
    """Chunks of 2, 2 and 1 epochs reuse one chunk's scratch: the same bits as one chunk of 5."""
    from chomp_amd import _lib
    G, theta, ref = five
    try:
        G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, 2)
        got = G.batch(theta)
    finally:
        G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, -1)
    assert numpy.array_equal(got, ref)
    assert numpy.array_equal(G.batch(theta), ref)


def test_single_theta_and_single_epoch(five):
    G, theta, ref = five
    assert numpy.array_equal(G.batch(theta[4:5]), G.single(theta[4:5]))
    assert numpy.array_equal(G.batch(theta[4:5])[:, 0], ref[:, 4])
    assert numpy.array_equal(G.batch(theta, 3, 1), ref[3:4])
    assert numpy.array_equal(G.batch(theta[8:9], 4, 1)[0, 0], ref[4, 8])


@pytest.mark.parametrize("over", [dict(divmax=8), dict(divmax=22), dict(kernel_npoints=72), "direct"])
def test_other_routes(g32, over):
    """A shallow node table (divmax 8), the node-by-node kernel beyond the table (divmax 22), with
    more kernel knots than a wavefront has lanes (72) and by CHOMP_TUNE_WTHETA_DIRECT: each equal
    to the per-epoch calls on that context."""
    from chomp_amd import _lib, defaults
    saved = copy.deepcopy(defaults.default_precision)
    theta = numpy.ascontiguousarray(g32["theta"][[0, 3, 5, 7, 8]])
    try:
        if over != "direct":
            defaults.default_precision.update(over)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")              # (divmax warnings of the shallow set-up)
            G = _Grid(_hods(g32)[1:], "power_gg")
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


def test_refusals(five):
    """CHOMP_ERR_SCOPE: narrowed precision, extrapolated and HaloFit spectra; CHOMP_ERR_ARG: an
    epoch range beyond the context's."""
    from chomp_amd import _lib
    G, theta, ref = five
    for code in (G.code | _lib.P_EXTRAPOLATE, G.code | _lib.P_HALOFIT):
        with pytest.raises(_lib.ChompScopeError):
            G.ctx.wtheta_epochs(code, 0, 5, *G.args, theta)
    with pytest.raises(ValueError):
        G.batch(theta, 3, 3)
    try:
        G.ctx.set_precision(_lib.PREC_F32_EVAL)
        with pytest.raises(_lib.ChompScopeError):
            G.batch(theta)
    finally:
        G.ctx.set_precision(_lib.PREC_F64)
    assert numpy.array_equal(G.batch(theta), ref)


def test_refuses_the_wiggle_transfer_function(g32):
    """A context with the wiggle transfer function is out of scope in C as in
    Correlation.correlation_hods (a grid of its own: the switch drops the context's tables)."""
    from chomp_amd import _lib
    G = _Grid(_hods(g32)[:2], "power_gg")
    theta = numpy.ascontiguousarray(g32["theta"][:3])
    assert G.batch(theta).shape == (2, 3)
    G.ctx.set_transfer(True)
    with pytest.raises(_lib.ChompScopeError, match="wiggle"):
        G.batch(theta)


def test_kept_grid_follows_the_precision_defaults(g32, corrs):
    """The kept grid is keyed by the configuration its context snapshots: another divmax between
    two calls builds another grid."""
    from chomp_amd import defaults
    corr, rows = corrs["power_gm"]
    theta = numpy.ascontiguousarray(g32["theta"][[2, 6]])
    hods = _hods(g32)
    first = corr.correlation_hods(theta, hods)
    hg = corr._hods_grid[1]
    saved = copy.deepcopy(defaults.default_precision)
    try:
        defaults.default_precision.update(divmax=19)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            corr.correlation_hods(theta, hods)
        assert corr._hods_grid[1] is not hg
        assert corr._hods_grid[1].ctx.config.divmax == 19
    finally:
        defaults.default_precision.clear()
        defaults.default_precision.update(saved)
    assert numpy.array_equal(corr.correlation_hods(theta, hods), first)
    assert corr._hods_grid[1].ctx.config.divmax == saved["divmax"]


@pytest.fixture(scope="module")
def corrs(g32):
    """Per spectrum: (Correlation, its correlation_hods rows over the fixture's HODs)."""
    from chomp_amd import correlation, halo
    kern = _kernel()
    theta = numpy.ascontiguousarray(g32["theta"])
    out = {}
    for ps in ("power_gg", "power_gm"):
        corr = correlation.Correlation(0.001, 1.0, kern, input_halo=halo.Halo(0.0), power_spec=ps)
        own = corr.halo.local_hod
        before = (corr.get_hod(), {key: getattr(own, key) for key in ZHENG_KEYS})
        rows = corr.correlation_hods(theta, _hods(g32))
        # the Correlation's own HOD is untouched
        assert corr.halo.local_hod is own
        assert (corr.get_hod(), {key: getattr(own, key) for key in ZHENG_KEYS}) == before
        rows.setflags(write=False)
        out[ps] = (corr, rows)
    return out


@pytest.mark.parametrize("ps", ["power_gg", "power_gm"])
def test_against_the_reference(g32, corrs, ps):
    corr, rows = corrs[ps]
    assert rows.shape == (4, 9)
    for i in range(4):
        err = rel_err(rows[i], g32["w_" + ps][i])
        print("G32 %s HOD %d: %.2e" % (ps, i, err))
        assert err < PROJ_RTOL, (ps, i, err)


@pytest.mark.parametrize("ps", ["power_gg", "power_gm"])
def test_against_the_loop(g32, corrs, ps):
    """The loop set_hod / set_hod_object + correlation on a second Correlation; a second call with
    other HODs reuses the grid."""
    from chomp_amd import correlation, halo
    corr, rows = corrs[ps]
    theta = numpy.ascontiguousarray(g32["theta"])
    loop = correlation.Correlation(0.001, 1.0, _kernel(), input_halo=halo.Halo(0.0), power_spec=ps)
    hods = _hods(g32)
    for i, h in enumerate(hods):
        if isinstance(h, dict):
            loop.set_hod(h)
        else:
            loop.set_hod_object(h)
        err = rel_err(rows[i], loop.correlation(theta))
        print("loop %s HOD %d: %.2e" % (ps, i, err))
        assert err < 2 * PROJ_RTOL, (ps, i, err)
    hg = corr._hods_grid[1]
    again = corr.correlation_hods(theta, hods[::-1])
    assert corr._hods_grid[1] is hg
    assert numpy.array_equal(again, rows[::-1])
    assert corr.correlation_hods(theta, hods[:2]).shape == (2, 9)   # (another size: another grid)
    assert corr.correlation_hods(theta[:0], hods).shape == (4, 0)
    assert corr.correlation_hods(theta, []).shape == (0, 9)


def test_device_buffers(g32, corrs):
    import torch
    corr, rows = corrs["power_gg"]
    theta = torch.as_tensor(g32["theta"], device="cuda")
    got, words = corr.correlation_hods(theta, _hods(g32), with_status=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == (4, 9)
    assert numpy.array_equal(got.cpu().numpy(), rows)
    assert words.shape == (4,) and not words.any()


def test_status_words_stay_with_their_points(g32):
    """A set-up whose Romberg integrals run out of levels flags the HODs that need the most of
    them.  With 2^16 nodes at the most (divmax = 16) the two-halo galaxy integrals of the steep
    satellite slope (alpha = 1.3 with log_M_1p = 13.8, HOD 2 here) still run out of levels and
    those of the Zehavi, sharp-cutoff and default HODs do not: its word, its warning, nobody
    else's; the float rows keep their shape."""
    from chomp_amd import _lib, correlation, defaults, halo
    saved = copy.deepcopy(defaults.default_precision)
    theta = numpy.ascontiguousarray(g32["theta"][[1, 4, 7]])
    hods = _hods(g32, with_default=True)
    del hods[3]                                  # (the Mandelbaum HOD is flagged at this depth too)
    try:
        defaults.default_precision.update(divmax=STATUS_DIVMAX)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            corr = correlation.Correlation(0.001, 1.0, _kernel(), input_halo=halo.Halo(0.0),
                                           power_spec="power_gg")
            rows, words = corr.correlation_hods(theta, hods, with_status=True)
    finally:
        defaults.default_precision.clear()
        defaults.default_precision.update(saved)
    print("status words at divmax %d: %s" % (STATUS_DIVMAX, [hex(int(w)) for w in words]))
    assert rows.shape == (4, 3) and rows.dtype == numpy.float64 and numpy.all(numpy.isfinite(rows))
    assert words.shape == (4,) and numpy.array_equal(words, corr.hods_status)
    flagged = [i for i, w in enumerate(words) if w]
    assert flagged == [2], [hex(int(w)) for w in words]
    assert int(words[2]) & _lib.ST_HALO_DIVMAX["pp_gg"]
    named = [str(w.message) for w in seen if issubclass(w.category, _lib.ChompAccuracyWarning)
             and str(w.message).startswith("HOD ")]
    assert len(named) == 1 and named[0].startswith("HOD 2: ")


def test_design_matches_the_loop(g32):
    from chomp_amd import correlation, halo, simulation_design
    theta = numpy.ascontiguousarray(g32["theta"][[0, 2, 4, 6, 8]])
    params = {"log_M_min": [12.14, 11.9, 12.4], "log_M_1p": [13.43, 13.1, 13.8]}
    corr = correlation.Correlation(0.001, 1.0, _kernel(), input_halo=halo.Halo(0.0),
                                   power_spec="power_gg")
    numpy.random.seed(7)
    des = simulation_design.SimulationDesignHODWakeAssumptions(
        corr, "correlation", params, n_design=6, independent_var=theta)
    assert des._batched()
    frame, status = des.run_design(with_status=True)
    assert frame.shape == (5, 6) and list(frame.columns) == list(des.points.index)
    assert list(status.index) == list(des.points.index) and not status.any()
    assert status is des.design_status
    loop = des.run_design(batched=False)
    assert des.design_status is None and loop.shape == (5, 6)
    for col in frame.columns:
        err = rel_err(frame[col].values, loop[col].values)
        print("design point %s: %.2e" % (col, err))
        assert err < 2 * PROJ_RTOL, (col, err)
    assert rel_err(frame[0].values, frame[1].values) > 1e-3     # (the points do differ)
