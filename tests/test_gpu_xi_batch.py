"""xi(r) with an epoch axis (chomp_xi3d_epochs) and its Python routes
(Correlation3d.raw_correlation_hods / raw_correlation_cosmologies, SimulationDesign over HOD or
cosmology parameters of Correlation3d.raw_correlation): bit for bit against the single-epoch call
on the same context, against the reference's loops (G35) and against the project's own loops.

The fixture's 7 separations stop at early and late Romberg levels with k_max = 10 and at 16 .. 20
(divmax) with the halo's own k_max = 100 (tests/test_xi_batch_cpu.py asserts that of the oracle's
levels)."""
import copy
import ctypes
import warnings

import numpy
import pytest

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
# the bar and scale rule of tests/test_gpu_next.py::test_correlation3d
RTOL = 1e-4
ZHENG_KEYS = ("log_M_min", "sigma", "log_M_0", "log_M_1p", "alpha")
COSMO_KEYS = ("omega_m0", "omega_b0", "omega_l0", "omega_r0", "cmb_temp", "h", "sigma_8",
              "n_scalar", "w0", "wa")
RANGES = {"full": (1e-3, 100.0), "cut": (1e-3, 10.0)}


@pytest.fixture(scope="module")
def g35():
    import torch
    assert torch.cuda.is_available()
    g = load_golden("g35_xi_batch")
    assert numpy.array_equal(g["k_ranges"], [RANGES["full"], RANGES["cut"]])
    return g


def _hods(g, with_default=False):
    """The fixture's HODs in its row order: three Zheng dictionaries, one Mandelbaum object."""
    from chomp_amd import defaults, hod
    out = [dict(zip(ZHENG_KEYS, (float(v) for v in row))) for row in g["zheng"]]
    out.append(hod.HODMandelbaum({"log_M_0": float(g["mandelbaum"][0]), "w": float(g["mandelbaum"][1])}))
    if with_default:
        out.append(dict(defaults.default_hod_dict))
    return out


def _cosmos(g):
    return [dict(zip(COSMO_KEYS, (float(v) for v in row))) for row in g["cosmo"]]


def _range_kw(tag):
    return {} if tag == "full" else dict(k_min=RANGES[tag][0], k_max=RANGES[tag][1])


class _Grid(object):
    """A HaloGrid of one epoch per HOD at z = 0 whose context never sees a projection set-up: what
    chomp_xi3d_epochs and chomp_xi3d are compared on."""

    def __init__(self, hods, spectrum):
        from chomp_amd import correlation, grid
        self.hg = grid.HaloGrid(numpy.zeros(len(hods)), hod_dict=list(hods))
        self.ctx = self.hg.ctx
        self.hg.setup(spectrum)
        self.code = correlation._POWER[spectrum][0]

    def batch(self, r, lim, epoch0=0, n=None):
        n = len(self.hg.idx) - epoch0 if n is None else n
        return self.ctx.xi3d_epochs(self.code, epoch0, n, lim[0], lim[1], r)

    def single(self, r, lim, epoch0=0, n=None):
        n = len(self.hg.idx) - epoch0 if n is None else n
        return numpy.array([self.ctx.xi3d(self.code, e, lim[0], lim[1], r)
                            for e in range(epoch0, epoch0 + n)])


@pytest.fixture(scope="module", params=["power_gg", "power_gm"])
def five(request, g35):
    """Five epochs (the fixture's HODs and the default one) and their single-epoch rows for both
    k ranges."""
    G = _Grid(_hods(g35, with_default=True), request.param)
    r = numpy.ascontiguousarray(g35["r"])
    ref = {tag: G.single(r, lim) for tag, lim in RANGES.items()}
    for rows in ref.values():
        rows.setflags(write=False)
    return G, r, ref


@pytest.mark.parametrize("tag", ["full", "cut"])
def test_same_context_bit_for_bit(five, tag):
    G, r, ref = five
    lim, want = RANGES[tag], ref[tag]
    assert want.shape == (5, 7) and numpy.all(numpy.isfinite(want))
    # (the epochs do differ; the default HOD, epoch 4, is the fixture's first)
    assert numpy.array_equal(want[4], want[0])
    for i in range(4):
        for j in range(i):
            assert numpy.max(numpy.abs(want[i] / want[j] - 1)) > 1e-3, (i, j)
    got = G.batch(r, lim)
    print("batch against the single calls, %s: %.2e" % (tag, rel_err(got, want)))
    assert got.shape == (5, 7) and numpy.array_equal(got, want)
    assert numpy.array_equal(G.batch(r, lim, 2, 2), want[2:4])


def test_chunk_seam(five):
    """Chunks of 2, 2 and 1 epochs reuse one chunk's node tables: the same bits as one chunk of 5,
    and the default chunk afterwards."""
    from chomp_amd import _lib
    G, r, ref = five
    for tag, lim in RANGES.items():
        try:
            G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, 2)
            got = G.batch(r, lim)
        finally:
            G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, -1)
        assert numpy.array_equal(got, ref[tag]), tag
        assert numpy.array_equal(G.batch(r, lim), ref[tag]), tag


def test_single_separation_and_single_epoch(five):
    G, r, ref = five
    lim = RANGES["full"]
    assert numpy.array_equal(G.batch(r, lim, 3, 1), ref["full"][3:4])
    for i in (0, 6):
        one = G.batch(r[i:i + 1], lim)
        assert one.shape == (5, 1) and numpy.array_equal(one, ref["full"][:, i:i + 1])
    assert numpy.array_equal(G.batch(r[4:5], RANGES["cut"], 4, 1), ref["cut"][4:5, 4:5])


def test_table_level_below_the_default(g35):
    """A context with divmax = 12 has a node table of level 12 and integrals that exhaust it: still
    the single call's bits, in one chunk and across a seam."""
    from chomp_amd import _lib, defaults
    saved = copy.deepcopy(defaults.default_precision)
    r = numpy.ascontiguousarray(g35["r"])
    lim = RANGES["full"]
    try:
        defaults.default_precision.update(divmax=12)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                  # (divmax warnings of the shallow set-up)
            G = _Grid(_hods(g35)[:3], "power_gg")
            assert G.ctx.config.divmax == 12
            want = G.single(r, lim)
            got = G.batch(r, lim)
            try:
                G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, 2)
                seam = G.batch(r, lim)
            finally:
                G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, -1)
    finally:
        defaults.default_precision.clear()
        defaults.default_precision.update(saved)
    assert want.shape == (3, 7) and numpy.all(numpy.isfinite(want))
    assert numpy.array_equal(got, want) and numpy.array_equal(seam, want)
    # (level 12 is not where these integrals converge: the default context's values differ)
    full = _Grid(_hods(g35)[:1], "power_gg").single(r, lim)
    assert numpy.max(numpy.abs(full[0] / want[0] - 1)) > 1e-6


def test_needs_no_projection_setup(five):
    """The context never had a kernel set-up: w(theta) refuses it, xi(r) of the batch does not."""
    from chomp_amd import _lib
    G, r, ref = five
    with pytest.raises(_lib.ChompError, match="kernel_setup"):
        G.ctx.wtheta(G.code, 0, 1e-3, 1e2, 1.0, numpy.array([1e-3]))
    assert numpy.array_equal(G.batch(r, RANGES["cut"]), ref["cut"])


def test_device_input(five):
    import torch
    G, r, ref = five
    rd = torch.as_tensor(r, device="cuda")
    got = G.batch(rd, RANGES["full"])
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == (5, 7)
    assert got.dtype == torch.float64
    assert numpy.array_equal(got.cpu().numpy(), ref["full"])
    empty = G.batch(rd[:0], RANGES["full"])
    assert isinstance(empty, torch.Tensor) and empty.shape == (5, 0)
    assert G.batch(r[:0], RANGES["full"]).shape == (5, 0)


def test_refusals(five):
    """CHOMP_ERR_SCOPE: narrowed precision, extrapolated and HaloFit spectra; CHOMP_ERR_ARG: an
    epoch range beyond the context's, a bad k range, an unknown spectrum; CHOMP_ERR_STATE: a
    spectrum whose tables were not built."""
    from chomp_amd import _lib
    G, r, ref = five
    lim = RANGES["cut"]
    for code, word in ((G.code | _lib.P_EXTRAPOLATE, "extrapolated"), (G.code | _lib.P_HALOFIT, "HaloFit")):
        with pytest.raises(_lib.ChompScopeError, match=word + ".*chomp_xi3d"):
            G.ctx.xi3d_epochs(code, 0, 5, lim[0], lim[1], r)
    with pytest.raises(ValueError):
        G.batch(r, lim, 3, 3)
    with pytest.raises(ValueError):
        G.batch(r, (1.0, 0.5))
    with pytest.raises(ValueError):
        G.batch(r, (0.0, 10.0))
    with pytest.raises(ValueError):
        G.ctx.xi3d_epochs(7, 0, 5, lim[0], lim[1], r)
    with pytest.raises(_lib.ChompError, match="not built"):
        G.ctx.xi3d_epochs(_lib.P_MM, 0, 5, lim[0], lim[1], r)
    try:
        G.ctx.set_precision(_lib.PREC_F32_EVAL)
        with pytest.raises(_lib.ChompScopeError, match="fp64 only"):
            G.batch(r, lim)
    finally:
        G.ctx.set_precision(_lib.PREC_F64)
    assert numpy.array_equal(G.batch(r, lim), ref["cut"])


def test_raw_bad_arguments(five):
    """The C entry point itself: null pointers, empty sizes, a product of sizes beyond 2^31, an
    unknown `mem` -- CHOMP_ERR_ARG each, nothing run, the context usable afterwards."""
    import torch
    from chomp_amd import _lib
    G, r, ref = five
    L, h = G.ctx._L, G.ctx._h
    x = torch.as_tensor(r, device="cuda")
    out = torch.zeros(5 * 7, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lo, hi = RANGES["cut"]
    calls = {
        "null r": lambda: L.chomp_xi3d_epochs(h, G.code, 0, 5, lo, hi, None, 7, p(out), _lib.DEVICE),
        "null out": lambda: L.chomp_xi3d_epochs(h, G.code, 0, 5, lo, hi, p(x), 7, None, _lib.DEVICE),
        "n = 0": lambda: L.chomp_xi3d_epochs(h, G.code, 0, 5, lo, hi, p(x), 0, p(out), _lib.DEVICE),
        "n_epoch = 0": lambda: L.chomp_xi3d_epochs(h, G.code, 0, 0, lo, hi, p(x), 7, p(out), _lib.DEVICE),
        "n * n_epoch": lambda: L.chomp_xi3d_epochs(h, G.code, 0, 5, lo, hi, p(x), 1 << 30, p(out),
                                                   _lib.DEVICE),
        "mem": lambda: L.chomp_xi3d_epochs(h, G.code, 0, 5, lo, hi, p(x), 7, p(out), 2),
        "null ctx": lambda: L.chomp_xi3d_epochs(None, G.code, 0, 5, lo, hi, p(x), 7, p(out), _lib.DEVICE),
    }
    for name, call in calls.items():
        assert call() == _lib.ERR_ARG, name
    torch.cuda.synchronize()
    assert torch.count_nonzero(out).item() == 0              # nothing ran
    assert numpy.array_equal(G.batch(r, RANGES["cut"]), ref["cut"])


def test_refuses_the_wiggle_transfer_function(g35):
    """A context with the wiggle transfer function is out of scope (a grid of its own: the switch
    drops the context's tables)."""
    from chomp_amd import _lib
    G = _Grid(_hods(g35)[:2], "power_gg")
    r = numpy.ascontiguousarray(g35["r"][:3])
    assert G.batch(r, RANGES["cut"]).shape == (2, 3)
    G.ctx.set_transfer(True)
    with pytest.raises(_lib.ChompScopeError, match="wiggle"):
        G.batch(r, RANGES["cut"])


def test_refuses_a_divmax_beyond_the_table(g35):
    """divmax = 22: the lean kernel has no route beyond the level-20 table; C and Python refuse."""
    from chomp_amd import _lib, correlation, defaults, halo
    saved = copy.deepcopy(defaults.default_precision)
    r = numpy.ascontiguousarray(g35["r"][:2])
    try:
        defaults.default_precision.update(divmax=22)
        G = _Grid(_hods(g35)[:2], "power_gg")
        with pytest.raises(_lib.ChompScopeError, match="divmax"):
            G.batch(r, RANGES["cut"])
        c3 = correlation.Correlation3d(0.1, 100.0, input_halo=halo.Halo(0.0), powSpec="power_gg")
        with pytest.raises(_lib.ChompScopeError, match="divmax"):
            c3.raw_correlation_hods(r, _hods(g35)[:2])
        with pytest.raises(_lib.ChompScopeError, match="divmax"):
            c3.raw_correlation_cosmologies(r, _cosmos(g35)[:2])
    finally:
        defaults.default_precision.clear()
        defaults.default_precision.update(saved)


def _against(rows, want, label):
    """test_correlation3d's rule: relative where |xi| > 1e-3 of the row's scale, absolute against
    the scale elsewhere (xi changes sign)."""
    assert rows.shape == want.shape
    for i in range(want.shape[0]):
        scale = numpy.max(numpy.abs(want[i]))
        big = numpy.abs(want[i]) > 1e-3 * scale
        err = rel_err(rows[i][big], want[i][big])
        print("G35 %s row %d: %.2e" % (label, i, err))
        assert err < RTOL, (label, i, err)
        assert numpy.max(numpy.abs(rows[i] - want[i])) < RTOL * scale, (label, i)


@pytest.fixture(scope="module")
def corrs(g35):
    """Per (spectrum, range): (Correlation3d, its raw_correlation_hods rows over the fixture's
    HODs)."""
    from chomp_amd import correlation, halo
    r = numpy.ascontiguousarray(g35["r"])
    out = {}
    for ps in ("power_gg", "power_gm"):
        for tag in RANGES:
            c3 = correlation.Correlation3d(0.1, 100.0, redshift=0.0, input_halo=halo.Halo(0.0),
                                           powSpec=ps, **_range_kw(tag))
            assert c3._k_lim == RANGES[tag] and not c3.halo.get_extrapolation()
            own_halo, own = c3.halo, c3.halo.local_hod
            before = (c3.get_hod(), {key: getattr(own, key) for key in ZHENG_KEYS})
            rows = c3.raw_correlation_hods(r, _hods(g35))
            # the object's own halo and HOD are untouched
            assert c3.halo is own_halo and c3.halo.local_hod is own
            assert (c3.get_hod(), {key: getattr(own, key) for key in ZHENG_KEYS}) == before
            rows.setflags(write=False)
            out[ps, tag] = (c3, rows)
    return out


@pytest.mark.parametrize("tag", ["full", "cut"])
@pytest.mark.parametrize("ps", ["power_gg", "power_gm"])
def test_hods_against_the_reference(g35, corrs, ps, tag):
    _against(corrs[ps, tag][1], g35["xi_%s_%s" % (ps, tag)], "%s %s" % (ps, tag))


@pytest.mark.parametrize("ps, tag", [("power_gg", "full"), ("power_gm", "cut")])
def test_hods_against_the_loop(g35, corrs, ps, tag):
    """The loop set_hod / set_hod_object + raw_correlation on a second Correlation3d, bit for bit; a
    second call with the HODs reversed reuses the kept grid."""
    from chomp_amd import correlation, halo
    c3, rows = corrs[ps, tag]
    r = numpy.ascontiguousarray(g35["r"])
    loop = correlation.Correlation3d(0.1, 100.0, redshift=0.0, input_halo=halo.Halo(0.0),
                                     powSpec=ps, **_range_kw(tag))
    hods = _hods(g35)
    for i, h in enumerate(hods):
        if isinstance(h, dict):
            loop.set_hod(h)
        else:
            loop.set_hod_object(h)
        assert numpy.array_equal(rows[i], loop.raw_correlation(r)), (ps, tag, i)
    hg = c3._hods_grid[1]
    again, words = c3.raw_correlation_hods(r, hods[::-1], with_status=True)
    assert c3._hods_grid[1] is hg
    assert numpy.array_equal(again, rows[::-1])
    assert words.shape == (4,) and numpy.array_equal(words, c3.hods_status)
    assert c3.raw_correlation_hods(r[:0], hods).shape == (4, 0)
    assert c3.raw_correlation_hods(r, []).shape == (0, 7)


def test_hods_device_buffers_and_status(g35, corrs):
    import torch
    c3, rows = corrs["power_gg", "full"]
    r = torch.as_tensor(g35["r"], device="cuda")
    got, words = c3.raw_correlation_hods(r, _hods(g35), with_status=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == (4, 7)
    assert numpy.array_equal(got.cpu().numpy(), rows)
    assert words.shape == (4,) and not words.any()


def _fresh(z, cosmo, hod_obj, ps, tag):
    from chomp_amd import correlation, cosmology, halo
    h = halo.Halo(z, hod_obj, cosmology.SingleEpoch(z, dict(cosmo)))
    return correlation.Correlation3d(0.1, 100.0, redshift=z, input_halo=h, powSpec=ps,
                                     **_range_kw(tag))


@pytest.fixture(scope="module")
def cosmo_rows(g35):
    """Per (spectrum, range): (Correlation3d at z = 0.5, its raw_correlation_cosmologies rows over
    the fixture's cosmologies)."""
    from chomp_amd import correlation, halo
    r = numpy.ascontiguousarray(g35["r"])
    z = float(g35["z_cosmo"])
    out = {}
    for ps in ("power_mm", "power_gg"):
        for tag in RANGES:
            c3 = correlation.Correlation3d(0.1, 100.0, redshift=z, input_halo=halo.Halo(z),
                                           powSpec=ps, **_range_kw(tag))
            before = dict(c3.halo.cosmo.cosmo_dict)
            rows, words = c3.raw_correlation_cosmologies(r, _cosmos(g35), with_status=True)
            assert dict(c3.halo.cosmo.cosmo_dict) == before
            assert words.shape == (3,) and numpy.array_equal(words, c3.cosmologies_status)
            rows.setflags(write=False)
            out[ps, tag] = (c3, rows)
    return out


@pytest.mark.parametrize("tag", ["full", "cut"])
@pytest.mark.parametrize("ps", ["power_mm", "power_gg"])
def test_cosmologies_against_the_reference(g35, cosmo_rows, ps, tag):
    _against(cosmo_rows[ps, tag][1], g35["xic_%s_%s" % (ps, tag)], "%s %s" % (ps, tag))


def test_cosmologies_against_fresh_objects(g35, cosmo_rows):
    """Fresh halos and objects per point, one w0-wa cosmology and per-point HODs among them, bit for
    bit; the kept grid serves the second call."""
    from chomp_amd import hod
    ps, tag = "power_gg", "cut"
    c3, rows = cosmo_rows[ps, tag]
    r = numpy.ascontiguousarray(g35["r"])
    z = float(g35["z_cosmo"])
    cosmos = _cosmos(g35)
    for i, c in enumerate(cosmos):
        assert numpy.array_equal(rows[i], _fresh(z, c, None, ps, tag).raw_correlation(r)), i
    hg = c3._cosmologies_grid[1]
    points = [cosmos[1], dict(cosmos[0], w0=-0.9, wa=0.2), cosmos[2]]
    hods = _hods(g35)[1:4]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = c3.raw_correlation_cosmologies(r, points, hods=hods)
        assert c3._cosmologies_grid[1] is hg
        assert got.shape == (3, 7)
        for i in range(3):
            obj = hods[i] if not isinstance(hods[i], dict) else hod.HODZheng(dict(hods[i]))
            assert numpy.array_equal(got[i], _fresh(z, points[i], obj, ps, tag).raw_correlation(r)), i
    assert numpy.max(numpy.abs(got[1] / rows[0] - 1)) > 1e-3     # (w0-wa and the HOD do matter)
    assert c3.raw_correlation_cosmologies(r, []).shape == (0, 7)
    assert c3.raw_correlation_cosmologies(r[:0], cosmos).shape == (3, 0)


def test_cosmologies_device_buffers(g35, cosmo_rows):
    import torch
    c3, rows = cosmo_rows["power_mm", "cut"]
    r = torch.as_tensor(g35["r"], device="cuda")
    got = c3.raw_correlation_cosmologies(r, _cosmos(g35))
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == (3, 7)
    assert numpy.array_equal(got.cpu().numpy(), rows)


def test_inherited_batches_name_the_raw_ones(g35, corrs):
    from chomp_amd import _lib
    c3, _ = corrs["power_gg", "cut"]
    with pytest.raises(_lib.ChompScopeError, match="raw_correlation_hods"):
        c3.correlation_hods(g35["r"], _hods(g35))
    with pytest.raises(_lib.ChompScopeError, match="raw_correlation_cosmologies"):
        c3.correlation_cosmologies(g35["r"], _cosmos(g35))


def test_designs_match_the_loop(g35):
    """run_design(batched=True) over HOD parameters and run_design(batched='cosmology') over
    cosmology + HOD parameters return the frame of the loop."""
    from chomp_amd import correlation, halo, simulation_design
    r = numpy.ascontiguousarray(g35["r"][1::2])
    lim = dict(k_min=1e-3, k_max=10.0)
    c3 = correlation.Correlation3d(0.1, 100.0, redshift=0.0, input_halo=halo.Halo(0.0),
                                   powSpec="power_gg", **lim)
    params = {"log_M_min": [12.14, 11.9, 12.4], "log_M_1p": [13.43, 13.1, 13.8]}
    numpy.random.seed(7)
    des = simulation_design.SimulationDesignHODWakeAssumptions(
        c3, "raw_correlation", params, n_design=4, independent_var=r)
    assert not des._batched()                                # (None keeps the loop)
    frame, status = des.run_design(batched=True, with_status=True)
    assert frame.shape == (r.size, 4) and list(frame.columns) == list(des.points.index)
    assert list(status.index) == list(des.points.index) and not status.any()
    loop = des.run_design(batched=False)
    assert des.design_status is None and loop.shape == (r.size, 4)
    assert numpy.array_equal(frame.values, loop.values)
    assert rel_err(frame[0].values, frame[1].values) > 1e-3  # (the points do differ)

    c3 = correlation.Correlation3d(0.1, 100.0, redshift=0.0, input_halo=halo.Halo(0.0),
                                   powSpec="power_gg", **lim)
    params = {"sigma_8": [0.8, 0.75, 0.85], "log_M_min": [12.14, 11.9, 12.4]}
    numpy.random.seed(11)
    des = simulation_design.SimulationDesign(c3, "raw_correlation", params, n_design=3,
                                             independent_var=r)
    frame, status = des.run_design(batched="cosmology", with_status=True)
    assert frame.shape == (r.size, 3) and not status.any()
    # (Correlation3d has no set_cosmology that works -- the inherited one asks for a kernel, in the
    #  reference too --, so the loop of a cosmology design is a fresh halo and object per point)
    from chomp_amd import defaults, hod
    for col, point in des.points.iterrows():
        cosmo = dict(defaults.default_cosmo_dict, sigma_8=point["sigma_8"])
        one = hod.HODZheng(dict(defaults.default_hod_dict, log_M_min=point["log_M_min"]))
        want = _fresh(0.0, cosmo, one, "power_gg", "cut").raw_correlation(r)
        assert numpy.array_equal(frame[col].values, want), col
    assert rel_err(frame[0].values, frame[1].values) > 1e-3
