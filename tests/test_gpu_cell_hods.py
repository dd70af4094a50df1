"""C_l with an epoch axis (chomp_cell_epochs) and its Python routes
(CorrelationFourier.correlation_hods, SimulationDesign over HOD parameters of
CorrelationFourier.correlation): bit for bit against the single-epoch call on the same context,
against the reference's loop over HODs (G33) and against the project's own loop.

The fixture's 22 multipoles stop at Romberg levels of every route of the C_l kernels -- a
wavefront's own levels, the block's cooperative walk, the deep kernel -- and the epochs list
different multipoles for the deep kernel (tests/test_cell_hods_cpu.py asserts that of the
oracle's levels)."""
import copy
import warnings

import numpy
import pytest

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
# the bar tests/test_gpu_projection.py holds the single call to
PROJ_RTOL = 1e-9
D2R = numpy.pi / 180.0
ZHENG_KEYS = ("log_M_min", "sigma", "log_M_0", "log_M_1p", "alpha")


@pytest.fixture(scope="module")
def g33():
    import torch
    assert torch.cuda.is_available()
    return load_golden("g33_cell_hods")


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
    what chomp_cell_epochs and chomp_cell are compared on."""

    def __init__(self, hods, spectrum):
        from chomp_amd import correlation, grid
        self.kern = _kernel()
        self.hg = grid.HaloGrid(numpy.full(len(hods), self.kern.z_bar), hod_dict=list(hods))
        self.ctx = self.kern._setup_on(self.hg.ctx)
        self.hg.setup(spectrum)
        self.code = correlation._POWER[spectrum][0]
        self.D_z = self.kern._get("D_zbar")

    def batch(self, ell, epoch0=0, n=None):
        n = len(self.hg.idx) - epoch0 if n is None else n
        return self.ctx.cell_epochs(self.code, epoch0, n, self.D_z, ell)

    def single(self, ell, epoch0=0, n=None):
        n = len(self.hg.idx) - epoch0 if n is None else n
        return numpy.array([self.ctx.cell(self.code, e, self.D_z, ell)
                            for e in range(epoch0, epoch0 + n)])


@pytest.fixture(scope="module", params=["power_gg", "power_gm"])
def five(request, g33):
    """Five epochs (the fixture's HODs and the default one) and their single-epoch rows."""
    G = _Grid(_hods(g33, with_default=True), request.param)
    ell = numpy.ascontiguousarray(g33["ell"])
    ref = G.single(ell)
    ref.setflags(write=False)
    return G, ell, ref


def test_same_context_bit_for_bit(five):
    G, ell, ref = five
    assert ref.shape == (5, 22) and numpy.all(numpy.isfinite(ref))
    assert numpy.max(numpy.abs(ref[1] / ref[0] - 1)) > 1e-3      # (the epochs do differ)
    got = G.batch(ell)
    assert got.shape == (5, 22) and numpy.array_equal(got, ref)
    assert numpy.array_equal(G.batch(ell, 2, 2), ref[2:4])


def test_chunk_seam(five):
    """Chunks of 2, 2 and 1 epochs reuse one chunk's slabs and lists: the same bits as one chunk
    of 5."""
    from chomp_amd import _lib
    G, ell, ref = five
    try:
        G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, 2)
        got = G.batch(ell)
    finally:
        G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, -1)
    assert numpy.array_equal(got, ref)
    assert numpy.array_equal(G.batch(ell), ref)


def test_single_multipole_and_single_epoch(five):
    G, ell, ref = five
    assert numpy.array_equal(G.batch(ell, 3, 1), ref[3:4])
    # (one multipole is the per-multipole kernel: its own launch of the single call to compare)
    for i in (4, 18):                                 # (l = 10000: a deep one for some epochs)
        one = G.batch(ell[i:i + 1])
        assert one.shape == (5, 1) and numpy.array_equal(one, G.single(ell[i:i + 1]))
    assert numpy.array_equal(G.batch(ell[18:19], 4, 1), G.single(ell[18:19], 4, 1))


def test_fewer_than_sixteen_multipoles(five):
    """n < 16: one multipole per block (k_cell) and its hand-over to the deep kernel."""
    from chomp_amd import _lib
    G, ell, ref = five
    sub = numpy.ascontiguousarray(ell[4:19])
    assert sub.size == 15 and sub[-1] == 10000.0
    want = G.single(sub)
    assert numpy.array_equal(G.batch(sub), want)
    try:
        G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, 2)
        assert numpy.array_equal(G.batch(sub), want)
    finally:
        G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, -1)


@pytest.mark.parametrize("over, one_kernel", [(dict(divmax=8), False), (dict(divmax=22), False),
                                              ({}, True), (dict(divmax=22), True)])
def test_other_routes(g33, over, one_kernel):
    """No deep launch (divmax 8); a divmax beyond the node table's level 16 (22: the deep kernel
    compiled with its node-by-node route); every level in the per-multipole kernel
    (CHOMP_TUNE_CELL_ONE_KERNEL), at the default divmax and at 22, where that kernel is the
    instance with the node-by-node route.  Each equal to the per-epoch calls on that context, in
    one chunk and across chunk seams."""
    from chomp_amd import _lib, defaults
    saved = copy.deepcopy(defaults.default_precision)
    ell = numpy.ascontiguousarray(g33["ell"][[0, 9, 17, 20, 18]])
    assert ell[3] == 9000.0 and ell[4] == 10000.0
    try:
        defaults.default_precision.update(over)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")              # (divmax warnings of the shallow set-up)
            G = _Grid(_hods(g33)[:3], "power_gg")
            try:
                if one_kernel:
                    G.ctx.set_tuning(_lib.TUNE_CELL_ONE_KERNEL, 1)
                ref = G.single(ell)
                got = G.batch(ell)
                try:
                    G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, 2)
                    seam = G.batch(ell)
                finally:
                    G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, -1)
            finally:
                G.ctx.set_tuning(_lib.TUNE_CELL_ONE_KERNEL, -1)
    finally:
        defaults.default_precision.clear()
        defaults.default_precision.update(saved)
    assert ref.shape == (3, 5) and numpy.all(numpy.isfinite(ref))
    assert numpy.array_equal(got, ref) and numpy.array_equal(seam, ref)


def test_refusals(five):
    """CHOMP_ERR_SCOPE: narrowed precision, extrapolated and HaloFit spectra; CHOMP_ERR_ARG: an
    epoch range beyond the context's."""
    from chomp_amd import _lib
    G, ell, ref = five
    for code in (G.code | _lib.P_EXTRAPOLATE, G.code | _lib.P_HALOFIT):
        with pytest.raises(_lib.ChompScopeError):
            G.ctx.cell_epochs(code, 0, 5, G.D_z, ell)
    with pytest.raises(ValueError):
        G.batch(ell, 3, 3)
    try:
        G.ctx.set_precision(_lib.PREC_F32_EVAL)
        with pytest.raises(_lib.ChompScopeError):
            G.batch(ell)
    finally:
        G.ctx.set_precision(_lib.PREC_F64)
    assert numpy.array_equal(G.batch(ell), ref)


def test_refuses_the_wiggle_transfer_function(g33):
    """A context with the wiggle transfer function is out of scope in C as in correlation_hods (a
    grid of its own: the switch drops the context's tables)."""
    from chomp_amd import _lib
    G = _Grid(_hods(g33)[:2], "power_gg")
    ell = numpy.ascontiguousarray(g33["ell"][:3])
    assert G.batch(ell).shape == (2, 3)
    G.ctx.set_transfer(True)
    with pytest.raises(_lib.ChompScopeError, match="wiggle"):
        G.batch(ell)


@pytest.fixture(scope="module")
def corrs(g33):
    """Per spectrum: (CorrelationFourier, its correlation_hods rows over the fixture's HODs)."""
    from chomp_amd import correlation, halo
    kern = _kernel()
    ell = numpy.ascontiguousarray(g33["ell"])
    out = {}
    for ps in ("power_gg", "power_gm"):
        cf = correlation.CorrelationFourier(10, 1e4, kern, input_halo=halo.Halo(0.0), powSpec=ps)
        own_halo, own = cf.halo, cf.halo.local_hod
        before = (cf.get_hod(), {key: getattr(own, key) for key in ZHENG_KEYS})
        rows = cf.correlation_hods(ell, _hods(g33))
        # the object's own halo and HOD are untouched
        assert cf.halo is own_halo and cf.halo.local_hod is own
        assert (cf.get_hod(), {key: getattr(own, key) for key in ZHENG_KEYS}) == before
        rows.setflags(write=False)
        out[ps] = (cf, rows)
    return out


@pytest.mark.parametrize("ps", ["power_gg", "power_gm"])
def test_against_the_reference(g33, corrs, ps):
    cf, rows = corrs[ps]
    assert rows.shape == (4, 22)
    for i in range(4):
        err = rel_err(rows[i], g33["cl_" + ps][i])
        print("G33 %s HOD %d: %.2e" % (ps, i, err))
        assert err < PROJ_RTOL, (ps, i, err)


@pytest.mark.parametrize("ps", ["power_gg", "power_gm"])
def test_against_the_loop(g33, corrs, ps):
    """The loop set_hod / set_hod_object + correlation on a second CorrelationFourier; a second
    call with the HODs reversed reuses the grid."""
    from chomp_amd import correlation, halo
    cf, rows = corrs[ps]
    ell = numpy.ascontiguousarray(g33["ell"])
    loop = correlation.CorrelationFourier(10, 1e4, _kernel(), input_halo=halo.Halo(0.0), powSpec=ps)
    hods = _hods(g33)
    for i, h in enumerate(hods):
        if isinstance(h, dict):
            loop.set_hod(h)
        else:
            loop.set_hod_object(h)
        err = rel_err(rows[i], loop.correlation(ell))
        print("loop %s HOD %d: %.2e" % (ps, i, err))
        assert err < 2 * PROJ_RTOL, (ps, i, err)
    hg = cf._hods_grid[1]
    again = cf.correlation_hods(ell, hods[::-1])
    assert cf._hods_grid[1] is hg
    assert numpy.array_equal(again, rows[::-1])
    assert cf.correlation_hods(ell[:0], hods).shape == (4, 0)
    assert cf.correlation_hods(ell, []).shape == (0, 22)


def test_device_buffers_and_status(g33, corrs):
    import torch
    cf, rows = corrs["power_gg"]
    ell = torch.as_tensor(g33["ell"], device="cuda")
    got, words = cf.correlation_hods(ell, _hods(g33), with_status=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == (4, 22)
    assert numpy.array_equal(got.cpu().numpy(), rows)
    assert words.shape == (4,) and not words.any()
    assert numpy.array_equal(words, cf.hods_status)


def test_design_matches_the_loop(g33):
    from chomp_amd import correlation, halo, simulation_design
    ell = numpy.ascontiguousarray(g33["ell"][::4])
    params = {"log_M_min": [12.14, 11.9, 12.4], "log_M_1p": [13.43, 13.1, 13.8]}
    cf = correlation.CorrelationFourier(10, 1e4, _kernel(), input_halo=halo.Halo(0.0),
                                        powSpec="power_gg")
    numpy.random.seed(7)
    des = simulation_design.SimulationDesignHODWakeAssumptions(
        cf, "correlation", params, n_design=6, independent_var=ell)
    assert des._batched()
    frame, status = des.run_design(with_status=True)
    assert frame.shape == (ell.size, 6) and list(frame.columns) == list(des.points.index)
    assert list(status.index) == list(des.points.index) and not status.any()
    loop = des.run_design(batched=False)
    assert des.design_status is None and loop.shape == (ell.size, 6)
    for col in frame.columns:
        err = rel_err(frame[col].values, loop[col].values)
        print("design point %s: %.2e" % (col, err))
        assert err < 2 * PROJ_RTOL, (col, err)
    assert rel_err(frame[0].values, frame[1].values) > 1e-3     # (the points do differ)
