"""The batch over kernels: chomp_kernel_setup_pairs (one projection set-up per window pair,
MultiEpoch range and cosmology), chomp_wtheta_sets behind it, chomp_cell_sets (C_l with a node
table per set) and Correlation.correlation_kernels: bit for bit against the single set-up and
the single call on the same context, against the reference's loop over kernels (G36) and against
the project's own loop of fresh objects."""
import copy
import warnings

import numpy
import pytest

from conftest import load_golden, rel_err
from test_kernels_batch_cpu import KTHETA, fixture_cosmo, fixture_hod, fixture_kernels

pytestmark = pytest.mark.gpu
# the bar tests/test_gpu_projection.py holds the single call to
PROJ_RTOL = 1e-9
TABLES = ("kernel", "levels", "wa", "wb", "wa_chi", "me_chi", "me_growth")
COSMO_KEYS = ("omega_m0", "omega_b0", "omega_l0", "omega_r0", "cmb_temp", "h", "sigma_8",
              "n_scalar", "w0", "wa")


@pytest.fixture(scope="module")
def g36():
    import torch
    assert torch.cuda.is_available()
    return load_golden("g36_kernels")


def _single_setup(ctx, kern):
    """chomp_kernel_setup of one kernel's own inputs."""
    ctx.kernel_setup(kern.cosmo.cosmo_dict, kern.cosmo.z_min, kern.cosmo.z_max, kern._ktheta[0],
                     kern._ktheta[1], kern.window_function_a._struct(),
                     kern.window_function_b._struct(), kern._order)


def _lensing_pair():
    """A flat convergence window against sources on one plane (the two window kinds the fixture
    does not hold), on a MultiEpoch range of its own."""
    from chomp_amd import cosmology, kernel
    me = cosmology.MultiEpoch(0.0, 3.0)
    wa = kernel.WindowFunctionFlatConvergence(0.2, 0.8, me)
    wb = kernel.WindowFunctionConvergenceDelta(1.1, me)
    return kernel.Kernel(KTHETA[0], KTHETA[1], wa, wb, me)


@pytest.mark.parametrize("tag", ["j0", "j2"])
def test_setup_pairs_bit_for_bit(g36, tag):
    from chomp_amd import _lib, cosmology, kernel
    kernels = fixture_kernels(g36, tag)
    if tag == "j0":
        kernels.append(_lensing_pair())
        assert kernels[-1].window_function_a._struct().kind == _lib.WINDOW_FLAT_CONVERGENCE
        assert kernels[-1].window_function_b._struct().kind == _lib.WINDOW_CONVERGENCE_DELTA
    ctx = cosmology._context()
    single = []
    for k in kernels:
        _single_setup(ctx, k)
        single.append((ctx.kernel_info(), {t: ctx.kernel_table(t) for t in TABLES}))
    last = ctx.kernel_info()
    assert kernel.Kernel._setup_pairs_on(ctx, kernels) is ctx
    info = ctx.kernel_info_sets()
    for s, (one, tabs) in enumerate(single):
        for name, value in one.items():
            assert numpy.array_equal(info[name][s], value), (s, name, info[name][s], value)
        for t in TABLES:
            assert numpy.array_equal(ctx.kernel_table_set(s, t), tabs[t]), (s, t)
    # the sets do differ, and the single set-up is as it was
    for s in range(len(kernels)):
        for r in range(s):
            assert not numpy.array_equal(single[s][1]["kernel"], single[r][1]["kernel"]), (s, r)
    after = ctx.kernel_info()
    assert all(numpy.array_equal(after[name], last[name]) for name in last)
    assert numpy.array_equal(ctx.kernel_table("kernel"), single[-1][1]["kernel"])
    with pytest.raises(ValueError):
        ctx.kernel_table_set(len(kernels), "kernel")
    assert all(k._done == {} and k._info is None for k in kernels)


def test_setup_sets_is_what_it_was():
    """chomp_kernel_setup_sets (now the launches it shares with chomp_kernel_setup_pairs, its range
    and windows broadcast) against chomp_kernel_setup per cosmology of G34, after a pairs set-up
    on the same context."""
    from chomp_amd import cosmology, kernel
    g34 = load_golden("g34_wtheta_cosmologies")
    cosmos = [dict(zip(COSMO_KEYS, (float(v) for v in row))) for row in g34["cosmo"]]
    me = cosmology.MultiEpoch(0.0, 5.0)
    wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), me)
    wb = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), me)
    kern = kernel.Kernel(KTHETA[0], KTHETA[1], wa, wb, me)
    ctx = cosmology._context()
    kernel.Kernel._setup_pairs_on(ctx, [_lensing_pair()] * 4)
    kern._setup_sets_on(ctx, cosmos)
    info = ctx.kernel_info_sets()
    assert info["z_bar"].shape == (3,) and numpy.array_equal(info["z_bar"], g34["z_bar"])
    for s, c in enumerate(cosmos):
        ctx.kernel_setup(c, 0.0, 5.0, KTHETA[0], KTHETA[1], wa._struct(), wb._struct(), 0)
        one = ctx.kernel_info()
        for name, value in one.items():
            assert numpy.array_equal(info[name][s], value), (s, name)
        for t in TABLES:
            assert numpy.array_equal(ctx.kernel_table_set(s, t), ctx.kernel_table(t)), (s, t)


class _Rows(object):
    """A HaloGrid of one epoch per kernel at that kernel's z_bar, with its cosmology and HOD, and
    the kernels staged on its context as sets: what chomp_wtheta_sets / chomp_cell_sets and
    chomp_kernel_setup + chomp_wtheta / chomp_cell are compared on."""

    def __init__(self, g, tag, spectrum, rows=None):
        from chomp_amd import correlation, defaults, grid
        n_all = g[tag + "_w"].shape[0]
        self.rows = list(range(n_all)) if rows is None else list(rows)
        self.kernels = [fixture_kernels(g, tag)[i] for i in self.rows]
        self.cosmos = [fixture_cosmo(g, tag, i) for i in self.rows]
        self.hods = [fixture_hod(g, tag, i) for i in self.rows]
        self.hg = grid.HaloGrid(numpy.zeros(len(self.rows)), cosmo_dict=self.cosmos,
                                hod_dict=self.hods)
        self.ctx = self.hg.ctx
        info = self.stage()
        self.z_bar, self.D = info["z_bar"], info["D_zbar"]
        self.hg.set_parameters(z=self.z_bar)
        self.hg.setup(spectrum)
        self.code = correlation._POWER[spectrum][0]
        self.k = (defaults.default_limits["k_min"], defaults.default_limits["k_max"])

    def stage(self, first=0, n=None):
        from chomp_amd import kernel
        n = len(self.kernels) - first if n is None else n
        kernel.Kernel._setup_pairs_on(self.ctx, self.kernels[first:first + n])
        return self.ctx.kernel_info_sets()

    def batch_w(self, theta):
        return self.ctx.wtheta_sets(self.code, 0, len(self.kernels), *self.k, self.D, theta)

    def batch_cl(self, ell):
        return self.ctx.cell_sets(self.code, 0, len(self.kernels), self.D, ell)

    def single(self, x, what):
        rows = []
        for e, kern in enumerate(self.kernels):
            _single_setup(self.ctx, kern)
            assert self.ctx.kernel_info()["D_zbar"] == self.D[e]
            rows.append(self.ctx.wtheta(self.code, e, *self.k, self.D[e], x) if what == "w"
                        else self.ctx.cell(self.code, e, self.D[e], x))
        return numpy.array(rows)


@pytest.fixture(scope="module")
def five(g36):
    """The five J0 rows as epochs and sets, with their single-call w(theta) and C_l."""
    G = _Rows(g36, "j0", "power_gg")
    theta, ell = numpy.ascontiguousarray(g36["theta"]), numpy.ascontiguousarray(g36["ell"])
    w, cl = G.single(theta, "w"), G.single(ell, "cl")
    w.setflags(write=False)
    cl.setflags(write=False)
    return G, theta, ell, w, cl


def test_wtheta_sets_after_a_pairs_setup(five, g36):
    from chomp_amd import _lib
    G, theta, ell, ref, _ = five
    assert ref.shape == (5, 9) and numpy.all(numpy.isfinite(ref))
    assert numpy.array_equal(G.z_bar, g36["j0_z_bar"])
    assert not G.hg.status().any()                               # (the fixture's condition)
    got = G.batch_w(theta)
    assert got.shape == (5, 9) and numpy.array_equal(got, ref)
    try:
        G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, 2)
        seam = G.batch_w(theta)
    finally:
        G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, -1)
    assert numpy.array_equal(seam, ref)


def test_cell_sets_bit_for_bit(five):
    """Default route (four multipoles to a block, the deep launch), seams at rows 2 and 4, one
    multipole, fewer than 16 multipoles (one multipole to a block), device buffers."""
    import torch
    from chomp_amd import _lib
    G, theta, ell, _, ref = five
    assert ref.shape == (5, 22) and numpy.all(numpy.isfinite(ref))
    for i in range(5):
        for j in range(i):
            assert numpy.max(numpy.abs(ref[i] / ref[j] - 1)) > 1e-3   # (the rows do differ)
    got = G.batch_cl(ell)
    assert got.shape == (5, 22) and numpy.array_equal(got, ref)
    try:
        G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, 2)
        seam = G.batch_cl(ell)
    finally:
        G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, -1)
    assert numpy.array_equal(seam, ref)
    # (fewer than 16 multipoles take the per-multipole kernel, whose sums are ordered otherwise:
    #  the single calls are made on the same multipoles)
    one = G.batch_cl(ell[18:19])
    assert one.shape == (5, 1) and numpy.array_equal(one, G.single(ell[18:19], "cl"))
    pick = [0, 5, 9, 13, 17, 18, 19, 20, 21]
    nine = numpy.ascontiguousarray(ell[pick])
    few = G.batch_cl(nine)
    assert few.shape == (5, 9) and numpy.array_equal(few, G.single(nine, "cl"))
    assert rel_err(few, ref[:, pick]) < 1e-9 and rel_err(one[:, 0], ref[:, 18]) < 1e-9
    dev = G.batch_cl(torch.as_tensor(ell, device="cuda"))
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.shape == (5, 22)
    assert numpy.array_equal(dev.cpu().numpy(), ref)
    assert numpy.array_equal(G.batch_cl(ell), ref)               # (and again from host buffers)


def test_cell_sets_single_set(five):
    """n_epoch = 1 with epoch0 = 1: one set (row 1's kernel), epoch 1 of the context."""
    G, theta, ell, _, ref = five
    try:
        info = G.stage(1, 1)
        assert numpy.array_equal(info["D_zbar"], G.D[1:2])
        got = G.ctx.cell_sets(G.code, 1, 1, G.D[1:2], ell)
    finally:
        G.stage()
    assert got.shape == (1, 22) and numpy.array_equal(got, ref[1:2])
    assert numpy.array_equal(G.batch_cl(ell), ref)


def _routes(g36, over, one_kernel, rows, ell):
    """(single calls, batch, batch across a chunk seam) of `rows` of J0 at the multipoles `ell` on a
    context created under default_precision + `over`, with CHOMP_TUNE_CELL_ONE_KERNEL if asked."""
    from chomp_amd import _lib, defaults
    saved = copy.deepcopy(defaults.default_precision)
    try:
        defaults.default_precision.update(over)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")              # (divmax warnings of the shallow set-up)
            G = _Rows(g36, "j0", "power_gg", rows=rows)
            try:
                if one_kernel:
                    G.ctx.set_tuning(_lib.TUNE_CELL_ONE_KERNEL, 1)
                ref = G.single(ell, "cl")
                got = G.batch_cl(ell)
                try:
                    G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, 2)
                    seam = G.batch_cl(ell)
                finally:
                    G.ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, -1)
            finally:
                G.ctx.set_tuning(_lib.TUNE_CELL_ONE_KERNEL, -1)
    finally:
        defaults.default_precision.clear()
        defaults.default_precision.update(saved)
    return ref, got, seam


@pytest.mark.parametrize("over, one_kernel", [
    (dict(divmax=8), False), (dict(divmax=22), False), ({}, True), (dict(divmax=22), True)],
    ids=["divmax8", "divmax22", "one-kernel", "one-kernel-divmax22"])
def test_cell_sets_other_routes(g36, over, one_kernel):
    """All five rows x the 22 multipoles on the other routes.  divmax 8: four multipoles to a block
    with no hand-over and a node table of level 8 (another row stride), no deep launch; divmax 22:
    four multipoles to a block, then the deep kernel compiled with its route beyond the node
    table's level 16; CHOMP_TUNE_CELL_ONE_KERNEL: every level in the per-multipole kernel, at the
    default divmax and at 22, where it is the instance with the node-by-node route.  Each equal to
    the single calls on that context, in one chunk and across the seams at rows 2 and 4."""
    ell = numpy.ascontiguousarray(g36["ell"])
    ref, got, seam = _routes(g36, over, one_kernel, None, ell)
    assert ref.shape == (5, 22) and numpy.all(numpy.isfinite(ref))
    for i in range(5):
        for j in range(i):
            assert numpy.max(numpy.abs(ref[i] / ref[j] - 1)) > 1e-3, (i, j)
    assert numpy.array_equal(got, ref) and numpy.array_equal(seam, ref)


@pytest.mark.parametrize("one_kernel", [False, True], ids=["deep-kernel", "one-kernel"])
def test_cell_sets_beyond_the_node_table(g36, one_kernel):
    """The fixture's integrals stop by level 14, so divmax 22 alone never walks a level beyond the
    node table.  With corr_precision = 1e-15 no integral meets its tolerance and every level up to
    divmax = 18 is walked (the oracle's levels for these rows and multipoles: 15 - 18): levels 17
    and 18 evaluate windows and growth from the staged projection tables of the row's own set, in
    the deep kernel and, with CHOMP_TUNE_CELL_ONE_KERNEL, in the per-multipole kernel.  Rows 0, 1
    and 3 (two window pairs, two cosmologies), five multipoles: single calls on the same five."""
    ell = numpy.ascontiguousarray(g36["ell"][[0, 9, 17, 18, 21]])
    ref, got, seam = _routes(g36, dict(divmax=18, corr_precision=1e-15), one_kernel, (0, 1, 3), ell)
    assert ref.shape == (3, 5) and numpy.all(numpy.isfinite(ref))
    assert numpy.max(numpy.abs(ref[1] / ref[0] - 1)) > 1e-3
    assert numpy.array_equal(got, ref) and numpy.array_equal(seam, ref)


def test_refusals(five, g36):
    """CHOMP_ERR_SCOPE naming the set for a tabulated distribution or a w0-wa cosmology in set 1;
    CHOMP_ERR_ARG for n_epoch that is not the number of sets, a D_z <= 0, lists of other lengths;
    CHOMP_ERR_STATE for chomp_cell_sets before any set-up of sets; the scope of chomp_cell_epochs."""
    from chomp_amd import _lib, cosmology, kernel
    G, theta, ell, _, ref = five
    with pytest.raises(_lib.ChompScopeError, match="cell_sets: HaloFit"):
        G.ctx.cell_sets(G.code | _lib.P_HALOFIT, 0, 5, G.D, ell)
    with pytest.raises(ValueError, match="number of sets"):
        G.ctx.cell_sets(G.code, 0, 2, G.D[:2], ell)
    with pytest.raises(ValueError, match="cell_sets: D_z"):
        G.ctx.cell_sets(G.code, 0, 5, numpy.array([1.0, 1.0, 0.0, 1.0, 1.0]), ell)
    with pytest.raises(ValueError, match="one growth factor per epoch"):
        G.ctx.cell_sets(G.code, 0, 5, G.D[:4], ell)
    try:
        G.ctx.set_precision(_lib.PREC_F32_EVAL)
        with pytest.raises(_lib.ChompScopeError, match="cell_sets: fp64 only"):
            G.batch_cl(ell)
    finally:
        G.ctx.set_precision(_lib.PREC_F64)
    fresh = cosmology._context()
    with pytest.raises(_lib.ChompError, match="cell_sets before"):
        fresh.cell_sets(G.code, 0, 5, G.D, ell)
    kern = G.kernels[0]
    z = numpy.linspace(0.0, 2.0, 33)
    tab = kernel.WindowFunctionGalaxy(kernel.dNdzInterpolation(z, z * z * numpy.exp(-z / 0.3)),
                                      kern.cosmo)
    wa = kern.window_function_a._struct()
    c = kern.cosmo.cosmo_dict
    args = (KTHETA[0], KTHETA[1])
    with pytest.raises(_lib.ChompScopeError, match="kernel_setup_pairs: set 1: a tabulated"):
        fresh.kernel_setup_pairs([c, c], [0.0, 0.0], [5.0, 5.0], *args, [wa, wa],
                                 [wa, tab._struct()], 0)
    with pytest.raises(_lib.ChompScopeError, match="kernel_setup_pairs: set 1: a w0/wa"):
        fresh.kernel_setup_pairs([c, dict(c, w0=-0.9)], [0.0, 0.0], [5.0, 5.0], *args, [wa, wa],
                                 [wa, wa], 0)
    with pytest.raises(ValueError, match="per set"):
        fresh.kernel_setup_pairs([c, c], [0.0], [5.0, 5.0], *args, [wa, wa], [wa, wa], 0)
    with pytest.raises(ValueError, match="sets in one call"):
        n = _lib.KERNEL_SETS_MAX + 1
        fresh.kernel_setup_pairs([c] * n, [0.0] * n, [5.0] * n, *args, [wa] * n, [wa] * n, 0)
    with pytest.raises(_lib.ChompError, match="before kernel_setup_sets"):   # (nothing was staged)
        fresh.kernel_info_sets()
    assert numpy.array_equal(G.batch_cl(ell), ref)


def test_refuses_the_wiggle_transfer_function(g36):
    """A context with the wiggle transfer function is out of scope, as for chomp_cell_epochs (a
    grid of its own: the switch drops the context's tables)."""
    from chomp_amd import _lib
    G = _Rows(g36, "j0", "power_gg", rows=(0, 1))
    ell = numpy.ascontiguousarray(g36["ell"][:3])
    assert G.batch_cl(ell).shape == (2, 3)
    G.ctx.set_transfer(True)
    with pytest.raises(_lib.ChompScopeError, match="cell_sets: the wiggle"):
        G.batch_cl(ell)
    with pytest.raises(_lib.ChompScopeError, match="wtheta_sets: the wiggle"):
        G.batch_w(numpy.ascontiguousarray(g36["theta"][:3]))


# -- Correlation.correlation_kernels -----------------------------------------------------------
def _fresh(g, tag, i, fourier):
    """A fresh Correlation / CorrelationFourier of row i, as correlation_kernels' contract has it."""
    from chomp_amd import correlation, cosmology, halo, hod as hod_mod
    from test_kernels_batch_cpu import fixture_kernel
    kern = fixture_kernel(g, tag, i)
    h = halo.Halo(0.0, hod_mod.HODZheng(fixture_hod(g, tag, i)),
                  cosmology.SingleEpoch(0.0, fixture_cosmo(g, tag, i)))
    ps = "power_gg" if tag == "j0" else "power_gm"
    if fourier:
        return correlation.CorrelationFourier(10, 1e4, kern, input_halo=h, powSpec=ps)
    return correlation.Correlation(0.001, 1.0, kern, input_halo=h, power_spec=ps)


@pytest.fixture(scope="module", params=[("j0", False), ("j0", True), ("j2", False)],
                ids=["J0-w", "J0-cl", "J2-w"])
def batch(request, g36):
    """(tag, fourier, x, the object the batch is called on, its rows, status, fixture rows)."""
    tag, fourier = request.param
    x = numpy.ascontiguousarray(g36["ell"] if fourier else g36["theta"])
    corr = _fresh(g36, tag, 0, fourier)
    n = g36[tag + "_w"].shape[0]
    hods = [fixture_hod(g36, tag, i) for i in range(n)]
    from chomp_amd import _lib
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got, words = corr.correlation_kernels(x, fixture_kernels(g36, tag), hods=hods,
                                              with_status=True)
    flagged = [str(w.message) for w in caught
               if issubclass(w.category, (_lib.ChompAccuracyWarning, _lib.ChompParityWarning))]
    assert not flagged, flagged                          # (a flagged row would warn "kernel i: ...")
    want = g36["j0_cl"] if fourier else g36[tag + "_w"]
    return tag, fourier, x, corr, got, words, want


def test_against_the_reference(batch, g36):
    tag, fourier, x, corr, got, words, want = batch
    assert got.shape == want.shape and words.dtype == numpy.uint32
    assert not words.any() and words is corr.kernels_status
    assert numpy.array_equal(corr.kernels_z_bar, g36[tag + "_z_bar"])
    assert rel_err(corr.kernels_D_z, g36[tag + "_D_z"]) < PROJ_RTOL
    for i in range(got.shape[0]):
        err = rel_err(got[i], want[i])
        print("%s %s row %d against G36: %.2e" % (tag, "C_l" if fourier else "w", i, err))
    for i in range(got.shape[0]):
        assert rel_err(got[i], want[i]) < PROJ_RTOL, (tag, fourier, i)


def test_against_the_loop(batch, g36):
    """Fresh objects, one per kernel, equal the batch rows; this object is not touched."""
    tag, fourier, x, corr, got, words, want = batch
    for i in range(got.shape[0]):
        one = _fresh(g36, tag, i, fourier).correlation(x)
        assert numpy.array_equal(one, got[i]), (tag, fourier, i, rel_err(got[i], one))
    assert numpy.array_equal(corr.correlation(x), got[0])
    assert corr.kernel._done and corr.kernel._z_bar_override is None


def test_hods_none_and_tensors(g36):
    """hods=None: this halo's HOD in every row (row 4 of J0 then differs from the fixture's, which
    has another HOD); a torch cuda input returns a tensor with equal values; one kept grid."""
    import torch
    ell = numpy.ascontiguousarray(g36["ell"][[0, 9, 18, 21]])
    kernels = fixture_kernels(g36, "j0")
    corr = _fresh(g36, "j0", 0, True)
    got = corr.correlation_kernels(ell, kernels)
    assert got.shape == (5, 4)
    kept = corr._kernels_grid[1]
    for i in (1, 4):
        one = _fresh(g36, "j0", i, True)
        one.set_hod(fixture_hod(g36, "j0", 0))
        assert numpy.array_equal(one.correlation(ell), got[i]), i
    assert rel_err(got[4], g36["j0_cl"][4][[0, 9, 18, 21]]) > 1e-3
    dev = corr.correlation_kernels(torch.as_tensor(ell, device="cuda"), kernels)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda
    assert numpy.array_equal(dev.cpu().numpy(), got)
    assert corr._kernels_grid[1] is kept
