"""The super-sample term of every block of a CovarianceMulti in one call:
chomp_covariance_ssc_blocks against the single-block calls on the same context (bit for bit),
CovarianceMulti.get_covariance_batched(ssc_cov=True, cross_terms=True) against the loop
get_covariance() on fresh objects and against the reference's numbers (G30), the seams of the
call and its refusals.

The fixture is that of tests/test_gpu_covariance_blocks.py: three correlations, each on its own
halo.Halo, on one MultiEpoch(0, 5) -- two galaxy auto-correlations and a galaxy x convergence
one; 4 bins, 10 pairs, six blocks, (0, 2) not adjacent to the diagonal.  The epochs carry FAM_SSC.
"""
import numpy
import pytest

from conftest import load_golden, rel_err
from params import hod_dict_2
from test_gpu_covariance_blocks import BLOCKS, setup_single, three_correlations
from test_gpu_covariance_cross import D2R, KWS
from test_gpu_covariance_cross_terms import RTOL_COV, RTOL_KERNEL, correlations as g30_correlations
from test_gpu_covariance_ssc import scaled_err

pytestmark = pytest.mark.gpu
SSC = dict(nongaussian_cov=False, ssc_cov=True, cross_terms=True)
# get_covariance_batched against the loop get_covariance() on fresh objects is bit-equal on the
# MI355X at the three correlations of these tests, and the tests against the loop assert equality.
# The halo set-up of an n-epoch grid is not bit for bit that of another number of epochs, though:
# at 15 correlations / 120 blocks the 150 x 150 matrix differs from the loop's by 1.33e-15 at
# worst (tools/time_cov_multi.py --ssc, profiles/covariance_multi_ssc_timing.json).  Where one
# batch is compared with a batch over another number of correlations (measured here: 6.1e-16)
# the bound is 8 x that measured difference against the loop.
LOOP_MEASURED = 1.33e-15
LOOP_BOUND = 8.0 * LOOP_MEASURED


def multi(corrs, **kws):
    from chomp_amd import covariance
    return covariance.CovarianceMulti(corrs, **dict(KWS, **dict(SSC, **kws)))


def same_across_grids(got, want, what):
    """Two batches over different numbers of correlations: equal, or within LOOP_BOUND."""
    if numpy.array_equal(got, want):
        return
    err = rel_err(got, want)
    print(what, "across grids", err)
    assert err < LOOP_BOUND, (what, err)


class Staged(object):
    """One context with the three kernels as projection sets and the three epochs of a HaloGrid
    at their z_bar, FAM_SSC included, and every block's sigma^2 knots: what
    get_covariance_batched hands chomp_covariance_ssc_blocks."""

    def __init__(self):
        from chomp_amd import correlation, grid
        self.corrs = three_correlations()
        self.kernels = [c.kernel for c in self.corrs]
        first = multi(self.corrs).covariance_list[0][0]
        kc = first.kernel
        self.area = first.area
        self.kt = (kc.ln_ktheta_min, kc.ln_ktheta_max, kc._j0_ssc_limit)
        c = numpy.array([b.center for b in first.annular_bins])
        iu = numpy.triu_indices(c.size)
        self.ta, self.tb = c[iu[0]], c[iu[1]]
        self.hg = grid.HaloGrid(numpy.zeros(3))
        self.ctx = self.hg.ctx
        self.code = correlation._POWER["power_mm"][0]
        self.stage()
        self.first = self.blocks()
        self.tables = [self.ctx.covariance_ssc_blocks_table(b, knots=True) for b in range(6)]
        self.singles = [self.single(b, self.sigma2) for b in range(6)]

    def stage(self):
        from chomp_amd import _lib, covariance, kernel
        kernel.Kernel._setup_pairs_on(self.ctx, self.kernels)
        self.z_bar = self.ctx.kernel_info_sets()["z_bar"]
        self.hg.set_parameters(z=self.z_bar)
        self.hg.setup("power_mm", families=_lib.FAM_SSC)
        self.ranges = self.ctx.covariance_ssc_blocks_range(3)
        self.ln_chi, self.sigma2 = covariance.CovarianceMulti._ssc_blocks_knots(
            [k.cosmo for k in self.kernels], self.ranges)

    def blocks(self, sigma2=None, theta=None, swapped=False, epochs=(0, 1, 2), ln_chi=None):
        sigma2 = self.sigma2 if sigma2 is None else sigma2
        ln_chi = self.ln_chi if ln_chi is None else ln_chi
        if theta is not None:
            return self.ctx.covariance_ssc_blocks(epochs, self.kt[0], self.kt[1], self.kt[2],
                                                  ln_chi, sigma2, self.area, theta)
        ta, tb = (self.tb, self.ta) if swapped else (self.ta, self.tb)
        return self.ctx.covariance_ssc_blocks(epochs, self.kt[0], self.kt[1], self.kt[2], ln_chi,
                                              sigma2, self.area, ta, tb)

    def single(self, b, sigma2):
        """Block b by the single-block calls on this context."""
        i, j = BLOCKS[b]
        ctx = self.ctx
        setup_single(ctx, self.kernels[i])
        out = {}
        if i == j:
            info = ctx.kernel_info()
            out["range"] = [info[k] for k in ("z_min", "z_max", "chi_min", "chi_max")]
            out["info"], out["table"], out["levels"] = ctx.kernel_ssc_setup(
                self.kt[0], self.kt[1], self.kt[2], self.ln_chi[b], sigma2[b])
            out["values"], out["kb"], out["kb_levels"] = ctx.covariance_ssc(
                i, self.area, self.ta, self.tb, knots=True)
            return out
        ctx.covariance_cross_stage(0, ctx, self.code, i)
        setup_single(ctx, self.kernels[j])
        ctx.covariance_cross_stage(1, ctx, self.code, j)
        out["range"] = list(ctx.covariance_cross_range())
        out["info"], out["table"], out["levels"] = ctx.kernel_ssc_setup(
            self.kt[0], self.kt[1], self.kt[2], self.ln_chi[b], sigma2[b], cross=True)
        out["values"], out["kb"], out["kb_levels"] = ctx.covariance_ssc_cross(
            self.area, self.ta, self.tb, knots=True)
        out["swapped"] = ctx.covariance_ssc_cross(self.area, self.tb, self.ta)
        return out


@pytest.fixture(scope="module")
def staged():
    return Staged()


def check_block(b, got_values, table, want):
    """One block of the batch against the single calls: everything, numpy.array_equal."""
    info, tab, lev, kb, kb_lev = table
    ij = BLOCKS[b]
    assert tab.shape == (50, 50) and numpy.array_equal(tab, tab.T), ij
    assert numpy.array_equal(tab, want["table"]), ij
    assert numpy.array_equal(lev, want["levels"]), ij
    assert numpy.array_equal(info[:3], want["info"]), (ij, info[:3], want["info"])
    assert numpy.array_equal(info[3:], want["range"]), (ij, info[3:], want["range"])
    assert kb.shape == want["kb"].shape == (10, 50)
    assert numpy.array_equal(kb, want["kb"]), ij
    assert numpy.array_equal(kb_lev, want["kb_levels"]), ij
    assert numpy.array_equal(got_values, want["values"]), (ij, got_values / want["values"] - 1)


def test_blocks_bit_for_bit_against_the_single_calls(staged):
    S = staged
    got = S.first
    assert got.shape == (6, 10) and numpy.all(numpy.isfinite(got))
    for b in range(6):
        check_block(b, got[b], S.tables[b], S.singles[b])
        # the range call: kernel_info of a diagonal block, covariance_cross_range of a cross one
        assert numpy.array_equal(S.ranges[b], S.singles[b]["range"]), BLOCKS[b]
        assert S.ranges[b, 0] < S.ranges[b, 1] and 0.0 < S.ranges[b, 2] < S.ranges[b, 3]
    # a cross block's range is the common one of its two sides (kernel.py:910-916)
    for b, (i, j) in enumerate(BLOCKS):
        di, dj = S.ranges[BLOCKS.index((i, i))], S.ranges[BLOCKS.index((j, j))]
        assert S.ranges[b, 0] == max(di[0], dj[0]) and S.ranges[b, 1] == min(di[1], dj[1]), (i, j)
    assert not numpy.array_equal(S.ranges[2], S.ranges[0])      # (the third kernel ends sooner)


def test_no_two_blocks_alike(staged):
    """Neither the values nor the tables; and with every block's sigma^2 knots scaled by a
    factor of its own, every block is still the single calls' with ITS knots."""
    S = staged
    for a in range(6):
        for b in range(a):
            assert rel_err(S.first[a], S.first[b]) > 1e-6, (a, b)
            assert scaled_err(S.tables[a][1], S.tables[b][1]) > 1e-6, (a, b)
            assert scaled_err(S.tables[a][3], S.tables[b][3]) > 1e-6, (a, b)
    sigma2 = S.sigma2 * (1.0 + 0.25 * numpy.arange(1.0, 7.0))[:, None]
    got = S.blocks(sigma2=sigma2)
    tables = [S.ctx.covariance_ssc_blocks_table(b, knots=True) for b in range(6)]
    for b in range(6):
        assert rel_err(got[b], S.first[b]) > 0.1, b
        check_block(b, got[b], tables[b], S.single(b, sigma2))
    assert numpy.array_equal(S.blocks(), S.first)


def test_the_order_of_the_angles(staged):
    S = staged
    swapped = S.blocks(swapped=True)
    off = S.ta != S.tb
    assert numpy.count_nonzero(off) == 6
    for b, (i, j) in enumerate(BLOCKS):
        if i == j:
            continue
        assert numpy.array_equal(swapped[b], S.singles[b]["swapped"]), (i, j)
        assert numpy.array_equal(swapped[b][~off], S.first[b][~off]), (i, j)
        assert numpy.all(numpy.abs(swapped[b][off] / S.first[b][off] - 1.0) > 1e-6), (i, j)
    assert numpy.array_equal(S.blocks(), S.first)


@pytest.fixture(scope="module")
def loop_and_batch():
    """(the loop's CovarianceMulti after get_covariance(), the batch's after
    get_covariance_batched()), each on fresh correlations."""
    cl = multi(three_correlations())
    cl.get_covariance()
    cb = multi(three_correlations())
    out, words = cb.get_covariance_batched(with_status=True)
    assert out is cb.wcovar and words is cb.blocks_status
    return cl, cb


def test_batched_against_the_loop(loop_and_batch):
    cl, cb = loop_and_batch
    assert cb.wcovar.shape == (12, 12) and numpy.all(numpy.isfinite(cb.wcovar))
    assert numpy.array_equal(cb.wcovar, cb.wcovar.T)
    assert not numpy.any(cb.blocks_status)
    # bit-equal on the MI355X at these three correlations: equality, and nothing weaker
    print("wcovar: batch against loop", rel_err(cb.wcovar, cl.wcovar))
    assert numpy.array_equal(cb.wcovar, cl.wcovar), rel_err(cb.wcovar, cl.wcovar)
    c = numpy.array([b.center for b in cb.annular_bins])
    iu = numpy.triu_indices(c.size)
    assert cb.blocks_ssc.shape == (6, 10) and numpy.all(numpy.isfinite(cb.blocks_ssc))
    blocks_l = [cov for row in cl.covariance_list for cov in row]
    blocks_b = [cov for row in cb.covariance_list for cov in row]
    for b, (cov_l, cov_b) in enumerate(zip(blocks_l, blocks_b)):
        assert numpy.array_equal(cov_b.covar, cov_l.covar), BLOCKS[b]
        # the super-sample term by itself (some 1e-9 of the Gaussian one for this survey): the
        # loop's covariance_ssc of the block
        want = cov_l._covariance_ssc_pairs(c[iu[0]], c[iu[1]])
        assert numpy.array_equal(cb.blocks_ssc[b], want), (BLOCKS[b], cb.blocks_ssc[b] / want - 1)
        assert numpy.all(cb.blocks_ssc[b] != 0.0)
    # ... and it is in the matrix: the Gaussian batch of the same correlations differs
    gm = multi(three_correlations(), ssc_cov=False, cross_terms=False)
    gauss = gm.get_covariance_batched()
    assert gm.blocks_ssc is None and not numpy.array_equal(cb.wcovar, gauss)
    for b, cov in enumerate(cov for row in gm.covariance_list for cov in row):
        i, j = numpy.triu_indices(4)
        assert numpy.array_equal(blocks_b[b].covar[i, j], cov.covar[i, j] + cb.blocks_ssc[b])
    # ... and neither the blocks' own kernel_ssc state nor their copies were built by the batch
    for row in cb.covariance_list:
        for cov in row:
            assert cov.kernel._ssc_key is None and not cov._initialized_halo_splines


@pytest.mark.parametrize("tag", ["gal", "wide"])
def test_batched_against_the_reference(tag):
    """G30: the cross block of a two-correlation CovarianceMulti -- its kernel_ssc table and its
    covar = covariance_G + covariance_ssc at the pairs i <= j -- at that fixture's bars."""
    g = load_golden("g30_covariance_cross_terms")
    cm = multi(list(g30_correlations(tag)))
    w = cm.get_covariance_batched()
    assert w.shape == (8, 8) and numpy.array_equal(w, w.T)
    _, tab, _ = cm._blocks_grid[1].ctx.covariance_ssc_blocks_table(1)
    err = scaled_err(tab, g[tag + "_kernel_ssc_array"])
    print(tag, "block (0, 1) kernel_ssc table error / scale", err)
    assert err < RTOL_KERNEL
    covar = cm.covariance_list[0][1].covar
    assert numpy.array_equal(covar, w[:4, 4:])
    want = g[tag + "_G"] + g[tag + "_ssc"]
    n = 0
    for p, (i, j) in enumerate(g[tag + "_pairs"]):
        if i <= j:
            e = abs(covar[i, j] / want[p] - 1.0)
            assert e < RTOL_COV, (tag, i, j, e)
            n += 1
    assert n == 10


def test_seams(staged):
    """One correlation alone; the call with a device theta; the single-block kernel_ssc state of
    the context untouched; fewer correlations on the same context."""
    import torch
    S = staged
    ctx = S.ctx
    # one correlation with ssc_cov and no cross_terms: a diagonal block alone
    one = multi(three_correlations()[:1], cross_terms=False)
    assert len(one.covariance_list) == 1 and len(one.covariance_list[0]) == 1
    w = one.get_covariance_batched()
    assert w.shape == (4, 4)
    loop = multi(three_correlations()[:1], cross_terms=False).get_covariance()
    assert numpy.array_equal(w, loop), rel_err(w, loop)
    assert one.blocks_ssc.shape == (1, 10)
    # a device theta
    pairs = torch.tensor(numpy.concatenate([S.ta, S.tb]), dtype=torch.float64, device="cuda")
    dev = S.blocks(theta=pairs)
    assert dev.is_cuda and dev.shape == (6, 10)
    assert numpy.array_equal(dev.cpu().numpy(), S.first)
    # a single-block state, the batch, and the single-block state again
    before = S.single(5, S.sigma2)
    raw = ctx.kernel_ssc_raw(numpy.array([-2.0]), numpy.array([-1.0]))
    assert numpy.array_equal(S.blocks(), S.first)
    assert numpy.array_equal(ctx.kernel_ssc_raw(numpy.array([-2.0]), numpy.array([-1.0])), raw)
    assert numpy.array_equal(ctx.covariance_ssc(2, S.area, S.ta, S.tb), before["values"])
    # the Gaussian batch's state is its own
    poisson = numpy.zeros((6, 4))
    j0 = multi(S.corrs).covariance_list[0][0]._j0_limit
    G = ctx.covariance_blocks(S.code, [0, 1, 2], j0, S.area, poisson, S.ta, S.tb)
    gt = ctx.covariance_blocks_table(2)
    assert numpy.array_equal(S.blocks(), S.first)
    assert numpy.array_equal(ctx.covariance_blocks_table(2)[1], gt[1])
    assert numpy.array_equal(ctx.covariance_blocks(S.code, [0, 1, 2], j0, S.area, poisson, S.ta,
                                                   S.tb), G)
    # fewer correlations: sets 0 and 1 alone give blocks (0, 0), (0, 1), (1, 1) of the three
    from chomp_amd import kernel
    kernel.Kernel._setup_pairs_on(ctx, S.kernels[:2])
    keep = [0, 1, 3]
    assert numpy.array_equal(ctx.covariance_ssc_blocks_range(2), S.ranges[keep])
    two = S.blocks(epochs=(0, 1), sigma2=S.sigma2[keep], ln_chi=S.ln_chi[keep])
    assert two.shape == (3, 10) and numpy.array_equal(two, S.first[keep])
    with pytest.raises(ValueError, match="covariance_ssc_blocks_table: block"):
        ctx.covariance_ssc_blocks_table(3)
    assert numpy.array_equal(ctx.covariance_ssc_blocks_table(1)[1], S.tables[1][1])
    kernel.Kernel._setup_pairs_on(ctx, S.kernels)
    assert numpy.array_equal(S.blocks(), S.first)


def test_batched_follows_the_hod():
    """power_gg (blocks built by hand: CovarianceMulti forwards no power_spec): a second call
    after moving one correlation's HOD changes that correlation's blocks and leaves the others
    bit-equal; a third with fewer correlations on the same object works."""
    from chomp_amd import covariance
    corrs = three_correlations()
    rows = [[covariance.Covariance(corrs[i], corrs[j], power_spec="power_gg", **dict(KWS, **SSC))
             for j in range(i, 3)] for i in range(3)]
    cm = multi(corrs[:1], cross_terms=False)
    cm.covariance_list = rows
    cm.wcovar = numpy.empty((12, 12))
    w0 = cm.get_covariance_batched().copy()
    kept = cm._blocks_grid[1]
    corrs[1].set_hod(hod_dict_2)
    w1 = cm.get_covariance_batched().copy()
    assert cm._blocks_grid[1] is kept
    assert numpy.all(numpy.isfinite(w0)) and numpy.all(numpy.isfinite(w1))
    for i, j in ((0, 0), (0, 2), (2, 2)):
        assert numpy.array_equal(w1[4 * i:4 * i + 4, 4 * j:4 * j + 4],
                                 w0[4 * i:4 * i + 4, 4 * j:4 * j + 4]), (i, j)
    for i, j in ((0, 1), (1, 1), (1, 2)):
        assert rel_err(w1[4 * i:4 * i + 4, 4 * j:4 * j + 4],
                       w0[4 * i:4 * i + 4, 4 * j:4 * j + 4]) > 1e-4, (i, j)
    # fewer correlations on the same object: correlations 0 and 2
    cm.covariance_list = [[rows[0][0], rows[0][2]], [rows[2][0]]]
    cm.wcovar = numpy.empty((8, 8))
    w2 = cm.get_covariance_batched()
    assert numpy.array_equal(cm.blocks_z_bar, [corrs[0].kernel.z_bar, corrs[2].kernel.z_bar])
    same_across_grids(w2[:4, :4], w1[:4, :4], "block (0, 0) of two")
    same_across_grids(w2[:4, 4:], w1[:4, 8:], "block (0, 2) of two")
    same_across_grids(w2[4:, 4:], w1[8:, 8:], "block (2, 2) of two")


def test_refusals(staged):
    from chomp_amd import _lib, covariance, cosmology, grid, kernel
    S = staged
    ctx = S.ctx
    kt, args = S.kt, (S.area, S.ta, S.tb)
    with pytest.raises(ValueError, match="covariance_ssc_blocks: correlation 2: power: epoch range"):
        S.blocks(epochs=(0, 1, 3))
    with pytest.raises(ValueError, match="covariance_ssc_blocks: area must be positive"):
        ctx.covariance_ssc_blocks([0, 1, 2], kt[0], kt[1], kt[2], S.ln_chi, S.sigma2, 0.0, S.ta, S.tb)
    with pytest.raises(ValueError, match="covariance_ssc_blocks: theta must be positive"):
        ctx.covariance_ssc_blocks([0, 1, 2], kt[0], kt[1], kt[2], S.ln_chi, S.sigma2, S.area, S.ta,
                                  -S.tb)
    with pytest.raises(ValueError, match=r"covariance_ssc_blocks: ln\(k theta\) range / J0 limit"):
        ctx.covariance_ssc_blocks([0, 1, 2], kt[1], kt[0], kt[2], S.ln_chi, S.sigma2, *args)
    with pytest.raises(ValueError, match="block 2: ln chi knots must increase"):
        bad = S.ln_chi.copy()
        bad[2] = bad[2][::-1]
        S.blocks(ln_chi=bad)
    with pytest.raises(ValueError, match=r"ln_chi and sigma2 must be \[6, n_sigma\]"):
        S.blocks(sigma2=S.sigma2[:3], ln_chi=S.ln_chi[:3])
    with pytest.raises(_lib.ChompError, match="covariance_ssc_blocks: n_corr is not the number of sets"):
        S.blocks(epochs=(0, 1), sigma2=S.sigma2[:3], ln_chi=S.ln_chi[:3])
    with pytest.raises(_lib.ChompError, match="covariance_ssc_blocks_range: n_corr is not the number"):
        ctx.covariance_ssc_blocks_range(2)
    with pytest.raises(ValueError, match="covariance_ssc_blocks_table: block"):
        ctx.covariance_ssc_blocks_table(6)
    # a refused call leaves the last result readable, its k_b knots included
    assert all(numpy.array_equal(x, y) for x, y in
               zip(ctx.covariance_ssc_blocks_table(1, knots=True), S.tables[1]))
    # a context without sets; epochs without the response's tables; sets of Bessel order 2
    hg = grid.HaloGrid(numpy.zeros(3))
    hg.setup("power_mm")
    with pytest.raises(_lib.ChompError, match="covariance_ssc_blocks before kernel_setup_pairs"):
        hg.ctx.covariance_ssc_blocks([0, 1, 2], kt[0], kt[1], kt[2], S.ln_chi, S.sigma2, *args)
    with pytest.raises(_lib.ChompError, match="covariance_ssc_blocks_range before kernel_setup_pairs"):
        hg.ctx.covariance_ssc_blocks_range(3)
    with pytest.raises(_lib.ChompError, match="covariance_ssc_blocks_table before covariance_ssc_blocks"):
        hg.ctx.covariance_ssc_blocks_table(0)
    kernel.Kernel._setup_pairs_on(hg.ctx, S.kernels)
    with pytest.raises(_lib.ChompError, match="covariance_ssc_blocks: correlation 0: power: knot "
                                              "tables of this spectrum were not built"):
        hg.ctx.covariance_ssc_blocks([0, 1, 2], kt[0], kt[1], kt[2], S.ln_chi, S.sigma2, *args)
    lens = [kernel.GalaxyGalaxyLensingKernel(k._ktheta[0], k._ktheta[1], k.window_function_a,
                                             k.window_function_b, k.cosmo) for k in S.kernels]
    kernel.Kernel._setup_pairs_on(hg.ctx, lens)
    with pytest.raises(_lib.ChompError, match="covariance_ssc_blocks: the sets are of Bessel order 2"):
        hg.ctx.covariance_ssc_blocks([0, 1, 2], kt[0], kt[1], kt[2], S.ln_chi, S.sigma2, *args)
    # windows with no redshift in common: the library names the block, and launches nothing
    cm = cosmology.MultiEpoch(0.0, 5.0)
    lo = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 0.5, 0.3, 0.1), cm)
    hi = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.5, 1.5, 1.0, 0.2), cm)
    mid = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 1.5, 0.7, 0.2), cm)
    apart = [kernel.Kernel(1e-6 * D2R, 100.0 * D2R, w, w, cm) for w in (mid, lo, hi)]
    kernel.Kernel._setup_pairs_on(hg.ctx, apart)
    match = r"block \(1, 2\): the four windows have no redshift in common"
    with pytest.raises(_lib.ChompScopeError, match="covariance_ssc_blocks_range: " + match):
        hg.ctx.covariance_ssc_blocks_range(3)
    with pytest.raises(_lib.ChompScopeError, match="covariance_ssc_blocks: " + match):
        hg.ctx.covariance_ssc_blocks([0, 1, 2], kt[0], kt[1], kt[2], S.ln_chi, S.sigma2, *args)
    # Python: the trispectrum term with its words, blocks that differ in ssc_cov
    from chomp_amd import halo_trispectrum
    tri = halo_trispectrum.HaloTrispectrumOneHalo(0.5)
    with pytest.raises(_lib.ChompScopeError, match=r"not the trispectrum \(nongaussian_cov\) or "
                                                   r"super-sample \(ssc_cov\) terms; use get_covariance"):
        multi(S.corrs, nongaussian_cov=True, input_halo_trispectrum=tri).get_covariance_batched()
    mixed = multi(S.corrs)
    mixed.covariance_list[1][1].ssc_cov = False
    with pytest.raises(_lib.ChompScopeError, match="the blocks differ in ssc_cov"):
        mixed.get_covariance_batched()
    assert not hasattr(mixed, "_blocks_grid")
    # ... and the staged context is as it was
    assert numpy.array_equal(S.blocks(), S.first)
