"""Every Gaussian block of a CovarianceMulti in one call: chomp_covariance_blocks against the
single-block calls on the same context (bit for bit), CovarianceMulti.get_covariance_batched
against the loop get_covariance() on fresh objects (bit for bit) and against the reference's
numbers (G29), the seams of the call and its refusals.

The fixture: three correlations, each on its own halo.Halo, on one MultiEpoch(0, 5) with the
bins of tests/test_gpu_covariance_cross.py (4 bins, 10 pairs) -- two galaxy auto-correlations
and a galaxy x convergence one.  Six blocks, three diagonal and three cross; (0, 2) is not
adjacent to the diagonal, so a slip in the block -> (i, j) map shows; two window kinds; the
redshift ranges overlap, so every cross block integrates over a non-empty chi range.
"""
import numpy
import pytest

from conftest import load_golden, rel_err
from params import hod_dict_2
from test_gpu_covariance_cross import D2R, KWS, RTOL, correlations

pytestmark = pytest.mark.gpu
BLOCKS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def three_correlations():
    from chomp_amd import correlation, cosmology, halo, kernel
    cm = cosmology.MultiEpoch(0.0, 5.0)

    def corr(wa, wb):
        kern = kernel.Kernel(1e-6 * D2R, 100.0 * D2R, wa, wb, cm)
        return correlation.Correlation(0.01, 1.0, kern, input_halo=halo.Halo(0.0),
                                       power_spec="power_mm")
    w1 = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 2.0, 0.8, 0.2))
    w2 = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2))
    wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0))
    wb = kernel.WindowFunctionConvergence(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2))
    return [corr(w1, w1), corr(w2, w2), corr(wa, wb)]


def multi(corrs):
    from chomp_amd import covariance
    return covariance.CovarianceMulti(corrs, nongaussian_cov=False, **KWS)


def setup_single(ctx, k):
    ctx.kernel_setup(k.cosmo.cosmo_dict, k.cosmo.z_min, k.cosmo.z_max, k._ktheta[0], k._ktheta[1],
                     k.window_function_a._struct(), k.window_function_b._struct(), k._order)


class Staged(object):
    """One context with the three kernels as projection sets and the three epochs of a HaloGrid
    at their z_bar: what get_covariance_batched hands chomp_covariance_blocks."""

    def __init__(self):
        from chomp_amd import correlation, grid
        self.corrs = three_correlations()
        self.kernels = [c.kernel for c in self.corrs]
        cm = multi(self.corrs)
        self.covs = [cov for row in cm.covariance_list for cov in row]
        first = self.covs[0]
        self.j0, self.area = first._j0_limit, first.area
        c = numpy.array([b.center for b in first.annular_bins])
        iu = numpy.triu_indices(c.size)
        self.ta, self.tb = c[iu[0]], c[iu[1]]
        # (the Poisson terms of the integrand are zero for these windows: give every block its
        #  own non-zero four, so that a block reading another's shows)
        self.poisson = 1e-9 * (1.0 + numpy.arange(24.0).reshape(6, 4))
        self.hg = grid.HaloGrid(numpy.zeros(3))
        self.ctx = self.hg.ctx
        self.code = correlation._POWER["power_mm"][0]
        self.stage()

    def stage(self):
        from chomp_amd import kernel
        kernel.Kernel._setup_pairs_on(self.ctx, self.kernels)
        info = self.ctx.kernel_info_sets()
        self.z_bar, self.D = info["z_bar"], info["D_zbar"]
        self.hg.set_parameters(z=self.z_bar)
        self.hg.setup("power_mm")

    def blocks(self, theta=None):
        if theta is not None:
            return self.ctx.covariance_blocks(self.code, [0, 1, 2], self.j0, self.area,
                                              self.poisson, theta)
        return self.ctx.covariance_blocks(self.code, [0, 1, 2], self.j0, self.area, self.poisson,
                                          self.ta, self.tb)

    def D_b(self, i, j):
        return float(self.kernels[i].cosmo.growth_factor(self.z_bar[j]))

    def single(self, b):
        """Block b by the single-block calls on this context: (ln_K, tables, levels, values)."""
        i, j = BLOCKS[b]
        ctx, p = self.ctx, self.poisson[b]
        setup_single(ctx, self.kernels[i])
        if i == j:
            ln_K, proj, lev = ctx.covariance_table(self.code, i, self.D[i])
            return ln_K, proj[None], lev[None], ctx.covariance_gaussian(
                self.j0, self.area, p[0], p[2], self.ta, self.tb)
        ctx.covariance_cross_stage(0, ctx, self.code, i)
        setup_single(ctx, self.kernels[j])
        ctx.covariance_cross_stage(1, ctx, self.code, j)
        ln_K, tab, lev = ctx.covariance_table_cross(self.D[i], self.D_b(i, j))
        return ln_K, tab, lev, ctx.covariance_gaussian_cross(self.j0, self.area, p, self.ta,
                                                             self.tb)


@pytest.fixture(scope="module")
def staged():
    return Staged()


def test_blocks_bit_for_bit_against_the_single_calls(staged):
    S = staged
    got = S.blocks()
    assert got.shape == (6, 10) and numpy.all(numpy.isfinite(got))
    tables = [S.ctx.covariance_blocks_table(b) for b in range(6)]
    for b, (i, j) in enumerate(BLOCKS):
        ln_K, tab, lev, sc = tables[b]
        w_ln_K, w_tab, w_lev, w_vals = S.single(b)
        rows = w_tab.shape[0]
        assert rows == (1 if i == j else 4)
        assert numpy.array_equal(ln_K, w_ln_K), (i, j)
        assert numpy.array_equal(tab[:rows], w_tab), (i, j)
        assert numpy.array_equal(lev[:rows], w_lev), (i, j)
        assert not numpy.any(tab[rows:]) and not numpy.any(lev[rows:])
        assert numpy.array_equal(got[b], w_vals), (i, j, got[b] / w_vals - 1)
        # the scalars: the growth factors k_cov_blocks_prep found, as the knots kernel used them
        D_a, D_b = S.D[i], (S.D[i] if i == j else S.D_b(i, j))
        me = S.kernels[i].cosmo
        print("block", (i, j), "D_a", sc[6], "D_b", sc[7], "host", D_a, D_b)
        assert sc[0] == ln_K[0] and sc[1] == ln_K[-1]
        assert numpy.array_equal(sc[6:8], [D_a, D_b]), (i, j)
        if i == j:
            assert numpy.array_equal(sc[2:6], [D_a, float(me.comoving_distance(D_a)), 0.0, 0.0])
        else:
            assert numpy.array_equal(sc[2:6], [D_a, D_b, float(me.comoving_distance(D_a)),
                                               float(me.comoving_distance(D_b))])
    # no two blocks alike (a block served from another's slab or Poisson terms would be)
    for a in range(6):
        for b in range(a):
            assert rel_err(got[a], got[b]) > 1e-6, (a, b)


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


def test_batched_equals_the_loop(loop_and_batch):
    cl, cb = loop_and_batch
    assert cb.wcovar.shape == (12, 12)
    assert numpy.array_equal(cb.wcovar, cb.wcovar.T)
    assert numpy.array_equal(cb.wcovar, cl.wcovar), rel_err(cb.wcovar, cl.wcovar)
    for row_l, row_b in zip(cl.covariance_list, cb.covariance_list):
        for cov_l, cov_b in zip(row_l, row_b):
            assert numpy.array_equal(cov_b.covar, cov_l.covar)
    # the Poisson diagonal is there (it is what the diagonal of a matching block is made of)
    first = cb.covariance_list[0][0]
    assert first.covariance_P(first.annular_bins[0].delta, first.annular_bins[0].center) > 0.0
    assert cb.blocks_status.dtype == numpy.uint32 and cb.blocks_status.shape == (3,)
    assert numpy.array_equal(cb.blocks_z_bar, [c.kernel.z_bar for c in
                                               (row[0].corr_a for row in cl.covariance_list)])


def test_batched_against_the_reference():
    """The two-correlation "gal" case of test_g29_covariance_multi, at its tolerance."""
    from chomp_amd import covariance
    g = load_golden("g29_covariance_cross")
    cm = covariance.CovarianceMulti(list(correlations("gal")), nongaussian_cov=False, **KWS)
    w = cm.get_covariance_batched()
    assert w.shape == (8, 8) and numpy.array_equal(w, w.T)
    print("batched wcovar error", rel_err(w, g["multi_wcovar"]))
    assert rel_err(w, g["multi_wcovar"]) < RTOL


def test_seams(staged, loop_and_batch):
    """The batch twice, after set_hod on one halo, with a device theta; the single-block
    covariance state of the context untouched by the call."""
    import torch
    S = staged
    first = S.blocks()
    assert numpy.array_equal(S.blocks(), first)
    pairs = torch.tensor(numpy.concatenate([S.ta, S.tb]), dtype=torch.float64, device="cuda")
    dev = S.blocks(theta=pairs)
    assert dev.is_cuda and dev.shape == (6, 10)
    assert numpy.array_equal(dev.cpu().numpy(), first)

    # a single-block state, the batch, and the single-block state again
    ctx = S.ctx
    setup_single(ctx, S.kernels[2])
    ln_K, proj, _ = ctx.covariance_table(S.code, 2, S.D[2])
    before = ctx.covariance_gaussian(S.j0, S.area, 0.0, 0.0, S.ta, S.tb)
    info = ctx.kernel_info()
    assert numpy.array_equal(S.blocks(), first)
    assert numpy.array_equal(ctx.covariance_gaussian(S.j0, S.area, 0.0, 0.0, S.ta, S.tb), before)
    assert ctx.kernel_info() == info
    again = ctx.covariance_table(S.code, 2, S.D[2])
    assert numpy.array_equal(again[0], ln_K) and numpy.array_equal(again[1], proj)
    assert numpy.array_equal(ctx.covariance_gaussian(S.j0, S.area, 0.0, 0.0, S.ta, S.tb), before)

    # Python: twice, then after set_hod on one halo -- against a fresh loop with that HOD
    _, cb = loop_and_batch
    w0 = cb.wcovar.copy()
    kept = cb._blocks_grid[1]
    assert numpy.array_equal(cb.get_covariance_batched(), w0)
    assert cb._blocks_grid[1] is kept
    cb.covariance_list[1][0].corr_a.set_hod(hod_dict_2)
    w1 = cb.get_covariance_batched().copy()
    assert cb._blocks_grid[1] is kept
    fresh = three_correlations()
    fresh[1].set_hod(hod_dict_2)
    assert numpy.array_equal(w1, multi(fresh).get_covariance())
    # power_mm does not read the HOD; power_gg does
    assert numpy.array_equal(w1, w0)


def test_batched_follows_the_hod():
    """power_gg: moving one correlation's HOD moves its row of blocks, and the kept grid
    follows."""
    from chomp_amd import covariance
    kws = dict(KWS, nongaussian_cov=False)

    def build(hod=None):
        corrs = three_correlations()
        if hod is not None:
            corrs[1].set_hod(hod)
        rows = []
        for i in range(3):
            rows.append([covariance.Covariance(corrs[i], corrs[j], power_spec="power_gg", **kws)
                         for j in range(i, 3)])
        cm = covariance.CovarianceMulti(corrs[:1], **kws)
        cm.covariance_list = rows
        cm.wcovar = numpy.empty((12, 12))
        return cm, corrs
    cm, corrs = build()
    w0 = cm.get_covariance_batched().copy()
    corrs[1].set_hod(hod_dict_2)
    w1 = cm.get_covariance_batched().copy()
    assert numpy.array_equal(w1[:4, :4], w0[:4, :4]) and numpy.array_equal(w1[8:, 8:], w0[8:, 8:])
    assert rel_err(w1[4:8, 4:8], w0[4:8, 4:8]) > 1e-3
    assert rel_err(w1[:4, 4:8], w0[:4, 4:8]) > 1e-4
    want = build(hod_dict_2)[0].get_covariance()
    assert numpy.array_equal(w1, want), rel_err(w1, want)


def test_refusals(staged):
    from chomp_amd import _lib, grid, kernel
    S = staged
    args = (S.j0, S.area, S.poisson, S.ta, S.tb)
    with pytest.raises(ValueError, match="power: epoch range"):
        S.ctx.covariance_blocks(S.code, [0, 1, 3], *args)
    with pytest.raises(ValueError, match="covariance_blocks: j0_limit and area must be positive"):
        S.ctx.covariance_blocks(S.code, [0, 1, 2], S.j0, 0.0, S.poisson, S.ta, S.tb)
    with pytest.raises(ValueError, match="covariance_blocks: j0_limit and area must be positive"):
        S.ctx.covariance_blocks(S.code, [0, 1, 2], S.j0, -1.0, S.poisson, S.ta, S.tb)
    with pytest.raises(ValueError, match="covariance_blocks: theta must be positive"):
        S.ctx.covariance_blocks(S.code, [0, 1, 2], S.j0, S.area, S.poisson, S.ta, -S.tb)
    with pytest.raises(_lib.ChompError, match="covariance_blocks: n_corr is not the number of sets"):
        S.ctx.covariance_blocks(S.code, [0, 1], S.j0, S.area, S.poisson[:3], S.ta, S.tb)
    with pytest.raises(ValueError, match=r"poisson must be \[6, 4\]"):
        S.ctx.covariance_blocks(S.code, [0, 1, 2], S.j0, S.area, S.poisson[:3], S.ta, S.tb)
    with pytest.raises(ValueError, match="covariance_blocks_table: block"):
        S.ctx.covariance_blocks_table(6)
    # a context without sets, and one whose sets are of Bessel order 2
    hg = grid.HaloGrid(numpy.zeros(3))
    hg.setup("power_mm")
    with pytest.raises(_lib.ChompError, match="covariance_blocks before kernel_setup_pairs"):
        hg.ctx.covariance_blocks(S.code, [0, 1, 2], *args)
    with pytest.raises(_lib.ChompError, match="covariance_blocks_table before covariance_blocks"):
        hg.ctx.covariance_blocks_table(0)
    lens = [kernel.GalaxyGalaxyLensingKernel(k._ktheta[0], k._ktheta[1], k.window_function_a,
                                             k.window_function_b, k.cosmo) for k in S.kernels]
    kernel.Kernel._setup_pairs_on(hg.ctx, lens)
    with pytest.raises(_lib.ChompError, match="covariance_blocks: the sets are of Bessel order 2"):
        hg.ctx.covariance_blocks(S.code, [0, 1, 2], *args)
    # ... and the staged context is as it was
    assert numpy.array_equal(S.blocks(), S.blocks())
