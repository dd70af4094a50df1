"""The one-halo trispectrum term of every block of a CovarianceMulti in one call:
Context.covariance_ng_blocks (chomp_covariance_ng_blocks) against the single-block calls on the same
context (bit for bit), CovarianceMulti.get_covariance_batched(trispectrum=True) against the loop
get_covariance() on fresh objects and against the reference's numbers (G30), the seams of the call
and its refusals.

The fixture is that of tests/test_gpu_covariance_blocks.py: three correlations, each on its own
halo.Halo, on one MultiEpoch(0, 5) -- two galaxy auto-correlations and a galaxy x convergence
one; 4 bins, 10 pairs, six blocks, (0, 2) not adjacent to the diagonal.  The trispectrum is a
HaloTrispectrumOneHalo(0.5), one object for all blocks.

The term reads no halo epoch (the I_0^4 table is the trispectrum object's, the windows are the
kernels'), so nothing here depends on how many epochs a grid sets up: every comparison of the
term itself is numpy.array_equal.  The full matrices are compared with array_equal at these three
correlations, as the Gaussian and super-sample tests assert for their terms.
"""
import numpy
import pytest

from conftest import load_golden, rel_err
from test_gpu_covariance_blocks import BLOCKS, setup_single, three_correlations
from test_gpu_covariance_cross import D2R, KWS
from test_gpu_covariance_cross_terms import (RTOL_COV, RTOL_KERNEL, correlations as g30_correlations,
                                             tri_object)
from test_gpu_covariance_ssc import scaled_err

pytestmark = pytest.mark.gpu
NG = dict(nongaussian_cov=True, cross_terms=True)
OLD_REFUSAL = ("get_covariance_batched: the batch serves the Gaussian and Poisson terms, not the "
               "trispectrum (nongaussian_cov) or super-sample (ssc_cov) terms; use get_covariance")


def multi(corrs, tri=None, **kws):
    """CovarianceMulti with the trispectrum term (nongaussian_cov=False in kws: without it)."""
    from chomp_amd import covariance
    kws = dict(KWS, **dict(NG, **kws))
    if kws["nongaussian_cov"]:
        kws["input_halo_trispectrum"] = tri_object() if tri is None else tri
    return covariance.CovarianceMulti(corrs, **kws)


def block_list(cm):
    return [cov for row in cm.covariance_list for cov in row]


class Staged(object):
    """One context with the three kernels as projection sets and the three epochs of a HaloGrid
    at their z_bar (with the response's families, for the super-sample batch of the seams), and
    the I_0^4 table of the trispectrum object: what get_covariance_batched(trispectrum=True)
    hands chomp_covariance_ng_blocks."""

    def __init__(self):
        from chomp_amd import _lib, correlation, grid, kernel
        self.corrs = three_correlations()
        self.kernels = [c.kernel for c in self.corrs]
        self.tri = tri_object()
        self.tri._initialize_i_0_4()
        self.table = numpy.array(self.tri._i_0_4_array, dtype=numpy.float64)
        self.k_range = (self.tri._k_min, self.tri._k_max)
        first = multi(self.corrs, self.tri).covariance_list[0][0]
        kc = first.kernel
        self.area = first.area
        self.kt = (kc.ln_ktheta_min, kc.ln_ktheta_max, kc._j0_limit)
        self.j0_ssc = kc._j0_ssc_limit
        c = numpy.array([b.center for b in first.annular_bins])
        iu = numpy.triu_indices(c.size)
        self.ta, self.tb = c[iu[0]], c[iu[1]]
        self.hg = grid.HaloGrid(numpy.zeros(3))
        self.ctx = self.hg.ctx
        self.code = correlation._POWER["power_mm"][0]
        kernel.Kernel._setup_pairs_on(self.ctx, self.kernels)
        self.z_bar = self.ctx.kernel_info_sets()["z_bar"]
        self.hg.set_parameters(z=self.z_bar)
        self.hg.setup("power_mm", families=_lib.FAM_SSC)
        # (the single calls need sigma^2 knots for kernel_ssc_setup; the trispectrum term reads
        #  none of them: any increasing knots do)
        self.ln_chi = numpy.linspace(1.0, 8.0, 50)
        self.sigma2 = numpy.ones(50)
        self.first = self.blocks()
        self.words = self.hg.status() & _ng_bit()        # (before the single calls write word 0)
        self.tables = [self.ctx.covariance_ng_blocks_table(b, knots=True) for b in range(6)]
        self.singles = [self.single(b, self.table) for b in range(6)]

    def blocks(self, table=None, theta=None, epochs=(0, 1, 2), **kws):
        a = dict(lo=self.kt[0], hi=self.kt[1], j0=self.kt[2], area=self.area,
                 k_min=self.k_range[0], k_max=self.k_range[1], ta=self.ta, tb=self.tb)
        a.update(kws)
        table = self.table if table is None else table
        if theta is not None:
            return self.ctx.covariance_ng_blocks(epochs, a["lo"], a["hi"], a["j0"], a["area"], table,
                                                 a["k_min"], a["k_max"], theta)
        return self.ctx.covariance_ng_blocks(epochs, a["lo"], a["hi"], a["j0"], a["area"], table,
                                             a["k_min"], a["k_max"], a["ta"], a["tb"])

    def single(self, b, table):
        """Block b by the single-block calls on this context."""
        i, j = BLOCKS[b]
        ctx = self.ctx
        setup_single(ctx, self.kernels[i])
        out = {}
        cross = i != j
        if cross:
            ctx.covariance_cross_stage(0, ctx, self.code, i)
            setup_single(ctx, self.kernels[j])
            ctx.covariance_cross_stage(1, ctx, self.code, j)
            out["range"] = list(ctx.covariance_cross_range())
        else:
            info = ctx.kernel_info()
            out["range"] = [info[k] for k in ("z_min", "z_max", "chi_min", "chi_max")]
        out["info"], _, _ = ctx.kernel_ssc_setup(self.kt[0], self.kt[1], self.j0_ssc, self.ln_chi,
                                                 self.sigma2, with_table=False, cross=cross)
        out["table"], out["levels"], out["min"] = ctx.kernel_ng_setup(self.kt[2])
        out["values"], out["kb"], out["kb_levels"] = ctx.covariance_ng(
            self.area, table, self.k_range[0], self.k_range[1], self.ta, self.tb, knots=True)
        # (kernel_ng_setup cleared the bit on the context's first word; the two calls set it)
        out["divmax"] = bool(ctx.status(0, 1)[0] & _ng_bit())
        return out


@pytest.fixture(scope="module")
def staged():
    return Staged()


def check_block(b, got_values, table, want):
    """One block of the batch against the single calls: everything, numpy.array_equal."""
    info, tab, lev, mn, kb, kb_lev = table
    ij = BLOCKS[b]
    assert tab.shape == (50, 50) and numpy.array_equal(tab, tab.T), ij
    assert numpy.array_equal(tab, want["table"]), ij
    assert numpy.array_equal(lev, want["levels"]), ij
    assert mn == want["min"] and mn == tab.min(), (ij, mn, want["min"])
    assert numpy.array_equal(info[:3], want["info"]), (ij, info[:3], want["info"])
    assert numpy.array_equal(info[3:], want["range"]), (ij, info[3:], want["range"])
    assert kb.shape == want["kb"].shape == (10, 50)
    assert numpy.array_equal(kb, want["kb"]), ij
    assert numpy.array_equal(kb_lev, want["kb_levels"]), ij
    assert numpy.array_equal(got_values, want["values"]), (ij, got_values / want["values"] - 1)


def test_blocks_bit_for_bit_against_the_single_calls(staged):
    S = staged
    got = S.first
    assert got.shape == (6, 10) and numpy.all(numpy.isfinite(got)) and numpy.all(got != 0.0)
    for b in range(6):
        check_block(b, got[b], S.tables[b], S.singles[b])
        info = S.tables[b][0]
        assert info[3] <= info[0] <= info[4] and 0.0 < info[5] <= info[1] <= info[6], BLOCKS[b]
    # a cross block's range is the common one of its two sides (kernel.py:910-916)
    for b, (i, j) in enumerate(BLOCKS):
        di, dj = S.tables[BLOCKS.index((i, i))][0], S.tables[BLOCKS.index((j, j))][0]
        assert S.tables[b][0][3] == max(di[3], dj[3]) and S.tables[b][0][4] == min(di[4], dj[4])
    # the status bit: block (i, j) reports on epoch[i]'s word what the single calls report (on
    # the context's first word) for that block
    want = [any(S.singles[b]["divmax"] for b, (i, _) in enumerate(BLOCKS) if i == c) for c in range(3)]
    print("ST_COV_NG_DIVMAX per correlation", S.words, "single calls per block",
          [S.singles[b]["divmax"] for b in range(6)], "deepest levels",
          [int(S.tables[b][2].max()) for b in range(6)], [int(S.tables[b][5].max()) for b in range(6)])
    assert [bool(w) for w in S.words] == want


def _ng_bit():
    from chomp_amd import _lib
    return numpy.uint32(_lib.ST_COV_NG_DIVMAX)


def test_no_two_blocks_alike(staged):
    """Neither the values nor the tables nor the k_b knots; a second call with another I_0^4
    table is the single calls' with THAT table; and the first call again is the first result."""
    S = staged
    for a in range(6):
        for b in range(a):
            assert rel_err(S.first[a], S.first[b]) > 1e-6, (a, b)
            assert scaled_err(S.tables[a][1], S.tables[b][1]) > 1e-6, (a, b)
            assert scaled_err(S.tables[a][4], S.tables[b][4]) > 1e-6, (a, b)
    ramp = numpy.linspace(1.0, 2.0, S.table.shape[0])
    other = S.table * numpy.sqrt(numpy.outer(ramp, ramp))
    got = S.blocks(table=other)
    tables = [S.ctx.covariance_ng_blocks_table(b, knots=True) for b in range(6)]
    for b in range(6):
        assert rel_err(got[b], S.first[b]) > 0.01, b
        check_block(b, got[b], tables[b], S.single(b, other))
        assert numpy.array_equal(tables[b][1], S.tables[b][1])       # (the kernel_NG table stays)
    assert numpy.array_equal(S.blocks(), S.first)
    for b in range(6):
        again = S.ctx.covariance_ng_blocks_table(b, knots=True)
        assert all(numpy.array_equal(x, y) for x, y in zip(again, S.tables[b])), b


def _loop_and_batch(**kws):
    cl = multi(three_correlations(), **kws)
    cl.get_covariance()
    cb = multi(three_correlations(), **kws)
    out, words = cb.get_covariance_batched(with_status=True, trispectrum=True)
    assert out is cb.wcovar and words is cb.blocks_status
    return cl, cb


@pytest.fixture(scope="module")
def loop_and_batch():
    """(the loop's CovarianceMulti after get_covariance(), the batch's after
    get_covariance_batched(trispectrum=True)), each on fresh correlations and its own
    trispectrum object."""
    return _loop_and_batch()


def check_against_the_loop(cl, cb):
    assert cb.wcovar.shape == (12, 12) and numpy.all(numpy.isfinite(cb.wcovar))
    assert numpy.array_equal(cb.wcovar, cb.wcovar.T)
    print("status words of the batch", cb.blocks_status)
    assert not numpy.any(cb.blocks_status & ~_ng_bit())
    c = numpy.array([b.center for b in cb.annular_bins])
    iu = numpy.triu_indices(c.size)
    assert cb.blocks_ng.shape == (6, 10) and numpy.all(numpy.isfinite(cb.blocks_ng))
    for b, (cov_l, cov_b) in enumerate(zip(block_list(cl), block_list(cb))):
        # the trispectrum term by itself: the loop's covariance_NG of the block
        want = cov_l._covariance_NG_pairs(c[iu[0]], c[iu[1]])
        assert numpy.array_equal(cb.blocks_ng[b], want), (BLOCKS[b], cb.blocks_ng[b] / want - 1)
        assert numpy.all(cb.blocks_ng[b] != 0.0)
    print("wcovar: batch against loop", rel_err(cb.wcovar, cl.wcovar))
    for b, (cov_l, cov_b) in enumerate(zip(block_list(cl), block_list(cb))):
        assert numpy.array_equal(cov_b.covar, cov_l.covar), (BLOCKS[b], rel_err(cov_b.covar, cov_l.covar))
    assert numpy.array_equal(cb.wcovar, cl.wcovar), rel_err(cb.wcovar, cl.wcovar)


def off_diagonal(cov):
    """(the covar entries (i, j), i < j, of a block; which of the 10 pair values they are).  The
    diagonal of a matching block carries the Poisson term as well, added after the others."""
    i, j = numpy.triu_indices(4)
    return cov.covar[i[i < j], j[i < j]], i < j


def test_batched_against_the_loop(loop_and_batch):
    cl, cb = loop_and_batch
    check_against_the_loop(cl, cb)
    assert cb.blocks_ssc is None
    # the term is in the matrix: the Gaussian batch of the same correlations differs, by it
    gm = multi(three_correlations(), nongaussian_cov=False, cross_terms=False)
    gauss = gm.get_covariance_batched()
    assert gm.blocks_ng is None and not numpy.array_equal(cb.wcovar, gauss)
    for b, (cov_g, cov_b) in enumerate(zip(block_list(gm), block_list(cb))):
        (G, off), (full, _) = off_diagonal(cov_g), off_diagonal(cov_b)
        assert numpy.array_equal(full, G + cb.blocks_ng[b][off]), BLOCKS[b]
        assert numpy.all(full != G), BLOCKS[b]
    # ... and the blocks' own kernel_NG state was not built by the batch
    for cov in block_list(cb):
        assert cov.kernel._ssc_key is None and cov.kernel._ng_key is None


def test_batched_against_the_loop_with_all_three_terms():
    """ssc_cov=True, nongaussian_cov=True, cross_terms=True: Gaussian, then trispectrum, then
    super-sample, the loop's order."""
    cl, cb = _loop_and_batch(ssc_cov=True)
    check_against_the_loop(cl, cb)
    assert cb.blocks_ssc.shape == (6, 10) and numpy.all(cb.blocks_ssc != 0.0)
    gm = multi(three_correlations(), nongaussian_cov=False, cross_terms=False)
    gm.get_covariance_batched()
    for b, (cov_g, cov_b) in enumerate(zip(block_list(gm), block_list(cb))):
        (G, off), (full, _) = off_diagonal(cov_g), off_diagonal(cov_b)
        assert numpy.array_equal(full, (G + cb.blocks_ng[b][off]) + cb.blocks_ssc[b][off]), BLOCKS[b]
    # the trispectrum values do not depend on the epochs' families
    assert numpy.array_equal(cb.blocks_ng, multi_ng_values())


def multi_ng_values():
    cm = multi(three_correlations())
    cm.get_covariance_batched(trispectrum=True)
    return cm.blocks_ng


def test_batched_against_the_reference():
    """G30 "gal": the cross block of a two-correlation CovarianceMulti with both terms -- its
    kernel_NG table, its covariance_NG at the pairs i <= j and its covar = covariance_G +
    covariance_NG + covariance_ssc -- at that fixture's bars."""
    g = load_golden("g30_covariance_cross_terms")
    cm = multi(list(g30_correlations("gal")), ssc_cov=True)
    w = cm.get_covariance_batched(trispectrum=True)
    assert w.shape == (8, 8) and numpy.array_equal(w, w.T)
    _, tab, _, mn = cm._blocks_grid[1].ctx.covariance_ng_blocks_table(1)
    err = scaled_err(tab, g["gal_kernel_array"])
    print("block (0, 1) kernel_NG table error / scale", err)
    assert err < RTOL_KERNEL
    assert abs(mn - g["gal_kernel_NG_min"][0]) < RTOL_KERNEL * numpy.max(numpy.abs(g["gal_kernel_array"]))
    iu = [tuple(p) for p in zip(*numpy.triu_indices(4))]
    n = 0
    for p, (i, j) in enumerate(g["gal_ng_pairs"]):
        if i <= j:
            got = cm.blocks_ng[1][iu.index((i, j))]
            e = abs(got / g["gal_NG"][p] - 1.0)
            print("covariance_NG", i, j, e)
            assert e < RTOL_COV, (i, j, e)
            n += 1
    assert n == 10
    err = rel_err(w[:4, 4:], g["gal_cov"])
    print("block (0, 1) covar error", err)
    assert err < RTOL_COV
    assert numpy.array_equal(cm.covariance_list[0][1].covar, w[:4, 4:])


def test_seams(staged):
    """One correlation alone; the call with a device theta; the single-block kernel_NG state of
    the context, the Gaussian batch's and the super-sample batch's states untouched; fewer
    correlations on the same context."""
    import torch
    from chomp_amd import covariance, kernel
    S = staged
    ctx = S.ctx
    # one correlation with the term and no cross_terms: a diagonal block alone
    one = multi(three_correlations()[:1], cross_terms=False)
    assert len(one.covariance_list) == 1 and len(one.covariance_list[0]) == 1
    w = one.get_covariance_batched(trispectrum=True)
    assert w.shape == (4, 4) and one.blocks_ng.shape == (1, 10)
    alone = multi(three_correlations()[:1], cross_terms=False)
    loop = alone.get_covariance()
    c = numpy.array([b.center for b in alone.annular_bins])
    iu = numpy.triu_indices(4)
    assert numpy.array_equal(one.blocks_ng[0],
                             alone.covariance_list[0][0]._covariance_NG_pairs(c[iu[0]], c[iu[1]]))
    assert numpy.array_equal(w, loop), rel_err(w, loop)
    # ... which is block (0, 0) of the three (the term reads no epoch)
    assert numpy.array_equal(one.blocks_ng[0], S.first[0])
    # a device theta
    pairs = torch.tensor(numpy.concatenate([S.ta, S.tb]), dtype=torch.float64, device="cuda")
    dev = S.blocks(theta=pairs)
    assert dev.is_cuda and dev.shape == (6, 10)
    assert numpy.array_equal(dev.cpu().numpy(), S.first)
    # a single-block state, the batch, and the single-block state again
    before = S.single(5, S.table)
    raw = ctx.kernel_ng_raw(numpy.array([-2.0]), numpy.array([-1.0]))
    ev = ctx.kernel_ng_eval(numpy.array([-2.0]), numpy.array([-1.0]))
    ssc_raw = ctx.kernel_ssc_raw(numpy.array([-2.0]), numpy.array([-1.0]))
    assert numpy.array_equal(S.blocks(), S.first)
    assert numpy.array_equal(ctx.kernel_ng_raw(numpy.array([-2.0]), numpy.array([-1.0])), raw)
    assert numpy.array_equal(ctx.kernel_ng_eval(numpy.array([-2.0]), numpy.array([-1.0])), ev)
    assert numpy.array_equal(ctx.kernel_ssc_raw(numpy.array([-2.0]), numpy.array([-1.0])), ssc_raw)
    assert numpy.array_equal(ctx.covariance_ng(S.area, S.table, S.k_range[0], S.k_range[1], S.ta,
                                               S.tb), before["values"])
    # ... and the two slots of a cross block: block (1, 2) staged, the batch, its values again
    cross = S.single(4, S.table)
    assert numpy.array_equal(S.blocks(), S.first)
    assert numpy.array_equal(ctx.covariance_ng(S.area, S.table, S.k_range[0], S.k_range[1], S.ta,
                                               S.tb), cross["values"])
    assert list(ctx.covariance_cross_range()) == cross["range"]
    # the Gaussian batch's state is its own
    poisson = numpy.zeros((6, 4))
    G = ctx.covariance_blocks(S.code, [0, 1, 2], S.kt[2], S.area, poisson, S.ta, S.tb)
    gt = ctx.covariance_blocks_table(2)
    assert numpy.array_equal(S.blocks(), S.first)
    assert numpy.array_equal(ctx.covariance_blocks_table(2)[1], gt[1])
    assert numpy.array_equal(ctx.covariance_blocks(S.code, [0, 1, 2], S.kt[2], S.area, poisson, S.ta,
                                                   S.tb), G)
    # ... and so is the super-sample batch's
    ranges = ctx.covariance_ssc_blocks_range(3)
    ln_chi, sigma2 = covariance.CovarianceMulti._ssc_blocks_knots([k.cosmo for k in S.kernels], ranges)
    args = ([0, 1, 2], S.kt[0], S.kt[1], S.j0_ssc, ln_chi, sigma2, S.area, S.ta, S.tb)
    ssc = ctx.covariance_ssc_blocks(*args)
    st = ctx.covariance_ssc_blocks_table(2, knots=True)
    assert numpy.array_equal(S.blocks(), S.first)
    assert all(numpy.array_equal(x, y) for x, y in zip(ctx.covariance_ssc_blocks_table(2, knots=True), st))
    assert numpy.array_equal(ctx.covariance_ssc_blocks(*args), ssc)
    assert all(numpy.array_equal(x, y) for x, y in
               zip(ctx.covariance_ng_blocks_table(2, knots=True), S.tables[2]))
    # fewer correlations: sets 0 and 1 alone give blocks (0, 0), (0, 1), (1, 1) of the three
    kernel.Kernel._setup_pairs_on(ctx, S.kernels[:2])
    keep = [0, 1, 3]
    two = S.blocks(epochs=(0, 1))
    assert two.shape == (3, 10) and numpy.array_equal(two, S.first[keep])
    with pytest.raises(ValueError, match="covariance_ng_blocks_table: block"):
        ctx.covariance_ng_blocks_table(3)
    assert numpy.array_equal(ctx.covariance_ng_blocks_table(1)[1], S.tables[1][1])
    kernel.Kernel._setup_pairs_on(ctx, S.kernels)
    assert numpy.array_equal(S.blocks(), S.first)


def test_null_epochs_give_the_same_values(staged):
    """epoch == NULL through the C call itself: the values are the same and no status word is
    touched -- a bit the call before left is still there, a bit cleared by hand stays clear."""
    import ctypes
    from chomp_amd import _lib
    S = staged
    assert numpy.array_equal(S.blocks(), S.first)
    assert numpy.array_equal(S.hg.status() & _ng_bit(), S.words)
    out = numpy.empty((6, 10))
    th = numpy.concatenate([S.ta, S.tb])
    S.ctx._check(S.ctx._L.chomp_covariance_ng_blocks(
        S.ctx._h, 3, None, S.kt[0], S.kt[1], S.kt[2], S.area, S.table.ctypes.data_as(_lib.c_double_p),
        S.table.shape[0], S.k_range[0], S.k_range[1], th.ctypes.data, 10, out.ctypes.data, _lib.HOST))
    assert numpy.array_equal(out, S.first)
    assert numpy.array_equal(S.hg.status() & _ng_bit(), S.words)
    # with fewer correlations only their words are written: correlation 2's keeps what it had
    from chomp_amd import kernel
    kernel.Kernel._setup_pairs_on(S.ctx, S.kernels[:2])
    assert numpy.array_equal(S.blocks(epochs=(0, 1)), S.first[[0, 1, 3]])
    assert (S.hg.status() & _ng_bit())[2] == S.words[2]
    kernel.Kernel._setup_pairs_on(S.ctx, S.kernels)
    assert numpy.array_equal(S.blocks(), S.first)
    assert numpy.array_equal(S.hg.status() & _ng_bit(), S.words)


def test_c_refusals(staged):
    from chomp_amd import _lib, cosmology, grid, kernel
    S = staged
    ctx = S.ctx
    A, E, X = ValueError, _lib.ChompError, _lib.ChompScopeError
    name = "covariance_ng_blocks"
    with pytest.raises(A, match=name + ": area must be positive"):
        S.blocks(area=0.0)
    with pytest.raises(A, match=name + ": arguments must be positive"):
        S.blocks(tb=-S.tb)
    with pytest.raises(A, match=name + r": ln\(k theta\) range / J0 limit"):
        S.blocks(lo=S.kt[1], hi=S.kt[0])
    with pytest.raises(A, match=name + r": ln\(k theta\) range / J0 limit"):
        S.blocks(j0=0.0)
    with pytest.raises(A, match=name + r": the I_0\^4 table must be 4..64 knots a side"):
        S.blocks(table=S.table[:3, :3])
    with pytest.raises(A, match=name + r": the I_0\^4 table must be 4..64 knots a side"):
        S.blocks(table=numpy.ones((65, 65)))
    with pytest.raises(A, match=name + r": the I_0\^4 table must be square"):
        S.blocks(table=S.table[:, :10])
    with pytest.raises(A, match=name + r": the I_0\^4 table's k range"):
        S.blocks(k_min=S.k_range[1], k_max=S.k_range[0])
    with pytest.raises(A, match=name + r": the I_0\^4 table's k range"):
        S.blocks(k_min=0.0)
    with pytest.raises(A, match=name + ": at most 65535 pairs a call"):
        S.blocks(ta=numpy.ones(65536), tb=numpy.ones(65536))
    with pytest.raises(A, match=name + ": correlation 2: epoch range"):
        S.blocks(epochs=(0, 1, 3))
    with pytest.raises(E, match=name + ": n_corr is not the number of sets"):
        S.blocks(epochs=(0, 1))
    with pytest.raises(A, match="covariance_ng_blocks_table: block"):
        ctx.covariance_ng_blocks_table(6)
    # a refused call leaves the last result readable, its k_b knots included
    assert all(numpy.array_equal(x, y) for x, y in
               zip(ctx.covariance_ng_blocks_table(1, knots=True), S.tables[1]))
    # a context without sets; sets of Bessel order 2; more than 65535 blocks
    hg = grid.HaloGrid(numpy.zeros(3))
    args = ([0, 1, 2], S.kt[0], S.kt[1], S.kt[2], S.area, S.table, S.k_range[0], S.k_range[1],
            S.ta, S.tb)
    with pytest.raises(E, match=name + " before kernel_setup_pairs"):
        hg.ctx.covariance_ng_blocks(*args)
    with pytest.raises(E, match="covariance_ng_blocks_table before covariance_ng_blocks"):
        hg.ctx.covariance_ng_blocks_table(0)
    with pytest.raises(E, match="covariance_ng_blocks_table before covariance_ng_blocks"):
        hg.ctx.covariance_ng_blocks_table(0, knots=True)
    lens = [kernel.GalaxyGalaxyLensingKernel(k._ktheta[0], k._ktheta[1], k.window_function_a,
                                             k.window_function_b, k.cosmo) for k in S.kernels]
    kernel.Kernel._setup_pairs_on(hg.ctx, lens)
    with pytest.raises(E, match=name + ": the sets are of Bessel order 2"):
        hg.ctx.covariance_ng_blocks(*args)
    kernel.Kernel._setup_pairs_on(hg.ctx, [S.kernels[0]] * 362)      # 362 * 363 / 2 = 65703 blocks
    with pytest.raises(A, match=name + ": more than 65535 blocks"):
        hg.ctx.covariance_ng_blocks(numpy.zeros(362, dtype=int), *args[1:])
    # windows with no redshift in common: the library names the block, and launches nothing
    cm = cosmology.MultiEpoch(0.0, 5.0)
    lo = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 0.5, 0.3, 0.1), cm)
    hi = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.5, 1.5, 1.0, 0.2), cm)
    mid = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 1.5, 0.7, 0.2), cm)
    apart = [kernel.Kernel(1e-6 * D2R, 100.0 * D2R, w, w, cm) for w in (mid, lo, hi)]
    kernel.Kernel._setup_pairs_on(hg.ctx, apart)
    with pytest.raises(X, match=name + r": block \(1, 2\): the four windows have no redshift in common"):
        hg.ctx.covariance_ng_blocks(*args)
    with pytest.raises(E, match="covariance_ng_blocks_table before covariance_ng_blocks"):
        hg.ctx.covariance_ng_blocks_table(0)
    # ... and the staged context is as it was
    assert numpy.array_equal(S.blocks(), S.first)


def test_python_refusals(staged):
    from chomp_amd import _lib, cosmology, correlation, halo, kernel
    S = staged
    X = _lib.ChompScopeError
    # without the keyword: refused as ever, word for word
    for kws in (dict(), dict(ssc_cov=True)):
        cm = multi(S.corrs, S.tri, **kws)
        with pytest.raises(X) as info:
            cm.get_covariance_batched()
        assert str(info.value) == OLD_REFUSAL
        with pytest.raises(X) as info:
            cm.get_covariance_batched(trispectrum=False)
        assert str(info.value) == OLD_REFUSAL
        assert not hasattr(cm, "_blocks_grid")
    cases = []
    cm = multi(S.corrs, S.tri)
    cm.covariance_list[1][1].nongaussian_cov = False
    cases.append(("the blocks differ in nongaussian_cov", cm))
    cm = multi(S.corrs, S.tri)
    cm.covariance_list[0][2].halo_tri = tri_object()
    cases.append(("the blocks do not share one halo_tri object", cm))
    cm = multi(S.corrs, S.tri)
    cm.covariance_list[0][1].kernel.ln_ktheta_max += 1.0
    cases.append(("block (0, 1): its KernelCovariance has another k theta range or J0 limit", cm))
    cm = multi(S.corrs, S.tri)
    cm.covariance_list[1][1].kernel._j0_limit *= 2.0
    cases.append(("block (1, 2): its KernelCovariance has another k theta range or J0 limit", cm))
    me = cosmology.MultiEpoch(0.0, 5.0)

    def corr(dist):
        w = kernel.WindowFunctionGalaxy(dist, me)
        return correlation.Correlation(0.01, 1.0, kernel.Kernel(1e-6 * D2R, 100.0 * D2R, w, w, me),
                                       input_halo=halo.Halo(0.0), power_spec="power_mm")
    apart = [corr(kernel.dNdzGaussian(0.0, 1.5, 0.7, 0.2)), corr(kernel.dNdzGaussian(0.0, 0.5, 0.3, 0.1)),
             corr(kernel.dNdzGaussian(0.5, 1.5, 1.0, 0.2))]
    cases.append(("block (1, 2): the four windows have no redshift in common (z_min = 0.5 >= "
                  "z_max = 0.5", multi(apart, S.tri)))
    for label, cm in cases:
        with pytest.raises(X) as info:
            cm.get_covariance_batched(trispectrum=True)
        text = str(info.value)
        assert label in text, (label, text)
        assert text.startswith("get_covariance_batched: ") and text.endswith("; use get_covariance")
        assert not hasattr(cm, "_blocks_grid"), label
    # the keyword with blocks that have no such term: the Gaussian batch, nothing else
    gm = multi(three_correlations(), nongaussian_cov=False, cross_terms=False)
    w = gm.get_covariance_batched(trispectrum=True).copy()
    assert gm.blocks_ng is None and gm.blocks_ssc is None
    assert numpy.array_equal(w, multi(three_correlations(), nongaussian_cov=False,
                                      cross_terms=False).get_covariance_batched())
    assert numpy.array_equal(S.blocks(), S.first)
