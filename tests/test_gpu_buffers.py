"""The context's buffers growing and shrinking under one context: a call at a small size, the
same call at a larger size (its buffers move), and the first call again.  Every result is compared
bit for bit with what a fresh context makes of the same inputs, and the third with the first: a
buffer that moved holds nothing of what it held, and a shadow that describes a buffer's old
contents does not outlive them.  No graph capture here (tests/test_gpu_properties.py and
tests/test_gpu_projection.py hold the rule for buffers a graph may reference).
"""
import numpy
import pytest

from conftest import load_golden
from test_gpu_covariance_blocks import three_correlations
from test_gpu_covariance_cross import KWS
from test_gpu_wtheta_cosmologies import _cosmos, _kernel

pytestmark = pytest.mark.gpu
SPECTRA = ("power_mm", "power_gg")


def _stage(ctx, z, cosmo=None, spectra=SPECTRA):
    """Epochs at `z` (one cosmology, or one per epoch) with the default halo and HOD, and the
    knot tables of `spectra`: HaloGrid.setup on a context of the caller's."""
    from chomp_amd import _lib, cosmology, defaults, grid
    z = numpy.ascontiguousarray(z, dtype=numpy.float64)
    n = z.size
    c = ctx.pack_cosmo(cosmo if cosmo is not None else defaults.default_cosmo_dict, n)
    h = ctx.pack_halo(defaults.default_halo_dict, n)
    hod = ctx.pack_hod(grid._hod_object(defaults.default_hod_dict), n)
    need = 0
    for s in spectra:
        need |= grid._WHICH[s][1]
    ctx.epochs_set(c, z, **cosmology._de_kw(c))
    ctx.stage_k(h, _lib.MF_ST, h, hod, need)
    return n


def _powers(ctx, n, k):
    from chomp_amd import grid
    return numpy.stack([ctx.power(grid._WHICH[s][0], k, 0, n) for s in SPECTRA])


def _there_and_back(step, sizes):
    """step(ctx, size) on one context for each of `sizes` (small, large, small), and on a fresh
    context each time."""
    from chomp_amd import cosmology
    ctx = cosmology._context()
    got = [step(ctx, s) for s in sizes]
    for g, s in zip(got, sizes):
        assert numpy.all(numpy.isfinite(g)), s
        fresh = step(cosmology._context(), s)
        assert g.shape == fresh.shape and numpy.array_equal(g, fresh), s
    assert sizes[0] == sizes[2] and numpy.array_equal(got[2], got[0])
    return got


def test_epoch_batch_grows_and_shrinks():
    """(a) 2 -> 5 -> 2 epochs: alloc_epochs moves all of the batch's buffers once."""
    k = numpy.logspace(-3, 2, 64)

    def step(ctx, n):
        _stage(ctx, numpy.linspace(0.0, 1.0, n))
        return _powers(ctx, n, k)
    got = _there_and_back(step, (2, 5, 2))
    assert got[0].shape == (2, 2, 64) and got[1].shape == (2, 5, 64)


def test_host_power_grows_and_shrinks():
    """(b) host-pointer Context.power with 16, 4096, 16 wavenumbers: the staging buffers, their
    pinned mirrors, the cached k grid and the Stage E work lists."""
    from chomp_amd import cosmology
    z = numpy.array([0.0, 0.5, 1.0])
    grids = {16: numpy.logspace(-3, 2, 16), 4096: numpy.logspace(-3, 2, 4096)}
    ctx = cosmology._context()
    _stage(ctx, z)
    got = [_powers(ctx, 3, grids[nk]) for nk in (16, 4096, 16)]
    assert numpy.array_equal(got[2], got[0])
    for g, nk in zip(got, (16, 4096, 16)):
        fresh = cosmology._context()
        _stage(fresh, z)
        assert g.shape == (2, 3, nk) and numpy.all(numpy.isfinite(g))
        assert numpy.array_equal(g, _powers(fresh, 3, grids[nk])), nk


def test_dark_energy_tables_grow_and_shrink():
    """(c) three w0-wa epochs with 1, 3, 1 distinct (w0, wa): the pressure tables, their keys
    and the epoch -> table map."""
    from chomp_amd import defaults
    k = numpy.logspace(-3, 2, 64)
    z = numpy.array([0.0, 0.5, 1.0])
    pairs = {1: [(-0.9, 0.1)] * 3, 3: [(-0.9, 0.1), (-1.1, -0.2), (-0.8, 0.3)]}

    def step(ctx, n_distinct):
        cosmos = [dict(defaults.default_cosmo_dict, w0=w0, wa=wa) for w0, wa in pairs[n_distinct]]
        _stage(ctx, z, cosmos)
        return _powers(ctx, 3, k)
    got = _there_and_back(step, (1, 3, 1))
    assert not numpy.array_equal(got[1][:, 1], got[0][:, 1])


def test_projection_sets_grow_and_shrink():
    """(d) kernel_setup_sets + wtheta_sets with 1, 3, 1 sets at 4 angles."""
    from chomp_amd import correlation, defaults
    g34 = load_golden("g34_wtheta_cosmologies")
    cosmos = _cosmos(g34)
    theta = numpy.ascontiguousarray(g34["theta"][:4])
    kern = _kernel()
    code = correlation._POWER["power_gg"][0]
    k_lim = (defaults.default_limits["k_min"], defaults.default_limits["k_max"])

    def step(ctx, n):
        kern._setup_sets_on(ctx, cosmos[:n])
        info = ctx.kernel_info_sets()
        _stage(ctx, info["z_bar"], cosmos[:n], ("power_gg",))
        return ctx.wtheta_sets(code, 0, n, *k_lim, info["D_zbar"], theta)
    got = _there_and_back(step, (1, 3, 1))
    assert got[0].shape == (1, 4) and got[1].shape == (3, 4)


def test_covariance_blocks_grow_and_shrink():
    """(e) covariance_blocks with 2, 3, 2 correlations (3, 6, 3 blocks) of the fixture of
    tests/test_gpu_covariance_blocks.py."""
    from chomp_amd import correlation, covariance, kernel
    corrs = three_correlations()
    kernels = [c.kernel for c in corrs]
    first = covariance.CovarianceMulti(corrs[:1], nongaussian_cov=False, **KWS).covariance_list[0][0]
    j0, area = first._j0_limit, first.area
    c = numpy.array([b.center for b in first.annular_bins])
    iu = numpy.triu_indices(c.size)
    ta, tb = c[iu[0]], c[iu[1]]
    code = correlation._POWER["power_mm"][0]

    def step(ctx, n):
        kernel.Kernel._setup_pairs_on(ctx, kernels[:n])
        _stage(ctx, ctx.kernel_info_sets()["z_bar"], None, ("power_mm",))
        n_blocks = n * (n + 1) // 2
        poisson = 1e-9 * (1.0 + numpy.arange(4.0 * n_blocks).reshape(n_blocks, 4))
        return ctx.covariance_blocks(code, list(range(n)), j0, area, poisson, ta, tb)
    got = _there_and_back(step, (2, 3, 2))
    assert got[0].shape == (3, 10) and got[1].shape == (6, 10)
