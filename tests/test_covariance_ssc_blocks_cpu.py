"""Host side of the super-sample term in CovarianceMulti.get_covariance_batched /
chomp_covariance_ssc_blocks: the C declarations and their bindings, what the batch's scope now
serves and what it still refuses (before any device context exists), the per-block sigma^2 knot
arrays and the route of the call on a stubbed grid and context.  No device."""
import ctypes
import os
import re

import numpy
import pytest

from conftest import ROOT
from test_covariance_blocks_cpu import D2R, bare, multi
from test_kernels_batch_cpu import KTHETA, no_device  # noqa: F401

SSC = dict(ssc_cov=True, cross_terms=True)


def test_header_declares_the_entry_points_and_the_bindings_match():
    from chomp_amd import _lib
    with open(os.path.join(ROOT, "include", "chomp_mi355x.h")) as f:
        header = f.read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    decls = {
        "chomp_covariance_ssc_blocks_range":
            "int chomp_covariance_ssc_blocks_range(chomp_ctx* ctx, size_t n_corr, double* info );",
        "chomp_covariance_ssc_blocks":
            "int chomp_covariance_ssc_blocks(chomp_ctx* ctx, size_t n_corr, const size_t* epoch , "
            "double ln_ktheta_min, double ln_ktheta_max, double j0_ssc_limit, "
            "const double* ln_chi , const double* sigma2 , size_t n_sigma, double area, "
            "const double* theta , size_t n_pairs, double* out , int mem);",
        "chomp_covariance_ssc_blocks_table":
            "int chomp_covariance_ssc_blocks_table(chomp_ctx* ctx, size_t block, double* info , "
            "double* table, double* levels, double* kb_knots, double* kb_levels);"}
    for decl in decls.values():
        assert decl in flat, decl
    # (the shapes as the issue states them)
    spaced = re.sub(r"\s+", " ", header)
    assert "double* info /*[n_blocks][4]*/" in spaced
    assert "const double* ln_chi /*[n_blocks][n_sigma]*/" in spaced
    assert "const double* sigma2 /*[n_blocks][n_sigma]*/" in spaced
    assert "const double* theta /*[2][n_pairs]: theta_a then theta_b*/" in spaced
    assert "double* out /*[n_blocks][n_pairs]*/" in spaced
    # the argtypes, from the declarations: arrays that follow `mem` travel as addresses
    vp, sz, dp = ctypes.c_void_p, ctypes.c_size_t, _lib.c_double_p
    kinds = {"chomp_ctx*": [vp], "int": [ctypes.c_int], "size_t": [sz], "double": [ctypes.c_double],
             "const size_t*": [ctypes.POINTER(sz)], "const double*": [vp, dp], "double*": [vp, dp]}
    L = _lib.lib()
    for name, decl in decls.items():
        assert name in _lib.EXPORTS
        assert hasattr(L, name), name
        params = decl[decl.index("(") + 1:decl.rindex(")")].split(",")
        types = [p.strip().rsplit(" ", 1)[0].strip() for p in params]
        got = getattr(L, name).argtypes
        assert len(got) == len(types), name
        for t, g in zip(types, got):
            assert g in kinds[t], (name, t, g)
    at = L.chomp_covariance_ssc_blocks.argtypes
    assert at[6] == dp and at[7] == dp                 # ln_chi, sigma2: host only
    assert at[10] == vp and at[12] == vp               # theta, out: host or device
    assert L.chomp_covariance_ssc_blocks_range.argtypes[2] == dp
    assert L.chomp_covariance_ssc_blocks_table.argtypes[2:] == [dp] * 5
    for name in ("covariance_ssc_blocks_range", "covariance_ssc_blocks",
                 "covariance_ssc_blocks_table"):
        assert callable(getattr(_lib.Context, name))


def _disjoint_kernel(lo):
    """A Kernel whose two windows lie on z = 0-0.5 (lo) or z = 0.5-1.5."""
    from chomp_amd import cosmology, kernel
    me = cosmology.MultiEpoch(0.0, 5.0)
    dist = (kernel.dNdzGaussian(0.0, 0.5, 0.3, 0.1) if lo
            else kernel.dNdzGaussian(0.5, 1.5, 1.0, 0.2))
    w = kernel.WindowFunctionGalaxy(dist, me)
    return kernel.Kernel(KTHETA[0], KTHETA[1], w, w, me)


def test_scope_serves_the_super_sample_blocks(no_device):  # noqa: F811
    """One correlation with ssc_cov (a diagonal block alone), several with cross_terms, and the
    Gaussian case as before: the scope returns the correlations and the spectrum's name."""
    for cm, n in ((multi([bare()], ssc_cov=True), 1), (multi([bare(), bare()], **SSC), 2),
                  (multi([bare(), bare(), bare()], **SSC), 3), (multi([bare(), bare()]), 2)):
        corrs, name = cm._batched_scope()
        assert len(corrs) == n and name == "power_mm"
        assert corrs == [row[0].corr_a for row in cm.covariance_list]
    cm = multi([bare(), bare()], **SSC)
    assert all(cov.ssc_cov for row in cm.covariance_list for cov in row)
    assert cm.covariance_list[0][1].kernel._four_windows
    assert not cm.covariance_list[0][0].kernel._four_windows


def test_scope_still_refuses(no_device):  # noqa: F811
    from chomp_amd import _lib, halo_trispectrum
    tri = halo_trispectrum.HaloTrispectrumOneHalo.__new__(halo_trispectrum.HaloTrispectrumOneHalo)
    cases = []
    # the trispectrum term, with the words it had
    old = ("get_covariance_batched: the batch serves the Gaussian and Poisson terms, not the "
           "trispectrum (nongaussian_cov) or super-sample (ssc_cov) terms; use get_covariance")
    for kws in (dict(), dict(ssc_cov=True), SSC):
        cm = multi([bare()] if "cross_terms" not in kws else [bare(), bare()],
                   nongaussian_cov=True, input_halo_trispectrum=tri, **kws)
        with pytest.raises(_lib.ChompScopeError) as info:
            cm.get_covariance_batched()
        assert str(info.value) == old
    # blocks that differ in ssc_cov
    cm = multi([bare(), bare()], **SSC)
    cm.covariance_list[0][1].ssc_cov = False
    cases.append(("the blocks differ in ssc_cov", cm))
    cm = multi([bare(), bare()])
    cm.covariance_list[1][0].ssc_cov = True
    cases.append(("the blocks differ in ssc_cov", cm))
    # windows with no redshift in common: the block is named, from the host's z_min / z_max
    cm = multi([bare(), bare(kern=_disjoint_kernel(True)), bare(kern=_disjoint_kernel(False))],
               **SSC)
    cases.append(("block (1, 2): the four windows have no redshift in common (z_min = 0.5 >= "
                  "z_max = 0.5", cm))
    # a block whose KernelCovariance was built over another k theta range
    cm = multi([bare(), bare()], **SSC)
    cm.covariance_list[0][1].kernel.ln_ktheta_max += 1.0
    cases.append(("block (0, 1): its KernelCovariance has another k theta range", cm))
    # everything else the scope refused stays refused with ssc_cov
    cases.append(("poisson_noise_only needs no device",
                  multi([bare(), bare()], poisson_noise_only=True, **SSC)))
    from chomp_amd import halo
    cases.append(("correlation 1: an extrapolated spectrum",
                  multi([bare(), bare(halo.Halo(0.0, extrapolate=True))], **SSC)))
    shared = halo.Halo(0.0)
    cases.append(("correlations 0 and 1 share one Halo object",
                  multi([bare(shared), bare(shared)], **SSC)))
    wide = bare()
    wide.log_theta_max = numpy.log10(10.0 * D2R)
    cases.append(("the blocks' angular bins or survey areas differ", multi([bare(), wide], **SSC)))
    for label, cm in cases:
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)) as info:
            cm.get_covariance_batched()
        assert str(info.value).startswith("get_covariance_batched: "), label
        assert str(info.value).endswith("; use get_covariance"), label
        assert not hasattr(cm, "_blocks_grid"), label


class _Cosmo(object):
    """A MultiEpoch's sigma_r, recorded: sigma = tag + 1e-3 chi."""

    def __init__(self, tag, calls):
        self.tag, self.calls = tag, calls

    def sigma_r(self, chi, z):
        chi = numpy.asarray(chi)
        self.calls.append((self.tag, chi.copy(), z))
        return self.tag + 1e-3 * chi


def test_knot_arrays_per_block_one_sigma_r_call_per_row():
    from chomp_amd import covariance, defaults
    npts = defaults.default_precision["corr_npoints"]
    calls = []
    cosmos = [_Cosmo(float(t), calls) for t in (1, 2, 3)]
    # block b: chi range [10 (b + 1), 1000 (b + 2)]
    ranges = numpy.array([[0.1, 1.0, 10.0 * (b + 1), 1000.0 * (b + 2)] for b in range(6)])
    ln_chi, sigma2 = covariance.CovarianceMulti._ssc_blocks_knots(cosmos, ranges)
    assert ln_chi.shape == (6, npts) and sigma2.shape == (6, npts)
    assert ln_chi.dtype == numpy.float64 and sigma2.dtype == numpy.float64
    # one call per row of blocks, with that row's MultiEpoch, at redshift 0.0
    assert [c[0] for c in calls] == [1.0, 2.0, 3.0]
    assert [c[1].size for c in calls] == [3 * npts, 2 * npts, npts]
    assert all(c[2] == 0.0 and isinstance(c[2], float) for c in calls)
    rows = [0, 0, 0, 1, 1, 2]                    # block -> i, the row-major upper triangle
    for b in range(6):
        chi = numpy.logspace(numpy.log10(ranges[b, 2]), numpy.log10(ranges[b, 3]), npts)
        assert numpy.array_equal(ln_chi[b], numpy.log(chi)), b
        sigma = (rows[b] + 1.0) + 1e-3 * chi
        assert numpy.array_equal(sigma2[b], sigma * sigma), b
        assert numpy.all(numpy.diff(ln_chi[b]) > 0.0)
    # ... the blocks of a row in the order of the call's chi
    assert numpy.array_equal(calls[1][1][npts:], numpy.logspace(
        numpy.log10(ranges[4, 2]), numpy.log10(ranges[4, 3]), npts))
    with pytest.raises(ValueError):
        covariance.CovarianceMulti._ssc_blocks_knots(cosmos, ranges[:5])


def test_route_of_the_batch_with_the_super_sample_term(monkeypatch):
    """On a stubbed grid and context: the epochs are set up with FAM_SSC beside the spectrum's
    families, the range is read once, the knots go to covariance_ssc_blocks with block (0, 0)'s
    k theta range and J0 limit, and the values are added to the Gaussian ones before the fill."""
    from chomp_amd import _lib, defaults, grid, kernel
    calls = []
    Z = numpy.array([0.3, 0.5])
    npts = defaults.default_precision["corr_npoints"]

    class Ctx(object):
        def kernel_info_sets(self):
            return {"z_bar": Z}

        def covariance_blocks(self, which, epochs, j0_limit, area, poisson, ta, tb):
            calls.append(("blocks",))
            return 100.0 * (1 + numpy.arange(3.0))[:, None] + numpy.arange(ta.size)[None, :]

        def covariance_ssc_blocks_range(self, n):
            calls.append(("range", n))
            return numpy.array([[0.1, 1.0, 10.0 * (b + 1), 1000.0] for b in range(3)])

        def covariance_ssc_blocks(self, epochs, lo, hi, limit, ln_chi, sigma2, area, ta, tb):
            calls.append(("ssc", list(epochs), lo, hi, limit, ln_chi, sigma2, area, ta, tb))
            return 0.25 * (1 + numpy.arange(3.0))[:, None] + 0.0 * ta[None, :]

    class Grid(object):
        def __init__(self, z, **kw):
            self.ctx = Ctx()

        def set_parameters(self, **kw):
            pass

        def setup(self, which, families=0):
            calls.append(("setup", which, families))

        def status(self):
            return numpy.zeros(2, dtype=numpy.uint32)
    monkeypatch.setattr(grid, "HaloGrid", Grid)
    monkeypatch.setattr(kernel.Kernel, "_setup_pairs_on", staticmethod(lambda ctx, kernels: ctx))
    corrs = [bare(), bare()]
    sig = []
    for c, z in zip(corrs, Z):
        c.halo._redshift = z
        c.kernel.cosmo.sigma_r = _Cosmo(1.0, sig).sigma_r     # (the MultiEpoch's, off the device)
    cm = multi(corrs, **SSC)
    w = cm.get_covariance_batched()
    assert [c[0] for c in calls] == ["setup", "blocks", "range", "ssc"]
    assert calls[0] == ("setup", "power_mm", _lib.FAM_SSC)
    assert calls[2] == ("range", 2)
    _, epochs, lo, hi, limit, ln_chi, sigma2, area, ta, tb = calls[3]
    first = cm.covariance_list[0][0]
    assert epochs == [0, 1]
    assert (lo, hi, limit) == (first.kernel.ln_ktheta_min, first.kernel.ln_ktheta_max,
                               first.kernel._j0_ssc_limit)
    assert area == first.area and ln_chi.shape == (3, npts) and sigma2.shape == (3, npts)
    assert len(sig) == 2                             # one sigma_r call per row
    centers = numpy.array([b.center for b in cm.annular_bins])
    iu = numpy.triu_indices(4)
    assert numpy.array_equal(ta, centers[iu[0]]) and numpy.array_equal(tb, centers[iu[1]])
    # block (0, 1): Gaussian 200 + p, super-sample 0.5, no Poisson diagonal
    want = numpy.zeros((4, 4))
    want[iu] = 200.0 + numpy.arange(10) + 0.5
    want[(iu[1], iu[0])] = want[iu]
    assert numpy.array_equal(cm.covariance_list[0][1].covar, want)
    assert numpy.array_equal(w[:4, 4:], want) and numpy.array_equal(w[4:, :4], want)
    assert numpy.array_equal(cm.blocks_ssc, 0.25 * (1 + numpy.arange(3.0))[:, None] * numpy.ones(10))
    # without ssc_cov the grid is set up as before: setup(which), no range, no second call
    del calls[:]
    plain = multi(corrs)
    plain.get_covariance_batched()
    assert calls == [("setup", "power_mm", 0), ("blocks",)] and plain.blocks_ssc is None


def test_halo_grid_setup_asks_for_further_families(monkeypatch):
    """HaloGrid.setup(which, families=...) adds families to those of the spectrum; without the
    argument the call builds what it built."""
    from chomp_amd import _lib, grid
    seen = []

    class Ctx(object):
        def epochs_set(self, *a, **k):
            pass

        def stage_k(self, halo, kind, profile, hod, need):
            seen.append(need)
    hg = grid.HaloGrid.__new__(grid.HaloGrid)
    hg.idx, hg.ctx, hg._delta_b, hg.kind = [0], Ctx(), None, _lib.MF_ST
    hg._c_cosmo = hg._c_halo = hg._c_hod = hg._z = None
    monkeypatch.setattr(grid.cosmology, "_de_kw", lambda c: {})
    hg.setup("power_mm")
    hg.setup("power_mm", families=_lib.FAM_SSC)
    hg.setup("power_gg", families=_lib.FAM_SSC)
    assert seen == [_lib.FAM_MM, _lib.FAM_MM | _lib.FAM_SSC, _lib.FAM_GG | _lib.FAM_SSC]
    assert hg._tables == _lib.FAM_GG | _lib.FAM_SSC


def test_the_knots_of_a_table_need_a_call_that_succeeded():
    """covariance_ssc_blocks_table and covariance_ng_blocks_table share one rule: the k_b knots are
    sized by the pairs of the last successful call, so knots=True before one raises, and the
    library is not called."""
    from chomp_amd import _lib

    def called(*args):
        raise AssertionError("the library was called")

    class L(object):
        chomp_covariance_ssc_blocks_table = chomp_covariance_ng_blocks_table = staticmethod(called)
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._L, ctx._h = L, None
    ctx.config = type("Config", (object,), {"kernel_npoints": 4})
    for term in ("ssc", "ng"):
        table = getattr(ctx, "covariance_%s_blocks_table" % term)
        with pytest.raises(_lib.ChompError) as e:
            table(0, knots=True)
        assert str(e.value) == "covariance_%s_blocks_table before covariance_%s_blocks" % (term, term)
        with pytest.raises(AssertionError, match="the library was called"):
            table(0)                                 # (without knots the C state decides)
