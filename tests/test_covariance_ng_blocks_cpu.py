"""Host side of the trispectrum term in CovarianceMulti.get_covariance_batched(trispectrum=True) /
chomp_covariance_ng_blocks: the C declarations and their bindings, what the batch's scope serves with the
keyword and what it refuses with and without it (before any device context exists), the plan of
the call -- its index block and the sizes of what it keeps on the device -- and the route of the
call on a stubbed grid and context.  No device."""
import ctypes
import os
import re

import numpy
import pytest

from conftest import ROOT
from test_covariance_blocks_cpu import D2R, bare, multi
from test_covariance_ssc_blocks_cpu import _disjoint_kernel
from test_kernels_batch_cpu import no_device  # noqa: F401

NG = dict(nongaussian_cov=True, cross_terms=True)
OLD_REFUSAL = ("get_covariance_batched: the batch serves the Gaussian and Poisson terms, not the "
               "trispectrum (nongaussian_cov) or super-sample (ssc_cov) terms; use get_covariance")


def tri_stub():
    """A HaloTrispectrumOneHalo without its constructor's device work, its I_0^4 table 'built'."""
    from chomp_amd import halo_trispectrum
    tri = halo_trispectrum.HaloTrispectrumOneHalo.__new__(halo_trispectrum.HaloTrispectrumOneHalo)
    tri._initialized_i_0_4 = True
    tri._i_0_4_array = numpy.arange(16.0).reshape(4, 4)
    tri._k_min, tri._k_max = 1e-3, 100.0
    return tri


def ng_multi(corrs, tri=None, **kws):
    return multi(corrs, input_halo_trispectrum=tri_stub() if tri is None else tri,
                 **dict(NG, **kws))


def test_header_declares_the_entry_points_and_the_bindings_match():
    from chomp_amd import _lib
    with open(os.path.join(ROOT, "include", "chomp_mi355x.h")) as f:
        header = f.read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    decls = {
        "chomp_covariance_ng_blocks":
            "int chomp_covariance_ng_blocks(chomp_ctx* ctx, size_t n_corr, const size_t* epoch , "
            "double ln_ktheta_min, double ln_ktheta_max, double j0_limit, double area, "
            "const double* tri_table, size_t n_tri, double tri_k_min, double tri_k_max, "
            "const double* theta , size_t n_pairs, double* out , int mem);",
        "chomp_covariance_ng_blocks_table":
            "int chomp_covariance_ng_blocks_table(chomp_ctx* ctx, size_t block, double* info , "
            "double* table, double* levels, double* table_min, double* kb_knots, "
            "double* kb_levels);",
        "chomp_covariance_ng_blocks_plan":
            "int chomp_covariance_ng_blocks_plan(size_t n_corr, const size_t* epoch , size_t n_pairs, "
            "size_t n_ktheta, size_t n_k, size_t n_tri, size_t* sizes , int* index );"}
    for decl in decls.values():
        assert decl in flat, decl
    spaced = re.sub(r"\s+", " ", header)
    assert "const size_t* epoch /*[n_corr] or NULL*/" in spaced
    assert "const double* theta /*[2][n_pairs]*/" in spaced
    assert "double* out /*[n_blocks][n_pairs]*/" in spaced
    assert "double* info /*[7]*/" in spaced
    # the argtypes, from the declarations: arrays that follow `mem` travel as addresses
    vp, sz, dp = ctypes.c_void_p, ctypes.c_size_t, _lib.c_double_p
    kinds = {"chomp_ctx*": [vp], "int": [ctypes.c_int], "size_t": [sz], "double": [ctypes.c_double],
             "const size_t*": [ctypes.POINTER(sz)], "size_t*": [ctypes.POINTER(sz)],
             "int*": [ctypes.POINTER(ctypes.c_int)], "const double*": [vp, dp], "double*": [vp, dp]}
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
        assert getattr(L, name).restype is ctypes.c_int
    at = L.chomp_covariance_ng_blocks.argtypes
    assert at[7] == dp                                  # tri_table: host only
    assert at[11] == vp and at[13] == vp                # theta, out: host or device
    assert L.chomp_covariance_ng_blocks_table.argtypes[2:] == [dp] * 6
    for name in ("covariance_ng_blocks", "covariance_ng_blocks_table"):
        assert callable(getattr(_lib.Context, name))
    # a null context is CHOMP_ERR_ARG, with no message to write
    for name in ("chomp_covariance_ng_blocks", "chomp_covariance_ng_blocks_table"):
        fn = getattr(L, name)
        args = [0.0 if t is ctypes.c_double else 0 if t in (ctypes.c_int, sz) else None
                for t in fn.argtypes]
        assert fn(*args) == _lib.ERR_ARG, name


def _slab(N):
    """NgLayout of N knots a side, in doubles: scalars 16 | ln k theta knots N | table, levels,
    log(table - 10 min) N^2 each | bicubic 16 (N - 1)^2 | row pieces 4 (N - 1) N | the build's
    scratch 4 (N - 1) 6 N; rounded up to 8."""
    o = 16 + N + 3 * N * N + 16 * (N - 1) ** 2 + 4 * (N - 1) * N + 24 * (N - 1) * N
    return (o + 7) // 8 * 8


def _tri(N):
    """NgTriLayout: ln k knots | table | bicubic | row pieces | scratch; rounded up to 8."""
    o = N + N * N + 16 * (N - 1) ** 2 + 4 * (N - 1) * N + 24 * (N - 1) * N
    return (o + 7) // 8 * 8


@pytest.mark.parametrize("n_corr,n_pairs", [(1, 10), (3, 10), (15, 55)])
def test_plan_index_block_and_sizes(n_corr, n_pairs):
    from chomp_amd import _lib
    n_blocks = n_corr * (n_corr + 1) // 2
    sizes, index = _lib.covariance_ng_blocks_plan(n_corr, n_pairs, 50, 50, 50)
    assert sizes == dict(n_blocks=n_blocks, slab=_slab(50), slabs=n_blocks * _slab(50),
                         kb=2 * n_blocks * n_pairs * 50, tri=_tri(50), index=n_corr + 3 * n_blocks)
    assert _slab(50) == 114584 and index.size == sizes["index"] and index.dtype == numpy.intc
    # epoch | (i, j) in the row-major order of the upper triangle | diagonal | cross
    assert list(index[:n_corr]) == list(range(n_corr))
    pairs = [(i, j) for i in range(n_corr) for j in range(i, n_corr)]
    assert [tuple(p) for p in index[n_corr:n_corr + 2 * n_blocks].reshape(-1, 2)] == pairs
    diag = list(index[n_corr + 2 * n_blocks:2 * n_corr + 2 * n_blocks])
    cross = list(index[2 * n_corr + 2 * n_blocks:])
    assert diag == [b for b, (i, j) in enumerate(pairs) if i == j] and len(diag) == n_corr
    assert cross == [b for b, (i, j) in enumerate(pairs) if i != j]
    assert sorted(diag + cross) == list(range(n_blocks))
    # every slab, k_b row and index entry of the launches lies inside what is kept
    assert (n_blocks - 1) * sizes["slab"] + sizes["slab"] <= sizes["slabs"]
    assert (2 * n_blocks - 1) * n_pairs * 50 + n_pairs * 50 <= sizes["kb"]
    # the caller's epochs, and other sizes
    ep = numpy.arange(n_corr)[::-1] + 2
    sizes2, index2 = _lib.covariance_ng_blocks_plan(n_corr, 3, 20, 30, 8, epochs=ep)
    assert list(index2[:n_corr]) == list(ep) and numpy.array_equal(index2[n_corr:], index[n_corr:])
    assert sizes2 == dict(n_blocks=n_blocks, slab=_slab(20), slabs=n_blocks * _slab(20),
                          kb=2 * n_blocks * 3 * 30, tri=_tri(8), index=index.size)


def test_plan_refuses_what_the_call_refuses():
    from chomp_amd import _lib
    for args in ((0, 10, 50, 50, 50), (3, 0, 50, 50, 50), (3, 65536, 50, 50, 50), (3, 10, 3, 50, 50),
                 (3, 10, 50, 257, 50), (3, 10, 50, 50, 3), (3, 10, 50, 50, 65), (1025, 10, 50, 50, 50),
                 (362, 10, 50, 50, 50)):                  # (362 * 363 / 2 = 65703 blocks)
        with pytest.raises(ValueError, match="covariance_ng_blocks_plan"):
            _lib.covariance_ng_blocks_plan(*args)
    assert _lib.covariance_ng_blocks_plan(361, 10, 50, 50, 50)[0]["n_blocks"] == 65341
    with pytest.raises(ValueError, match=r"epochs must be \[n_corr\]"):
        _lib.covariance_ng_blocks_plan(3, 10, 50, 50, 50, epochs=[0, 1])


def test_scope_serves_the_trispectrum_blocks_with_the_keyword(no_device):  # noqa: F811
    tri = tri_stub()
    for cm, n in ((ng_multi([bare()], tri, cross_terms=False), 1), (ng_multi([bare(), bare()], tri), 2),
                  (ng_multi([bare(), bare(), bare()], tri, ssc_cov=True), 3)):
        corrs, name = cm._batched_scope(trispectrum=True)
        assert len(corrs) == n and name == "power_mm"
        assert corrs == [row[0].corr_a for row in cm.covariance_list]
        assert all(cov.halo_tri is tri for row in cm.covariance_list for cov in row)
    # the keyword with Gaussian blocks changes nothing
    cm = multi([bare(), bare()])
    assert cm._batched_scope(trispectrum=True)[1] == cm._batched_scope()[1] == "power_mm"


def test_scope_refuses(no_device):  # noqa: F811
    from chomp_amd import _lib
    # without the keyword (or with trispectrum=False): the words the refusal always had
    for kws in (dict(cross_terms=False), dict(cross_terms=False, ssc_cov=True), dict(ssc_cov=True)):
        cm = ng_multi([bare()] if not kws.get("cross_terms", True) else [bare(), bare()], **kws)
        for call in (cm.get_covariance_batched, lambda: cm.get_covariance_batched(trispectrum=False),
                     cm._batched_scope):
            with pytest.raises(_lib.ChompScopeError) as info:
                call()
            assert str(info.value) == OLD_REFUSAL
        assert not hasattr(cm, "_blocks_grid")
    cases = []
    cm = ng_multi([bare(), bare()])
    cm.covariance_list[1][0].nongaussian_cov = False
    cases.append(("the blocks differ in nongaussian_cov: the batch adds the trispectrum term to "
                  "every block or to none", cm))
    cm = multi([bare(), bare()])
    cm.covariance_list[0][1].nongaussian_cov = True
    cases.append(("the blocks differ in nongaussian_cov", cm))
    cm = ng_multi([bare(), bare()])
    cm.covariance_list[0][1].halo_tri = tri_stub()
    cases.append(("the blocks do not share one halo_tri object", cm))
    cm = ng_multi([bare(), bare()])
    cm.covariance_list[0][1].kernel.ln_ktheta_min -= 1.0
    cases.append(("block (0, 1): its KernelCovariance has another k theta range or J0 limit than "
                  "that of block (0, 0)", cm))
    cm = ng_multi([bare(), bare()])
    cm.covariance_list[1][0].kernel._j0_limit += 1.0
    cases.append(("block (1, 1): its KernelCovariance has another k theta range or J0 limit", cm))
    # (the super-sample J0 limit is not the trispectrum term's: it may differ without ssc_cov)
    cm = ng_multi([bare(), bare()])
    cm.covariance_list[1][0].kernel._j0_ssc_limit += 1.0
    assert cm._batched_scope(trispectrum=True)[1] == "power_mm"
    cm = ng_multi([bare(), bare()], ssc_cov=True)
    cm.covariance_list[1][0].kernel._j0_ssc_limit += 1.0
    cases.append(("block (1, 1): its KernelCovariance has another k theta range or J0 limit", cm))
    cm = ng_multi([bare(), bare(kern=_disjoint_kernel(True)), bare(kern=_disjoint_kernel(False))])
    cases.append(("block (1, 2): the four windows have no redshift in common (z_min = 0.5 >= "
                  "z_max = 0.5", cm))
    # everything else the scope refused stays refused with the term
    cases.append(("poisson_noise_only needs no device",
                  ng_multi([bare(), bare()], poisson_noise_only=True)))
    from chomp_amd import halo
    shared = halo.Halo(0.0)
    cases.append(("correlations 0 and 1 share one Halo object",
                  ng_multi([bare(shared), bare(shared)])))
    wide = bare()
    wide.log_theta_max = numpy.log10(10.0 * D2R)
    cases.append(("the blocks' angular bins or survey areas differ", ng_multi([bare(), wide])))
    for label, cm in cases:
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)) as info:
            cm.get_covariance_batched(trispectrum=True)
        assert str(info.value).startswith("get_covariance_batched: "), label
        assert str(info.value).endswith("; use get_covariance"), label
        assert not hasattr(cm, "_blocks_grid"), label


def test_route_of_the_batch_with_the_trispectrum_term(monkeypatch):
    """On a stubbed grid and context: the I_0^4 table is built if it was not, one
    covariance_ng_blocks call gets block (0, 0)'s k theta range, _j0_limit, the area and the
    table, no range is read back, and the values are added Gaussian + trispectrum + super-sample."""
    from chomp_amd import _lib, grid, kernel
    calls = []
    Z = numpy.array([0.3, 0.5])

    class Ctx(object):
        def kernel_info_sets(self):
            return {"z_bar": Z}

        def covariance_blocks(self, which, epochs, j0_limit, area, poisson, ta, tb):
            calls.append(("blocks",))
            return 100.0 * (1 + numpy.arange(3.0))[:, None] + numpy.arange(ta.size)[None, :]

        def covariance_ng_blocks(self, epochs, lo, hi, limit, area, table, k_min, k_max, ta, tb):
            calls.append(("ng", list(epochs), lo, hi, limit, area, table, k_min, k_max, ta, tb))
            return 0.5 * (1 + numpy.arange(3.0))[:, None] + 0.0 * ta[None, :]

        def covariance_ssc_blocks_range(self, n):
            calls.append(("range", n))
            return numpy.array([[0.1, 1.0, 10.0 * (b + 1), 1000.0] for b in range(3)])

        def covariance_ssc_blocks(self, epochs, lo, hi, limit, ln_chi, sigma2, area, ta, tb):
            calls.append(("ssc", limit))
            return 0.0625 * (1 + numpy.arange(3.0))[:, None] + 0.0 * ta[None, :]

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
    for c, z in zip(corrs, Z):
        c.halo._redshift = z
        c.kernel.cosmo.sigma_r = lambda chi, z: 1.0 + 0.0 * numpy.asarray(chi)
    tri = tri_stub()
    tri._initialized_i_0_4 = False
    built = []

    def initialize():
        built.append(1)
        tri._initialized_i_0_4 = True
    tri._initialize_i_0_4 = initialize
    cm = ng_multi(corrs, tri)
    w = cm.get_covariance_batched(trispectrum=True)
    assert built == [1]
    assert [c[0] for c in calls] == ["setup", "blocks", "ng"]
    assert calls[0] == ("setup", "power_mm", 0)
    _, epochs, lo, hi, limit, area, table, k_min, k_max, ta, tb = calls[2]
    first = cm.covariance_list[0][0]
    assert epochs == [0, 1]
    assert (lo, hi, limit) == (first.kernel.ln_ktheta_min, first.kernel.ln_ktheta_max,
                               first.kernel._j0_limit)
    assert limit != first.kernel._j0_ssc_limit
    assert area == first.area and table is tri._i_0_4_array and (k_min, k_max) == (1e-3, 100.0)
    centers = numpy.array([b.center for b in cm.annular_bins])
    iu = numpy.triu_indices(4)
    assert numpy.array_equal(ta, centers[iu[0]]) and numpy.array_equal(tb, centers[iu[1]])
    # block (0, 1): Gaussian 200 + p, trispectrum 1.0, no Poisson diagonal
    want = numpy.zeros((4, 4))
    want[iu] = 200.0 + numpy.arange(10) + 1.0
    want[(iu[1], iu[0])] = want[iu]
    assert numpy.array_equal(cm.covariance_list[0][1].covar, want)
    assert numpy.array_equal(w[:4, 4:], want) and numpy.array_equal(w[4:, :4], want)
    assert numpy.array_equal(cm.blocks_ng, 0.5 * (1 + numpy.arange(3.0))[:, None] * numpy.ones(10))
    assert cm.blocks_ssc is None
    # a second call builds no table again; all three terms: Gaussian, trispectrum, super-sample
    del calls[:]
    both = ng_multi(corrs, tri, ssc_cov=True)
    w = both.get_covariance_batched(trispectrum=True)
    assert built == [1]
    assert [c[0] for c in calls] == ["setup", "blocks", "ng", "range", "ssc"]
    assert calls[0] == ("setup", "power_mm", _lib.FAM_SSC)
    assert calls[4] == ("ssc", first.kernel._j0_ssc_limit)
    want[iu] = (200.0 + numpy.arange(10) + 1.0) + 0.125
    want[(iu[1], iu[0])] = want[iu]
    assert numpy.array_equal(w[:4, 4:], want)
    # without the term: as before, and blocks_ng is None
    del calls[:]
    plain = multi(corrs)
    plain.get_covariance_batched(trispectrum=True)
    assert calls == [("setup", "power_mm", 0), ("blocks",)]
    assert plain.blocks_ng is None and plain.blocks_ssc is None
