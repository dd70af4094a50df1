"""Host side of CovarianceMulti.get_covariance_batched / chomp_covariance_blocks: the C
declarations and their bindings, every refusal of the batch (before any device context exists),
the block order and the assembly of wcovar from a stubbed Context.covariance_blocks.  No device."""
import ctypes
import os
import re

import numpy
import pytest

from conftest import ROOT
from test_kernels_batch_cpu import KTHETA, _bare, _kernel, no_device  # noqa: F401

D2R = numpy.pi / 180.0
KWS = dict(bins_per_decade=2.0, survey_area_deg2=25.0, n_a=[1.0e10, 1.0e10],
           n_b=[1.0e10, 1.0e10], variance=1.0, nongaussian_cov=False)


def bare(h=None, kern=None):
    """A Correlation without its constructor's device work, with what Covariance reads."""
    from chomp_amd import halo
    corr = _bare(halo.Halo(0.0) if h is None else h, power_name="power_mm", kern=kern)
    corr.log_theta_min = numpy.log10(0.01 * D2R)
    corr.log_theta_max = numpy.log10(1.0 * D2R)
    return corr


def multi(corrs, **kws):
    from chomp_amd import covariance
    return covariance.CovarianceMulti(corrs, **dict(KWS, **kws))


def test_header_declares_the_entry_points_and_the_bindings_match():
    from chomp_amd import _lib, covariance
    with open(os.path.join(ROOT, "include", "chomp_mi355x.h")) as f:
        header = f.read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    decls = {
        "chomp_covariance_blocks":
            "int chomp_covariance_blocks(chomp_ctx* ctx, int which, size_t n_corr, "
            "const size_t* epoch , double j0_limit, double area, const double* poisson , "
            "const double* theta , size_t n_pairs, double* out , int mem);",
        "chomp_covariance_blocks_table":
            "int chomp_covariance_blocks_table(chomp_ctx* ctx, size_t block, double* ln_K, "
            "double* tables , double* levels , double* scalars , size_t n);"}
    for decl in decls.values():
        assert decl in flat, decl
    # (the shapes as the issue states them)
    spaced = re.sub(r"\s+", " ", header)
    assert "const double* poisson /*[n_blocks][4]*/" in spaced
    assert "const double* theta /*[2][n_pairs]: theta_a then theta_b*/" in spaced
    assert "double* out /*[n_blocks][n_pairs]*/" in spaced
    # the argtypes, from the declarations: arrays that follow `mem` travel as addresses
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    kinds = {"chomp_ctx*": [vp], "int": [ctypes.c_int], "size_t": [sz], "double": [ctypes.c_double],
             "const size_t*": [ctypes.POINTER(sz)], "const double*": [vp],
             "double*": [vp, _lib.c_double_p]}
    L = _lib.lib()
    for name, decl in decls.items():
        assert name in _lib.EXPORTS
        params = decl[decl.index("(") + 1:decl.rindex(")")].split(",")
        types = [p.strip().rsplit(" ", 1)[0].strip() for p in params]
        got = getattr(L, name).argtypes
        assert len(got) == len(types), name
        for t, g in zip(types, got):
            assert g in kinds[t], (name, t, g)
    assert L.chomp_covariance_blocks.argtypes[9] == vp            # out: host or device
    assert L.chomp_covariance_blocks_table.argtypes[2:6] == [_lib.c_double_p] * 4   # host only
    assert callable(_lib.Context.covariance_blocks)
    assert callable(_lib.Context.covariance_blocks_table)
    assert callable(covariance.CovarianceMulti.get_covariance_batched)


def _out_of_scope():
    """(label, CovarianceMulti) of every case get_covariance_batched refuses."""
    from chomp_amd import cosmology, defaults, halo, halo_trispectrum, hod, kernel
    cases = []
    tri = halo_trispectrum.HaloTrispectrumOneHalo.__new__(halo_trispectrum.HaloTrispectrumOneHalo)
    cases.append(("not the trispectrum (nongaussian_cov) or super-sample (ssc_cov) terms",
                  multi([bare()], nongaussian_cov=True, input_halo_trispectrum=tri)))
    cases.append(("poisson_noise_only needs no device", multi([bare()], poisson_noise_only=True)))

    class Other(kernel.Kernel):
        pass
    cases.append(("the kernel of correlation 1 is a Other, the batch takes kernel.Kernel",
                  multi([bare(), bare(kern=_kernel(Other))])))
    cases.append(("the kernel of correlation 0 is a GalaxyGalaxyLensingKernel",
                  multi([bare(kern=_kernel(kernel.GalaxyGalaxyLensingKernel)), bare()])))
    moved = _kernel()
    moved.z_bar = 0.4
    cases.append(("the kernel of correlation 1 has an assigned z_bar", multi([bare(), bare(kern=moved)])))
    z = numpy.linspace(0.0, 2.0, 17)
    tab = kernel.dNdzInterpolation(z, z * z * numpy.exp(-z / 0.3))
    cases.append(("correlation 1: window_function_b has a tabulated redshift distribution "
                  "(dNdzInterpolation)", multi([bare(), bare(kern=_kernel(dist_b=tab))])))
    de = dict(defaults.default_cosmo_dict, w0=-0.9, wa=0.1)
    cases.append(("the kernel of correlation 0 has a w0-wa cosmology",
                  multi([bare(kern=_kernel(cosmo=de))])))
    cases.append(("the kernel of correlation 1 has another k theta range",
                  multi([bare(), bare(kern=_kernel(ktheta=(KTHETA[0], 2.0 * KTHETA[1])))])))
    # what Correlation._hods_scope refuses
    fit = halo.HaloFit.__new__(halo.HaloFit)
    fit.__dict__.update(halo.Halo(0.0).__dict__)
    cases.append(("correlation 1: the halo is a HaloFit", multi([bare(), bare(fit)])))
    cases.append(("correlation 0: the halo is a HaloExclusion",
                  multi([bare(halo.HaloExclusion(0.0)), bare()])))
    cases.append(("correlation 1: a general_profile halo",
                  multi([bare(), bare(halo.Halo(0.0, general_profile=True))])))
    cases.append(("correlation 1: an extrapolated spectrum",
                  multi([bare(), bare(halo.Halo(0.0, extrapolate=True))])))
    h = halo.Halo(0.0, cosmo_single_epoch=cosmology.SingleEpoch(0.0, with_bao=True))
    cases.append(("correlation 0: a with_bao cosmology", multi([bare(h)])))
    h = halo.Halo(0.0)
    h.set_halo(dict(h.get_halo(), c0=7.5))
    cases.append(("correlation 1: the halo's profile and mass-function dictionaries differ",
                  multi([bare(), bare(h)])))
    cases.append(("the HOD of correlation 1 is a HOD",
                  multi([bare(), bare(halo.Halo(0.0, input_hod=hod.HOD({})))])))
    # halos that one HaloGrid does not hold
    other = dict(defaults.default_halo_dict, c0=7.5)
    cases.append(("the halo of correlation 1 has another halo dictionary or mass function",
                  multi([bare(), bare(halo.Halo(0.0, halo_dict=other))])))
    shared = halo.Halo(0.0)
    cases.append(("correlations 0 and 2 share one Halo object",
                  multi([bare(shared), bare(), bare(shared)])))
    # blocks that do not belong together
    cm = multi([bare(), bare()])
    cm.covariance_list[0][1].power_spec = "power_gg"
    cases.append(("the blocks' power_spec differ (power_gg, power_mm)", cm))
    wide = bare()
    wide.log_theta_max = numpy.log10(10.0 * D2R)
    cm = multi([bare(), bare()])
    from chomp_amd import covariance
    cm.covariance_list[1][0] = covariance.Covariance(wide, wide, **KWS)
    cases.append(("the blocks' angular bins or survey areas differ", cm))
    # what Covariance._check_cross refuses (here: made so after the blocks were built)
    cm = multi([bare(), bare()])
    cm.covariance_list[1][0].corr_a.kernel.cosmo.cosmo_dict = dict(
        defaults.default_cosmo_dict, sigma_8=0.9)
    cases.append(("Covariance of two correlations whose MultiEpoch cosmologies differ", cm))
    return cases


def test_get_covariance_batched_refuses_what_it_does_not_serve(no_device):  # noqa: F811
    from chomp_amd import _lib
    cases = _out_of_scope()
    assert len(cases) == 20
    for label, cm in cases:
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)) as info:
            cm.get_covariance_batched()
        assert str(info.value).startswith("get_covariance_batched: "), label
        assert str(info.value).endswith("; use get_covariance"), label
        assert not hasattr(cm, "_blocks_grid"), label


def test_block_order_and_assembly(monkeypatch):
    """The route of get_covariance_batched on a stubbed grid and context: the kernels staged in
    the order of the correlations, one epoch per correlation at its z_bar, the blocks of
    covariance_blocks in the order of covariance_list, their mirrors and the Poisson diagonal of
    the matching blocks in wcovar."""
    from chomp_amd import covariance, grid, kernel
    calls = []
    Z = numpy.array([0.3, 0.5, 0.7])
    words = numpy.array([0, 0, 0], dtype=numpy.uint32)

    class Ctx(object):
        def kernel_info_sets(self):
            calls.append(("info",))
            return {"z_bar": Z, "D_zbar": 1.0 / (1.0 + Z)}

        def covariance_blocks(self, which, epochs, j0_limit, area, poisson, ta, tb):
            calls.append(("blocks", which, list(epochs), j0_limit, area,
                          numpy.array(poisson), ta, tb))
            # block b, pair p: 100 (b + 1) + p
            return 100.0 * (1 + numpy.arange(6.0))[:, None] + numpy.arange(ta.size)[None, :]

    class Grid(object):
        def __init__(self, z, **kw):
            calls.append(("grid", len(z), kw))
            self.ctx = Ctx()

        def set_parameters(self, **kw):
            calls.append(("set", kw))

        def setup(self, which):
            calls.append(("setup", which))

        def status(self):
            return words
    monkeypatch.setattr(grid, "HaloGrid", Grid)
    monkeypatch.setattr(kernel.Kernel, "_setup_pairs_on",
                        staticmethod(lambda ctx, kernels: calls.append(("pairs", ctx, kernels))))
    corrs = [bare(), bare(), bare()]
    for c, z in zip(corrs, Z):
        c.halo._redshift = z             # (where the constructor leaves a halo: at z_bar)
    cm = multi(corrs)
    out, status = cm.get_covariance_batched(with_status=True)
    names = [c[0] for c in calls]
    assert names == ["grid", "pairs", "info", "set", "setup", "blocks"]
    assert calls[0][1] == 3 and calls[0][2]["mass_function"] == "st"
    assert calls[1][2] == [c.kernel for c in corrs]
    assert numpy.array_equal(calls[3][1]["z"], Z)
    assert calls[3][1]["hod"] == [c.halo.local_hod for c in corrs]
    assert calls[4][1] == "power_mm"
    _, which, epochs, j0, area, poisson, ta, tb = calls[5]
    first = cm.covariance_list[0][0]
    assert epochs == [0, 1, 2] and j0 == first._j0_limit and area == first.area
    assert poisson.shape == (6, 4) and not numpy.any(poisson)
    centers = numpy.array([b.center for b in cm.annular_bins])
    iu = numpy.triu_indices(4)
    assert numpy.array_equal(ta, centers[iu[0]]) and numpy.array_equal(tb, centers[iu[1]])
    assert status is words and cm.blocks_status is words and cm.blocks_z_bar is Z
    assert out is cm.wcovar and out.shape == (12, 12) and numpy.array_equal(out, out.T)
    b = 0
    for i in range(3):
        for j in range(i, 3):
            want = numpy.zeros((4, 4))
            want[iu] = 100.0 * (b + 1) + numpy.arange(10)
            want[(iu[1], iu[0])] = want[iu]
            cov = cm.covariance_list[i][j - i]
            if i == j:
                for q, ab in enumerate(cov.annular_bins):
                    P = cov.covariance_P(ab.delta, ab.center)
                    assert P > 0.0
                    want[q, q] += P
            assert numpy.array_equal(cov.covar, want), (i, j)
            assert numpy.array_equal(out[4 * i:4 * i + 4, 4 * j:4 * j + 4], want), (i, j)
            assert numpy.array_equal(out[4 * j:4 * j + 4, 4 * i:4 * i + 4], want), (i, j)
            b += 1
    # a second call keeps the grid
    del calls[:]
    cm.get_covariance_batched()
    assert [c[0] for c in calls] == ["pairs", "info", "set", "setup", "blocks"]
    # correlation 0's halo away from its z_bar: the loop's first block is evaluated there
    from chomp_amd import _lib
    corrs[0].halo._redshift = 0.0
    with pytest.raises(_lib.ChompScopeError, match="keep_halo_z_bar") as info:
        cm.get_covariance_batched()
    assert str(info.value).startswith("get_covariance_batched: ")
    assert str(info.value).endswith("use get_covariance")


def test_status_words_are_raised_naming_the_correlation(monkeypatch):
    from chomp_amd import _lib, grid, kernel

    class Ctx(object):
        def kernel_info_sets(self):
            return {"z_bar": numpy.zeros(2)}

        def covariance_blocks(self, which, epochs, j0_limit, area, poisson, ta, tb):
            return numpy.ones((3, ta.size))

    class Grid(object):
        def __init__(self, z, **kw):
            self.ctx = Ctx()

        def set_parameters(self, **kw):
            pass

        def setup(self, which):
            pass

        def status(self):
            return numpy.array([0, _lib.ST_SIGMA_DIVMAX], dtype=numpy.uint32)
    monkeypatch.setattr(grid, "HaloGrid", Grid)
    monkeypatch.setattr(kernel.Kernel, "_setup_pairs_on", staticmethod(lambda ctx, kernels: ctx))
    cm = multi([bare(), bare()])
    with pytest.warns(_lib.ChompAccuracyWarning, match="^correlation 1: "):
        cm.get_covariance_batched()
    assert list(cm.blocks_status) == [0, _lib.ST_SIGMA_DIVMAX]


def test_loop_is_assembled_as_before():
    """get_covariance() goes through the same assembly: block (i, j) and its mirror."""
    cm = multi([bare(), bare()])
    for b, cov in enumerate(c for row in cm.covariance_list for c in row):
        cov.get_covariance = lambda cov=cov, b=b: setattr(cov, "covar", numpy.full((4, 4), b + 1.0))
    w = cm.get_covariance()
    assert numpy.array_equal(w[:4, :4], numpy.full((4, 4), 1.0))
    assert numpy.array_equal(w[:4, 4:], numpy.full((4, 4), 2.0))
    assert numpy.array_equal(w[4:, :4], numpy.full((4, 4), 2.0))
    assert numpy.array_equal(w[4:, 4:], numpy.full((4, 4), 3.0))
