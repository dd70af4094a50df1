"""G30: the trispectrum and super-sample terms of a cross block on the MI355X (pytest -m gpu) --
Covariance(corr_a, corr_b, nongaussian_cov=True, ssc_cov=True, cross_terms=True) on
KernelCovariance(four_windows=True) -- against the reference's own numbers
(tests/golden/make_golden_cov_cross_terms.py) and the NumPy restatement of
test_covariance_cross_terms_cpu.

Bars: the project's existing ones.  RTOL_KERNEL, relative to the table's scale, for tables, raw
values, spline values and k_b knots; RTOL_COV per element for covariance_NG, covariance_ssc,
covariance_G and the full matrix.  Every knot and every pair counts."""
import copy

import numpy
import pytest

from conftest import load_golden, rel_err
from test_covariance_cross_terms_cpu import SWAPPED, four_state
from test_gpu_covariance_cross import KWS, correlations as g29_correlations
from test_gpu_covariance_ssc import scaled_err

pytestmark = pytest.mark.gpu

RTOL_COV = 1e-4          # the G12 bar, per element
RTOL_KERNEL = 1e-5       # kernel_precision 1.48e-6 of the integrals, relative to the table's scale
D2R = numpy.pi / 180.0
Z_TRI = 0.5


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from chomp_amd import _lib
    _lib.lib()
    return _lib


def correlations(tag, z0_b=None):
    """The fixture's pairs: "wide" MagLim galaxy x convergence against a galaxy Gaussian on
    z = 0-1.5; "gal" G29's; "far" G29's "mix" windows; each correlation on its own Halo(0.0)."""
    from chomp_amd import correlation, cosmology, halo, kernel
    if tag == "gal":
        return g29_correlations("gal") if z0_b is None else g29_correlations("gal", z0_b=z0_b)
    cm = cosmology.MultiEpoch(0.0, 5.0)

    def corr(wa, wb):
        kern = kernel.Kernel(1e-6 * D2R, 100.0 * D2R, wa, wb, cm)
        return correlation.Correlation(0.01, 1.0, kern, input_halo=halo.Halo(0.0),
                                       power_spec="power_mm")
    wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0))
    wb = kernel.WindowFunctionConvergence(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2))
    if tag == "wide":
        wc = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 1.5, 0.7, 0.2))
    else:
        wc = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.5, 1.5, 1.0, 0.2))
    return corr(wa, wb), corr(wc, wc)


def tri_object():
    from chomp_amd import halo_trispectrum
    return halo_trispectrum.HaloTrispectrumOneHalo(Z_TRI)


def block(tag, ng=True, ssc=True, **kws):
    from chomp_amd import covariance
    ca, cb = correlations(tag, **kws)
    return covariance.Covariance(ca, cb, nongaussian_cov=ng, ssc_cov=ssc, cross_terms=True,
                                 input_halo_trispectrum=tri_object() if ng else None, **KWS)


def pair_err(got, ref):
    return float(numpy.max(numpy.abs(numpy.asarray(got) / numpy.asarray(ref) - 1.0)))


@pytest.mark.parametrize("tag", ["wide", "gal"])
def test_g30_cross_block(lib, tag):
    g = load_golden("g30_covariance_cross_terms")
    cv = block(tag)
    kc = cv.kernel
    sc = g[tag + "_scalars"]
    assert cv.matching_corrs is False and kc._four_windows
    print(tag, "z_bar_NG", kc.z_bar_NG, "D", cv.D_z_NG / sc[1] - 1, "chi", kc.chi_min / sc[2] - 1,
          kc.chi_max / sc[3] - 1)
    assert kc.z_bar_NG == sc[0]                                  # the argmax index, exactly
    assert abs(cv.D_z_NG / sc[1] - 1.0) < 1e-10
    assert abs(kc.chi_min / sc[2] - 1.0) < 1e-9 and abs(kc.chi_max / sc[3] - 1.0) < 1e-9
    assert (kc.ln_ktheta_min, kc.ln_ktheta_max) == (sc[4], sc[5])
    assert (kc._j0_limit, kc._j0_ssc_limit, kc._j1_limit) == (sc[6], sc[7], sc[8])
    assert cv.area == sc[9] and (kc.z_min, kc.z_max) == (sc[10], sc[11])
    assert numpy.array_equal(kc._ln_ktheta_array, g[tag + "_ln_ktheta"])
    assert numpy.max(numpy.abs(kc._sigma2_ln_chi - g[tag + "_sigma2_ln_chi"])) < 1e-12
    assert rel_err(kc._sigma2_knots, g[tag + "_sigma2"]) < 1e-8
    a, b = g[tag + "_probe_a"], g[tag + "_probe_b"]
    kt = four_state(tag)
    for name, got, raw_fn, eval_fn, levels, restated in (
            ("ssc", kc._kernel_ssc_array, kc.raw_kernel_ssc, kc.kernel_ssc,
             kc._kernel_ssc_levels, kt.raw_kernel_ssc),
            ("ng", kc._kernel_array, kc.raw_kernel_NG, kc.kernel_NG, kc._kernel_levels,
             kt.raw_kernel_NG)):
        tab = g[tag + ("_kernel_ssc_array" if name == "ssc" else "_kernel_array")]
        scale = numpy.max(numpy.abs(tab))
        assert got.shape == (50, 50) and numpy.array_equal(got, got.T)
        assert numpy.array_equal(levels, levels.T)
        raw = raw_fn(a, b)
        spl = numpy.array([eval_fn(x, y)[0][0] for x, y in zip(a, b)])
        errs = (scaled_err(got, tab), numpy.max(numpy.abs(raw - g[tag + "_%s_raw" % name])) / scale,
                numpy.max(numpy.abs(spl - g[tag + "_%s_spline" % name])) / scale)
        print(tag, name, "table, raw, spline errors / scale", errs)
        assert max(errs) < RTOL_KERNEL
        assert numpy.array_equal(spl == 0.0, g[tag + "_%s_spline" % name] == 0.0)   # the zero rule
        for i, j in ((0, 0), (9, 37), (24, 49), (49, 49)):
            assert levels[i, j] == restated(kt.ln_kt[i], kt.ln_kt[j])[1], (name, i, j)
    scale = numpy.max(numpy.abs(g[tag + "_kernel_array"]))
    assert abs(kc._kernel_NG_min - g[tag + "_kernel_NG_min"][0]) < RTOL_KERNEL * scale
    # the three terms at all pairs i <= j and at the swapped pairs (3, 0), (2, 1)
    c = numpy.array([x.center for x in cv.annular_bins])
    assert numpy.array_equal(c, g[tag + "_center"])
    pairs = g[tag + "_pairs"]
    ta, tb = c[pairs[:, 0]], c[pairs[:, 1]]
    G = cv.covariance_G(ta, tb)
    NG = cv.covariance_NG(ta, tb)
    ssc = cv.covariance_ssc(ta, tb)
    errs = (pair_err(G, g[tag + "_G"]), pair_err(NG, g[tag + "_NG"]), pair_err(ssc, g[tag + "_ssc"]))
    print(tag, "covariance_G, _NG, _ssc errors", errs)
    assert max(errs) < RTOL_COV
    plist = [tuple(p) for p in pairs]
    for i, j in SWAPPED:                     # a and b are not interchanged: each its own value
        p, q = plist.index((i, j)), plist.index((j, i))
        assert abs(NG[p] / NG[q] - 1.0) > 2 * RTOL_COV and abs(ssc[p] / ssc[q] - 1.0) > 2 * RTOL_COV
        assert abs(NG[p] / g[tag + "_NG"][q] - 1.0) > RTOL_COV
        assert abs(ssc[p] / g[tag + "_ssc"][q] - 1.0) > RTOL_COV
    # one pair at a time: bit for bit the batched values
    for p in (3, len(plist) - 2):
        assert cv.covariance_NG(ta[p], tb[p]) == NG[p]
        assert cv.covariance_ssc(ta[p], tb[p]) == ssc[p]
    # the k_b knots of one pair
    _, knots, _ = cv._covariance_NG_pairs(c[:1], c[-1:], knots=True)
    ref = g[tag + "_ng_kb_knots"]
    e_ng = numpy.max(numpy.abs(knots[0] - ref)) / numpy.max(numpy.abs(ref))
    _, knots, _ = cv._covariance_ssc_pairs(c[:1], c[-1:], knots=True)
    ref = g[tag + "_ssc_kb_knots"]
    e_ssc = numpy.max(numpy.abs(knots[0] - ref)) / numpy.max(numpy.abs(ref))
    print(tag, "k_b knots errors / scale: NG", e_ng, "ssc", e_ssc)
    assert max(e_ng, e_ssc) < RTOL_KERNEL
    full = cv.get_covariance()
    assert full.shape == (4, 4) and numpy.array_equal(full, full.T)
    print(tag, "get_covariance error", rel_err(full, g[tag + "_cov"]))
    assert rel_err(full, g[tag + "_cov"]) < RTOL_COV


def test_g30_far(lib):
    """The common range starts at z = 0.5: kernel_ssc is identically 0 and covariance_ssc NaN,
    as in the reference; the trispectrum term is within the bars."""
    g = load_golden("g30_covariance_cross_terms")
    cv = block("far")
    kc = cv.kernel
    sc = g["far_scalars"]
    assert kc.z_bar_NG == sc[0] and abs(cv.D_z_NG / sc[1] - 1.0) < 1e-10
    assert (kc.z_min, kc.z_max) == (sc[10], sc[11])
    assert numpy.all(kc._kernel_ssc_array == 0.0)
    a, b = g["far_probe_a"], g["far_probe_b"]
    assert numpy.all(kc.raw_kernel_ssc(a, b) == 0.0)
    tab = g["far_kernel_array"]
    scale = numpy.max(numpy.abs(tab))
    spl = numpy.array([kc.kernel_NG(x, y)[0][0] for x, y in zip(a, b)])
    errs = (scaled_err(kc._kernel_array, tab),
            numpy.max(numpy.abs(kc.raw_kernel_NG(a, b) - g["far_ng_raw"])) / scale,
            numpy.max(numpy.abs(spl - g["far_ng_spline"])) / scale)
    print("far NG table, raw, spline errors / scale", errs)
    assert max(errs) < RTOL_KERNEL
    assert abs(kc._kernel_NG_min - g["far_kernel_NG_min"][0]) < RTOL_KERNEL * scale
    c = numpy.array([x.center for x in cv.annular_bins])
    pairs = g["far_ng_pairs"]
    NG = cv.covariance_NG(c[pairs[:, 0]], c[pairs[:, 1]])
    print("far covariance_NG error", pair_err(NG, g["far_NG"]))
    assert pair_err(NG, g["far_NG"]) < RTOL_COV
    _, knots, _ = cv._covariance_NG_pairs(c[:1], c[-1:], knots=True)
    ref = g["far_ng_kb_knots"]
    assert numpy.max(numpy.abs(knots[0] - ref)) < RTOL_KERNEL * numpy.max(numpy.abs(ref))
    pairs = g["far_pairs"]
    G = cv.covariance_G(c[pairs[:, 0]], c[pairs[:, 1]])
    assert pair_err(G, g["far_G"]) < RTOL_COV
    p = g["far_ssc_pairs"]
    ssc = cv.covariance_ssc(c[p[:, 0]], c[p[:, 1]])
    assert numpy.array_equal(numpy.isnan(ssc), numpy.isnan(g["far_ssc"])) and numpy.all(numpy.isnan(ssc))
    full = block("far", ng=False).get_covariance()
    assert numpy.array_equal(numpy.isnan(full), numpy.isnan(g["far_cov"]))


def test_cross_path_agrees_with_matching_path(lib):
    """A correlation and a copy.copy of it: the four-window tables and all three terms are the
    matching path's."""
    from chomp_amd import covariance
    ca = g29_correlations("mix", only_a=True)
    kws = dict(KWS, nongaussian_cov=True, ssc_cov=True)
    same = covariance.Covariance(ca, ca, input_halo_trispectrum=tri_object(), **kws)
    cv = covariance.Covariance(ca, copy.copy(ca), input_halo_trispectrum=tri_object(),
                               cross_terms=True, **kws)
    assert cv.matching_corrs is False and cv.kernel._four_windows and not same.kernel._four_windows
    assert cv.kernel.z_bar_NG == same.kernel.z_bar_NG and cv.D_z_NG == same.D_z_NG
    errs = (scaled_err(cv.kernel._kernel_ssc_array, same.kernel._kernel_ssc_array),
            scaled_err(cv.kernel._kernel_array, same.kernel._kernel_array))
    print("cross vs matching tables (ssc, NG)", errs)
    assert max(errs) < RTOL_KERNEL
    c = numpy.array([x.center for x in cv.annular_bins])
    iu = numpy.triu_indices(len(c))
    ta, tb = c[iu[0]], c[iu[1]]
    errs = (pair_err(cv.covariance_G(ta, tb), same.covariance_G(ta, tb)),
            pair_err(cv.covariance_NG(ta, tb), same.covariance_NG(ta, tb)),
            pair_err(cv.covariance_ssc(ta, tb), same.covariance_ssc(ta, tb)))
    print("cross vs matching covariance_G, _NG, _ssc", errs)
    assert max(errs) < RTOL_COV


def test_covariance_multi_with_both_terms(lib):
    from chomp_amd import covariance
    ca, cb = correlations("gal")
    tri = tri_object()
    kws = dict(KWS, nongaussian_cov=True, ssc_cov=True, cross_terms=True,
               input_halo_trispectrum=tri)
    cm = covariance.CovarianceMulti([ca, cb], **kws)
    w = cm.get_covariance()
    assert w.shape == (8, 8) and numpy.array_equal(w, w.T) and numpy.all(numpy.isfinite(w))
    blocks = {(0, 0): (ca, ca), (0, 1): (ca, cb), (1, 1): (cb, cb)}
    for (i, j), (x, y) in blocks.items():
        one = covariance.Covariance(x, y, **kws).get_covariance()
        err = rel_err(w[4 * i:4 * i + 4, 4 * j:4 * j + 4], one)
        print("block", i, j, "against the block built alone", err)
        assert err < 1e-12
        assert numpy.array_equal(w[4 * j:4 * j + 4, 4 * i:4 * i + 4],
                                 w[4 * i:4 * i + 4, 4 * j:4 * j + 4])       # mirrored as it is
    g = load_golden("g30_covariance_cross_terms")
    assert rel_err(w[:4, 4:], g["gal_cov"]) < RTOL_COV


def test_cross_terms_follow_corr_b(lib):
    """After a first evaluation a change of corr_b's redshift window moves the trispectrum and
    super-sample terms of the block, to what a block built from such correlations holds."""
    cv = block("gal")
    first = cv.get_covariance().copy()
    ng0, ssc0 = cv.covariance_NG(0.001, 0.002), cv.covariance_ssc(0.001, 0.002)
    tab = cv.kernel._kernel_array
    assert cv.kernel._kernel_array is tab                          # nothing changed: kept
    cv.corr_b.kernel.window_function_a._redshift_dist.z0 = 0.9       # (one object: both windows)
    ng1, ssc1 = cv.covariance_NG(0.001, 0.002), cv.covariance_ssc(0.001, 0.002)
    assert abs(ng1 / ng0 - 1) > 1e-3 and abs(ssc1 / ssc0 - 1) > 1e-3
    fresh = block("gal", z0_b=0.9)
    assert cv.kernel.z_bar_NG == fresh.kernel.z_bar_NG
    errs = (abs(ng1 / fresh.covariance_NG(0.001, 0.002) - 1),
            abs(ssc1 / fresh.covariance_ssc(0.001, 0.002) - 1))
    print("moved block against a fresh one: NG, ssc", errs)
    assert max(errs) < 1e-12
    assert rel_err(cv.get_covariance(), fresh.get_covariance()) < 1e-12
    assert rel_err(first, cv.covar) > 1e-3


def test_cross_terms_follow_corr_b_hod(lib):
    """... and a change of corr_b's HOD: the HaloSuperSampleCovariance copy of that side shares the
    HOD object and would keep the tables of the old one; it is made again, and the block holds
    what one built from such correlations holds."""
    from chomp_amd import covariance
    from params import hod_dict_2
    kws = dict(KWS, nongaussian_cov=True, ssc_cov=True, cross_terms=True, power_spec="power_gg")
    ca, cb = g29_correlations("gal", "power_gg")
    cv = covariance.Covariance(ca, cb, input_halo_trispectrum=tri_object(), **kws)
    first = cv.get_covariance().copy()
    copy_a, copy_b = cv.halo_a, cv.halo_b
    cb.set_hod(hod_dict_2)
    moved = cv.get_covariance().copy()
    assert cv.halo_a is copy_a and cv.halo_b is not copy_b          # b's side alone
    assert rel_err(moved, first) > 1e-3
    fa, fb = g29_correlations("gal", "power_gg")
    fb.set_hod(hod_dict_2)
    fresh = covariance.Covariance(fa, fb, input_halo_trispectrum=tri_object(), **kws)
    err = rel_err(moved, fresh.get_covariance())
    print("HOD of corr_b changed: block against a fresh one", err)
    assert err < 1e-12


def test_kernel_covariance_with_four_windows_alone(lib):
    """KernelCovariance(four_windows=True) outside a Covariance: the two pairs of windows are
    staged from two Kernels of its own, projection set-ups alone (CHOMP_CROSS_WINDOWS), and the
    state and the raw kernels are G30's "wide"."""
    from chomp_amd import covariance
    g = load_golden("g30_covariance_cross_terms")
    sc = g["wide_scalars"]
    ca, cb = correlations("wide")
    ka, kb = ca.kernel, cb.kernel
    kc = covariance.KernelCovariance(
        numpy.exp(sc[4]), numpy.exp(sc[5]), ka.window_function_a, ka.window_function_b,
        kb.window_function_a, kb.window_function_b, ka.cosmo, trispectrum_kernel=True,
        four_windows=True)
    assert kc.z_bar_NG == sc[0]
    assert abs(kc._D_z_NG / sc[1] - 1.0) < 1e-10
    assert abs(kc.chi_min / sc[2] - 1.0) < 1e-9 and abs(kc.chi_max / sc[3] - 1.0) < 1e-9
    a, b = g["wide_probe_a"], g["wide_probe_b"]
    e_ssc = numpy.max(numpy.abs(kc.raw_kernel_ssc(a, b) - g["wide_ssc_raw"])) / \
        numpy.max(numpy.abs(g["wide_kernel_ssc_array"]))
    e_ng = numpy.max(numpy.abs(kc.raw_kernel_NG(a, b) - g["wide_ng_raw"])) / \
        numpy.max(numpy.abs(g["wide_kernel_array"]))
    print("stand-alone raw_kernel_ssc, raw_kernel_NG errors / scale", e_ssc, e_ng)
    assert max(e_ssc, e_ng) < RTOL_KERNEL
    x = kc._ln_ktheta_array[[3, 20, 41]]
    got = kc.kernel_ssc(x, x)
    ref = g["wide_kernel_ssc_array"][numpy.ix_([3, 20, 41], [3, 20, 41])]
    assert scaled_err(got, ref) < RTOL_KERNEL
    # slots that hold windows only serve the kernels, not the block's projected spectra
    ctx, _ = kc._stage_own()
    with pytest.raises(lib.ChompError, match="windows only"):
        ctx.covariance_table_cross(1.0, 1.0)


def test_windows_with_no_common_redshift_are_refused_by_the_library(lib):
    """The C API's own refusal (Python's comes first for a KernelCovariance): two staged sides
    whose windows share no redshift are CHOMP_ERR_SCOPE, before any launch."""
    from chomp_amd import cosmology, kernel
    cm = cosmology.MultiEpoch(0.0, 5.0)
    lo = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 0.5, 0.3, 0.1), cm)
    hi = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.5, 1.5, 1.0, 0.2), cm)
    ka = kernel.Kernel(1e-6 * D2R, 100.0 * D2R, lo, lo, cm)
    kb = kernel.Kernel(1e-6 * D2R, 100.0 * D2R, hi, hi, cm)
    ctx = ka._dev()
    ctx.covariance_cross_stage(0, ctx, lib.CROSS_WINDOWS)
    ctx.covariance_cross_stage(1, kb._dev(), lib.CROSS_WINDOWS)
    with pytest.raises(lib.ChompScopeError, match="no redshift in common"):
        ctx.covariance_cross_range()
    x = numpy.linspace(1.0, 2.0, 8)
    with pytest.raises(lib.ChompScopeError, match="no redshift in common"):
        ctx.kernel_ssc_setup(-10.0, 1.0, 100.0, x, x, with_table=False, cross=True)
