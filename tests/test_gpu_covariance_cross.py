"""G29: the Gaussian cross-covariance of two w(theta) -- Covariance(corr_a, corr_b) of two
different correlations, the four projected spectra and covariance_G with two two-point terms
(covariance.py:422-453, 495-541) -- and CovarianceMulti (covariance.py:796-871) on the device,
against the reference's own numbers (tests/golden/make_golden_cov_cross.py).

Tolerance: the relative 1e-4 that the G12 test (test_gpu_next.py) applies to the matching
path's table and matrix.  Table knots carry an absolute floor of that tolerance times
max|table|: the reference's tables hold knots of order 1e-30 (and, where the two chi ranges
differ, of order -1e-15) at the ends of the common ln K grid.  No knot and no pair is left out.
"""
import copy

import numpy
import pytest

from conftest import load_golden, rel_err
from params import hod_dict_2

pytestmark = pytest.mark.gpu
RTOL = 1e-4                      # test_gpu_next.py: g12_covariance_gaussian's table and matrix
D2R = numpy.pi / 180.0
KWS = dict(bins_per_decade=2.0, survey_area_deg2=25.0, n_a=[1.0e10, 1.0e10],
           n_b=[1.0e10, 1.0e10], variance=1.0)
NAMES = ("a", "b", "ab", "ba")


def correlations(tag, power_spec="power_mm", z0_b=1.0, only_a=False):
    """The fixture's correlations: "gal" two galaxy windows, each used twice, each correlation on
    its own Halo; "mix" galaxy x convergence and a galaxy auto-correlation on z = 0.5-1.5 that
    share one Halo object."""
    from chomp_amd import correlation, cosmology, halo, kernel
    cm = cosmology.MultiEpoch(0.0, 5.0)

    def corr(wa, wb, h):
        kern = kernel.Kernel(1e-6 * D2R, 100.0 * D2R, wa, wb, cm)
        return correlation.Correlation(0.01, 1.0, kern, input_halo=h, power_spec=power_spec)
    if tag == "gal":
        w1 = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 2.0, 0.8, 0.2))
        w2 = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 2.0, z0_b, 0.2))
        return corr(w1, w1, halo.Halo(0.0)), corr(w2, w2, halo.Halo(0.0))
    h = halo.Halo(0.0)
    wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0))
    wb = kernel.WindowFunctionConvergence(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2))
    if only_a:                   # (b's constructor would move the shared halo to its z_bar)
        return corr(wa, wb, h)
    wc = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.5, 1.5, 1.0, 0.2))
    return corr(wa, wb, h), corr(wc, wc, h)


def table_err(got, ref):
    """max over the knots of |got - ref| / max(|ref|, max|ref|-floor): every knot counts."""
    ref = numpy.asarray(ref, dtype=float)
    den = numpy.maximum(numpy.abs(ref), numpy.max(numpy.abs(ref)))
    return float(numpy.max(numpy.abs(numpy.asarray(got, dtype=float) - ref) / den))


def all_pairs_G(cv):
    bins = cv.annular_bins
    return numpy.array([[cv.covariance_G(a.center, b.center, a.delta, b.delta) for b in bins]
                        for a in bins])


@pytest.mark.parametrize("tag", ["gal", "mix"])
def test_g29_cross_block(tag):
    from chomp_amd import covariance
    g = load_golden("g29_covariance_cross")
    ca, cb = correlations(tag)
    cv = covariance.Covariance(ca, cb, nongaussian_cov=False, **KWS)
    assert cv.matching_corrs is False
    assert list(cv.equal_windows) == list(g[tag + "_equal_windows"])
    cv._initialize_halo_splines()
    sc = g[tag + "_scalars"]
    print(tag, "z_bar", cv._z_bar_G_a, cv._z_bar_G_b, "D", cv._D_z_a / sc[2] - 1,
          cv._D_z_b / sc[3] - 1)
    assert abs(cv._z_bar_G_a - sc[0]) < 1e-12 and abs(cv._z_bar_G_b - sc[1]) < 1e-12
    assert abs(cv._D_z_a / sc[2] - 1) < 1e-9 and abs(cv._D_z_b / sc[3] - 1) < 1e-9
    assert abs(cv._ln_K_min - sc[10]) < 1e-9 and abs(cv._ln_K_max - sc[11]) < 1e-9
    assert numpy.allclose(cv._ln_K_array, g[tag + "_ln_K"], rtol=0, atol=1e-9)
    errs = {}
    for name in NAMES:
        got = getattr(cv, "_halo_%s_array" % name)
        lev = getattr(cv, "_halo_%s_levels" % name)
        assert got.shape == (50,) and lev.shape == (50,) and numpy.all(numpy.isfinite(got))
        errs[name] = table_err(got, g[tag + "_" + name])
    print(tag, "table errors", errs)
    assert max(errs.values()) < RTOL
    # the look-ups are the tables' splines
    K = numpy.exp(cv._ln_K_array[[5, 25, 40]])
    for name in NAMES:
        got = getattr(cv, "_projected_halo_" + name)(K)
        assert table_err(got, g[tag + "_" + name][[5, 25, 40]]) < RTOL
    G = all_pairs_G(cv)
    print(tag, "covariance_G error", rel_err(G, g[tag + "_G"]))
    assert rel_err(G, g[tag + "_G"]) < RTOL
    full = cv.get_covariance()
    assert full.shape == (4, 4) and numpy.array_equal(full, full.T)
    assert rel_err(full, g[tag + "_cov"]) < RTOL
    bins = cv.annular_bins
    assert abs(cv.covariance(bins[1], bins[1]) / g[tag + "_cov"][1, 1] - 1) < RTOL
    assert abs(cv.covariance(bins[0], bins[3]) / g[tag + "_cov"][0, 3] - 1) < RTOL


def test_g29_covariance_multi():
    from chomp_amd import covariance
    g = load_golden("g29_covariance_cross")
    ca, cb = correlations("gal")
    cm = covariance.CovarianceMulti([ca, cb], nongaussian_cov=False, **KWS)
    w = cm.get_covariance()
    assert w.shape == (8, 8) and numpy.array_equal(w, w.T)
    print("wcovar error", rel_err(w, g["multi_wcovar"]))
    assert rel_err(w, g["multi_wcovar"]) < RTOL


def test_cross_path_agrees_with_matching_path():
    """A correlation and a copy.copy of it: all four cross tables are the matching path's one
    table, and covariance_G the matching one (the Poisson terms of the integrand are zero in
    both: the windows a1, a2 are never equal)."""
    from chomp_amd import covariance
    ca = correlations("mix", only_a=True)
    twin = copy.copy(ca)
    same = covariance.Covariance(ca, ca, nongaussian_cov=False, **KWS)
    same._initialize_halo_splines()
    ref = same._halo_a_array.copy()
    G_ref = all_pairs_G(same)
    cv = covariance.Covariance(ca, twin, nongaussian_cov=False, **KWS)
    assert cv.matching_corrs is False
    assert list(cv.equal_windows) == [False, False, False, False, True, True]
    cv._initialize_halo_splines()
    assert numpy.array_equal(cv._ln_K_array, same._ln_K_array)
    assert cv._D_z_a == same._D_z_a and abs(cv._D_z_b / same._D_z_a - 1) < 1e-12
    errs = {n: table_err(getattr(cv, "_halo_%s_array" % n), ref) for n in NAMES}
    print("cross vs matching tables", errs)
    assert max(errs.values()) < RTOL
    G = all_pairs_G(cv)
    print("cross vs matching covariance_G", rel_err(G, G_ref))
    assert rel_err(G, G_ref) < RTOL


def test_cross_tables_follow_corr_b():
    """The table key: a change of corr_b's HOD or redshift window after a first evaluation
    rebuilds the tables, to what a block built from such correlations holds."""
    from chomp_amd import covariance
    ca, cb = correlations("gal", "power_gg")
    cv = covariance.Covariance(ca, cb, nongaussian_cov=False, power_spec="power_gg", **KWS)
    G0 = cv.covariance_G(0.001, 0.002)
    first = {n: getattr(cv, "_halo_%s_array" % n) for n in NAMES}
    cv._tables()                                                     # nothing changed: kept
    assert all(getattr(cv, "_halo_%s_array" % n) is first[n] for n in NAMES)

    cb.set_hod(hod_dict_2)
    G1 = cv.covariance_G(0.001, 0.002)
    assert numpy.array_equal(cv._halo_a_array, first["a"])           # a's side did not move
    for n in ("b", "ab", "ba"):
        assert table_err(getattr(cv, "_halo_%s_array" % n), first[n]) > 1e-2, n
    assert abs(G1 / G0 - 1) > 1e-3
    fa, fb = correlations("gal", "power_gg")
    fb.set_hod(hod_dict_2)
    fresh = covariance.Covariance(fa, fb, nongaussian_cov=False, power_spec="power_gg", **KWS)
    fresh._initialize_halo_splines()
    for n in NAMES:
        assert numpy.allclose(getattr(cv, "_halo_%s_array" % n),
                              getattr(fresh, "_halo_%s_array" % n), rtol=1e-12, atol=0), n

    cb.kernel.window_function_a._redshift_dist.z0 = 0.9              # (one object: both windows)
    moved = cv.covariance_G(0.001, 0.002)
    assert abs(cv._z_bar_G_b - fresh._z_bar_G_b) > 0.05
    fa, fb = correlations("gal", "power_gg", z0_b=0.9)
    fb.set_hod(hod_dict_2)
    fresh = covariance.Covariance(fa, fb, nongaussian_cov=False, power_spec="power_gg", **KWS)
    assert abs(moved / fresh.covariance_G(0.001, 0.002) - 1) < 1e-12
    assert cv._z_bar_G_b == fresh._z_bar_G_b
    for n in NAMES:
        assert numpy.allclose(getattr(cv, "_halo_%s_array" % n),
                              getattr(fresh, "_halo_%s_array" % n), rtol=1e-12, atol=0), n


def test_pairs_on_the_device_stay_there():
    """A torch cuda tensor of pairs goes to the kernel in place and the result stays on the
    device; same numbers as the host path."""
    import torch
    from chomp_amd import covariance
    ca, cb = correlations("gal")
    cv = covariance.Covariance(ca, cb, nongaussian_cov=False, **KWS)
    c = numpy.array([b.center for b in cv.annular_bins])
    iu = numpy.triu_indices(c.size)
    host = cv._covariance_G_pairs(c[iu[0]], c[iu[1]])
    ctx = cv._tables()
    pairs = torch.tensor(numpy.concatenate([c[iu[0]], c[iu[1]]]), dtype=torch.float64,
                         device="cuda")
    out = ctx.covariance_gaussian_cross(cv._j0_limit, cv.area, [0.0] * 4, pairs)
    assert out.is_cuda and out.shape == (10,)
    assert numpy.array_equal(out.cpu().numpy(), host)
