"""Host side of the cross-covariance of two correlations and of CovarianceMulti
(covariance.py:47-205, 796-871), and the G29 fixture's own consistency.  No device."""
import numpy
import pytest

from conftest import load_golden

D2R = numpy.pi / 180.0
KWS = dict(bins_per_decade=2.0, survey_area_deg2=25.0, n_a=[1.0e10, 1.0e10],
           n_b=[1.0e10, 1.0e10], variance=1.0)


def _bare(kern, h, power_name=None):
    """A Correlation without its device work: what Covariance's constructor reads."""
    from chomp_amd import correlation
    corr = correlation.Correlation.__new__(correlation.Correlation)
    corr.log_theta_min = numpy.log10(0.01 * D2R)
    corr.log_theta_max = numpy.log10(1.0 * D2R)
    corr.kernel = kern
    corr.halo = h
    if power_name is not None:
        corr._power_name = power_name
    return corr


def _pair(tag, cosmo_b=None, shared_kernel=False):
    from chomp_amd import cosmology, halo, kernel
    cm = cosmology.MultiEpoch(0.0, 5.0)
    cmb = cm if cosmo_b is None else cosmology.MultiEpoch(0.0, 5.0, cosmo_dict=cosmo_b)

    def kern(wa, wb, c):
        return kernel.Kernel(1e-6 * D2R, 100.0 * D2R, wa, wb, c)
    if tag == "gal":
        w1 = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 2.0, 0.8, 0.2))
        w2 = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2))
        ka = kern(w1, w1, cm)
        kb = ka if shared_kernel else kern(w2, w2, cmb)
        return _bare(ka, halo.Halo(0.0)), _bare(kb, halo.Halo(0.0))
    h = halo.Halo(0.0)
    wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0))
    wb = kernel.WindowFunctionConvergence(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2))
    wc = kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.5, 1.5, 1.0, 0.2))
    return _bare(kern(wa, wb, cm), h), _bare(kern(wc, wc, cmb), h)


def test_fixture_is_self_consistent():
    g = load_golden("g29_covariance_cross")
    for tag in ("gal", "mix"):
        n = g[tag + "_center"].size
        assert n == 4 and g[tag + "_ln_K"].size == 50
        for name in ("a", "b", "ab", "ba"):
            t = g[tag + "_" + name]
            assert t.shape == (50,) and numpy.all(numpy.isfinite(t))
        G, cov = g[tag + "_G"], g[tag + "_cov"]
        assert G.shape == cov.shape == (n, n)
        assert numpy.array_equal(G, G.T) and numpy.array_equal(cov, cov.T)
        # no Poisson term on a cross block's diagonal (covariance.py:312)
        assert numpy.array_equal(cov, G)
        assert not g[tag + "_equal_windows"].any()
        sc = g[tag + "_scalars"]
        assert abs(g[tag + "_ln_K"][0] - sc[10]) < 1e-12 and abs(g[tag + "_ln_K"][-1] - sc[11]) < 1e-12
    # (one convergence window among the four makes no shear pair, covariance.py:195-205)
    assert list(g["gal_cosmic_shear"]) == list(g["mix_cosmic_shear"]) == [False, False]
    sc = g["gal_scalars"]
    assert sc[0] != sc[1] and sc[2] != sc[3]                 # z_bar_a != z_bar_b, D_a != D_b
    sc = g["mix_scalars"]
    # the chi ranges overlap without either holding the other: both clamps act (:496-515)
    assert sc[6] < sc[8] < sc[7] < sc[9]
    # wcovar's blocks are the stored block matrices; the cross block is gal's and symmetric
    w, nb = g["multi_wcovar"], int(g["multi_theta_bins"][0])
    assert w.shape == (2 * nb, 2 * nb) and numpy.array_equal(w, w.T)
    for i, j in ((0, 0), (0, 1), (1, 1)):
        blk = g["multi_block_%d_%d" % (i, j)]
        assert numpy.array_equal(w[i * nb:(i + 1) * nb, j * nb:(j + 1) * nb], blk)
        assert numpy.array_equal(blk, blk.T)
    assert numpy.array_equal(g["multi_block_0_1"], g["gal_cov"])


@pytest.mark.parametrize("tag", ["gal", "mix"])
def test_cross_covariance_constructs_without_a_device(tag):
    from chomp_amd import covariance
    g = load_golden("g29_covariance_cross")
    c1, c2 = _pair(tag)
    cv = covariance.Covariance(c1, c2, nongaussian_cov=False, **KWS)
    assert cv.matching_corrs is False
    assert cv.corr_a is c1 and cv.corr_b is c2
    assert cv.halo_a is c1.halo and cv.halo_b is c2.halo
    assert list(cv.equal_windows) == list(g[tag + "_equal_windows"])
    assert [bool(x) for x in cv.cosmic_shear] == list(g[tag + "_cosmic_shear"])
    assert numpy.allclose([b.center for b in cv.annular_bins], g[tag + "_center"], rtol=1e-15)
    assert numpy.allclose([b.inner for b in cv.annular_bins], g[tag + "_inner"], rtol=1e-15)
    k = cv.kernel
    assert k.window_function_a1 is c1.kernel.window_function_a
    assert k.window_function_a2 is c1.kernel.window_function_b
    assert k.window_function_b1 is c2.kernel.window_function_a
    assert k.window_function_b2 is c2.kernel.window_function_b
    assert k.cosmo is c1.kernel.cosmo
    sc = g[tag + "_scalars"]
    assert abs(cv._j0_limit / sc[12] - 1) < 1e-14 and abs(cv.area / sc[13] - 1) < 1e-14
    assert all(cv.proj_power_poisson(p) == 0.0 for p in range(6))
    # a cross block has no Poisson term even where a window pair is shared (covariance.py:312)
    assert cv.covariance_P(1.0, 1.0) == 0.0


def test_equal_windows_follow_the_shared_kernel():
    """covariance.py:104-111 with kernel.py:248-259, 592-593: windows are equal by identity, and
    two correlations hold the same window objects only through one shared Kernel."""
    from chomp_amd import covariance
    c1, c2 = _pair("gal", shared_kernel=True)
    cv = covariance.Covariance(c1, c2, nongaussian_cov=False, **KWS)
    assert cv.matching_corrs is False
    assert list(cv.equal_windows) == [False, False, False, False, True, True]
    assert cv.proj_power_poisson(4) == 1.0 / (1.0e10 / cv.area)


def test_cross_covariance_refusals():
    from chomp_amd import _lib, covariance, halo_trispectrum
    from chomp_amd import defaults
    c1, c2 = _pair("gal")
    tri = halo_trispectrum.HaloTrispectrumOneHalo(0.5)
    with pytest.raises(_lib.ChompScopeError, match="nongaussian_cov=False"):
        covariance.Covariance(c1, c2, nongaussian_cov=True, input_halo_trispectrum=tri)
    with pytest.raises(_lib.ChompScopeError, match="nongaussian_cov=False"):
        covariance.Covariance(c1, c2)                       # the default: the term is on
    with pytest.raises(_lib.ChompScopeError, match="super-sample"):
        covariance.Covariance(c1, c2, nongaussian_cov=False, ssc_cov=True)
    cv = covariance.Covariance(c1, c2, nongaussian_cov=False)
    with pytest.raises(_lib.ChompScopeError, match="set_cosmology"):
        cv.set_cosmology(dict(defaults.default_cosmo_dict))
    other = dict(defaults.default_cosmo_dict)
    other["omega_m0"] = other["omega_m0"] + 0.01
    other["omega_l0"] = other["omega_l0"] - 0.01
    d1, d2 = _pair("gal", cosmo_b=other)
    with pytest.raises(_lib.ChompScopeError, match="cosmolog"):
        covariance.Covariance(d1, d2, nongaussian_cov=False)
    c1._power_name, c2._power_name = "power_mm", "power_gg"
    with pytest.raises(_lib.ChompScopeError, match="power_spec"):
        covariance.Covariance(c1, c2, nongaussian_cov=False)
    c2._power_name = "power_mm"
    assert covariance.Covariance(c1, c2, nongaussian_cov=False).matching_corrs is False


def test_covariance_multi_assembles_blocks():
    from chomp_amd import _lib, covariance
    g = load_golden("g29_covariance_cross")
    c1, c2 = _pair("gal")
    with pytest.raises(_lib.ChompScopeError, match="nongaussian_cov=False"):
        covariance.CovarianceMulti([c1, c2])                # nongaussian_cov defaults to True
    cm = covariance.CovarianceMulti([c1, c2], nongaussian_cov=False, **KWS)
    assert isinstance(cm, covariance.Covariance)
    assert [len(r) for r in cm.covariance_list] == [2, 1]
    assert cm.covariance_list[0][0].matching_corrs and cm.covariance_list[1][0].matching_corrs
    cross = cm.covariance_list[0][1]
    assert not cross.matching_corrs and cross.corr_a is c1 and cross.corr_b is c2
    assert cm.annular_bins is cm.covariance_list[0][0].annular_bins
    nb = cm.theta_bins
    assert nb == int(g["multi_theta_bins"][0]) and cm.wcovar.shape == (2 * nb, 2 * nb)
    for i, row in enumerate(cm.covariance_list):
        for j, cv in enumerate(row):
            def fill(cv=cv, blk=g["multi_block_%d_%d" % (i, i + j)]):
                cv.covar = blk
                return blk
            cv.get_covariance = fill
    w = cm.get_covariance()
    assert w is cm.wcovar and numpy.array_equal(w, g["multi_wcovar"])
    # the reference's defaults (covariance.py:820-824)
    one = covariance.CovarianceMulti([c1], nongaussian_cov=False)
    only = one.covariance_list[0][0]
    assert only.bins_per_decade == 5 and (only.n_a1, only.n_b2) == (1e6, 1e6)
    assert abs(only.area / (4 * numpy.pi) - 1) < 1e-15
    # three correlations with non-symmetric stand-in blocks: the reference's index arithmetic
    # (covariance.py:865-870) writes the block, not its transpose, into the mirror
    c3, _ = _pair("mix")
    cm3 = covariance.CovarianceMulti([c1, c2, c3], nongaussian_cov=False, **KWS)
    rng = numpy.random.RandomState(29)
    blocks = {}
    for i, row in enumerate(cm3.covariance_list):
        for j, cv in enumerate(row):
            blk = blocks[(i, i + j)] = rng.rand(nb, nb)

            def fill(cv=cv, blk=blk):
                cv.covar = blk
                return blk
            cv.get_covariance = fill
    w = cm3.get_covariance()
    assert w.shape == (3 * nb, 3 * nb)
    for (i, j), blk in blocks.items():
        assert numpy.array_equal(w[i * nb:(i + 1) * nb, j * nb:(j + 1) * nb], blk)
        if i != j:
            assert numpy.array_equal(w[j * nb:(j + 1) * nb, i * nb:(i + 1) * nb], blk)


def test_covariance_multi_has_no_prints(capsys):
    from chomp_amd import covariance
    c1, c2 = _pair("gal")
    cm = covariance.CovarianceMulti([c1, c2], nongaussian_cov=False, **KWS)
    for row in cm.covariance_list:
        for cv in row:
            cv.get_covariance = lambda cv=cv: setattr(cv, "covar", numpy.zeros((4, 4)))
    cm.get_covariance()
    assert capsys.readouterr().out == ""
