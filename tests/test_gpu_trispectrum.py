"""HaloTrispectrum on the device against tests/golden/g26_trispectrum.npz (the reference's
halo_trispectrum.py:153-837, recorded by tests/golden/make_golden_tri.py).

Bars: tables 1e-8 of the table's scale and every Romberg level equal to the reference's (as G24);
spline look-ups 1e-7; the terms and tri_spec_proj_integral 1e-5 (the covariance_NG per-element
bar) on a cancellation-aware scale, the sum of the absolute values of a term's addends as the NumPy
restatement of tests/test_trispectrum_cpu.py forms them on the oracle's tables (so neither the
scale nor the expected Romberg levels come from the code under test).
"""
import os
import warnings

import numpy
import pytest

from test_trispectrum_cpu import oracle_g26

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G26 = os.path.join(HERE, "golden", "g26_trispectrum.npz")
TABLES = ("i_0_4", "i_1_2", "i_1_3", "i_2_1", "i_2_2")
CASES = ("a_", "b_", "c_")


@pytest.fixture(scope="module")
def g():
    return numpy.load(G26)


def _make(tag):
    import chomp_amd as c
    from params import c_dict_2, h_dict_2
    if tag == "c_":
        cosmo = c.cosmology.SingleEpoch(0.3)
        h = c.halo_trispectrum.HaloTrispectrum(
            0.3, cosmo, c.mass_function.MassFunctionSecondOrder(0.3, cosmo, h_dict_2), None,
            h_dict_2)
        h.set_cosmology(c_dict_2)
        return h
    z = 0.0 if tag == "a_" else 0.5
    cosmo = c.cosmology.SingleEpoch(z)
    return c.halo_trispectrum.HaloTrispectrum(
        z, cosmo, c.mass_function.MassFunctionSecondOrder(z, cosmo))


@pytest.fixture(scope="module")
def objs():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return {tag: _make(tag) for tag in CASES}


def _triu(a):
    return a[numpy.triu_indices(a.shape[0])] if a.ndim == 2 else a


@pytest.mark.parametrize("tag", CASES)
def test_tables_and_levels(g, objs, tag):
    h = objs[tag]
    for name in TABLES:
        getattr(h, "_initialize_" + name)()
        assert getattr(h, "_initialized_" + name)
        tab = _triu(getattr(h, "_%s_array" % name))
        lev = _triu(getattr(h, "_%s_levels" % name))
        ref = g[tag + name]
        err = numpy.max(numpy.abs(tab - ref)) / numpy.max(numpy.abs(ref))
        nlev = int(numpy.sum(lev != g[tag + name + "_levels"]))
        print("%s%s: table err %.3e of scale, %d levels differ, max level %d"
              % (tag, name, err, nlev, lev.max()))
        assert err < 1e-8
        assert nlev == 0
        assert numpy.array_equal(lev, _triu(oracle_g26(tag)["r"].lev[name]))
    full = h._i_1_3_array
    assert numpy.array_equal(full, full.T)


@pytest.mark.parametrize("tag", CASES)
def test_lookups(g, objs, tag):
    h = objs[tag]
    cfg, ref = g["configs"], g[tag + "lookups"]
    got = numpy.array([[h.i_1_2(a, b), h.i_1_3_parallelogram(a, b), h.i_1_3_parallelogram(b, a),
                        h.i_2_2(a, b), h.i_2_1(a), h.i_2_1(b)] for a, b in cfg[:, :2]])
    scale = numpy.max(numpy.abs(ref), axis=0)
    err = numpy.max(numpy.abs(got - ref) / scale)
    print("%slookups: %.3e" % (tag, err))
    assert err < 1e-7
    assert numpy.array_equal(got == 0.0, ref == 0.0)          # exact zeros above k_max
    hm = numpy.array([h.i_1_1(k) for k in cfg[:, 0]])
    assert numpy.max(numpy.abs(hm - g[tag + "h_m"])) < 1e-7 * numpy.max(numpy.abs(g[tag + "h_m"]))
    assert numpy.array_equal(hm == 0.0, g[tag + "h_m"] == 0.0)
    # under the k_min clamp: the value at k_min
    for fn in (h.i_1_2, h.i_2_2, h.i_1_3_parallelogram, h.i_0_4_parallelogram):
        assert fn(5e-4, 1.0) == fn(h._k_min, 1.0)
        assert fn(1.0, 2e-4) == fn(1.0, h._k_min)
        assert fn(150.0, 1.0) == 0.0 and fn(1.0, 100.1) == 0.0
    assert h.i_2_1(5e-4) == h.i_2_1(h._k_min) and h.i_2_1(100.1) == 0.0


@pytest.mark.parametrize("tag", CASES)
def test_terms(g, objs, tag):
    h = objs[tag]
    cfg, ref = g["configs"], g[tag + "terms"]
    got = h.terms_many(cfg)
    assert got.shape == (cfg.shape[0], 4)
    scale = oracle_g26(tag)["scales"]
    assert numpy.all(numpy.isfinite(got)) and numpy.all(numpy.isfinite(ref))
    assert numpy.all(numpy.isfinite(scale))
    with numpy.errstate(invalid="ignore", divide="ignore"):
        rel = numpy.where(scale > 0, numpy.abs(got - ref) / scale, numpy.abs(got - ref))
    print("%sterms: max err on the addend scale per term %s" % (tag, numpy.nanmax(rel, axis=0)))
    assert numpy.all(numpy.isfinite(rel)) and rel.max() < 1e-5
    tot = numpy.array([h.trispectrum_parallelogram(*c) for c in cfg])
    rt = numpy.abs(tot - ref.sum(axis=1)) / scale.sum(axis=1).clip(1e-300)
    print("%strispectrum_parallelogram: %.3e" % (tag, rt.max()))
    assert numpy.all(numpy.isfinite(rt)) and rt.max() < 1e-5
    # the scalar methods are the batch call
    for n in (0, 7, 17, 25):
        k1, k2, z = cfg[n]
        assert h.t_1_h(k1, k2) == got[n, 0]
        assert h.t_2_h(k1, k2, z) == got[n, 1]
        assert h.t_3_h(k1, k2, z) == got[n, 2]
        assert h.t_4_h(k1, k2, z) == got[n, 3]
    tpt = numpy.array([h.t_PT(*c) for c in cfg])
    ok = numpy.isfinite(g[tag + "t_pt"])
    assert numpy.allclose(tpt[ok], g[tag + "t_pt"][ok], rtol=1e-6, atol=0)


@pytest.mark.parametrize("tag", CASES)
def test_proj(g, objs, tag):
    """The scale of a pair is |t_1_h| + 2 / pi times the trapezoid sum, over the 2^level + 1
    nodes the Romberg stops on, of the three terms' addend scales (the restatement's
    _Restated.proj): the quadrature's own sum is where those addends cancel, and for k1 close to
    k2 they grow steeply towards theta = 0, which a coarser sampling of theta does not see."""
    import chomp_amd as c
    h = objs[tag]
    pairs, ref, rlev = g["pairs"], g[tag + "proj"], g[tag + "proj_levels"]
    fin = numpy.isfinite(ref)
    assert (~fin).sum() == 3          # k1 = k2 twice; (1, 150): norm = 1 / 0, the integrand 0 * inf
    ctx = h._ready()
    out, lev, flag = h.tri_spec_proj_integral_many(pairs[fin], levels=True)
    assert not (ctx.status(0, 1)[0] & c._lib.ST_TRI_DIVMAX)
    assert numpy.all(flag == 0.0)
    d = oracle_g26(tag)
    scale = d["proj_scales"][fin]
    assert numpy.all(numpy.isfinite(scale)) and numpy.array_equal(d["proj_levels"], rlev)
    rel = numpy.abs(out - ref[fin]) / scale
    print("%sproj: max err %.3e %s; levels %s (reference %s)" % (tag, rel.max(), rel, lev, rlev[fin]))
    assert numpy.all(numpy.isfinite(rel)) and rel.max() < 1e-5
    assert numpy.array_equal(lev, rlev[fin])
    with pytest.warns(c._lib.ChompAccuracyWarning):
        out, lev, flag = h.tri_spec_proj_integral_many(pairs, levels=True)
    assert numpy.array_equal(numpy.isnan(out), ~fin)
    assert numpy.array_equal(flag == 1.0, ~fin)
    assert ctx.status(0, 1)[0] & c._lib.ST_TRI_DIVMAX
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert numpy.isnan(h.tri_spec_proj_integral(1.0, 1.0))
    # the status bit stays up, but a call whose own pairs are all finite does not warn
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        h.tri_spec_proj_integral_many(pairs[fin][:3])


@pytest.mark.parametrize("tag", CASES)
def test_i_1_3_triples(g, objs, tag):
    h = objs[tag]
    trip = g["triples"]
    out, lev = h.i_1_3_many(trip, levels=True)
    ref = g[tag + "i_1_3_triples"]
    err = numpy.max(numpy.abs(out - ref) / numpy.abs(ref))
    print("%si_1_3 triples: %.3e, levels %s (reference %s)"
          % (tag, err, lev, g[tag + "i_1_3_triples_levels"]))
    assert err < 1e-8
    assert numpy.array_equal(lev, g[tag + "i_1_3_triples_levels"])
    # the table's (i, i, j) entries through the general path
    h._initialize_i_1_3()
    k = numpy.exp(h._ln_k_array)
    ij = [(3, 3), (5, 20), (12, 40), (30, 49)]
    got = h.i_1_3_many(numpy.array([[k[i], k[i], k[j]] for i, j in ij]))
    tab = numpy.array([h._i_1_3_array[i, j] for i, j in ij])
    assert numpy.max(numpy.abs(got / tab - 1.0)) < 1e-12


def test_i_0_4_quad_path_bit_identical():
    """i_0_4 through the quadruple kernel gives the bits and the Romberg levels it gave before the
    kernel took its arity parameter (tests/golden/make_golden_quad_bits.py, recorded on the
    MI355X with the commit before HaloTrispectrum)."""
    import chomp_amd as c
    g27 = numpy.load(os.path.join(HERE, "golden", "g27_i_0_4_quad_bits.npz"))
    for tag, z, spec in (("z000_mmmm", 0.0, "power_mmmm"), ("z050_mmmm", 0.5, "power_mmmm"),
                         ("z030_gggg", 0.3, "power_gggg")):
        h = c.halo_trispectrum.HaloTrispectrumOneHalo(z, power_spec=spec)
        v, lev = h._sync(0).tri1h_quad(c._lib.TRI_MOMENT[spec], g27["quads"], 0, levels=True)
        assert numpy.array_equal(v, g27[tag + "_value"])
        assert numpy.array_equal(lev, g27[tag + "_level"])


def test_torch_equals_numpy(g, objs):
    import torch
    h = objs["a_"]
    cfg, pairs = g["configs"], g["pairs"][:9]
    a = h.terms_many(cfg)
    b = h.terms_many(torch.tensor(cfg, dtype=torch.float64, device="cuda"))
    assert isinstance(b, torch.Tensor) and b.is_cuda
    assert numpy.array_equal(a, b.cpu().numpy(), equal_nan=True)
    p = h.tri_spec_proj_integral_many(pairs)
    q = h.tri_spec_proj_integral_many(torch.tensor(pairs, dtype=torch.float64, device="cuda"))
    assert numpy.array_equal(p, q.cpu().numpy())


def test_epoch_batch_equals_single(objs):
    """chomp_tri_setup over an epoch range gives each epoch the single-epoch set-up's bits."""
    import chomp_amd as c
    from chomp_amd import cosmology, defaults
    h = objs["b_"]
    for name in TABLES:
        getattr(h, "_initialize_" + name)()
    ctx = cosmology._context()
    ctx.set_second_order(True)
    ctx.epochs_set(defaults.default_cosmo_dict, [0.0, 0.5], False)
    ctx.stage_k(h.mass.halo_dict, h.mass._kind, h._profile(), h.local_hod, c._lib.T_H_M)
    tab, lev = ctx.tri_setup(0, 2, copy_out=True)
    for name in TABLES:
        assert numpy.array_equal(tab[name][1], getattr(h, "_%s_array" % name))
        assert numpy.array_equal(lev[name][1], getattr(h, "_%s_levels" % name))


def test_unknown_mem_refused(objs):
    import ctypes
    h = objs["a_"]
    ctx = h._ready()
    x = numpy.ones(3)
    out = numpy.empty(4)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    L = ctx._L
    assert L.chomp_tri_terms(ctx._h, 0, 0, p(x), 1, p(out), 7) != 0
    assert L.chomp_tri_proj(ctx._h, 0, 0, p(x), 1, p(out), None, None, 7) != 0
    assert L.chomp_tri_table_eval(ctx._h, 0, 0, p(x), p(x), 1, p(out), 7) != 0
    assert L.chomp_tri_triple(ctx._h, 0, p(x), 1, p(out), None, 7) != 0


def test_set_cosmology_sequence(g):
    """After set_cosmology every flag resets and the PT terms move to the new cosmology."""
    from params import c_dict_2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        h = _make("a_")
        before = h.t_PT(0.1, 1.0, 0.3)
        h.t_4_h(0.1, 1.0, 0.3)
        assert all(getattr(h, "_initialized_" + n) for n in TABLES)
        h.set_cosmology(c_dict_2)
        assert not any(getattr(h, "_initialized_" + n) for n in TABLES)
        assert h.pert.cosmo is h.cosmo
        after = h.t_PT(0.1, 1.0, 0.3)
        assert after != before
        assert h.t_4_h(0.1, 1.0, 0.3) != 0.0
        assert all(getattr(h, "_initialized_" + n) for n in ("i_2_1",))
