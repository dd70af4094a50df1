"""Host side of the batches of xi(r) over many HODs and cosmologies: the C declaration and its
binding, the scope of Correlation3d.raw_correlation_hods / raw_correlation_cosmologies and of
SimulationDesign's routes for them, and the G35 fixture -- its shape, the oracle's agreement with
it and the Romberg levels that make the device test stop early and late.  No device."""
import os
import re

import numpy
import pytest

from conftest import ROOT, load_golden, rel_err

R = numpy.array([0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0])
ZEHAVI = {"log_M_min": 12.14, "sigma": 0.15, "log_M_0": 12.14, "log_M_1p": 13.43, "alpha": 1.0}
ZHENG_KEYS = ("log_M_min", "sigma", "log_M_0", "log_M_1p", "alpha")
COSMO_KEYS = ("omega_m0", "omega_b0", "omega_l0", "omega_r0", "cmb_temp", "h", "sigma_8",
              "n_scalar", "w0", "wa")
HODS_LOOP = "use the loop set_hod / set_hod_object + raw_correlation"
COSMOLOGIES_LOOP = "use the loop fresh Correlation3d objects (+ set_hod_object) + raw_correlation"


def _bare(h, power_name="power_gg", cls=None):
    """A Correlation3d around a given halo, without its constructor."""
    from chomp_amd import correlation
    cls = correlation.Correlation3d if cls is None else cls
    c3 = cls.__new__(cls)
    c3.halo = h
    c3._k_lim = (h._k_min, h._k_max)
    c3._power_name = power_name
    c3.initialized_spline = False
    return c3


def _cosmos():
    from chomp_amd import defaults
    c = dict(defaults.default_cosmo_dict)
    return [c, dict(c, sigma_8=0.9, h=0.65)]


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to create a device context fails the test."""
    from chomp_amd import cosmology

    def boom(*a, **k):
        raise AssertionError("a device context was asked for")
    monkeypatch.setattr(cosmology, "_context", boom)


def test_header_declares_the_entry_point():
    from chomp_amd import _lib
    with open(os.path.join(ROOT, "include", "chomp_mi355x.h")) as f:
        header = f.read()
    flat = re.sub(r"\s+", " ", header)
    assert ("int chomp_xi3d_epochs(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, "
            "double k_min, double k_max, const double* r, size_t n, double* out, int mem);") in flat
    # no new knob: the chunk is that of the batched projections
    assert re.search(r"#define CHOMP_TUNE_COUNT 12\b", header)
    assert "chomp_xi3d_epochs" in _lib.EXPORTS
    assert callable(_lib.Context.xi3d_epochs)


def _out_of_scope():
    """(label, Correlation3d, hods) of every case the batches refuse: the cases of
    tests/test_wtheta_hods_cpu.py."""
    from chomp_amd import cosmology, halo, hod
    # (HaloFit's constructor reads omega_m off the device: the class is what matters here)
    fit = halo.HaloFit.__new__(halo.HaloFit)
    fit.__dict__.update(halo.Halo(0.0).__dict__)
    cases = [("HaloFit", _bare(fit), [ZEHAVI, ZEHAVI]),
             ("HaloExclusion", _bare(halo.HaloExclusion(0.0)), [ZEHAVI, ZEHAVI]),
             ("HaloSuperSampleCovariance", _bare(halo.HaloSuperSampleCovariance(0.0)), [ZEHAVI, ZEHAVI]),
             ("general_profile", _bare(halo.Halo(0.0, general_profile=True)), [ZEHAVI, ZEHAVI]),
             ("an extrapolated spectrum (chomp_xi3d_epochs takes none)",
              _bare(halo.Halo(0.0, extrapolate=True)), [ZEHAVI, ZEHAVI])]
    h = halo.Halo(0.0, cosmo_single_epoch=cosmology.SingleEpoch(0.0, with_bao=True))
    cases.append(("with_bao", _bare(h), [ZEHAVI, ZEHAVI]))
    h = halo.Halo(0.0)
    h.set_halo(dict(h.get_halo(), c0=7.5))
    cases.append(("set_halo", _bare(h), [ZEHAVI, ZEHAVI]))
    cases.append(("hods[1]", _bare(halo.Halo(0.0)), [ZEHAVI, hod.HOD(dict(ZEHAVI))]))
    return cases


def test_batches_refuse_what_they_do_not_serve(no_device):
    from chomp_amd import _lib
    cases = _out_of_scope()
    assert len(cases) == 8
    for label, c3, hods in cases:
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)) as info:
            c3.raw_correlation_hods(R, hods)
        assert str(info.value).startswith("raw_correlation_hods: ")
        assert str(info.value).endswith(HODS_LOOP)
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)) as info:
            c3.raw_correlation_cosmologies(R, _cosmos(), hods=hods)
        assert str(info.value).startswith("raw_correlation_cosmologies: ")
        assert str(info.value).endswith(COSMOLOGIES_LOOP)


def test_an_extrapolating_k_range_is_refused(no_device):
    """A k range beyond the halo's switches extrapolation on in the constructor
    (correlation.py:435-438): the loop's business."""
    from chomp_amd import _lib, correlation
    c3 = correlation.Correlation3d(0.1, 50.0, powSpec="power_mm", k_min=1e-4, k_max=1e3)
    with pytest.raises(_lib.ChompScopeError, match="extrapolated"):
        c3.raw_correlation_hods(R, [ZEHAVI])
    with pytest.raises(_lib.ChompScopeError, match="extrapolated"):
        c3.raw_correlation_cosmologies(R, _cosmos())


def test_a_divmax_beyond_the_table_is_refused(no_device, monkeypatch):
    from chomp_amd import _lib, defaults, halo
    c3 = _bare(halo.Halo(0.0))
    monkeypatch.setitem(defaults.default_precision, "divmax", 21)
    with pytest.raises(_lib.ChompScopeError, match="divmax") as info:
        c3.raw_correlation_hods(R, [ZEHAVI])
    assert str(info.value).startswith("raw_correlation_hods: ") and str(info.value).endswith(HODS_LOOP)
    with pytest.raises(_lib.ChompScopeError, match="divmax") as info:
        c3.raw_correlation_cosmologies(R, _cosmos())
    assert str(info.value).startswith("raw_correlation_cosmologies: ")
    assert str(info.value).endswith(COSMOLOGIES_LOOP)


def test_hods_must_match_the_points(no_device):
    from chomp_amd import halo
    with pytest.raises(ValueError, match="1 hods for 2 cosmologies"):
        _bare(halo.Halo(0.0)).raw_correlation_cosmologies(R, _cosmos(), hods=[ZEHAVI])


def test_inherited_batches_name_the_raw_ones(no_device):
    from chomp_amd import _lib, halo
    c3 = _bare(halo.Halo(0.0))
    with pytest.raises(_lib.ChompScopeError, match="raw_correlation_hods"):
        c3.correlation_hods(R, [ZEHAVI])
    with pytest.raises(_lib.ChompScopeError, match="raw_correlation_cosmologies"):
        c3.correlation_cosmologies(R, _cosmos())


def test_empty_inputs_need_no_device(no_device):
    from chomp_amd import halo
    c3 = _bare(halo.Halo(0.0))
    out, words = c3.raw_correlation_hods(R, [], with_status=True)
    assert out.shape == (0, 7) and words.shape == (0,) and words.dtype == numpy.uint32
    out, words = c3.raw_correlation_hods(R[:0], [ZEHAVI, ZEHAVI], with_status=True)
    assert out.shape == (2, 0) and words.shape == (2,) and words.dtype == numpy.uint32
    assert numpy.array_equal(c3.hods_status, words)
    out, words = c3.raw_correlation_cosmologies(R, [], with_status=True)
    assert out.shape == (0, 7) and words.shape == (0,) and words.dtype == numpy.uint32
    assert c3.raw_correlation_cosmologies(R[:0], _cosmos()).shape == (2, 0)
    assert c3.cosmologies_status.shape == (2,)


def test_the_w_theta_batches_are_as_they_were(no_device):
    """Correlation.correlation_hods went through a new helper: its scope messages are unchanged."""
    from chomp_amd import _lib, correlation, halo
    corr = correlation.Correlation.__new__(correlation.Correlation)
    corr.halo = halo.Halo(0.0, extrapolate=True)
    corr._power_name = "power_gg"
    with pytest.raises(_lib.ChompScopeError) as info:
        corr.correlation_hods(R, [ZEHAVI])
    assert str(info.value) == ("correlation_hods: an extrapolated spectrum (chomp_wtheta_epochs takes "
                               "none); use the loop set_hod / set_hod_object + correlation")


def test_design_routes(no_device, monkeypatch):
    from chomp_amd import _lib, correlation, halo, simulation_design
    SD = simulation_design.SimulationDesign
    c3 = _bare(halo.Halo(0.0))
    hod_only = {"log_M_min": [12.14, 11.9, 12.4], "log_M_1p": [13.43, 13.0, 13.9]}
    with_cosmo = dict(hod_only, sigma_8=[0.8, 0.7, 0.9])
    cosmo_only = {"sigma_8": [0.8, 0.7, 0.9]}
    # batched=None keeps the loop, whatever varies
    for params in (hod_only, with_cosmo, cosmo_only):
        assert SD(c3, "raw_correlation", params, 4, independent_var=R)._batched() is False

    calls = []

    def hods_batch(r, hods, with_status=False):
        calls.append(("hods", len(hods), [h["log_M_min"] for h in hods]))
        assert numpy.array_equal(r, R) and with_status
        out = numpy.arange(len(hods) * r.size, dtype=float).reshape(len(hods), r.size)
        return out, numpy.zeros(len(hods), dtype=numpy.uint32)

    def cosmologies_batch(r, cosmo_dicts, hods=None, with_status=False):
        calls.append(("cosmologies", [c["sigma_8"] for c in cosmo_dicts],
                      None if hods is None else [h["log_M_min"] for h in hods]))
        assert numpy.array_equal(r, R) and with_status
        n = len(cosmo_dicts)
        return (numpy.arange(n * r.size, dtype=float).reshape(n, r.size),
                numpy.zeros(n, dtype=numpy.uint32))

    def one(r):
        calls.append(("loop", c3.halo.get_hod()["log_M_min"]))
        return numpy.zeros(numpy.size(r))
    monkeypatch.setattr(c3, "raw_correlation_hods", hods_batch, raising=False)
    monkeypatch.setattr(c3, "raw_correlation_cosmologies", cosmologies_batch, raising=False)
    monkeypatch.setattr(c3, "raw_correlation", one, raising=False)

    # an HOD design: batched=True is one raw_correlation_hods call with the points' HODs
    numpy.random.seed(3)
    des = SD(c3, "raw_correlation", hod_only, 4, independent_var=R)
    frame, status = des.run_design(batched=True, with_status=True)
    assert calls == [("hods", 4, list(des.points["log_M_min"]))]
    assert frame.shape == (7, 4) and list(status.index) == list(des.points.index)
    assert numpy.array_equal(frame[2].values, numpy.arange(14.0, 21.0)) and not status.any()
    del calls[:]
    des.run_design()                                        # (None: the loop, as before)
    assert [c[0] for c in calls] == ["loop"] * 4 and des.design_status is None
    assert [c[1] for c in calls] == list(des.points["log_M_min"])
    del calls[:]
    des.run_design(batched=False)
    assert [c[0] for c in calls] == ["loop"] * 4
    del calls[:]

    # a cosmology (+ HOD) design: batched="cosmology" is one raw_correlation_cosmologies call
    des = SD(c3, "raw_correlation", with_cosmo, 3, independent_var=R)
    frame, status = des.run_design(batched="cosmology", with_status=True)
    assert calls == [("cosmologies", list(des.points["sigma_8"]), list(des.points["log_M_min"]))]
    assert frame.shape == (7, 3) and not status.any()
    del calls[:]
    des = SD(c3, "raw_correlation", cosmo_only, 3, independent_var=R)
    des.run_design(batched="cosmology")
    assert calls == [("cosmologies", list(des.points["sigma_8"]), None)]
    del calls[:]

    # what the routes refuse, each before anything is evaluated
    refused = [
        (SD(c3, "raw_correlation", with_cosmo, 3, independent_var=R), True, "a cosmology parameter varies"),
        (SD(c3, "raw_correlation", cosmo_only, 3, independent_var=R), True, "no HOD parameter varies"),
        (SD(c3, "raw_correlation", hod_only, 3, independent_var=R), "cosmology",
         "no cosmology parameter varies"),
        (SD(c3, "raw_correlation", dict(hod_only, c0=[9.0, 8.0, 10.0]), 3, independent_var=R), True,
         "a halo parameter varies"),
        (SD(c3, "raw_correlation", dict(with_cosmo, c0=[9.0, 8.0, 10.0]), 3, independent_var=R),
         "cosmology", "a halo parameter varies"),
        (SD(c3, "raw_correlation", hod_only, 3), True, "no independent_var"),
        (SD(c3, "correlation", hod_only, 3, independent_var=R), True, "the method is 'correlation'"),
        (SD(c3, "correlation", with_cosmo, 3, independent_var=R), "cosmology",
         "the method is 'correlation'"),
    ]
    for des, how, why in refused:
        with pytest.raises(_lib.ChompScopeError, match=re.escape(why)):
            des.run_design(batched=how)
    assert calls == []
    # ... the object's own scope included
    out = _bare(halo.Halo(0.0, extrapolate=True))
    with pytest.raises(_lib.ChompScopeError, match="raw_correlation_hods: an extrapolated"):
        SD(out, "raw_correlation", hod_only, 3, independent_var=R).run_design(batched=True)
    with pytest.raises(_lib.ChompScopeError, match="raw_correlation_cosmologies: an extrapolated"):
        SD(out, "raw_correlation", cosmo_only, 3, independent_var=R).run_design(batched="cosmology")

    # a subclass may evaluate something else under the same name: it keeps the refusal it had
    class Sub(correlation.Correlation3d):
        pass
    sub = _bare(halo.Halo(0.0), cls=Sub)
    with pytest.raises(_lib.ChompScopeError, match="Sub"):
        SD(sub, "raw_correlation", hod_only, 3, independent_var=R).run_design(batched=True)
    with pytest.raises(_lib.ChompScopeError, match="Sub"):
        SD(sub, "raw_correlation", cosmo_only, 3, independent_var=R).run_design(batched="cosmology")
    with pytest.raises(ValueError):
        SD(c3, "raw_correlation", cosmo_only, 3, independent_var=R).run_design(batched="hods")


def test_fixture_is_well_formed():
    g = load_golden("g35_xi_batch")
    assert numpy.array_equal(g["r"], R)
    assert numpy.array_equal(g["k_ranges"], [[1e-3, 100.0], [1e-3, 10.0]])
    g32, g34 = load_golden("g32_wtheta_hods"), load_golden("g34_wtheta_cosmologies")
    assert numpy.array_equal(g["zheng"], g32["zheng"]) and g["zheng"].shape == (3, 5)
    assert numpy.array_equal(g["mandelbaum"], g32["mandelbaum"]) and g["mandelbaum"].shape == (2,)
    assert numpy.array_equal(g["cosmo"], g34["cosmo"]) and g["cosmo"].shape == (3, 10)
    assert float(g["z_cosmo"]) == 0.5
    names = ["cosmo", "k_ranges", "mandelbaum", "r", "z_cosmo", "zheng"]
    for tag in ("full", "cut"):
        for prefix, n, spectra in (("xi", 4, ("power_gg", "power_gm")),
                                   ("xic", 3, ("power_mm", "power_gg"))):
            for ps in spectra:
                name = "%s_%s_%s" % (prefix, ps, tag)
                names.append(name)
                xi = g[name]
                assert xi.shape == (n, 7) and xi.dtype == numpy.float64
                assert numpy.all(numpy.isfinite(xi))
                # different HODs / cosmologies give different curves
                for i in range(n):
                    for j in range(i):
                        assert numpy.max(numpy.abs(xi[i] / xi[j] - 1)) > 1e-3, (name, i, j)
        # ... and so do the two k ranges
        assert rel_err(g["xi_power_gg_full"], g["xi_power_gg_cut"]) > 1e-3
    assert sorted(g.files) == sorted(names)
    for name in g.files:
        assert g[name].dtype.kind == "f", name


def _zheng_table(g, i, families):
    from oracle import chomp_oracle as o
    e = o.epoch(None, 0.0)
    hod = o.zheng(dict(zip(ZHENG_KEYS, (float(v) for v in g["zheng"][i]))))
    return o.halo_table(e, o.mass_table(e), hod, families=families)


@pytest.fixture(scope="module")
def oracle_cut():
    """The oracle's xi(r) and Romberg levels with k_max = 10: power_gg of the fixture's three Zheng
    HODs, then power_mm of its second cosmology at z = 0.5."""
    from oracle import chomp_oracle as o
    g = load_golden("g35_xi_batch")
    values, levels = [], []
    tables = [(_zheng_table(g, i, ("gg",)), "gg") for i in range(3)]
    e = o.epoch(dict(zip(COSMO_KEYS, (float(v) for v in g["cosmo"][1]))), float(g["z_cosmo"]))
    tables.append((o.halo_table(e, o.mass_table(e), families=("mm",)), "mm"))
    for t, fam in tables:
        lev = []
        values.append(o.xi3d_raw(lambda k: o.halo_power(t, fam, k), R, 1e-3, 10.0, levels=lev))
        levels.append([int(x) for x in lev])
    return g, numpy.array(values), numpy.array(levels)


@pytest.fixture(scope="module")
def oracle_full():
    """... and over the halo's own range, k_max = 100 (2^20 nodes per separation on the CPU: one
    Zheng row)."""
    from oracle import chomp_oracle as o
    g = load_golden("g35_xi_batch")
    t = _zheng_table(g, 1, ("gm",))
    lev = []
    xi = o.xi3d_raw(lambda k: o.halo_power(t, "gm", k), R, 1e-3, 100.0, levels=lev)
    return g, xi, numpy.array([int(x) for x in lev])


def test_oracle_reproduces_the_fixture(oracle_cut, oracle_full):
    """The bar tests/test_oracle.py holds xi3d_raw to, 1e-11."""
    g, values, _ = oracle_cut
    for i in range(3):
        err = rel_err(values[i], g["xi_power_gg_cut"][i])
        print("oracle against G35 power_gg cut HOD %d: %.2e" % (i, err))
        assert err < 1e-11, (i, err)
    err = rel_err(values[3], g["xic_power_mm_cut"][1])
    print("oracle against G35 power_mm cut cosmology 1: %.2e" % err)
    assert err < 1e-11, err
    g, xi, _ = oracle_full
    err = rel_err(xi, g["xi_power_gm_full"][1])
    print("oracle against G35 power_gm full HOD 1: %.2e" % err)
    assert err < 1e-11, err


def test_fixture_stops_early_and_late(oracle_cut, oracle_full):
    """With k_max = 10 the integrals stop between the first round of the device's Romberg group
    (levels up to 7 on 256 threads) and deep levels; over the halo's own range all of them run deep
    and some exhaust divmax = 20, the level of the node table."""
    _, _, levels = oracle_cut
    print("levels, k_max = 10:\n%s" % levels)
    assert levels.shape == (4, 7)
    assert numpy.any(levels[:3] <= 9) and numpy.any(levels[:3] >= 14)
    _, _, full = oracle_full
    print("levels, k_max = 100: %s" % full)
    assert full.shape == (7,)
    assert numpy.all(full >= 16) and numpy.any(full == 20)
