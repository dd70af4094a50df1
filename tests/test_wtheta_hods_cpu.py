"""Host side of the batch of w(theta) over many HODs: the C declaration and its binding, the
scope of Correlation.correlation_hods and of SimulationDesign's Correlation route, the HOD design
the reference ships (SimulationDesignHODWakeAssumptions) and the G32 fixture.  No device."""
import os
import re

import numpy
import pytest

from conftest import ROOT, load_golden

D2R = numpy.pi / 180.0
THETA = numpy.logspace(-3, 0, 5) * D2R
ZEHAVI = {"log_M_min": 12.14, "sigma": 0.15, "log_M_0": 12.14, "log_M_1p": 13.43, "alpha": 1.0}


class _Kernel(object):
    """What correlation_hods reads off a Kernel before any device work."""
    z_bar = 0.0
    _z_bar_override = None


def _bare(h, power_name="power_gg"):
    """A Correlation without its constructor's device work."""
    from chomp_amd import correlation
    corr = correlation.Correlation.__new__(correlation.Correlation)
    corr.kernel = _Kernel()
    corr.halo = h
    corr.D_z = 1.0
    corr._k_lim = (h._k_min, h._k_max)
    corr._power_name = power_name
    return corr


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to create a device context fails the test."""
    from chomp_amd import cosmology

    def boom(*a, **k):
        raise AssertionError("a device context was asked for")
    monkeypatch.setattr(cosmology, "_context", boom)


def test_header_declares_the_entry_point_and_the_knob():
    from chomp_amd import _lib
    with open(os.path.join(ROOT, "include", "chomp_mi355x.h")) as f:
        header = f.read()
    flat = re.sub(r"\s+", " ", header)
    assert ("int chomp_wtheta_epochs(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, "
            "double k_min, double k_max, double D_z, const double* theta, size_t n, double* out, "
            "int mem);") in flat
    assert re.search(r"#define CHOMP_TUNE_WTHETA_EPOCH_CHUNK 11\b", header)
    assert re.search(r"#define CHOMP_TUNE_COUNT 12\b", header)
    assert "chomp_wtheta_epochs" in _lib.EXPORTS
    assert _lib.TUNE_WTHETA_EPOCH_CHUNK == 11 and _lib.TUNE_COUNT == 12
    assert callable(_lib.Context.wtheta_epochs)


def _out_of_scope():
    """(label, Correlation, hods) of every case correlation_hods refuses."""
    from chomp_amd import cosmology, halo, hod
    # (HaloFit's constructor reads omega_m off the device: the class is what matters here)
    fit = halo.HaloFit.__new__(halo.HaloFit)
    fit.__dict__.update(halo.Halo(0.0).__dict__)
    cases = [("HaloFit", _bare(fit), [ZEHAVI]),
             ("HaloExclusion", _bare(halo.HaloExclusion(0.0)), [ZEHAVI]),
             ("HaloSuperSampleCovariance", _bare(halo.HaloSuperSampleCovariance(0.0)), [ZEHAVI]),
             ("general_profile", _bare(halo.Halo(0.0, general_profile=True)), [ZEHAVI]),
             ("extrapolat", _bare(halo.Halo(0.0, extrapolate=True)), [ZEHAVI])]
    h = halo.Halo(0.0, cosmo_single_epoch=cosmology.SingleEpoch(0.0, with_bao=True))
    cases.append(("with_bao", _bare(h), [ZEHAVI]))
    h = halo.Halo(0.0)
    h.set_halo(dict(h.get_halo(), c0=7.5))
    cases.append(("set_halo", _bare(h), [ZEHAVI]))
    cases.append(("hods[1]", _bare(halo.Halo(0.0)), [ZEHAVI, hod.HOD(dict(ZEHAVI))]))
    return cases


def test_correlation_hods_refuses_what_it_does_not_serve(no_device):
    from chomp_amd import _lib
    for label, corr, hods in _out_of_scope():
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)):
            corr.correlation_hods(THETA, hods)


def test_design_route_refuses_the_same(no_device):
    """Picked by itself (batched=None) an out-of-scope Correlation keeps the loop; the batched
    route forced on it raises before anything is launched."""
    from chomp_amd import _lib, simulation_design
    params = {"log_M_min": [12.14, 11.9, 12.4], "log_M_1p": [13.43, 13.0, 13.9]}
    for label, corr, hods in _out_of_scope():
        if label == "hods[1]":           # (a design builds its HODs itself)
            continue
        des = simulation_design.SimulationDesign(corr, "correlation", params, n_design=3,
                                                 independent_var=THETA)
        assert des._batched() is False, label
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)):
            des.run_design(batched=True)


def test_forced_batch_refuses_an_out_of_scope_design(no_device, monkeypatch):
    """batched=True on an in-scope Correlation but a design the batch does not serve -- a
    cosmology or halo parameter (or "alpha") beside the HOD's, another method, no independent
    variable, a subclass -- raises instead of dropping what a point sets."""
    from chomp_amd import _lib, correlation, halo, simulation_design
    SD = simulation_design.SimulationDesign
    corr = _bare(halo.Halo(0.0))

    def never(*a, **k):
        raise AssertionError("the batch was evaluated")
    monkeypatch.setattr(corr, "correlation_hods", never, raising=False)
    hod_only = {"log_M_min": [12.14, 11.9, 12.4]}

    class Sub(correlation.Correlation):
        pass
    sub = Sub.__new__(Sub)
    sub.__dict__.update(corr.__dict__)
    for des, why in (
            (SD(corr, "correlation", dict(hod_only, sigma_8=[0.8, 0.7, 0.9]), 3, independent_var=THETA),
             "cosmology parameter"),
            (SD(corr, "correlation", dict(hod_only, c0=[9.0, 8.0, 10.0]), 3, independent_var=THETA),
             "halo parameter"),
            (SD(corr, "correlation", dict(hod_only, alpha=[1.0, 0.8, 1.3]), 3, independent_var=THETA),
             "halo parameter"),
            (SD(corr, "correlation", {"sigma_8": [0.8, 0.7, 0.9]}, 3, independent_var=THETA),
             "no HOD parameter"),
            (SD(corr, "compute_correlation", hod_only, 3, independent_var=THETA), "method"),
            (SD(corr, "correlation", hod_only, 3), "independent_var"),
            (SD(sub, "correlation", hod_only, 3, independent_var=THETA), "Sub")):
        assert des._batched() is False
        with pytest.raises(_lib.ChompScopeError, match=why):
            des.run_design(batched=True)


def test_batched_only_for_hod_designs_of_correlation(no_device, monkeypatch):
    from chomp_amd import correlation, halo, simulation_design
    SD = simulation_design.SimulationDesign
    corr = _bare(halo.Halo(0.0))
    hod_only = {"log_M_min": [12.14, 11.9, 12.4], "log_M_1p": [13.43, 13.0, 13.9]}
    assert SD(corr, "correlation", hod_only, 4, independent_var=THETA)._batched() is True
    # ("alpha" names the halo profile's slope before the HOD's: a halo parameter to a design, as
    #  in simulation_design.py:77-98)
    assert SD(corr, "correlation", dict(hod_only, alpha=[1.0, 0.8, 1.3]), 4,
              independent_var=THETA)._batched() is False
    # a cosmology or a halo parameter among them, no independent variable, another method
    assert SD(corr, "correlation", dict(hod_only, sigma_8=[0.8, 0.7, 0.9]), 4,
              independent_var=THETA)._batched() is False
    assert SD(corr, "correlation", dict(hod_only, c0=[9.0, 8.0, 10.0]), 4,
              independent_var=THETA)._batched() is False
    assert SD(corr, "correlation", {"sigma_8": [0.8, 0.7, 0.9]}, 4,
              independent_var=THETA)._batched() is False
    assert SD(corr, "correlation", hod_only, 4)._batched() is False
    assert SD(corr, "compute_correlation", hod_only, 4, independent_var=THETA)._batched() is False

    class Sub(correlation.Correlation):
        pass
    sub = Sub.__new__(Sub)
    sub.__dict__.update(corr.__dict__)
    assert SD(sub, "correlation", hod_only, 4, independent_var=THETA)._batched() is False

    # run_design: the batch by default, the loop with batched=False
    calls = []

    def batch(theta, hods, with_status=False):
        calls.append(("batch", len(hods)))
        out = numpy.arange(len(hods) * theta.size, dtype=float).reshape(len(hods), theta.size)
        return out, numpy.zeros(len(hods), dtype=numpy.uint32)

    def one(theta):
        calls.append(("loop", corr.halo.get_hod()["log_M_min"]))
        return numpy.zeros(numpy.size(theta))
    monkeypatch.setattr(corr, "correlation_hods", batch, raising=False)
    monkeypatch.setattr(corr, "correlation", one, raising=False)
    numpy.random.seed(3)
    des = SD(corr, "correlation", hod_only, 4, independent_var=THETA)
    frame, status = des.run_design(with_status=True)
    assert calls == [("batch", 4)]
    assert frame.shape == (THETA.size, 4) and list(status.index) == list(des.points.index)
    assert numpy.array_equal(frame[2].values, numpy.arange(10.0, 15.0)) and not status.any()
    del calls[:]
    frame = des.run_design(batched=False)
    assert [c[0] for c in calls] == ["loop"] * 4 and des.design_status is None
    assert [c[1] for c in calls] == list(des.points["log_M_min"])


def test_wake_assumptions_derive_their_parameters(no_device):
    """simulation_design.py:275-293: set_hod writes the point's values into the HOD dictionary and
    then sets log_M_0 = log_M_min (line 291); set_cosmology closes the universe, omega_l0 = 1 -
    omega_m0 - omega_r0 (lines 281-282).  Each hands the dictionary to the object's setter."""
    from chomp_amd import defaults, simulation_design
    seen = simulation_design._Recorder()
    params = {"log_M_min": [12.14, 11.9, 12.4], "log_M_1p": [13.43, 13.0, 13.9],
              "sigma": [0.15, 0.05, 0.4]}
    numpy.random.seed(11)
    des = simulation_design.SimulationDesignHODWakeAssumptions(
        seen, "correlation", params, n_design=5, independent_var=THETA)
    assert des._vary_hod and not des._vary_cosmology and not des._vary_halo
    des._init_design_points()
    numpy.random.seed(11)
    lhs = simulation_design.random_lhs(5, 3)
    for i, (_, point) in enumerate(des.points.iterrows()):
        des._apply_point(point)
        assert seen.cosmo is None and seen.halo is None
        want = dict(defaults.default_hod_dict)
        for col, (name, (_, lo, hi)) in enumerate(params.items()):
            want[name] = lo + lhs[i, col] * (hi - lo)
            assert want[name] == pytest.approx(seen.hod[name], rel=1e-15)
            want[name] = seen.hod[name]
        want["log_M_0"] = want["log_M_min"]
        assert seen.hod == want
    # the caller's defaults are not written to
    assert defaults.default_hod_dict["log_M_0"] == 12.14
    cos = simulation_design.SimulationDesignHODWakeAssumptions(
        seen, "correlation", {"omega_m0": [0.27, 0.2, 0.35], "log_M_min": [12.14, 11.9, 12.4]},
        n_design=3, independent_var=THETA)
    cos._init_design_points()
    for _, point in cos.points.iterrows():
        cos._apply_point(point)
        c = seen.cosmo
        assert c["omega_m0"] == point["omega_m0"]
        assert c["omega_l0"] == 1.0 - point["omega_m0"] - c["omega_r0"]
        assert seen.hod["log_M_0"] == seen.hod["log_M_min"] == point["log_M_min"]
    assert cos._batched() is False


def test_fixture_is_well_formed():
    g = load_golden("g32_wtheta_hods")
    theta = g["theta"]
    assert theta.shape == (9,) and numpy.all(numpy.diff(theta) > 0)
    assert theta[0] == pytest.approx(1e-3 * D2R) and theta[-1] == pytest.approx(1.0 * D2R)
    assert g["zheng"].shape == (3, 5) and g["mandelbaum"].shape == (2,)
    assert list(g["zheng"][0]) == [ZEHAVI[k] for k in ("log_M_min", "sigma", "log_M_0", "log_M_1p", "alpha")]
    assert g["zheng"][1][1] == 0.05 and list(g["zheng"][2][3:]) == [13.8, 1.3]
    assert list(g["mandelbaum"]) == [12.8, 0.5]
    g6 = load_golden("g6_limber_galgal")
    assert float(g["z_bar"]) == float(g6["z_bar"]) and float(g["D_z"]) == float(g6["D_z"])
    for ps in ("power_gg", "power_gm"):
        w = g["w_" + ps]
        assert w.shape == (4, 9) and w.dtype == numpy.float64 and numpy.all(numpy.isfinite(w))
        # four different HODs give four different curves
        for i in range(4):
            for j in range(i):
                assert numpy.max(numpy.abs(w[i] / w[j] - 1)) > 1e-3, (ps, i, j)
    # the Zehavi row is the G6 curve where the two theta grids meet (every fourth of G6's 33)
    assert numpy.allclose(g6["theta"][::4], theta, rtol=1e-14)
    assert numpy.allclose(g["w_power_gg"][0], g6["w_power_gg"][::4], rtol=1e-9)
    for name in g.files:
        assert g[name].dtype.kind == "f", name
