"""Host side of the batch of C_l over many HODs: the C declaration and its binding, the scope of
CorrelationFourier.correlation_hods and of SimulationDesign's route for it, and the G33 fixture --
its shape, the oracle's agreement with it and the Romberg levels that make the device test visit
every route of the C_l kernels.  No device."""
import os
import re

import numpy
import pytest

from conftest import ROOT, load_golden

ELL = numpy.logspace(1, 4, 5)
ZEHAVI = {"log_M_min": 12.14, "sigma": 0.15, "log_M_0": 12.14, "log_M_1p": 13.43, "alpha": 1.0}
ZHENG_KEYS = ("log_M_min", "sigma", "log_M_0", "log_M_1p", "alpha")


class _Kernel(object):
    """What correlation_hods reads off a Kernel before any device work."""
    z_bar = 0.0
    _z_bar_override = None


def _bare(h, power_name="power_gg", cls=None):
    """A CorrelationFourier without its constructor's device work (it has no k range)."""
    from chomp_amd import correlation
    cls = correlation.CorrelationFourier if cls is None else cls
    corr = cls.__new__(cls)
    corr.kernel = _Kernel()
    corr.halo = h
    corr.D_z = 1.0
    corr._power_name = power_name
    return corr


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
    assert ("int chomp_cell_epochs(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, "
            "double D_z, const double* ell, size_t n, double* out, int mem);") in flat
    # no new knob: the chunk of both batched projections is knob 11
    assert re.search(r"#define CHOMP_TUNE_COUNT 12\b", header)
    assert "chomp_cell_epochs" in _lib.EXPORTS
    assert _lib.TUNE_COUNT == 12
    assert callable(_lib.Context.cell_epochs)


def _out_of_scope():
    """(label, CorrelationFourier, hods) of every case correlation_hods refuses: the cases of
    tests/test_wtheta_hods_cpu.py."""
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
    cases = _out_of_scope()
    assert len(cases) == 8
    for label, corr, hods in cases:
        assert not hasattr(corr, "_k_lim")
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)):
            corr.correlation_hods(ELL, hods)


def test_design_route(no_device, monkeypatch):
    from chomp_amd import _lib, correlation, halo, simulation_design
    SD = simulation_design.SimulationDesign
    cf = _bare(halo.Halo(0.0))
    hod_only = {"log_M_min": [12.14, 11.9, 12.4], "log_M_1p": [13.43, 13.0, 13.9]}
    assert SD(cf, "correlation", hod_only, 4, independent_var=ELL)._batched() is True
    # a cosmology or a halo parameter among the HOD's, no independent variable, another method
    assert SD(cf, "correlation", dict(hod_only, sigma_8=[0.8, 0.7, 0.9]), 4,
              independent_var=ELL)._batched() is False
    assert SD(cf, "correlation", dict(hod_only, c0=[9.0, 8.0, 10.0]), 4,
              independent_var=ELL)._batched() is False
    assert SD(cf, "correlation", hod_only, 4)._batched() is False
    assert SD(cf, "compute_correlation", hod_only, 4, independent_var=ELL)._batched() is False

    # a subclass may evaluate something else under the same name: the loop, and the refusal of the
    # forced batch names the class
    class Sub(correlation.CorrelationFourier):
        pass
    sub = _bare(halo.Halo(0.0), cls=Sub)
    des = SD(sub, "correlation", hod_only, 4, independent_var=ELL)
    assert des._batched() is False
    with pytest.raises(_lib.ChompScopeError, match="Sub"):
        des.run_design(batched=True)

    # run_design: the batch, once, by default; the loop with batched=False
    calls = []

    def batch(ell, hods, with_status=False):
        calls.append(("batch", len(hods)))
        assert numpy.array_equal(ell, ELL)
        out = numpy.arange(len(hods) * ell.size, dtype=float).reshape(len(hods), ell.size)
        return out, numpy.zeros(len(hods), dtype=numpy.uint32)

    def one(ell):
        calls.append(("loop", cf.halo.get_hod()["log_M_min"]))
        return numpy.zeros(numpy.size(ell))
    monkeypatch.setattr(cf, "correlation_hods", batch, raising=False)
    monkeypatch.setattr(cf, "correlation", one, raising=False)
    numpy.random.seed(3)
    des = SD(cf, "correlation", hod_only, 4, independent_var=ELL)
    frame, status = des.run_design(with_status=True)
    assert calls == [("batch", 4)]
    assert frame.shape == (ELL.size, 4) and list(status.index) == list(des.points.index)
    assert numpy.array_equal(frame[2].values, numpy.arange(10.0, 15.0)) and not status.any()
    del calls[:]
    des.run_design(batched=False)
    assert [c[0] for c in calls] == ["loop"] * 4 and des.design_status is None
    assert [c[1] for c in calls] == list(des.points["log_M_min"])


def test_fixture_is_well_formed():
    g = load_golden("g33_cell_hods")
    ell = g["ell"]
    assert ell.shape == (22,)
    assert numpy.array_equal(ell, numpy.concatenate([numpy.logspace(1, 4, 19), [8000., 9000., 9500.]]))
    g32 = load_golden("g32_wtheta_hods")
    assert numpy.array_equal(g["zheng"], g32["zheng"]) and g["zheng"].shape == (3, 5)
    assert numpy.array_equal(g["mandelbaum"], g32["mandelbaum"]) and g["mandelbaum"].shape == (2,)
    g6 = load_golden("g6_limber_galgal")
    assert float(g["z_bar"]) == float(g6["z_bar"]) and float(g["D_z"]) == float(g6["D_z"])
    for ps in ("power_gg", "power_gm"):
        cl = g["cl_" + ps]
        assert cl.shape == (4, 22) and cl.dtype == numpy.float64 and numpy.all(numpy.isfinite(cl))
        # four different HODs give four different curves
        for i in range(4):
            for j in range(i):
                assert numpy.max(numpy.abs(cl[i] / cl[j] - 1)) > 1e-3, (ps, i, j)
    assert sorted(g.files) == ["D_z", "cl_power_gg", "cl_power_gm", "ell", "mandelbaum", "z_bar",
                               "zheng"]
    for name in g.files:
        assert g[name].dtype.kind == "f", name


@pytest.fixture(scope="module")
def oracle_rows():
    """The oracle's C_l and Romberg levels for power_gg of the fixture's three Zheng HODs (the
    recipe of tests/test_gpu_next.py for the G6 projection, with the HOD)."""
    from oracle import chomp_oracle as o
    g = load_golden("g33_cell_hods")
    d2r = numpy.pi / 180.0
    me = o.multi_epoch(0.0, 5.0)
    ow = o.window_table("galaxy", o.dndz_maglim(0.0, 2.0, 2.0, 0.3, 2.0), me)
    kt = o.kernel_table(1e-6 * d2r, 100 * d2r, ow, ow, me)
    e = o.epoch(None, kt.z_bar)
    m = o.mass_table(e)
    values, levels = [], []
    for row in g["zheng"]:
        t = o.halo_table(e, m, o.zheng(dict(zip(ZHENG_KEYS, (float(v) for v in row)))),
                         families=("gg",))
        lev = []
        values.append(numpy.asarray(
            o.cell(kt, lambda k: o.halo_power(t, "gg", k), g["ell"], float(g["D_z"]), levels=lev)))
        levels.append([int(x) for x in lev])
    return g, numpy.array(values), numpy.array(levels)


def test_oracle_reproduces_the_fixture(oracle_rows):
    """The bar tests/test_gpu_projection.py holds the device to, 1e-9."""
    g, values, levels = oracle_rows
    assert values.shape == (3, 22)
    for i in range(3):
        err = numpy.max(numpy.abs(values[i] / g["cl_power_gg"][i] - 1))
        print("oracle against G33 power_gg HOD %d: %.2e" % (i, err))
        assert err < 1e-9, (i, err)


def test_fixture_covers_every_route(oracle_rows):
    """The levels at which the integrals stop decide the route of a multipole on the device: up to
    8 a wavefront's own levels, 9..11 the block's cooperative walk, 12 and beyond the deep kernel
    and its per-epoch lists.  All three must occur, and two HODs must list different multipoles for
    the deep kernel, or the device test would pass without an epoch axis on the lists."""
    g, values, levels = oracle_rows
    print("levels:\n%s" % levels)
    assert levels.shape == (3, 22)
    assert numpy.any(levels <= 8)
    assert numpy.any((levels >= 9) & (levels <= 11))
    assert numpy.any(levels >= 12)
    deep = [frozenset(numpy.nonzero(row >= 12)[0]) for row in levels]
    assert len(set(deep)) >= 2, deep
