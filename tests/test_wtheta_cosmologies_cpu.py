"""Host side of the batch of w(theta) over many cosmologies: the C declarations and their bindings,
the scope of Correlation.correlation_cosmologies and of SimulationDesign's batched="cosmology"
route, the flat-universe design the reference ships, HaloGrid.set_parameters(z=...) and the G34
fixture.  No device."""
import os
import re

import numpy
import pytest

from conftest import ROOT, load_golden

D2R = numpy.pi / 180.0
THETA = numpy.logspace(-3, 0, 5) * D2R
ZEHAVI = {"log_M_min": 12.14, "sigma": 0.15, "log_M_0": 12.14, "log_M_1p": 13.43, "alpha": 1.0}


class _Window(object):
    def __init__(self, dist=None):
        self._redshift_dist = dist


class _Kernel(object):
    """What correlation_cosmologies reads off a Kernel before any device work."""
    z_bar = 0.0
    _z_bar_override = None

    def __init__(self, dist_b=None):
        self.window_function_a = _Window()
        self.window_function_b = _Window(dist_b)


def _bare(h, power_name="power_gg", cls=None, kern=None):
    """A Correlation without its constructor's device work."""
    from chomp_amd import correlation
    cls = correlation.Correlation if cls is None else cls
    corr = cls.__new__(cls)
    corr.kernel = _Kernel() if kern is None else kern
    corr.halo = h
    corr.D_z = 1.0
    corr._k_lim = (h._k_min, h._k_max)
    corr._power_name = power_name
    return corr


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


def test_header_declares_the_entry_points():
    from chomp_amd import _lib
    with open(os.path.join(ROOT, "include", "chomp_mi355x.h")) as f:
        header = f.read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    for decl in (
            "int chomp_kernel_setup_sets(chomp_ctx* ctx, size_t n_set, const chomp_cosmo* cosmo , "
            "double me_z_min, double me_z_max, double ktheta_min, double ktheta_max, "
            "const chomp_window* a, const chomp_window* b, int bessel_order);",
            "int chomp_kernel_info_sets(chomp_ctx* ctx, double* out );",
            "int chomp_kernel_table_set(chomp_ctx* ctx, size_t set, int table, double* out, size_t n);",
            "int chomp_wtheta_sets(chomp_ctx* ctx, int which, size_t epoch0, size_t n_epoch, "
            "double k_min, double k_max, const double* D_z , const double* theta, size_t n, "
            "double* out, int mem);"):
        assert decl in flat, decl
    m = re.search(r"#define CHOMP_KERNEL_SETS_MAX (\d+)\b", header)
    assert m and int(m.group(1)) == _lib.KERNEL_SETS_MAX and _lib.KERNEL_SETS_MAX <= 65535
    with open(os.path.join(ROOT, "chomp_amd", "csrc", "chomp_proj_kernels.h")) as f:
        assert "kProjSetsMax = CHOMP_KERNEL_SETS_MAX" in f.read()
    for name in ("kernel_setup_sets", "kernel_info_sets", "kernel_table_set", "wtheta_sets"):
        assert "chomp_" + name in _lib.EXPORTS
        assert callable(getattr(_lib.Context, name))


def _out_of_scope():
    """(label, Correlation, cosmologies, hods) of every case correlation_cosmologies refuses."""
    from chomp_amd import cosmology, halo, hod, kernel
    fit = halo.HaloFit.__new__(halo.HaloFit)
    fit.__dict__.update(halo.Halo(0.0).__dict__)
    two = _cosmos()
    cases = [("HaloFit", _bare(fit), two, None),
             ("HaloExclusion", _bare(halo.HaloExclusion(0.0)), two, None),
             ("general_profile", _bare(halo.Halo(0.0, general_profile=True)), two, None),
             ("extrapolat", _bare(halo.Halo(0.0, extrapolate=True)), two, None)]
    h = halo.Halo(0.0, cosmo_single_epoch=cosmology.SingleEpoch(0.0, with_bao=True))
    cases.append(("with_bao", _bare(h), two, None))
    h = halo.Halo(0.0)
    h.set_halo(dict(h.get_halo(), c0=7.5))
    cases.append(("set_halo", _bare(h), two, None))
    cases.append(("hods[1]", _bare(halo.Halo(0.0)), two, [ZEHAVI, hod.HOD(dict(ZEHAVI))]))
    # what the cosmology axis adds
    moved = _bare(halo.Halo(0.0))
    moved.kernel._z_bar_override = 0.4
    cases.append(("assigned z_bar", moved, two, None))
    z = numpy.linspace(0.0, 2.0, 17)
    tab = kernel.dNdzInterpolation(z, z * z * numpy.exp(-z / 0.3))
    cases.append(("window_function_b has a tabulated redshift distribution (dNdzInterpolation)",
                  _bare(halo.Halo(0.0), kern=_Kernel(tab)), two, None))
    cases.append(("cosmology 1 has w0-wa", _bare(halo.Halo(0.0)),
                  [two[0], dict(two[1], w0=-0.9, wa=0.1)], None))
    return cases


def test_correlation_cosmologies_refuses_what_it_does_not_serve(no_device):
    from chomp_amd import _lib
    for label, corr, cosmos, hods in _out_of_scope():
        with pytest.raises(_lib.ChompScopeError, match=re.escape(label)) as info:
            corr.correlation_cosmologies(THETA, cosmos, hods=hods)
        assert str(info.value).startswith("correlation_cosmologies: ")
        assert "set_cosmology" in str(info.value)


def test_hods_refusals_keep_their_wording(no_device):
    """correlation_hods shares the scope function: its own messages are as they were."""
    from chomp_amd import _lib, halo
    corr = _bare(halo.Halo(0.0, extrapolate=True))
    with pytest.raises(_lib.ChompScopeError) as info:
        corr.correlation_hods(THETA, [ZEHAVI])
    assert str(info.value).startswith("correlation_hods: ")
    assert str(info.value).endswith("use the loop set_hod / set_hod_object + correlation")


def test_hods_must_match_the_points(no_device):
    from chomp_amd import halo
    with pytest.raises(ValueError, match="1 hods for 2 cosmologies"):
        _bare(halo.Halo(0.0)).correlation_cosmologies(THETA, _cosmos(), hods=[ZEHAVI])


def test_empty_inputs_need_no_device(no_device):
    from chomp_amd import halo
    corr = _bare(halo.Halo(0.0))
    out, words = corr.correlation_cosmologies(THETA, [], with_status=True)
    assert out.shape == (0, 5) and words.shape == (0,) and words.dtype == numpy.uint32
    assert corr.correlation_cosmologies(THETA[:0], _cosmos()).shape == (2, 0)
    assert corr.cosmologies_z_bar.shape == (2,)


def test_fourier_refuses_and_names_the_follow_up(no_device):
    from chomp_amd import _lib, correlation, halo
    corr = _bare(halo.Halo(0.0), cls=correlation.CorrelationFourier)
    with pytest.raises(_lib.ChompScopeError, match="chomp_cell_epochs"):
        corr.correlation_cosmologies(numpy.array([10.0, 100.0]), _cosmos())
    from chomp_amd import simulation_design
    des = simulation_design.SimulationDesign(corr, "correlation", {"sigma_8": [0.8, 0.7, 0.9]}, 3,
                                             independent_var=numpy.array([10.0, 100.0]))
    with pytest.raises(_lib.ChompScopeError, match="CorrelationFourier"):
        des.run_design(batched="cosmology")


def test_design_records_the_points(no_device, monkeypatch):
    """run_design(batched="cosmology") hands correlation_cosmologies one dictionary per point, the
    flat-universe tie included (simulation_design.py:223-241), and HODs only when they vary."""
    from chomp_amd import defaults, halo, simulation_design
    corr = _bare(halo.Halo(0.0))
    calls = []

    def batch(theta, cosmo_dicts, hods=None, with_status=False):
        calls.append(([dict(c) for c in cosmo_dicts], hods))
        n = len(cosmo_dicts)
        out = numpy.arange(n * theta.size, dtype=float).reshape(n, theta.size)
        words = numpy.zeros(n, dtype=numpy.uint32)
        words[1] = 1                                     # (a saturated mass-limit search)
        return out, words
    monkeypatch.setattr(corr, "correlation_cosmologies", batch, raising=False)
    monkeypatch.setattr(corr, "set_cosmology", lambda c: None, raising=False)   # (the centre point)
    params = {"omega_m0": [0.3, 0.25, 0.35], "sigma_8": [0.8, 0.7, 0.9]}
    numpy.random.seed(5)
    des = simulation_design.SimulationDesignFlatUniverse(corr, "correlation", params, n_design=4,
                                                         independent_var=THETA)
    from chomp_amd import _lib
    with pytest.warns(_lib.ChompParityWarning, match="design point 1"):
        frame, status = des.run_design(batched="cosmology", with_status=True)
    assert len(calls) == 1 and calls[0][1] is None
    assert frame.shape == (THETA.size, 4) and list(frame.columns) == list(des.points.index)
    assert numpy.array_equal(frame[2].values, numpy.arange(10.0, 15.0))
    assert list(status) == [0, 1, 0, 0] and status is des.design_status
    for c, (_, point) in zip(calls[0][0], des.points.iterrows()):
        want = dict(defaults.default_cosmo_dict, omega_m0=point["omega_m0"], sigma_8=point["sigma_8"])
        want["omega_l0"] = 1.0 - point["omega_m0"] - want["omega_r0"]
        assert c == want
    assert len({c["omega_m0"] for c in calls[0][0]}) == 4
    assert corr.halo is des._input_object.halo               # (the recorder is gone)
    # the caller's defaults are not written to
    assert defaults.default_cosmo_dict["omega_m0"] != calls[0][0][-1]["omega_m0"]
    # HOD parameters beside the cosmology's: one HOD per point
    del calls[:]
    des = simulation_design.SimulationDesign(
        corr, "correlation", dict(params, log_M_min=[12.14, 11.9, 12.4]), 3, independent_var=THETA)
    with pytest.warns(_lib.ChompParityWarning):
        des.run_design(batched="cosmology")
    hods = calls[0][1]
    assert len(hods) == 3 and [h["log_M_min"] for h in hods] == list(des.points["log_M_min"])
    assert [c["sigma_8"] for c in calls[0][0]] == list(des.points["sigma_8"])
    with pytest.raises(ValueError):
        des.run_design(batched="cosmologies")


def test_design_route_refuses_what_it_does_not_serve(no_device, monkeypatch):
    from chomp_amd import _lib, correlation, halo, simulation_design
    SD = simulation_design.SimulationDesign
    corr = _bare(halo.Halo(0.0))

    def never(*a, **k):
        raise AssertionError("the batch was evaluated")
    monkeypatch.setattr(corr, "correlation_cosmologies", never, raising=False)
    cosmo_only = {"sigma_8": [0.8, 0.7, 0.9]}

    class Sub(correlation.Correlation):
        pass
    sub = Sub.__new__(Sub)
    sub.__dict__.update(corr.__dict__)
    out = _bare(halo.Halo(0.0, extrapolate=True))
    for des, why in (
            (SD(corr, "correlation", dict(cosmo_only, c0=[9.0, 8.0, 10.0]), 3, independent_var=THETA),
             "halo parameter"),
            (SD(corr, "correlation", dict(cosmo_only, alpha=[1.0, 0.8, 1.3]), 3, independent_var=THETA),
             "halo parameter"),
            (SD(corr, "correlation", {"log_M_min": [12.14, 11.9, 12.4]}, 3, independent_var=THETA),
             "no cosmology parameter"),
            (SD(corr, "compute_correlation", cosmo_only, 3, independent_var=THETA), "method"),
            (SD(corr, "correlation", cosmo_only, 3), "independent_var"),
            (SD(sub, "correlation", cosmo_only, 3, independent_var=THETA), "Sub"),
            (SD(out, "correlation", cosmo_only, 3, independent_var=THETA), "extrapolat")):
        with pytest.raises(_lib.ChompScopeError, match=why):
            des.run_design(batched="cosmology")


def test_none_and_true_behave_as_before(no_device, monkeypatch):
    """batched=None keeps the loop for a cosmology design of a Correlation and batched=True
    refuses it, whatever batched="cosmology" would do."""
    from chomp_amd import _lib, halo, simulation_design
    corr = _bare(halo.Halo(0.0))
    calls = []

    def never(*a, **k):
        raise AssertionError("the batch was evaluated")

    def one(theta):
        calls.append(corr.seen["sigma_8"])
        return numpy.zeros(numpy.size(theta))
    monkeypatch.setattr(corr, "correlation_cosmologies", never, raising=False)
    monkeypatch.setattr(corr, "correlation", one, raising=False)
    monkeypatch.setattr(corr, "set_cosmology", lambda c: setattr(corr, "seen", dict(c)),
                        raising=False)
    numpy.random.seed(2)
    des = simulation_design.SimulationDesign(corr, "correlation", {"sigma_8": [0.8, 0.7, 0.9]}, 3,
                                             independent_var=THETA)
    assert des._batched() is False and des._batched_route() is None
    frame = des.run_design()
    assert frame.shape == (THETA.size, 3) and calls == list(des.points["sigma_8"])
    assert des.design_status is None
    with pytest.raises(_lib.ChompScopeError, match="no HOD parameter"):
        des.run_design(batched=True)
    both = simulation_design.SimulationDesign(
        corr, "correlation", {"sigma_8": [0.8, 0.7, 0.9], "log_M_min": [12.14, 11.9, 12.4]}, 3,
        independent_var=THETA)
    assert both._batched() is False
    with pytest.raises(_lib.ChompScopeError, match="cosmology parameter"):
        both.run_design(batched=True)


class _Ctx(object):
    """The Context a HaloGrid talks to, recording the set-up calls."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def pack_cosmo(c, n):
        return [("cosmo", c)] * n

    @staticmethod
    def pack_halo(h, n):
        return [("halo", h)] * n

    @staticmethod
    def pack_hod(h, n):
        return [("hod", h)] * n

    def epochs_set(self, cosmo, z, **kw):
        self.calls.append(("epochs_set", numpy.array(z)))

    def stage_k(self, *a, **k):
        self.calls.append(("stage_k",))

    def set_delta_b(self, db, e0):
        self.calls.append(("delta_b", numpy.array(db)))


def test_halo_grid_takes_new_redshifts(monkeypatch):
    from chomp_amd import cosmology, grid
    ctx = _Ctx()
    monkeypatch.setattr(cosmology, "_context", lambda **k: ctx)
    monkeypatch.setattr(cosmology, "_de_kw", lambda c: {})
    mine = numpy.array([0.1, 0.2, 0.3])
    hg = grid.HaloGrid(mine)
    hg.setup("power_mm")
    assert numpy.array_equal(ctx.calls[0][1], [0.1, 0.2, 0.3]) and hg._tables
    # without the keyword nothing changes
    hg.set_parameters(delta_b=0.01)
    assert hg._tables and numpy.array_equal(hg.z, [0.1, 0.2, 0.3])
    hg.set_parameters(z=[0.5, 0.6, 0.7])
    assert hg._tables == 0                                   # (takes effect at the next setup())
    assert numpy.array_equal(hg.z, [0.5, 0.6, 0.7]) and numpy.array_equal(hg.z_all, hg.z)
    assert numpy.array_equal(mine, [0.1, 0.2, 0.3])          # (the caller's array is not written to)
    del ctx.calls[:]
    hg.setup("power_mm")
    assert ctx.calls[0][0] == "epochs_set" and numpy.array_equal(ctx.calls[0][1], [0.5, 0.6, 0.7])
    assert numpy.array_equal(ctx.calls[-1][1], [0.01] * 3)   # (delta_b survives)
    hg.set_parameters(z=0.25, cosmo={"x": 1})
    assert numpy.array_equal(hg.z, [0.25] * 3) and hg._c_cosmo == [("cosmo", {"x": 1})] * 3
    with pytest.raises(ValueError):
        hg.set_parameters(z=[0.1, 0.2])
    # a sharded grid: this rank's epochs only
    part = grid.HaloGrid(numpy.array([0.1, 0.2, 0.3, 0.4]), rank=1, world=2)
    part.set_parameters(z=[0.9, 0.8])
    assert numpy.array_equal(part.z_all, [0.1, 0.9, 0.3, 0.8])


def test_fixture_is_well_formed():
    from params import c_dict
    g = load_golden("g34_wtheta_cosmologies")
    g32 = load_golden("g32_wtheta_hods")
    assert numpy.array_equal(g["theta"], g32["theta"])
    cosmo = g["cosmo"]
    assert cosmo.shape == (3, 10)
    keys = ("omega_m0", "omega_b0", "omega_l0", "omega_r0", "cmb_temp", "h", "sigma_8", "n_scalar",
            "w0", "wa")
    assert list(cosmo[0]) == [c_dict[k] for k in keys]
    # a flat-universe point; a point in sigma_8 and h; no dark energy anywhere
    assert cosmo[1][0] > cosmo[0][0] and cosmo[1][2] == 1.0 - cosmo[1][0] - cosmo[1][3]
    assert list(cosmo[2][5:7]) == [0.65, 0.9] and list(cosmo[2][:5]) == list(cosmo[0][:5])
    assert numpy.all(cosmo[:, 8] == -1.0) and numpy.all(cosmo[:, 9] == 0.0)
    assert g["z_bar"].shape == (3,) and g["D_z"].shape == (3,)
    assert numpy.all(g["z_bar"] < 0.5)                       # (well below 1: VERDICT.md's hazard)
    assert numpy.all((g["D_z"] > 0.5) & (g["D_z"] < 1.0))
    for ps in ("power_gg", "power_mm"):
        w = g["w_" + ps]
        assert w.shape == (3, 9) and w.dtype == numpy.float64 and numpy.all(numpy.isfinite(w))
        for i in range(3):
            for j in range(i):
                assert numpy.max(numpy.abs(w[i] / w[j] - 1)) > 1e-3, (ps, i, j)
    for name in g.files:
        assert g[name].dtype.kind == "f", name
