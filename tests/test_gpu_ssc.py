"""HaloSuperSampleCovariance on the MI355X (pytest -m gpu): the I_1^2 knot table of Stage K and
the response / P_mm_ssc of Stage E against the reference's G19 and the oracle composition."""
import numpy
import pytest

from conftest import load_golden, rel_err
from params import c_dict, c_dict_2, h_dict_2
from test_ssc_cpu import oracle_case, ssc_mm, ssc_response, ssc_table

pytestmark = pytest.mark.gpu

RTOL_KNOT = 1e-8
RTOL_E = 1e-7


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from chomp_amd import _lib
    _lib.lib()
    return _lib


def _check_case(h, g, tag):
    k = g["k"]
    assert rel_err(h._knots("i_1_2", h._flag_bits[-1][1]), g[tag + "i_1_2"]) < RTOL_KNOT
    resp = h.dln_power_ddelta_b(k)
    ref = g[tag + "resp"]
    out = ref == 0.0
    assert numpy.all(resp[out] == 0.0)                 # exact 0, not NaN, outside the range
    assert rel_err(resp[~out], ref[~out]) < RTOL_E
    mm_ssc = h.power_mm_ssc(k)
    mm = h.power_mm(k)
    lo = k < h._k_min
    assert numpy.array_equal(mm_ssc[lo], mm[lo])       # P_mm itself below k_min, bit for bit
    assert numpy.all(mm_ssc[k > h._k_max] == 0.0)
    nz = g[tag + "mm_ssc"] != 0.0
    assert rel_err(mm_ssc[nz], g[tag + "mm_ssc"][nz]) < RTOL_E


@pytest.mark.parametrize("z", [0.0, 0.5])
def test_default_knots_levels_and_spectra(lib, z):
    from chomp_amd import halo
    g = load_golden("g19_halo_ssc")
    tag = "z%03d_" % round(100 * z)
    h = halo.HaloSuperSampleCovariance(z, delta_b=float(g["delta_b"]))
    _check_case(h, g, tag)
    assert h._initialized_i_1_2 and h._initialized_h_m and h._initialized_pp_mm
    t = oracle_case(tag)
    assert numpy.array_equal(h._ctx.table("levels_i_1_2", 0), t.i_1_2_levels)
    assert h.status == 0


def test_tinker_alt_cosmology(lib):
    from chomp_amd import cosmology, halo, mass_function
    g = load_golden("g19_halo_ssc")
    cosmo = cosmology.SingleEpoch(0.3, c_dict_2)
    mass = mass_function.TinkerMassFunction(0.3, cosmo, h_dict_2)
    h = halo.HaloSuperSampleCovariance(0.3, None, cosmo, mass, h_dict_2,
                                       delta_b=float(g["delta_b"]))
    _check_case(h, g, "alt_")


def test_init_from_halo_and_stale_sequence(lib):
    from chomp_amd import halo
    g = load_golden("g19_halo_ssc")
    k = g["k"]
    src = halo.Halo(0.2, extrapolate=True)
    assert rel_err(src.power_mm(k)[k > 100.0], g["from_src_mm"][k > 100.0]) < 1e-4
    h = halo.HaloSuperSampleCovariance.init_from_halo(src, delta_b=float(g["delta_b"]))
    assert h._extrapolate is False and h._initialized_h_m and h._initialized_pp_mm
    assert float(h.power_mm(numpy.array([150.0]))[0]) == 0.0
    _check_case(h, g, "from_")
    # the copied tables are the source's, bit for bit
    for name in ("h_m", "pp_mm"):
        assert numpy.array_equal(h._ctx.table(name, 0), src._ctx.table(name, 0))
    s = halo.HaloSuperSampleCovariance(0.0, delta_b=float(g["delta_b"]))
    r0 = s.dln_power_ddelta_b(k)
    inside = g["stale_resp0"] != 0.0
    assert rel_err(r0[inside], g["stale_resp0"][inside]) < RTOL_E
    s.set_redshift(0.5)
    assert s._initialized_i_1_2 is True               # no setter resets it (halo.py:135-235)
    _check_case(s, g, "stale_")


def test_power_mm_ssc_as_the_first_call_and_after_set_redshift(lib):
    """power_mm_ssc with nothing built before it, and right after a setter that rebuilds the
    epoch (which resets the device's delta_b): the reference's values, not plain P_mm."""
    from chomp_amd import halo
    g = load_golden("g19_halo_ssc")
    k = g["k"]
    db = float(g["delta_b"])
    nz = g["z000_mm_ssc"] != 0.0
    h = halo.HaloSuperSampleCovariance(0.0, delta_b=db)
    got = h.power_mm_ssc(k)                           # the very first call
    assert rel_err(got[nz], g["z000_mm_ssc"][nz]) < RTOL_E
    assert numpy.all(got[~nz] == 0.0)
    h.set_redshift(0.5)                               # then straight to power_mm_ssc again
    got = h.power_mm_ssc(k)                           # (stale I_1^2 of z = 0, halo.py:135-235)
    nz = g["stale_mm_ssc"] != 0.0
    assert rel_err(got[nz], g["stale_mm_ssc"][nz]) < RTOL_E
    assert not numpy.allclose(got[nz], h.power_mm(k)[nz], rtol=1e-6, atol=0.0)
    h2 = halo.HaloSuperSampleCovariance(0.0, delta_b=db)
    h2.set_redshift(0.5)                              # a setter before anything was built
    got = h2.power_mm_ssc(k)
    nz = g["z050_mm_ssc"] != 0.0
    assert rel_err(got[nz], g["z050_mm_ssc"][nz]) < RTOL_E


def test_put_table_counts_for_its_epoch_only(lib):
    ctx = _ctx_setup(lib, lib.FAM_MM)
    ref = _ctx_setup(lib, lib.FAM_SSC)
    k = numpy.logspace(-3, 2, 64)
    ctx.put_table("i_1_2", ref.table("i_1_2", 0), 0)
    with pytest.raises(lib.ChompError):               # epoch 1 has no I_1^2 table
        ctx.power(lib.P_SSC_RESPONSE, k)
    assert numpy.array_equal(ctx.power(lib.P_SSC_RESPONSE, k, 0, 1), ref.power(lib.P_SSC_RESPONSE, k, 0, 1))
    ctx.put_table("i_1_2", ref.table("i_1_2", 1), 1)
    assert numpy.array_equal(ctx.power(lib.P_SSC_RESPONSE, k), ref.power(lib.P_SSC_RESPONSE, k))


def _ctx_setup(lib, tables, z=(0.0, 0.5), prec=None):
    from chomp_amd import cosmology, defaults
    p = dict(defaults.default_precision, **(prec or {}))
    cfg = lib.make_config(defaults.default_limits, p)
    ctx = lib.Context(cfg, device=cosmology._lib.current_device())
    n = len(z)
    ctx.epochs_set([c_dict] * n, numpy.asarray(z, dtype=float))
    ctx.stage_k([defaults.default_halo_dict] * n, lib.MF_ST, [defaults.default_halo_dict] * n,
                [__import__("chomp_amd").hod.HODZheng()] * n, tables)
    return ctx


def test_mm_tables_identical_with_and_without_i_1_2(lib):
    a = _ctx_setup(lib, lib.FAM_MM)
    b = _ctx_setup(lib, lib.FAM_SSC)
    k = numpy.logspace(-3, 2, 200)
    for e in (0, 1):
        for name in ("h_m", "pp_mm", "levels"):
            ta, tb = a.table(name, e), b.table(name, e)
            if name == "levels":
                ta, tb = ta[:2 * ta.size // 5], tb[:2 * tb.size // 5]
            assert numpy.array_equal(ta, tb)
    assert numpy.array_equal(a.power(lib.P_MM, k), b.power(lib.P_MM, k))
    # the codes: state and argument errors
    with pytest.raises(lib.ChompError):
        a.power(lib.P_SSC_RESPONSE, k)                # I_1^2 not built
    for bad in (lib.P_SSC_RESPONSE | lib.P_HALOFIT, lib.P_MM_SSC | lib.P_EXTRAPOLATE, 6, 7):
        with pytest.raises(ValueError):             # CHOMP_ERR_ARG
            b.power(bad, k)
    # delta_b = 0: P_mm_ssc is P_mm bit for bit
    assert numpy.array_equal(b.power(lib.P_MM_SSC, k), b.power(lib.P_MM, k))


def test_launch_shapes_agree_bit_for_bit(lib):
    import torch
    ctx = _ctx_setup(lib, lib.FAM_SSC, z=(0.0, 0.25, 0.5, 1.0))
    ctx.set_delta_b([0.01, -0.02, 0.03, 0.0])
    k = torch.logspace(-4.5, 3.5, 4096, dtype=torch.float64, device="cuda")
    for code in (lib.P_SSC_RESPONSE, lib.P_MM_SSC):
        ctx.set_tuning(lib.TUNE_E_STREAM_MIN, 1 << 40)      # row-walking grid kernel
        grid = ctx.power(code, k).cpu().numpy()
        ctx.set_tuning(lib.TUNE_E_STREAM_MIN, 0)            # streaming shape
        stream = ctx.power(code, k).cpu().numpy()
        ctx.power_plan(k)                                   # registered grid
        planned = ctx.power(code, k).cpu().numpy()
        ctx.set_tuning(lib.TUNE_E_STREAM_MIN, None)
        host = ctx.power(code, k.cpu().numpy())
        assert numpy.array_equal(grid, stream)
        assert numpy.array_equal(grid, planned)
        assert numpy.array_equal(grid, host)
        kk = k.cpu().numpy()
        if code == lib.P_SSC_RESPONSE:
            assert numpy.all(grid[:, (kk < 1e-3) | (kk > 100.0)] == 0.0)
        else:
            assert numpy.all(grid[:, kk > 100.0] == 0.0)


def test_deep_path_literal_vs_fast(lib):
    """halo_precision 1.48e-9 (as test_tight_halo_precision_lists_smooth_knots_too): I_1^2 knots
    run past the node tables.  A set-up without HOD groups evaluates them literally in the SELF
    instance of k_halo_knots_fast, which CHOMP_TUNE_DEEP_LITERAL does not change: the checker
    setting must leave every bit as it was (the route beside HOD groups is
    test_deep_i_1_2_knots_beside_hod_groups)."""
    prec = {"halo_precision": 1.48e-9}
    fast = _ctx_setup(lib, lib.FAM_SSC, z=(0.0,), prec=prec)
    lev = fast.table("levels_i_1_2", 0)
    assert lev.max() > 10, lev                        # some knot really went beyond the node tables
    assert fast.deep_stats()[1] > 0
    from chomp_amd import cosmology, defaults
    p = dict(defaults.default_precision, **prec)
    lit = lib.Context(lib.make_config(defaults.default_limits, p),
                      device=cosmology._lib.current_device())
    lit.set_tuning(lib.TUNE_DEEP_LITERAL, 1)
    lit.epochs_set([c_dict], numpy.array([0.0]))
    lit.stage_k([defaults.default_halo_dict], lib.MF_ST, [defaults.default_halo_dict],
                [__import__("chomp_amd").hod.HODZheng()], lib.FAM_SSC)
    assert numpy.array_equal(fast.table("i_1_2", 0), lit.table("i_1_2", 0))
    assert numpy.array_equal(lev, lit.table("levels_i_1_2", 0))
    # against the oracle at the same precision
    from oracle import chomp_oracle as o
    e = o.epoch(c_dict, 0.0, prec=p)
    t = ssc_table(o.halo_table(e, o.mass_table(e)))
    assert numpy.array_equal(lev, t.i_1_2_levels)
    assert rel_err(fast.table("i_1_2", 0), t.i_1_2) < RTOL_KNOT


def test_deep_i_1_2_knots_beside_hod_groups(lib):
    """With HOD groups in the same set-up (FAM_SSC | FAM_GG) the deep route is the fast level
    sums; k_halo_knots_fast hands the I_1^2 knots past the node tables to the literal list, whose
    instance evaluates them.  Knots and levels against the oracle, and the I_1^2 table equal to
    the one of a set-up without HOD groups."""
    prec = {"halo_precision": 1.48e-9}
    both = _ctx_setup(lib, lib.FAM_SSC | lib.FAM_GG, z=(0.0,), prec=prec)
    lev = both.table("levels_i_1_2", 0)
    assert lev.max() > 10
    assert both.deep_stats()[1] > 0                   # done by the literal evaluation
    alone = _ctx_setup(lib, lib.FAM_SSC, z=(0.0,), prec=prec)
    assert numpy.array_equal(both.table("i_1_2", 0), alone.table("i_1_2", 0))
    assert numpy.array_equal(lev, alone.table("levels_i_1_2", 0))
    from chomp_amd import defaults
    from oracle import chomp_oracle as o
    p = dict(defaults.default_precision, **prec)
    e = o.epoch(c_dict, 0.0, prec=p)
    t = ssc_table(o.halo_table(e, o.mass_table(e)))
    assert numpy.array_equal(lev, t.i_1_2_levels)
    assert rel_err(both.table("i_1_2", 0), t.i_1_2) < RTOL_KNOT
    k = numpy.logspace(-3, 2, 64)
    # (h_m and pp_mm knots past the node tables take the fast level sums beside HOD groups and
    #  the literal Romberg without them -- the same knots to the sums' self-check, 1e-9)
    assert rel_err(both.power(lib.P_SSC_RESPONSE, k), alone.power(lib.P_SSC_RESPONSE, k)) < 1e-8


def test_halo_grid_64_epochs_mixed(lib):
    from chomp_amd import grid, halo, cosmology
    n = 64
    z = numpy.linspace(0.0, 1.5, n)
    cos = [dict(c_dict, sigma_8=0.75 + 0.1 * (i % 4) / 3.0) for i in range(n)]
    db = numpy.linspace(-0.05, 0.05, n)
    hg = grid.HaloGrid(z, cosmo_dict=cos)
    hg.set_parameters(delta_b=db)
    k = numpy.logspace(-3.5, 2.5, 256)
    resp = hg.power("dln_power_ddelta_b", k)
    mm = hg.power("power_mm_ssc", k)
    # the single-object mirror (a one-epoch set-up: other launch shapes of the knot integrals,
    # so the knots agree to rounding -- as test_c2_full_grid_properties holds P_mm to 1e-12)
    for i in (0, 17, 40, 63):
        h = halo.HaloSuperSampleCovariance(z[i], cosmo_single_epoch=cosmology.SingleEpoch(z[i], cos[i]),
                                           delta_b=float(db[i]))
        r1, m1 = h.dln_power_ddelta_b(k), h.power_mm_ssc(k)
        assert numpy.array_equal(r1 == 0.0, resp[i] == 0.0)
        assert rel_err(resp[i][r1 != 0.0], r1[r1 != 0.0]) < 1e-12
        assert numpy.array_equal(m1 == 0.0, mm[i] == 0.0)
        assert rel_err(mm[i][m1 != 0.0], m1[m1 != 0.0]) < 1e-12
    # per-epoch delta_b: a new value needs no new set-up
    hg.set_parameters(delta_b=0.0)
    assert numpy.array_equal(hg.power("power_mm_ssc", k), hg.power("power_mm", k))
    from oracle import chomp_oracle as o
    for i in (0, 63):
        e = o.epoch(cos[i], float(z[i]))
        t = ssc_table(o.halo_table(e, o.mass_table(e)))
        ref = ssc_response(t, k)
        nz = ref != 0.0
        assert numpy.all(resp[i][~nz] == 0.0)
        assert rel_err(resp[i][nz], ref[nz]) < RTOL_E
        refm = ssc_mm(t, k, float(db[i]))
        nzm = refm != 0.0
        assert rel_err(mm[i][nzm], refm[nzm]) < RTOL_E


def test_get_put_round_trip(lib):
    ctx = _ctx_setup(lib, lib.FAM_SSC)
    ctx.set_delta_b([0.02, 0.04])
    k = numpy.logspace(-3.5, 2.5, 300)
    before = [ctx.power(c, k) for c in (lib.P_MM, lib.P_SSC_RESPONSE, lib.P_MM_SSC)]
    for name in ("h_m", "pp_mm", "i_1_2"):
        for e in (0, 1):
            ctx.put_table(name, ctx.table(name, e), e)
    after = [ctx.power(c, k) for c in (lib.P_MM, lib.P_SSC_RESPONSE, lib.P_MM_SSC)]
    for a, b in zip(before, after):
        assert numpy.array_equal(a, b)
