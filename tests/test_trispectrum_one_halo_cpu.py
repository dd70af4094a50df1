"""HaloTrispectrumOneHalo (halo_trispectrum.py:13-151) without a device: the reference's fixture
G24 against an oracle composition of i_0_4 and its table, the fixture's quirks, and the host side
of the mirror class.  oracle_tri(tag) also gives the GPU test the oracle's Romberg levels."""
import functools
import warnings

import numpy
import pytest

from conftest import load_golden, rel_err
from params import c_dict_2, h_dict_2

N = 50
MOMENT = {"z000_": 0, "z050_": 0, "gmmm_": 1, "ggmm_": 2, "gggm_": 3, "gggg_": 4, "mand_": 4,
          "alt_": 0, "mso_": 0}
TAGS = tuple(MOMENT)


def full(tri):
    """The 50 x 50 table from its stored upper triangle."""
    a = numpy.zeros((N, N))
    iu = numpy.triu_indices(N)
    a[iu] = tri
    a.T[iu] = tri
    return a


def _moments(tag, hod_dict):
    """(first, second) moments of the case's HOD (hod.py:156-299)."""
    from oracle import chomp_oracle as o
    if tag == "mand_":
        log_m0, w = hod_dict
        log_m_min = numpy.log10(3.0) + log_m0

        def sat(mass):
            return numpy.where(numpy.log10(mass) < log_m_min,
                               (mass / 10 ** log_m_min) ** 2 * w, mass / 10 ** log_m_min * w)

        def first(mass):
            return numpy.where(numpy.log10(mass) >= log_m0, 1.0, 0.0) + sat(mass)

        def second(mass):
            ns = sat(mass)
            return (2 + ns) * ns
        return first, second
    h = o.zheng()
    return (lambda m: o.zheng_first(h, m)), (lambda m: o.zheng_second(h, m))


def _nth(first, second, mass, n):
    """hod.py:68-92."""
    f = first(mass)
    out = f ** n
    with numpy.errstate(all="ignore"):
        a = numpy.where(f != 0.0, second(mass) / f ** 2, 0.0)
    for j in range(n):
        out *= (j * a - j + 1)
    return out


class _Case(object):
    """An oracle halo table with the i_0_4 integrand of halo_trispectrum.py:133-151; y(k, M) is
    memoised per (k, nodes), since every pair of a table integrates on the same nodes."""

    def __init__(self, tag, t, moment, first, second):
        self.t, self.moment, self.first, self.second = t, moment, first, second
        self._y = {}

    def n_of(self, mass):
        if self.moment == 0:
            return numpy.ones(mass.shape)
        if self.moment == 1:
            return self.first(mass)
        if self.moment == 2:
            return self.second(mass)
        return _nth(self.first, self.second, mass, self.moment)

    def y(self, ln_k, ln_nu):
        from oracle import chomp_oracle as o
        key = (float(ln_k), ln_nu.tobytes())
        if key not in self._y:
            mass = o.mass_of_nu(self.t.m, numpy.exp(ln_nu))
            self._y[key] = o.y_nfw(self.t, ln_k, mass)
        return self._y[key]

    def integrand(self, ln_nu, k1, k2, k3, k4):
        from oracle import chomp_oracle as o
        ln_nu = numpy.atleast_1d(numpy.asarray(ln_nu, dtype=float))
        nu = numpy.exp(ln_nu)
        mass = o.mass_of_nu(self.t.m, nu)
        ys = [self.y(numpy.log(k), ln_nu) for k in (k1, k2, k3, k4)]
        return (nu * o.f_nu(self.t.m, nu) * ys[0] * ys[1] * ys[2] * ys[3] * mass * mass * mass *
                self.n_of(mass))

    def i_0_4(self, k1, k2, k3, k4):
        """halo_trispectrum.py:60-95: (value, Romberg level)."""
        from oracle.romberg import romberg
        t, prec = self.t, self.t.e.prec
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            val, level = romberg(self.integrand, numpy.log(t.m.nu_min), numpy.log(t.m.nu_max),
                                 args=(k1, k2, k3, k4), vec_func=True,
                                 tol=prec["global_precision"], rtol=prec["halo_precision"],
                                 divmax=prec["divmax"], return_level=True)
        val = float(numpy.asarray(val).ravel()[0])
        return val / (t.rho_bar * t.rho_bar * t.rho_bar), level

    def table(self):
        """halo_trispectrum.py:104-123: the table and the levels of its entries."""
        tab = numpy.empty((N, N))
        lev = numpy.empty((N, N))
        for i in range(N):
            for j in range(i, N):
                k1, k2 = numpy.exp(self.t.ln_k[i]), numpy.exp(self.t.ln_k[j])
                v, lv = self.i_0_4(k1, k1, k2, k2)
                tab[i, j] = tab[j, i] = v
                lev[i, j] = lev[j, i] = lv
        return tab, lev


@functools.lru_cache(maxsize=None)
def oracle_case(tag):
    from oracle import chomp_oracle as o
    g = load_golden("g24_trispectrum_one_halo")
    if tag == "alt_":
        e = o.epoch(c_dict_2, 0.3)
        t = o.halo_table(e, o.mass_table(e, h_dict_2, kind="tinker"), halo_dict=h_dict_2)
    else:
        z = {"z000_": 0.0, "z050_": 0.5, "mso_": 0.2}.get(tag, 0.3)
        e = o.epoch(None, z)
        t = o.halo_table(e, o.mass_table(e))
    first, second = _moments(tag, g["mand_hod"] if tag == "mand_" else None)
    return _Case(tag, t, MOMENT[tag], first, second)


@functools.lru_cache(maxsize=None)
def oracle_tri(tag):
    """(table, levels, quadruple values, quadruple levels) of the oracle composition."""
    g = load_golden("g24_trispectrum_one_halo")
    c = oracle_case(tag)
    tab, lev = c.table()
    q = [c.i_0_4(*row) for row in g["quads"]]
    return tab, lev, numpy.array([v for v, _ in q]), numpy.array([lv for _, lv in q])


def spline_of(tab, ln_k):
    from scipy.interpolate import RectBivariateSpline
    return RectBivariateSpline(ln_k, ln_k, tab, kx=3, ky=3, s=0)


def parallelogram(spline, k_min, k_max, k1, k2):
    """halo_trispectrum.py:97-102."""
    k1 = numpy.where(k1 < k_min, k_min, k1)
    k2 = numpy.where(k2 < k_min, k_min, k2)
    return numpy.where(numpy.logical_and(k1 <= k_max, k2 <= k_max),
                       spline(numpy.log(k1), numpy.log(k2)), 0.0)


@pytest.mark.parametrize("tag", TAGS)
def test_g24_against_oracle_composition(tag):
    g = load_golden("g24_trispectrum_one_halo")
    tab, lev, q, qlev = oracle_tri(tag)
    t = oracle_case(tag).t
    assert rel_err(tab, full(g[tag + "table"])) < 1e-10
    assert rel_err(q, g[tag + "quad"]) < 1e-10
    assert abs(t.rho_bar / float(g[tag + "rho_bar"]) - 1) < 1e-12
    # the table's Romberg stops between levels 5 and 12 with the default precision
    assert lev.min() >= 5 and lev.max() <= 12 and qlev.max() < 20
    if tag + "scal" in g.files:
        sp = spline_of(tab, t.ln_k)
        got = numpy.array([parallelogram(sp, t.k_min, t.k_max, a, b).ravel()[0]
                           for a, b in g["pairs"]])
        ref = g[tag + "scal"]
        assert numpy.array_equal(got == 0.0, ref == 0.0)
        nz = ref != 0.0
        assert rel_err(got[nz], ref[nz]) < 1e-9


def test_g24_reference_numbers_and_quirks():
    g = load_golden("g24_trispectrum_one_halo")
    # the issue's numbers at z = 0
    assert abs(float(g["z000_default_0_1"]) / 4.93e10 - 1) < 1e-2
    p = [tuple(r) for r in g["pairs"]].index((0.5, 2.0))
    assert abs(g["z000_scal"][p] / 1.10e10 - 1) < 1e-2
    # 1-D arguments: the k_max mask zeroes the last COLUMN; the row with k1 = 200 > k_max
    # holds spline values (FITPACK clamps to the last knot)
    out = g["arr_out"]
    assert tuple(g["arr_shape"]) == (3, 3)
    assert numpy.all(out[:, 2] == 0.0) and numpy.all(out[2, :2] > 0.0)
    assert tuple(g["arr_col_shape"]) == (3, 3) and tuple(g["arr_row_shape"]) == (1, 3)
    # the stale sequence: set_redshift raised after moving the halo, the flag stayed True and
    # the z = 0 table was served; i_0_4 itself is computed at the new redshift
    assert int(g["stale_raised"]) == 1 and float(g["stale_redshift"]) == 0.5
    assert int(g["stale_flag"]) == 1
    assert numpy.array_equal(g["stale_scal"], g["z000_scal"])
    assert rel_err(g["stale_quad"], g["z050_quad"][:8]) < 1e-14
    # with a PerturbationTheory the table is rebuilt at the new redshift
    assert int(g["rebuilt_flag"]) == 0
    assert numpy.array_equal(g["rebuilt_scal"], g["z050_scal"])


def test_mirror_surface_without_device():
    import chomp_amd
    from chomp_amd import _lib, halo, halo_trispectrum, hod
    assert "halo_trispectrum" in chomp_amd.__all__
    assert chomp_amd.halo_trispectrum is halo_trispectrum
    h = halo_trispectrum.HaloTrispectrumOneHalo(0.5)
    assert isinstance(h, halo.Halo)
    assert h.power_spec == "power_mmmm" and h.pert is None and h._initialized_i_0_4 is False
    assert isinstance(h.local_hod, hod.HODZheng) and h.get_redshift() == 0.5
    for name in ("trispectrum", "trispectrum_parallelogram", "i_0_4", "i_0_4_parallelogram",
                 "i_0_4_many", "set_cosmology", "set_redshift"):
        assert callable(getattr(h, name))
    assert halo_trispectrum.HaloTrispectrumOneHalo(0.0, power_spec="power_gggm")._moment() == 3
    assert halo_trispectrum.HaloTrispectrumOneHalo(0.0, power_spec="other")._moment() == 0
    mand = hod.HODMandelbaum({"log_M_0": 12.14, "w": 1.0})
    assert halo_trispectrum.HaloTrispectrumOneHalo(0.0, input_hod=mand).local_hod is mand
    with pytest.raises(_lib.ChompScopeError):
        halo_trispectrum.HaloTrispectrumOneHalo(0.0, input_hod=hod.HODPoisson())
    with pytest.raises(_lib.ChompScopeError):
        halo_trispectrum.HaloTrispectrumOneHalo(0.0, halo_dict=dict(h_dict_2, alpha=-1.5))
    with pytest.raises(_lib.ChompScopeError):
        halo_trispectrum.HaloTrispectrum(0.0)
    with pytest.raises(AttributeError):          # (the reference: no spline before the build)
        h.i_0_4_parallelogram(1.0, 1.0)
    with pytest.raises(ValueError):
        h.i_0_4_many(numpy.ones((3, 3)))
    # set_redshift with pert=None raises after the halo has moved, the flag untouched
    h._initialized_i_0_4 = True
    with pytest.raises(AttributeError):
        h.set_redshift(0.2)
    assert h.get_redshift() == 0.2 and h._initialized_i_0_4 is True


def test_abi_constants():
    from chomp_amd import _lib
    for name in ("chomp_tri1h_setup", "chomp_tri1h_eval", "chomp_tri1h_quad"):
        assert name in _lib.EXPORTS
    assert _lib.ST_TRI1H_DIVMAX == 0x40
    assert _lib.TRI_MOMENT == {"power_mmmm": 0, "power_gmmm": 1, "power_ggmm": 2,
                               "power_gggm": 3, "power_gggg": 4}
    assert any("trispectrum" in s for s in _lib.describe_status(_lib.ST_TRI1H_DIVMAX))
    import os
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include",
                            "chomp_mi355x.h")).read()
    assert "#define CHOMP_ST_TRI1H_DIVMAX 0x40u" in hdr
    for i, n in enumerate(("MMMM", "GMMM", "GGMM", "GGGM", "GGGG")):
        assert "#define CHOMP_TRI_%s %d" % (n, i) in hdr
