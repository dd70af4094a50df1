"""The halo-model physics of chomp_amd/csrc/chomp_math.h AS COMPILED FOR THE DEVICE
(tests/devcheck/devphys.hip, the product's compiler flags) against mpmath at 50 digits: the epoch
background, both Eisenstein-Hu transfer functions and the power forms built on them, the
sigma(R) integrands, f(nu) / b(nu) and mf_node, the Zheng and Mandelbaum moments with their node
forms and step decisions, the three forms of the NFW transform, the exclusion window and
linspace_at -- what tests/test_hostmath.py checks for the g++ build only (no FMA contraction,
glibc's log10 / erf / pow / cbrt, one cosmology).

The references evaluate the formula the reference code states (the cosmology.py /
mass_function.py / hod.py / halo.py lines chomp_math.h cites beside each function) on the same
double inputs and, for the per-function checks, on the Epoch constants read back from the
device; test_epoch_constants compares those constants with mpmath from the raw inputs.

Every tolerance is one of three kinds, named beside it: [project] a bound test_hostmath.py
asserts for the host build; [derived] a first-order propagated bound times two; [measured] K =
twice the maximum measured against mpmath, rounded up to a power of two (the measured maxima
are in DESIGN.md section 3).  Each test prints what it measured before it asserts."""
import ctypes

import mpmath
import numpy
import pytest

import devcheck_build as dcb
from devcheck_build import call, ptr
import hostcheck_build
from params import c_dict
from oracle import chomp_oracle as o

pytestmark = pytest.mark.gpu

mp = mpmath.mp.clone()
mp.dps = 50
EPS = 2.0 ** -52
INF = numpy.inf
LOG10E = 0.43429448190325182765


def M(x):
    return mp.mpf(float(x))


COSMO_KEYS = ("omega_m0", "omega_b0", "omega_l0", "omega_r0", "cmb_temp", "h", "sigma_8",
              "n_scalar")
COSMOS = {
    "default": o.default_cosmo_dict,
    "alt": dict(o.default_cosmo_dict, omega_m0=0.22563, omega_b0=0.04499, omega_l0=0.77429,
                h=0.7203, sigma_8=0.70574, n_scalar=0.93183),
    # the cosmology the w0-wa goldens vary (tests/golden/params.py); the Epoch is filled at
    # w = -1, and test_E0_de drives its dark-energy E0 at DE_W0, DE_WA
    "golden": c_dict,
}
DE_W0, DE_WA = -0.9, 0.2          # case "a_" of tests/golden/make_golden_de.py
REDSHIFTS = (0.0, 0.5, 1.5, 3.0)
DELTA_VS = (200.0, 300.0, 800.0, 1600.0)
ST = dict(kind=0, stq=0.3, st_a=0.707, f_norm=0.3222, bias_norm=1.0)
# Tinker10 parameters at delta_v = 200 (mass_function.py:466-480 at z = 0)
TINKER = dict(kind=1, t_alpha=0.368, t_beta=0.589, t_gamma=0.864, t_phi=-0.729, t_eta=-0.243,
              f_norm=1.0, bias_norm=1.0)
ZHENG = dict(model=0, log_M_min=12.14, sigma=0.15, log_M_0=12.14, log_M_1p=13.43, alpha=1.0,
             w=0.0)


@pytest.fixture(scope="module")
def dp():
    return dcb.load("devphys")


class Ep:
    """An Epoch filled on the device (dp_epoch) and read back whole."""

    def __init__(self, L, cosmo, z, with_bao=0, mf=None, delta_v=200.0, halo=None, hod=None,
                 sigma_norm=1.0, shape_only=0, cosmo_precision=1.48e-8, k_min=0.001, k_max=100.0,
                 m_star=2.1e12):
        mf = dict(ST if mf is None else mf)
        halo = dict(c0=9.0, beta=-0.13, delta_v=-1.0) if halo is None else halo
        hod = dict(ZHENG if hod is None else hod)
        v = numpy.zeros(L.dp_epoch_inputs())
        v[:8] = [cosmo[k] for k in COSMO_KEYS]
        v[8:14] = [z, cosmo_precision, k_min, k_max, with_bao, sigma_norm]
        v[14:20] = [mf["kind"], mf.get("stq", 0.0), mf.get("st_a", 1.0), mf["f_norm"],
                    mf["bias_norm"], delta_v]
        v[20:25] = [mf.get(k, 1.0) for k in ("t_alpha", "t_beta", "t_gamma", "t_phi", "t_eta")]
        v[25:29] = [m_star, halo["c0"], halo["beta"], halo["delta_v"]]
        v[29:36] = [hod["model"], hod.get("log_M_min", 0.0), hod.get("sigma", 0.0),
                    hod["log_M_0"], hod.get("log_M_1p", 13.0), hod.get("alpha", 1.0), hod["w"]]
        v[36] = shape_only
        self.inputs = v
        self.buf = numpy.zeros(L.dp_sizeof_epoch(), dtype=numpy.uint8)
        call(L, "dp_epoch", ptr(v), self.buf.ctypes.data_as(ctypes.c_void_p))
        self._fields = dcb.epoch_fields(L)

    @property
    def p(self):
        return self.buf.ctypes.data_as(ctypes.c_void_p)

    def __getattr__(self, name):
        try:
            off, is_int = self.__dict__["_fields"][name]
        except KeyError:
            raise AttributeError(name)
        return (int(self.buf[off:off + 4].view(numpy.int32)[0]) if is_int
                else float(self.buf[off:off + 8].view(numpy.float64)[0]))


def _rel(a, b):
    a, b = numpy.asarray(a, dtype=float), numpy.asarray(b, dtype=float)
    return float(numpy.max(numpy.abs(a - b) / numpy.maximum(numpy.abs(b), 1e-300)))


def _fl(seq):
    return numpy.array([float(v) for v in seq])


def _ulp(x):
    x = numpy.abs(numpy.asarray(x, dtype=float))
    return numpy.nextafter(x, INF) - x


# -------------------------------------------------------------------------------------------
# mpmath: the formulas
# -------------------------------------------------------------------------------------------
def mp_E0(om0, ol0, or0, z):                                  # cosmology.py:165-178
    a = 1 / (1 + M(z))
    return M(ol0) + M(om0) / a ** 3 + M(or0) / a ** 4


def mp_growth_approx(om0, ol0, a):                             # cosmology.py:215-231
    om = M(om0) / a ** 3
    den = M(ol0) + om
    Om, Ol = om / den, M(ol0) / den
    return (5 * Om / (2 / a)) / (Om * (M(4) / 7) - Ol + (1 + Om / 2) * (1 + Ol / 70))


def mp_background(c, z, cosmo_precision=1.48e-8):
    """cosmology.py:39-119, 375-447, 460-466 from the raw inputs."""
    om0, ob0, ol0, or0, tcmb, h, _, ns = [c[k] for k in COSMO_KEYS]
    r = {}
    r["H0"] = M(100.0) / (M(2.998) * M(100000.0))
    r["ln_H0"] = mp.log(r["H0"])
    tot = M(om0) + M(ol0) + M(or0)
    flat = abs(tot - 1) <= M(cosmo_precision)
    opn = tot <= 1 - M(cosmo_precision)
    r["delta_H"] = (M(1.94e-5) * M(om0) ** (M(-0.785) - M(0.05) * mp.log(M(om0))) *
                    mp.exp(M(-0.95) * (M(ns) - 1) - M(0.169) * (M(ns) - 1) ** 2))
    r["growth_norm"] = mp_growth_approx(om0, ol0, mp.mpf(1))
    r["growth"] = mp_growth_approx(om0, ol0, 1 / (1 + M(z))) / r["growth_norm"]
    r["E0z"] = mp_E0(om0, ol0, or0, z)
    r["omega_m_z"] = M(om0) * (1 + M(z)) ** 3 / r["E0z"]
    r["omega_l_z"] = M(ol0) / r["E0z"]
    dc = M(0.15) * (12 * mp.pi) ** (M(2) / 3)
    dv = M(178.0)
    if opn:
        dc *= r["omega_m_z"] ** M(0.0185)
        dv /= r["omega_m_z"] ** M(0.7)
    if flat and om0 < 1.0001:
        dc *= r["omega_m_z"] ** M(0.0055)
        dv /= r["omega_m_z"] ** M(0.55)
    r["delta_c"] = dc
    r["delta_v"] = dv / r["growth"]
    r["rho_bar"] = (M(1.879) / M(1.989) * M(3.086) ** 3 * M(1e10) * r["E0z"]) * r["omega_m_z"]
    Omh2 = M(om0) * M(h) ** 2
    ratio = M(ob0) / M(om0)
    r["eh_theta"] = M(tcmb) / M(2.7)
    r["eh_s"] = M(44.5) * mp.log(M(9.83) / Omh2) / mp.sqrt(11)
    r["eh_alpha"] = (1 - M(0.328) * mp.log(431 * Omh2) * ratio +
                     M(0.38) * mp.log(M(22.3) * Omh2) * ratio ** 2)
    r["eh_omh"] = M(om0) * M(h)
    r["amp"] = r["delta_H"] ** 2 / M(h) * r["growth"] ** 2
    return r


def mp_bao_constants(c):
    """cosmology.py:484-527."""
    om0, ob0, _, _, tcmb, h, _, _ = [M(c[k]) for k in COSMO_KEYS]
    theta = tcmb / M(2.7)
    Ob, Om, Oc = ob0, om0, om0 - ob0
    Obh2, Oh2, ObO = Ob * h * h, Om * h * h, Ob / Om
    zeq = M(2.5e4) * Oh2 / theta ** 4
    keq = M(7.46e-2) * Oh2 / theta ** 2
    b1 = M(0.313) * Oh2 ** M(-0.419) * (1 + M(0.607) * Oh2 ** M(0.674))
    b2 = M(0.238) * Oh2 ** M(0.223)
    zd = 1291 * (Oh2 ** M(0.251) / (1 + M(0.659) * Oh2 ** M(0.828))) * (1 + b1 * Obh2 ** b2)
    Req = M(31.5) * Obh2 / theta ** 4 * (1000 / zeq)
    Rd = M(31.5) * Obh2 / theta ** 4 * (1000 / zd)
    s = (2 / (3 * keq)) * mp.sqrt(6 / Req) * mp.log(
        (mp.sqrt(1 + Rd) + mp.sqrt(Rd + Req)) / (1 + mp.sqrt(Req)))
    kSilk = M(1.6) * Obh2 ** M(0.52) * Oh2 ** M(0.73) * (1 + (M(10.4) * Oh2) ** M(-0.95))
    y = (1 + zeq) / (1 + zd)
    G = y * (-6 * mp.sqrt(1 + y) + (2 + 3 * y) * mp.log((mp.sqrt(1 + y) + 1) /
                                                       (mp.sqrt(1 + y) - 1)))
    r = {}
    r["bao_alpha_b"] = M(2.07) * keq * s * (1 + Rd) ** (-M(3) / 4) * G
    r["bao_beta_b"] = M(0.5) + ObO + (3 - 2 * ObO) * mp.sqrt((M(17.2) * Oh2) ** 2 + 1)
    a1 = (M(46.9) * Oh2) ** M(0.670) * (1 + (M(32.1) * Oh2) ** M(-0.532))
    a2 = (12 * Oh2) ** M(0.424) * (1 + (45 * Oh2) ** M(-0.582))
    r["bao_alpha_c"] = a1 ** (-ObO) * a2 ** (-(ObO ** 3))
    b1 = M(0.944) / (1 + (458 * Oh2) ** M(-0.708))
    b2 = (M(0.395) * Oh2) ** M(-0.0266)
    r["bao_beta_c"] = 1 / (1 + b1 * ((Oc / Om) ** b2 - 1))
    r["bao_beta_node"] = M(8.41) * Oh2 ** M(0.435)
    r["bao_s"] = s
    r["bao_hs"] = h * s
    r["bao_q_scale"] = h / (M(13.41) * keq)
    r["bao_ksilk_h"] = h / kSilk
    r["bao_ObO"] = ObO
    r["bao_OcO"] = Oc / Om
    return r


def mp_eh(e, k):                                               # cosmology.py:449-472
    k = M(k)
    G = M(e.eh_omh) * (M(e.eh_alpha) + (1 - M(e.eh_alpha)) / (1 + M(0.43) * k * M(e.eh_s)) ** 4)
    q = k * M(e.eh_theta) / G
    L0 = mp.log(2 * mp.e + M(1.8) * q)
    C0 = M(14.2) + 731 / (1 + M(62.5) * q)
    return L0 / (L0 + C0 * q * q)


def mp_eh_bao(e, k):                                           # cosmology.py:474-538
    k = M(k)
    ks, q = k * M(e.bao_hs), k * M(e.bao_q_scale)
    c386 = 386 / (1 + M(69.9) * q ** M(1.08))

    def T0t(a, b):
        L = mp.log(mp.e + M(1.8) * b * q)
        return L / (L + (M(14.2) / a + c386) * q * q)

    f = 1 / (1 + (ks / M(5.4)) ** 4)
    Tc = f * T0t(1, M(e.bao_beta_c)) + (1 - f) * T0t(M(e.bao_alpha_c), M(e.bao_beta_c))
    stilde = M(e.bao_s) / mp.cbrt(1 + (M(e.bao_beta_node) / ks) ** 3)
    Tb1 = T0t(1, 1) / (1 + (ks / M(5.2)) ** 2)
    Tb2 = (M(e.bao_alpha_b) / (1 + (M(e.bao_beta_b) / ks) ** 3)) * \
        mp.exp(-(k * M(e.bao_ksilk_h)) ** M(1.4))
    x = k * stilde
    return M(e.bao_ObO) * (mp.sin(x) / x * (Tb1 + Tb2)) + M(e.bao_OcO) * Tc


def mp_delta_k(e, k, T):                                       # cosmology.py:574-587
    return (M(e.amp) * M(e.sigma_norm) ** 2 * (M(k) / M(e.H0)) ** (3 + M(e.ns)) * T * T)


# -------------------------------------------------------------------------------------------
# constants
# -------------------------------------------------------------------------------------------
BG_FIELDS = ("H0", "ln_H0", "delta_H", "growth_norm", "growth", "E0z", "omega_m_z", "omega_l_z",
             "delta_c", "delta_v", "rho_bar", "eh_theta", "eh_s", "eh_alpha", "eh_omh", "amp")


@pytest.mark.parametrize("name", sorted(COSMOS))
def test_epoch_constants(dp, name):
    """epoch_background / bao_constants / epoch_shape_only on the device against mpmath from the
    raw inputs.  [project] 1e-14, test_hostmath.py's bound for the background scalars, the BAO
    constants included -- but for bao_alpha_b, which gets [derived] 2e-13: its G(y) = y (-6 sqrt(1 + y) + (2 + 3 y) ln(..)) cancels
    two terms of ~12.5 to ~0.15 (a factor ~83) behind a chain of ~6 pow / log / sqrt roundings of
    eps each: 83 x 6 x 2.2e-16 = 1.1e-13, twice that."""
    c = COSMOS[name]
    worst = {}
    bao_ref = mp_bao_constants(c)
    for z in REDSHIFTS:
        ref = mp_background(c, z)
        for bao in (0, 1):
            e = Ep(dp, c, z, with_bao=bao)
            assert e.with_bao == bao and e.z == z and e.sigma_norm == 1.0
            for f in BG_FIELDS:
                worst[f] = max(worst.get(f, 0.0), abs(float((M(getattr(e, f)) - ref[f]) / ref[f])))
            if bao:
                for f, r in bao_ref.items():
                    worst[f] = max(worst.get(f, 0.0), abs(float((M(getattr(e, f)) - r) / r)))
            tot = c["omega_m0"] + c["omega_l0"] + c["omega_r0"]
            assert (e.flat, e.open, e.closed) == (int(abs(tot - 1) <= 1.48e-8),
                                                  int(tot <= 1 - 1.48e-8), int(tot > 1 + 1.48e-8))
            # epoch_k_range
            assert abs(e.ln_k_min - numpy.log(0.001)) < 4e-15 and abs(e.ln_k_max - numpy.log(100.0)) < 2e-15
            assert abs(e.gtab_dx * 8192 - numpy.log(1e9)) < 1e-13 and e.gtab_inv_dx == 1.0 / e.gtab_dx
            # epoch_shape_only: the same transfer-function constants, amp = 1
            s = Ep(dp, c, z, with_bao=bao, shape_only=1)
            assert s.amp == 1.0 and s.sigma_norm == 1.0
            for f in ("H0", "ln_H0", "eh_theta", "eh_s", "eh_alpha", "eh_omh") + \
                    (tuple(bao_ref) if bao else ()):
                assert getattr(s, f) == getattr(e, f), f
    for f in sorted(worst):
        print("%-14s %.2e" % (f, worst[f]))
    assert max(worst[f] for f in BG_FIELDS) < 1e-14, worst
    assert max(worst[f] for f in bao_ref if f != "bao_alpha_b") < 1e-14, worst
    assert worst["bao_alpha_b"] < 2e-13, worst


def test_E0_de(dp):
    """E0_de and DeSpline::factor (cosmology.py:165-182 with the pressure spline) of the w0-wa
    cosmology w0 = -0.9, wa = 0.2, on a 50-knot pressure table laid out as k_de_spline leaves it:
    the knots ln a_i of cosmology.py:98-102, P_i = 3 int_0^z_i (1 + w) / (1 + z) dz in closed form,
    the not-a-knot spline built on the device (returned).  The reference is mpmath on the returned
    coefficients and the double a = 1 / (1 + z): an error in the spline build is test_gpu_devmath's
    to find, an error in the interval search, the polynomial, log, exp or the sum is this test's.
    [project] 1e-14 for E0_de (background scalars).  [derived] factor = exp(S(ln a)): ln a is
    rounded by eps |ln a|, which moves S by |S'| eps |ln a| with |S'| = 3 |1 + w| <= 0.9 here; the
    Horner form rounds S by eps |S| (each piece has terms of one sign); exp and log add eps each
    and d = ln a - x_i another: (0.9 |ln a| + |S| + 3) eps relative, asserted at twice that."""
    c = COSMOS["golden"]
    e = Ep(dp, c, 0.5)
    n = 50
    a = 10.0 ** numpy.linspace(numpy.log10(1.48e-8), 0.0, n)
    ln_a, zk = numpy.log(a), 1.0 / a - 1.0
    P = 3.0 * ((1.0 + DE_W0 + DE_WA) * numpy.log1p(zk) - DE_WA * zk / (1.0 + zk))
    z = numpy.array([0.0, 0.01, 0.1, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0, 10.0, 100.0, 1e4])
    pp, out = numpy.empty(4 * (n - 1)), numpy.empty(2 * z.size)
    call(dp, "dp_e0_de", e.p, ptr(ln_a), ptr(P), n, ptr(z), z.size, ptr(pp), ptr(out))
    E0, fac = out.reshape(2, -1)
    assert numpy.array_equal(pp[0::4], P[:-1])                # each piece starts at its knot value
    worst_E, worst_f, worst_true = 0.0, 0.0, 0.0
    for j, zz in enumerate(z):
        aa = 1.0 / (1.0 + zz)                                  # the double E0_de forms
        xv = mp.log(M(aa))
        i = max([k for k in range(n - 1) if M(ln_a[k]) <= xv] or [0])
        d = xv - M(ln_a[i])
        S = M(pp[4 * i]) + d * (M(pp[4 * i + 1]) + d * (M(pp[4 * i + 2]) + d * M(pp[4 * i + 3])))
        f_ref = mp.exp(S)
        E_ref = M(c["omega_l0"]) * f_ref + M(c["omega_m0"]) / M(aa) ** 3 + M(c["omega_r0"]) / M(aa) ** 4
        bound = 2 * (0.9 * abs(float(xv)) + abs(float(S)) + 3) * EPS
        worst_f = max(worst_f, abs(float((M(fac[j]) - f_ref) / f_ref)) / bound)
        worst_E = max(worst_E, abs(float((M(E0[j]) - E_ref) / E_ref)))
        P_true = 3 * ((1 + M(DE_W0) + M(DE_WA)) * mp.log(1 + M(zz)) - M(DE_WA) * M(zz) / (1 + M(zz)))
        worst_true = max(worst_true, abs(float(f_ref / mp.exp(P_true) - 1)))
    print("E0_de %.2e relative; factor %.3f of the derived bound; the spline against the closed "
          "form %.1e (not asserted: the table's resolution)" % (worst_E, worst_f, worst_true))
    assert worst_E < 1e-14 and worst_f <= 1.0
    # it is the dark-energy E0: not E0_of of the same densities
    assert abs(E0[4] / float(mp_E0(c["omega_m0"], c["omega_l0"], c["omega_r0"], 1.0)) - 1) > 1e-3


def test_scalars_halo_tinker_mandelbaum_constants(dp):
    """E0_of, growth_approx, scale_of_mass (the device cbrt), halo_constants with delta_v_in = -1
    and explicit, tinker_bias_constants at four delta_v, mandelbaum_constants.  [project] 1e-14
    (background scalars)."""
    worst = {}

    def rec(key, got, ref):
        worst[key] = max(worst.get(key, 0.0), abs(float((M(got) - ref) / ref)))

    z = numpy.array([0.0, 0.1, 0.5, 1.5, 3.0, 7.0, 1100.0])
    mass = numpy.logspace(5, 17, z.size)
    for name, c in COSMOS.items():
        for dv_in in (-1.0, 200.0):
            e = Ep(dp, c, 0.5, halo=dict(c0=9.0, beta=-0.13, delta_v=dv_in), m_star=1.7e12)
            out = numpy.empty(3 * z.size)
            call(dp, "dp_scalars", e.p, ptr(z), ptr(mass), z.size, ptr(out))
            E0, gr, sc = out.reshape(3, -1)
            for i in range(z.size):
                rec("E0_of", E0[i], mp_E0(c["omega_m0"], c["omega_l0"], c["omega_r0"], z[i]))
                rec("growth_approx", gr[i],
                    mp_growth_approx(c["omega_m0"], c["omega_l0"], 1 / (1 + M(z[i]))))
                rec("scale_of_mass", sc[i],                    # cosmology.py:671
                    mp.cbrt(3 * M(mass[i]) / (4 * mp.pi * M(e.rho_bar))))
            # halo.py:71-83, 873-902
            assert e.prof_delta_v == (e.delta_v if dv_in == -1.0 else dv_in)
            assert e.beta == -0.13
            rec("c0", e.c0, M(9.0) / (1 + M(0.5)))
            rec("ln_rv_const", e.ln_rv_const,
                mp.log(3 / (4 * mp.pi * M(e.prof_delta_v) * M(e.rho_bar))))
            rec("ln_c_const", e.ln_c_const, mp.log(M(e.c0)) - M(e.beta) * mp.log(M(1.7e12)))
    for dv in DELTA_VS:                                        # mass_function.py:521-528
        e = Ep(dp, COSMOS["default"], 0.0, mf=TINKER, delta_v=dv)
        y = mp.log10(M(dv))
        ex = mp.exp(-(4 / y) ** 4)
        rec("tb_A", e.tb_A, 1 + M(0.24) * y * ex)
        rec("tb_a", e.tb_a, M(0.44) * y - M(0.88))
        rec("tb_C", e.tb_C, M(0.019) + M(0.107) * y + M(0.19) * ex)
        rec("tb_dca", e.tb_dca, M(e.delta_c) ** M(e.tb_a))
        rec("ln_t_beta", e.ln_t_beta, mp.log(M(e.t_beta)))
    for lm0 in (11.8, 12.63):                                  # hod.py:248-259
        e = Ep(dp, COSMOS["default"], 0.0, hod=dict(model=1, log_M_0=lm0, w=0.2))
        rec("log_M_min", e.hod_log_M_min, mp.log10(3) + M(lm0))
        rec("M_min", e.hod_M_min, 10 ** M(e.hod_log_M_min))
        rec("hod_M0", e.hod_M0, 10 ** M(lm0))
    for f in sorted(worst):
        print("%-14s %.2e" % (f, worst[f]))
    assert max(worst.values()) < 1e-14, worst


# -------------------------------------------------------------------------------------------
# transfer functions and power
# -------------------------------------------------------------------------------------------
def _k_grid(e):
    """k = 1e-6 .. 1e5 h/Mpc log-spaced, and the ends of epoch_k_range with their neighbours."""
    ends = []
    for v in (e.k_min, e.k_max, e.k_min / 100.0, e.k_max * 100.0):
        ends += [v, numpy.nextafter(v, 0.0), numpy.nextafter(v, INF)]
    return numpy.concatenate([numpy.logspace(-6, 5, 67), ends])


_T_CACHE = {}


def _transfer_ref(e, name, bao, k):
    """T(k) does not depend on z: one mpmath evaluation per (cosmology, transfer function)."""
    key = (name, bao)
    if key not in _T_CACHE:
        _T_CACHE[key] = ([mp_eh(e, v) for v in k], [mp_eh_bao(e, v) for v in k] if bao else None)
    return _T_CACHE[key]


@pytest.mark.parametrize("bao", [0, 1])
@pytest.mark.parametrize("name", sorted(COSMOS))
def test_transfer_and_power(dp, name, bao):
    """[project] 2e-13 linear power, 5e-13 BAO transfer, 1e-12 BAO power; eh_transfer [derived]
    1e-13: half the bound of the power it is squared in."""
    c = COSMOS[name]
    worst = {}
    for z in REDSHIFTS:
        e = Ep(dp, c, z, with_bao=bao, sigma_norm=0.93)
        k = _k_grid(e)
        nf = dp.dp_power_fields()
        out = numpy.empty(nf * k.size)
        call(dp, "dp_power", e.p, ptr(k), k.size, ptr(out))
        (eh, ehb, tf, tt, lp, lpt, dk, dkt, ps, pst, lk, flk) = out.reshape(nf, -1)
        T_eh, T_bao = _transfer_ref(e, name, bao, k)
        T = T_bao if bao else T_eh
        ref_dk = [mp_delta_k(e, kv, t) for kv, t in zip(k, T)]
        ref_lp = [2 * mp.pi ** 2 * d / M(kv) ** 3 for kv, d in zip(k, ref_dk)]
        for key, got, ref in (("eh_transfer", eh, T_eh), ("transfer_function", tf, T),
                              ("transfer_t", tt, T), ("linear_power", lp, ref_lp),
                              ("linear_power_t", lpt, ref_lp), ("delta_k_ln", dk, ref_dk),
                              ("delta_k_ln_t", dkt, ref_dk), ("power_shape", ps, ref_lp),
                              ("power_shape_t", pst, ref_lp)) + \
                ((("eh_bao_transfer", ehb, T_bao),) if bao else ()):
            worst[key] = max(worst.get(key, 0.0), _rel(got, _fl(ref)))
        assert numpy.array_equal(tf, tt) and numpy.array_equal(lp, lpt)
        assert numpy.array_equal(dk, dkt) and numpy.array_equal(ps, pst)
    for f in sorted(worst):
        print("%-18s %.2e" % (f, worst[f]))
    assert worst["eh_transfer"] < 1e-13
    bound_T, bound_P = (5e-13, 1e-12) if bao else (1e-13, 2e-13)
    for f in ("transfer_function", "transfer_t") + (("eh_bao_transfer",) if bao else ()):
        assert worst[f] < bound_T, (f, worst[f])
    for f in ("linear_power", "linear_power_t", "delta_k_ln", "delta_k_ln_t", "power_shape",
              "power_shape_t"):
        assert worst[f] < bound_P, (f, worst[f])


@pytest.mark.parametrize("bao", [0, 1])
def test_sigma_integrands(dp, bao):
    """SigmaIntegrandT and HalofitSigmaIntegrand at R in {0.05, 8, 120} over sigma_limits'
    range.  [project] test_hostmath.py's bound: 1e-9 of the integrand's maximum."""
    worst = 0.0
    for name in ("default", "alt"):
        e = Ep(dp, COSMOS[name], 0.5, with_bao=bao, sigma_norm=0.9)
        for R in (0.05, 8.0, 120.0):
            lim = numpy.empty(2)
            dummy = numpy.zeros(1)
            call(dp, "dp_sigma", e.p, R, ptr(dummy), 0, ptr(lim), ptr(dummy))
            # cosmology.py:611-632
            lo, hi = e.k_min, e.k_max
            need_lo, need_hi = 1.0 / R / 10.0, 1.0 / R * 14.0662
            if need_lo <= lo:
                lo = need_lo if need_lo > e.k_min / 100.0 else e.k_min / 100.0
            if need_hi >= hi:
                hi = need_hi if need_hi < e.k_max * 100.0 else e.k_max * 100.0
            assert abs(lim[0] - numpy.log(lo)) < 4e-15 and abs(lim[1] - numpy.log(hi)) < 4e-15
            lnk = numpy.linspace(lim[0], lim[1], 61)
            out = numpy.empty(2 * lnk.size)
            call(dp, "dp_sigma", e.p, R, ptr(lnk), lnk.size, ptr(lim), ptr(out))
            got_s, got_h = out.reshape(2, -1)
            ref_s, ref_h = [], []
            for x in lnk:
                k = mp.exp(M(x))
                T = mp_eh_bao(e, float(k)) if bao else mp_eh(e, float(k))
                d = M(e.amp) * M(e.sigma_norm) ** 2 * (k / M(e.H0)) ** (3 + M(e.ns)) * T * T
                kR = k * M(R)
                W = 3 * (mp.sin(kR) - kR * mp.cos(kR)) / kR ** 3       # cosmology.py:644-660
                ref_s.append(d * W * W)
                ref_h.append(d * mp.exp(-k * k * M(R) ** 2))            # halo.py:1321-1323
            ref_s, ref_h = _fl(ref_s), _fl(ref_h)
            worst = max(worst, numpy.max(numpy.abs(got_s - ref_s)) / ref_s.max(),
                        numpy.max(numpy.abs(got_h - ref_h)) / ref_h.max())
    print("sigma integrands: %.2e of the maximum" % worst)
    assert worst < 1e-9


# -------------------------------------------------------------------------------------------
# mass function
# -------------------------------------------------------------------------------------------
def mp_f_nu(e, nu):
    nu = M(nu)
    if e.mf_kind == 0:                                         # mass_function.py:243-255
        n_ = nu * M(e.st_a)
        return M(e.f_norm) * (1 + n_ ** (-M(e.stq))) * mp.sqrt(n_) * mp.exp(-n_ / 2) / nu
    sq = mp.sqrt(nu)                                           # :494-509
    return (M(e.t_alpha) * (1 + (M(e.t_beta) * sq) ** (-2 * M(e.t_phi))) * nu ** M(e.t_eta) *
            mp.exp(-M(e.t_gamma) * nu / 2) / sq)


def mp_bias_addends(e, nu):
    """b(nu) / bias_norm as its addends (mass_function.py:290-302, 511-530)."""
    nu = M(nu)
    if e.mf_kind == 0:
        n_ = nu * M(e.st_a)
        return [mp.mpf(1), (n_ - 1) / M(e.delta_c),
                2 * M(e.stq) / (M(e.delta_c) * (1 + n_ ** M(e.stq)))]
    sq = mp.sqrt(nu)
    sa = sq ** M(e.tb_a)
    return [mp.mpf(1), -M(e.tb_A) * sa / (sa + M(e.tb_dca)), M(0.183) * sq ** M(1.5),
            M(e.tb_C) * sq ** M(2.4)]


def _mf_epochs(L):
    yield "sheth-tormen", Ep(L, COSMOS["default"], 0.5, mf=ST)
    for dv in DELTA_VS:
        yield "tinker %g" % dv, Ep(L, COSMOS["default"], 0.5, mf=TINKER, delta_v=dv)


def test_mass_function(dp):
    """f_nu, bias_nu and mf_node on nu = 1e-3 .. 1e2.
    [project] 1e-13 for f and b (relative; b as 1e-13 of the sum of its addends' magnitudes:
    Sheth-Tormen's b crosses zero inside the range where bias_norm (nu' - 1) / delta_c cancels 1).
    [derived] mf_node against f_nu nu and bias_nu: ln_nu is a double, one ulp of it (<= |ln nu|
    eps / 2 ... eps |ln nu|) moves nu^p by |p ln nu| eps; the largest |p| is 1.2 (Tinker bias),
    eta + 1/2 and q for f; and exp(-nu' / 2) is shared.  First order: (sum over the powers taken
    of |p| |ln nu| + |arg| / 2 + 4) eps, with arg the argument of the exponential that carries
    exp(-nu' / 2) (its rounding to a double moves the result by |arg| eps / 2) and the 4 for the
    roundings of the ~4 exps and products; asserted at twice that."""
    nu = numpy.logspace(-3, 2, 301)
    ln_nu = numpy.log(nu)                      # the double the product would hold: x, nu = exp(x)
    nu = numpy.exp(ln_nu)
    nf_ = dp.dp_mf_fields()
    report = []
    for label, e in _mf_epochs(dp):
        out = numpy.empty(nf_ * nu.size)
        call(dp, "dp_mf", e.p, ptr(nu), ptr(ln_nu), nu.size, ptr(out))
        f, b, nf, nb, nf2 = out.reshape(nf_, -1)
        ref_f = _fl([mp_f_nu(e, v) for v in nu])
        add = [mp_bias_addends(e, v) for v in nu]
        ref_b = _fl([M(e.bias_norm) * sum(a) for a in add])
        mag_b = _fl([M(e.bias_norm) * sum(abs(x) for x in a) for a in add])
        err_f = _rel(f, ref_f)
        err_b = float(numpy.max(numpy.abs(b - ref_b) / mag_b))
        assert numpy.array_equal(nf, nf2)                   # (want_bias changes nothing of nu f)
        L = numpy.abs(ln_nu)
        if e.mf_kind == 0:
            arg = numpy.abs(0.5 * (ln_nu + e.ln_st_a) - 0.5 * nu * e.st_a)
            bound_f = (e.stq + 0.5) * (L + abs(e.ln_st_a)) + 0.5 * arg + 4
            bound_b = e.stq * (L + abs(e.ln_st_a)) + 4
        else:
            arg = numpy.abs((e.t_eta + 0.5) * ln_nu - 0.5 * e.t_gamma * nu)
            bound_f = (2 * abs(e.t_phi) * (0.5 * L + abs(e.ln_t_beta)) + abs(e.t_eta + 0.5) * L
                       + 0.5 * arg + 4)
            bound_b = (0.5 * abs(e.tb_a) + 0.75 + 1.2) * L + 4
        r_f = numpy.abs(nf - f * nu) / numpy.abs(f * nu) / EPS / bound_f
        r_fm = numpy.abs(nf - ref_f * nu) / numpy.abs(ref_f * nu) / EPS / bound_f
        r_b = numpy.abs(nb - b) / mag_b / EPS / bound_b
        r_bm = numpy.abs(nb - ref_b) / mag_b / EPS / bound_b
        report.append((label, err_f, err_b, r_f.max(), r_fm.max(), r_b.max(), r_bm.max(),
                       float(numpy.max(numpy.abs(nf - ref_f * nu) / numpy.abs(ref_f * nu))),
                       float(numpy.max(numpy.abs(nb - ref_b) / mag_b))))
    for row in report:
        print("%-14s f %.2e  b %.2e | mf_node / first-order bound: f vs f_nu %.2f, vs mpmath %.2f;"
              " b vs bias_nu %.2f, vs mpmath %.2f | mf_node relative: f %.2e b %.2e" % row)
    for row in report:
        assert row[1] < 1e-13 and row[2] < 1e-13, row
        assert max(row[3:7]) <= 2.0, row


# -------------------------------------------------------------------------------------------
# HOD
# -------------------------------------------------------------------------------------------
H_MASS, H_LOG10, H_ROUTE, H_NC, H_NS, H_N1, H_N2, H_NODE1, H_NODE2, H_STATE = range(10)
H_MC, H_MS, H_Z1, H_Z2, H_ZN1, H_ZN2 = range(10, 16)


def _hod_run(L, e, ln_mass):
    n = L.dp_hod_fields()
    out = numpy.empty(n * ln_mass.size)
    call(L, "dp_hod", e.p, ptr(ln_mass), ln_mass.size, ptr(out))
    return out.reshape(n, -1)


def _ln_masses(thresholds_log10):
    """ln M for M = 1e9 .. 1e16, and around every threshold (given as log10 M) the masses whose
    log10 is the threshold and its +-1, 2, 4, 8, 16 ulp neighbours (ulps of the threshold),
    formed as halo_node_fields holds them: the double ln M, M = exp(ln M) on the device.  Also
    the ln M nearest each threshold whose node route fl(ln M log10 e) IS the threshold double (one
    exists: an ulp of ln M is less than an ulp of log10 M after the multiplication), where a
    strict comparison and a non-strict one part."""
    lnm = [numpy.linspace(numpy.log(1e9), numpy.log(1e16), 141)]
    for t in thresholds_log10:
        u = float(_ulp(t))
        steps = [0] + [s * k for k in (1, 2, 4, 8, 16) for s in (-1, 1)]
        lnm.append(_fl([(M(t) + k * M(u)) * mp.log(10) for k in steps]))
        x = float(M(t) * mp.log(10))
        near = [x]
        for _ in range(4):
            near = [numpy.nextafter(near[0], -INF)] + near + [numpy.nextafter(near[-1], INF)]
        hit = [v for v in near if v * LOG10E == t]
        assert hit, t
        lnm.append(_fl([min(hit, key=lambda v: abs(v - x))]))
    return numpy.sort(numpy.concatenate(lnm))


def _zheng_cases():
    for sigma in (0.15, 0.01, 0.0, -1.0):
        for alpha in (1.0, 0.9, 1.3):
            for lm0 in (12.14, 11.62, 12.7):       # M0 at, below and above M_min
                if sigma == 0.15 and (alpha, lm0) not in ((1.0, 12.14), (0.9, 11.62)):
                    continue
                yield dict(ZHENG, sigma=sigma, alpha=alpha, log_M_0=lm0)


def test_device_log10_and_threshold_band(dp):
    """The device's log10 and the node route ln M log10 e on the HOD test masses, in ulps against
    mpmath: the band B = 1 + the measured maximum must be <= 3 for both."""
    e = Ep(dp, COSMOS["default"], 0.5)
    lnm = _ln_masses([12.14, 11.62, 12.7, 11.8, 12.63, float(numpy.log10(3.0) + 11.8)])
    r = _hod_run(dp, e, lnm)
    exact = [mp.log10(M(v)) for v in r[H_MASS]]
    u = _ulp(_fl(exact))
    err_lib = numpy.max(numpy.abs(_fl([(M(a) - x) for a, x in zip(r[H_LOG10], exact)])) / u)
    err_route = numpy.max(numpy.abs(_fl([(M(a) - x) for a, x in zip(r[H_ROUTE], exact)])) / u)
    print("log10(M) on %d masses: device library %.3f ulp, ln M log10 e %.3f ulp"
          % (lnm.size, err_lib, err_route))
    assert 1 + err_lib <= 3 and 1 + err_route <= 3


def _band_check(label, mass_exact_log10, thr, B, decision, exact_side, neighbours_ulps=None):
    """decision: 0 / 1 per mass (sorted by mass).  Outside the band of B ulps of the threshold it
    must be the exact one; at least four masses on each side outside it; monotone."""
    u = float(_ulp(thr))
    d = _fl([(x - M(thr)) / M(u) for x in mass_exact_log10])
    outside = numpy.abs(d) > B
    below, above = outside & (d < 0), outside & (d > 0)
    assert below.sum() >= 4 and above.sum() >= 4, label
    near = numpy.abs(d) < 20
    assert (near & below).sum() >= 3 and (near & above).sum() >= 3, (label, d[near])
    assert numpy.array_equal(decision[outside], exact_side[outside]), \
        (label, d[outside][decision[outside] != exact_side[outside]])
    assert numpy.all(numpy.diff(decision) >= 0), label
    return int((~outside).sum())


@pytest.mark.parametrize("hod", list(_zheng_cases()),
                         ids=lambda h: "s%g_a%g_m%g" % (h["sigma"], h["alpha"], h["log_M_0"]))
def test_zheng(dp, hod):
    """zheng_* / hod_* / zheng_node / hod_node against hod.py:189-230 in mpmath on the exact
    log10 M.
    [derived] N_c: the erf argument moves by (error of log10 M) / sigma; with B - 1 <= 2 ulp of
    |lm| eps that is 2 |lm| eps / sigma, times erf' <= 2 / sqrt(pi), times 1/2: |dN_c| <=
    2 |lm| eps / (sigma sqrt(pi)), plus 2 eps for erf's own rounding and the sum -- asserted at
    twice the two.  [project] 1e-12 relative for the rest of each moment (test_hostmath.py), on
    top of dN_c carried through N_s = N_c r^alpha, first = N_c + N_s, second = (2 + N_s) N_s.
    Step models (sigma <= 0): N_c is a decision, exact outside the band (see _band_check)."""
    e = Ep(dp, COSMOS["default"], 0.5, hod=hod)
    thr = e.hod_log_M_min
    lnm = _ln_masses([thr, float(numpy.log10(e.hod_M0))])
    r = _hod_run(dp, e, lnm)
    mass = r[H_MASS]
    assert numpy.all(numpy.diff(mass) >= 0)
    exact = [mp.log10(M(v)) for v in mass]
    u = _ulp(_fl(exact))
    B_lib = 1 + numpy.max(numpy.abs(_fl([M(a) - x for a, x in zip(r[H_LOG10], exact)])) / u)
    B_route = 1 + numpy.max(numpy.abs(_fl([M(a) - x for a, x in zip(r[H_ROUTE], exact)])) / u)
    assert B_lib <= 3 and B_route <= 3, (B_lib, B_route)
    step = hod["sigma"] <= 0.0
    # the references
    if step:
        nc = [mp.mpf(1) if x > M(thr) else mp.mpf(0) for x in exact]
        tol_nc = numpy.zeros(mass.size)
    else:
        nc = [(1 + mp.erf((x - M(thr)) / M(e.hod_sigma))) / 2 for x in exact]
        tol_nc = 2 * (2 * numpy.abs(_fl(exact)) * EPS / (e.hod_sigma * numpy.sqrt(numpy.pi))
                      + 2 * EPS)
    ra = [((M(v) - M(e.hod_M0)) / M(e.hod_M1p)) ** M(e.hod_alpha) if v > e.hod_M0 else mp.mpf(0)
          for v in mass]
    ns = [a * b for a, b in zip(nc, ra)]
    nc_f, ns_f, ra_f = _fl(nc), _fl(ns), _fl(ra)
    tol_ns = ra_f * tol_nc + 1e-12 * ns_f
    n1_f, n2_f = _fl([a + b for a, b in zip(nc, ns)]), _fl([(2 + b) * b for b in ns])
    tol_1 = tol_nc + tol_ns + 1e-12 * n1_f
    tol_2 = (2 + 2 * ns_f) * tol_ns + 1e-12 * n2_f
    if step:
        # the decisions: evaluator on the library's log10, node on ln M log10 e
        side = (_fl(exact) > thr).astype(float)
        for label, dec, B in (("zheng_central", r[H_MC], B_lib), ("hod_central", r[H_NC], B_lib),
                              ("zheng_node", (r[H_ZN1] != 0.0).astype(float), B_route),
                              ("hod_node", (r[H_NODE1] != 0.0).astype(float), B_route),
                              ("state bit 2", (r[H_STATE].astype(int) >> 2 & 1).astype(float),
                               B_route)):
            assert set(numpy.unique(dec)) <= {0.0, 1.0}, label
            inside = _band_check(label, exact, thr, B, dec, side)
            print("%-14s band %.2f ulp: %d masses inside" % (label, B, inside))
        # the +-4 .. 16 ulp neighbours are outside the band, so only +-1, 2 (and 0) can be inside
        d = numpy.abs(_fl([(x - M(thr)) / M(float(_ulp(thr))) for x in exact]))
        assert numpy.sum(d <= max(B_lib, B_route)) <= 5 + 5     # (two thresholds may coincide)
        # bit 2 <=> N_c = 1, at every mass
        assert numpy.array_equal(r[H_STATE].astype(int) >> 2 & 1, (r[H_NODE1] != 0.0).astype(int))
        # compare values only where the decision is certain
        keep = d > max(B_lib, B_route)
    else:
        assert numpy.all(r[H_STATE].astype(int) & 4 == 0)
        keep = numpy.ones(mass.size, dtype=bool)
    # bit 1 <=> the satellite term is on (mass - M0 > 0), exact
    assert numpy.array_equal(r[H_STATE].astype(int) >> 1 & 1, (mass > e.hod_M0).astype(int))
    assert numpy.array_equal(r[H_NS] > 0, (mass > e.hod_M0) & (r[H_NC] > 0))
    worst = {}
    for label, got, ref, tol in (("central", r[H_NC], nc_f, tol_nc), ("satellite", r[H_NS], ns_f, tol_ns),
                                 ("first", r[H_N1], n1_f, tol_1), ("second", r[H_N2], n2_f, tol_2),
                                 ("node first", r[H_NODE1], n1_f, tol_1),
                                 ("node second", r[H_NODE2], n2_f, tol_2)):
        err = numpy.abs(got - ref)[keep]
        t = tol[keep]
        ratio = numpy.max(numpy.where(t > 0, err / numpy.where(t > 0, t, 1.0),
                                      numpy.where(err > 0, INF, 0.0)))
        worst[label] = ratio
    print("zheng %s: error / bound %s" % (hod, {k: "%.3f" % v for k, v in worst.items()}))
    # the dispatching and the direct forms are the same code
    for a, b in ((H_MC, H_NC), (H_MS, H_NS), (H_Z1, H_N1), (H_Z2, H_N2), (H_ZN1, H_NODE1),
                 (H_ZN2, H_NODE2)):
        assert numpy.array_equal(r[a], r[b])
    assert max(worst.values()) <= 1.0, worst
    # node against evaluator, directly.  [derived] The two differ in the route to log10 M only
    # (the library's against ln M log10 e), each within B - 1 <= 2 ulp of the exact one; tol_nc
    # and what it is carried into are twice the first-order effect of ONE such error, which is
    # the first-order effect of the two together: the distance between the two forms is held to
    # the bound each has against mpmath, not to twice it.
    direct = {}
    for label, node, ev, tol in (("first", r[H_NODE1], r[H_N1], tol_1),
                                 ("second", r[H_NODE2], r[H_N2], tol_2)):
        err = numpy.abs(node - ev)[keep]
        t = tol[keep]
        direct[label] = float(numpy.max(numpy.where(t > 0, err / numpy.where(t > 0, t, 1.0),
                                                    numpy.where(err > 0, INF, 0.0))))
    print("zheng_node against zheng_first / _second: %s of the bound"
          % {k: "%.3f" % v for k, v in direct.items()})
    assert max(direct.values()) <= 1.0, direct


@pytest.mark.parametrize("lm0,w", [(11.8, 0.2), (12.63, 1.7)])
def test_mandelbaum(dp, lm0, w):
    """mandelbaum_* / hod_* / hod_node against hod.py:232-299 in mpmath: N_c = [log10 M >= log_M_0],
    N_s = w (M / M_min)^2 below log_M_min, w M / M_min from there.  [project] 1e-12 relative on
    the moments where the decisions are certain; the decisions by _band_check."""
    e = Ep(dp, COSMOS["default"], 0.5, hod=dict(model=1, log_M_0=lm0, w=w))
    t0, t1 = e.hod_log_M_0, e.hod_log_M_min
    lnm = _ln_masses([t0, t1])
    r = _hod_run(dp, e, lnm)
    mass = r[H_MASS]
    exact = [mp.log10(M(v)) for v in mass]
    ex_f = _fl(exact)
    u = _ulp(ex_f)
    B = 1 + numpy.max(numpy.abs(_fl([M(a) - x for a, x in zip(r[H_LOG10], exact)])) / u)
    print("mandelbaum log_M_0 = %g: band %.2f ulp" % (lm0, B))
    assert B <= 3
    st = r[H_STATE].astype(int)
    nc_node = numpy.rint(r[H_NODE1] - r[H_NS])
    for label, dec in (("mandelbaum_central", r[H_MC]), ("hod_central", r[H_NC]),
                       ("hod_node N_c", nc_node), ("state bit 2", (st >> 2 & 1).astype(float))):
        _band_check(label, exact, t0, B, dec, (ex_f >= t0).astype(float))
    # the satellite branch: 1 where the upper one (w r) was taken
    rr = mass / e.hod_M_min
    upper_eval = numpy.where(numpy.abs(r[H_NS] - w * rr) <= numpy.abs(r[H_NS] - w * rr * rr), 1.0, 0.0)
    clear = numpy.abs(rr - 1) > 1e-9            # (the two branches differ by the factor r)
    _band_check("state bit 1", exact, t1, B, (st >> 1 & 1).astype(float), (ex_f >= t1).astype(float))
    assert numpy.array_equal(upper_eval[clear], (ex_f >= t1).astype(float)[clear])
    # the bits are the decisions hod_node took on the device's own log10
    assert numpy.array_equal(st >> 1 & 1, (r[H_LOG10] >= t1).astype(int))
    assert numpy.array_equal(st >> 2 & 1, (r[H_LOG10] >= t0).astype(int))
    assert numpy.array_equal(st >> 2 & 1, nc_node.astype(int))
    ud = float(_ulp(t0))
    d0 = numpy.abs(_fl([(x - M(t0)) / M(ud) for x in exact]))
    d1 = numpy.abs(_fl([(x - M(t1)) / M(float(_ulp(t1))) for x in exact]))
    assert numpy.sum(d0 <= B) <= 5 and numpy.sum(d1 <= B) <= 5
    keep = (d0 > B) & (d1 > B)
    nc = (ex_f >= t0).astype(float)
    ns = _fl([M(w) * (M(v) / M(e.hod_M_min)) ** (2 if x < M(t1) else 1) for v, x in zip(mass, exact)])
    for label, got, ref in (("central", r[H_NC], nc), ("satellite", r[H_NS], ns),
                            ("first", r[H_N1], nc + ns), ("second", r[H_N2], (2 + ns) * ns),
                            ("node first", r[H_NODE1], nc + ns), ("node second", r[H_NODE2], (2 + ns) * ns)):
        err = _rel(got[keep], ref[keep])
        print("mandelbaum %-12s %.2e" % (label, err))
        assert err < 1e-12, label
    assert numpy.array_equal(r[H_MC], r[H_NC]) and numpy.array_equal(r[H_MS], r[H_NS])
    # node against evaluator.  They share the log10, so N_c and the satellite branch are the same
    # decisions and N_s = w r^p (products only) the same double.  What may differ is contraction:
    # N_c + N_s and 2 + N_s each end a product in a sum, and the device compiler may fuse that
    # (x + t w as one fma) in one inlined copy and not in the other.  [derived] The sum is then
    # rounded once from the exact product and once from the rounded one; these differ by at most
    # half an ulp of N_s, which is at most half an ulp of the sum, and rounding is monotone, so the
    # two sums are the same double or neighbours: 1 ulp for N_c + N_s.  In (2 + N_s) N_s the factor
    # 2 + N_s moves by that 1 ulp, at most eps relative, which is at most 2 ulp of the product, and
    # the rounding of the product keeps the order: 2 ulp.  Asserted at twice each.
    # Measured on the MI355X: 1 ulp and 2 ulp, at 7 to 13 of the 165 masses.
    def ulps(a, b):
        return float(numpy.max(numpy.abs(a - b) / _ulp(numpy.maximum(numpy.abs(a), numpy.abs(b)))))
    d1, d2 = ulps(r[H_NODE1], r[H_N1]), ulps(r[H_NODE2], r[H_N2])
    print("mandelbaum hod_node against hod_first %.1f ulp (%d masses differ), against hod_second "
          "%.1f ulp (%d)" % (d1, numpy.sum(r[H_NODE1] != r[H_N1]), d2,
                             numpy.sum(r[H_NODE2] != r[H_N2])))
    assert d1 <= 2.0 and d2 <= 4.0


# -------------------------------------------------------------------------------------------
# NFW transform and exclusion window
# -------------------------------------------------------------------------------------------
# [measured] K of |device - mpmath| <= K eps sum|addends|: twice the measured maximum (DESIGN.md
# section 3), rounded up to a power of two.  Measured on the MI355X: 17.44 (y_nfw_core_tab at
# k r_s = 3.16, c = 79.6; y_nfw and y_nfw_core 7.61; the host build 16.31, 9.10, 7.25) and 7.92
# (exclusion_window at kR = 3.98; the host build 7.91)
K_NFW = 64.0            # 2 x 17.44 = 34.9
K_EXCLUSION = 16.0      # 2 x 7.92 = 15.8


def mp_y_addends(z, con, mass_k_inv):
    """halo.py:561-585 as its five addends (the products of cos z, sin z with each Ci, Si, and the
    sine term), times 1 / (ln(1 + c) - c / (1 + c))."""
    z, con = M(z), M(con)
    cp = 1 + con
    t = [mp.cos(z) * mp.ci(cp * z), -mp.cos(z) * mp.ci(z), mp.sin(z) * mp.si(cp * z),
         -mp.sin(z) * mp.si(z), -mp.sin(con * z) / (cp * z)]
    return [v * mass_k_inv for v in t]


def _hostcheck():
    return hostcheck_build.load()


def test_y_nfw(dp):
    """y_nfw, y_nfw_core and y_nfw_core_tab on k r_s = 1e-8 .. 1e4, c = 0.5 .. 200, against
    mpmath (Si, Ci at 50 digits) on the node fields the device formed, and against each other.
    [project] 5e-13 absolute (test_hostmath.py) at every point; [measured] K_NFW eps sum|addends|,
    which is the tighter one where y is O(1 / z^2) of its addends -- also asserted of the host
    build (tests/hostcheck), so that a device-only excess is a finding;
    [derived] the core forms against y_nfw: they differ in how z = k r_s is formed (one exp of a
    sum against a product of two exps: |ln z| eps + 2 eps relative in z), and y moves by at most
    sum|addends| (1 + c) z ... per unit relative change of z at large z (the phases), so the
    three agree to 2 (|ln z| + 4) (1 + (1 + c) z) eps sum|addends|."""
    e = Ep(dp, COSMOS["default"], 0.5, m_star=2.1e12)
    # c = exp(ln_c_const + beta ln M): ln M for c = 0.5 .. 200
    cons = numpy.geomspace(0.5, 200.0, 14)
    lnm1 = (numpy.log(cons) - e.ln_c_const) / e.beta
    zs = numpy.geomspace(1e-8, 1e4, 49)
    lnm = numpy.repeat(lnm1, zs.size)
    ln_rs = (e.ln_rv_const + lnm) / 3.0 - (e.ln_c_const + e.beta * lnm)
    lnk = numpy.log(numpy.tile(zs, cons.size)) - ln_rs
    nf = dp.dp_nfw_fields()
    out = numpy.empty(nf * lnm.size)
    call(dp, "dp_nfw", e.p, ptr(lnk), ptr(lnm), lnm.size, ptr(out))
    (y, yc, yt, z1, z2, d_lnrs, con, ln_cp, imk, rs, icprs, kk, ik) = out.reshape(nf, -1)
    assert con.min() < 0.51 and con.max() > 199 and z1.min() < 1.1e-8 and z1.max() > 0.9e4
    # the node fields themselves ([project] 1e-14, the background scalars' bound)
    assert _rel(con, _fl([mp.exp(M(e.ln_c_const) + M(e.beta) * M(v)) for v in lnm])) < 1e-13
    assert _rel(ln_cp, _fl([mp.log(1 + M(v)) for v in con])) < 1e-14
    assert _rel(imk, _fl([1 / (M(a) - M(b) / (1 + M(b))) for a, b in zip(ln_cp, con)])) < 1e-14
    assert _rel(rs, _fl([mp.exp(M(v)) for v in d_lnrs])) < 1e-14
    assert _rel(icprs, _fl([1 / ((1 + M(a)) * M(b)) for a, b in zip(con, rs)])) < 1e-14
    # z_out: k r_s by one exp, and by the product
    zref = _fl([mp.exp(M(a) + M(b)) for a, b in zip(lnk, d_lnrs)])
    print("z_out: core %.2e, core_tab %.2e" % (_rel(z1, zref), _rel(z2, zref)))
    assert _rel(z1, zref) < 1e-14
    assert numpy.all(numpy.abs(z2 - zref) <= (numpy.abs(lnk) + numpy.abs(d_lnrs) + 4) * EPS * zref)
    # the references at the z each form used
    hc = _hostcheck()
    ratios = {}
    ref_all = {}
    for name, got, zz in (("y_nfw", y, z1), ("y_nfw_core", yc, z1), ("y_nfw_core_tab", yt, z2)):
        add = [mp_y_addends(a, b, M(c)) for a, b, c in zip(zz, con, imk)]
        ref = _fl([sum(a) for a in add])
        mag = _fl([sum(abs(x) for x in a) for a in add])
        ref_all[name] = (ref, mag)
        ratios[name] = numpy.abs(got - ref) / (EPS * mag)
        print("%-15s max |err| %.2e, max |err| / (eps sum|addends|) %.2f at z = %.3g, c = %.3g"
              % (name, numpy.max(numpy.abs(got - ref)), ratios[name].max(),
                 zz[ratios[name].argmax()], con[ratios[name].argmax()]))
    # the host build of the same three, on the same node fields
    hy = numpy.empty((3, lnm.size))
    hc.hc_nfw_forms(e.p, ptr(lnk), ptr(lnm), lnm.size, ptr(d_lnrs), ptr(con), ptr(ln_cp), ptr(imk),
                    ptr(rs), ptr(icprs), ptr(kk), ptr(ik), ptr(hy))
    for j, name in enumerate(("y_nfw", "y_nfw_core", "y_nfw_core_tab")):
        ref, mag = ref_all[name]
        hr = numpy.abs(hy[j] - ref) / (EPS * mag)
        print("host %-15s max |err| / (eps sum|addends|) %.2f" % (name, hr.max()))
        ratios["host " + name] = hr
    for name, rr in ratios.items():
        assert rr.max() <= K_NFW, (name, rr.max())
    for name, got in (("y_nfw", y), ("y_nfw_core", yc), ("y_nfw_core_tab", yt)):
        assert numpy.max(numpy.abs(got - ref_all[name][0])) < 5e-13, name
    # the three against each other
    mag = ref_all["y_nfw"][1]
    prop = 2 * (numpy.abs(numpy.log(z1)) + 4) * (1 + (1 + con) * z1) * EPS * mag
    for name, got in (("y_nfw_core", yc), ("y_nfw_core_tab", yt)):
        rr = numpy.abs(got - y) / prop
        print("%-15s against y_nfw: %.3f of the propagated bound" % (name, rr.max()))
        assert rr.max() <= 1.0, name


def test_exclusion_window(dp):
    """exclusion_window on kR = 1e-8 .. 1e4 against halo.py:1223-1233 in mpmath.  At large kR the
    addends are O(kR^2) and the result O(1 / kR); the reference's own formula cancels the same
    way, so this is kept.  [measured] K_EXCLUSION eps sum|addends|, host build included."""
    kR = numpy.concatenate([numpy.geomspace(1e-8, 1e4, 481), [4.0, numpy.nextafter(4.0, 0.0)]])
    out = numpy.empty_like(kR)
    call(dp, "dp_exclusion", ptr(kR), kR.size, ptr(out))
    host = numpy.empty_like(kR)
    _hostcheck().hc_exclusion(ptr(kR), kR.size, ptr(host))
    ref, mag = [], []
    for v in kR:
        x = M(v)
        add = [x * mp.cos(x) / (3 * x), x ** 3 * mp.ci(x) / (3 * x), (2 - x * x) * mp.sin(x) / (3 * x)]
        ref.append(sum(add))
        mag.append(sum(abs(a) for a in add))
    ref, mag = _fl(ref), _fl(mag)
    r_dev = numpy.abs(out - ref) / (EPS * mag)
    r_host = numpy.abs(host - ref) / (EPS * mag)
    small = kR < 1e-2
    print("exclusion_window: device %.2f (at kR = %.3g), host %.2f eps sum|addends|; "
          "relative for kR < 1e-2: %.2e" % (r_dev.max(), kR[r_dev.argmax()], r_host.max(),
                                            _rel(out[small], ref[small])))
    assert r_dev.max() <= K_EXCLUSION and r_host.max() <= K_EXCLUSION


# -------------------------------------------------------------------------------------------
# linspace_at
# -------------------------------------------------------------------------------------------
def test_linspace_at_bits(dp):
    """linspace_at(a, b, n, i) == numpy.linspace(a, b, n)[i] bit for bit, inlined in a kernel
    compiled with contraction on whose next operation is a multiply-add on the result."""
    rng = numpy.random.default_rng(2049)
    grids = [(numpy.log(1e9), numpy.log(1e16), 50), (numpy.log(1e-3), numpy.log(1e2), 50),
             (numpy.log(0.001), numpy.log(100.0), 196), (numpy.log10(1.48e-8), 0.0, 50),
             (numpy.log(1.1234e10), numpy.log(7.7e15), 50), (-18.4, 9.2, 50), (0.0, 1.0, 2),
             (numpy.log(1e-5), numpy.log(1e5), 2049)]
    for _ in range(200):
        n = int(rng.integers(2, 2050))
        a, b = rng.normal(0, 30, 2) if rng.random() < 0.5 else numpy.sort(rng.uniform(-40, 40, 2))
        grids.append((float(a), float(b), n))
    a = numpy.concatenate([numpy.full(n, a_) for a_, _, n in grids])
    b = numpy.concatenate([numpy.full(n, b_) for _, b_, n in grids])
    nn = numpy.concatenate([numpy.full(n, float(n)) for _, _, n in grids])
    ii = numpy.concatenate([numpy.arange(n, dtype=float) for _, _, n in grids])
    ref = numpy.concatenate([numpy.linspace(a_, b_, n) for a_, b_, n in grids])
    out = numpy.empty(2 * a.size)
    s, t = 1.0000001, -0.3
    call(dp, "dp_linspace", ptr(a), ptr(b), ptr(nn), ptr(ii), a.size, s, t, ptr(out))
    got, used = out.reshape(2, -1)
    diff = got.view(numpy.int64) != ref.view(numpy.int64)
    print("linspace_at: %d of %d points differ from numpy.linspace in a bit" % (diff.sum(), a.size))
    for j in numpy.flatnonzero(diff)[:10]:
        print("   a = %r b = %r n = %d i = %d: %r, numpy %r" % (a[j], b[j], nn[j], ii[j], got[j], ref[j]))
    assert not diff.any()
    # the use behind it: v s + t of the same v, contracted or not (either is within one ulp of
    # the product of the exact value)
    exact = _fl([M(v) * M(s) + M(t) for v in got[::37]])
    assert numpy.all(numpy.abs(used[::37] - exact) <= _ulp(got[::37] * s) + _ulp(exact))
