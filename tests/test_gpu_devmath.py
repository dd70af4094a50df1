"""The fp64 primitives of chomp_amd/csrc/chomp_math.h and the reductions of chomp_romberg.h AS
COMPILED FOR THE DEVICE (tests/devcheck, the product's compiler flags), against mpmath at 50
digits rounded to double -- what tests/test_hostmath.py cannot see: the branches under
__HIP_DEVICE_COMPILE__ (fma_k, the hand-written exp, sincos_lead), hipcc's FMA contraction, the
device library's log / cos / sin / sqrt, and the DPP / v_readlane reductions.

Every accuracy bound is the one test_hostmath.py asserts for the host build of the same function
(named beside each use); each test prints the maximum it measured before it asserts."""
from fractions import Fraction

import mpmath
import numpy
import pytest
from scipy import special
from scipy.interpolate import InterpolatedUnivariateSpline

import devcheck_build as dcb
from devcheck_build import call, ptr

pytestmark = pytest.mark.gpu

mp = mpmath.mp.clone()
mp.dps = 50
EPS = 2.0 ** -52
INF = numpy.inf


@pytest.fixture(scope="module")
def dc():
    return dcb.load()


def _ref(fn, x):
    """fn at every x, evaluated with 50 digits and rounded to the nearest double."""
    return numpy.array([float(fn(mp.mpf(float(v)))) for v in x])


def _around(x, k=3):
    """x and its k neighbours in the doubles on either side."""
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo = numpy.nextafter(lo, -INF)
        hi = numpy.nextafter(hi, INF)
        out += [lo, hi]
    return out


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.int64)


def _ulps(a, b):
    """Distance in units of the last place between non-negative doubles."""
    return numpy.abs(_bits(a) - _bits(b))


def _odd(x):
    """The inputs as a contiguous array whose length is no multiple of 64."""
    x = numpy.ascontiguousarray(x, dtype=numpy.float64)
    if x.size % 64 == 0:
        x = numpy.concatenate([x, x[:1]])
    return x


# -------------------------------------------------------------------------------------------
# exp
# -------------------------------------------------------------------------------------------
EXP_OVERFLOW = 709.782712893384          # exp(x) = inf for every double above ln(DBL_MAX)
EXP_UNDERFLOW = -745.1332191019412       # exp(x) rounds to 0 below ln(2^-1075)


def _exp_inputs():
    finite = numpy.concatenate([
        numpy.linspace(-745.2, 709.8, 12001),
        numpy.linspace(-745.2, -708.3, 2001),                # subnormal results
        _around(EXP_OVERFLOW, 20), _around(EXP_UNDERFLOW, 20),
        _around(-708.3964185322641, 20),                     # ln(DBL_MIN): first subnormal result
        [0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e-300, -1e-300, 3e-301, -7e-305,
         1e3, -1e3, 1e10, -1e10, 1e300, -1e300, 1.0, -1.0, 0.5, -0.5]])
    return _odd(numpy.concatenate([finite, [INF, -INF, numpy.nan]]))


def test_exp(dc):
    """chomp::exp is the device library's exp, bit for bit, at every finite argument (the
    header's own claim), within 1 ulp of the true value, and returns the library's 0 / inf / NaN
    beyond the thresholds and at the non-finite arguments."""
    x = _exp_inputs()
    assert x.size % 64 != 0
    mine, lib = numpy.empty_like(x), numpy.empty_like(x)
    call(dc, "dc_exp", ptr(x), x.size, ptr(mine), ptr(lib))
    fin = numpy.isfinite(x)
    ref = _ref(mp.exp, x[fin])
    # the required results off the finite range
    at = {float(v): float(m) for v, m in zip(x, mine)}
    print("exp(-inf) = %r, exp(+inf) = %r, exp(-1e300) = %r, exp(1e300) = %r, exp(1e10) = %r"
          % (at[-INF], at[INF], at[-1e300], at[1e300], at[1e10]))
    diff = _bits(mine[fin]) != _bits(lib[fin])
    print("exp: %d of %d finite arguments differ from the library's bits" % (diff.sum(), fin.sum()))
    for v, m, l in list(zip(x[fin][diff], mine[fin][diff], lib[fin][diff]))[:20]:
        print("   x = %r: chomp::exp %r, ::exp %r" % (v, m, l))
    ok = numpy.isfinite(mine[fin])
    u = _ulps(mine[fin][ok], ref[ok])
    print("exp: max distance from the true value %d ulp (library: %d ulp)"
          % (u.max(), _ulps(lib[fin], ref).max()))
    assert at[-INF] == 0.0
    assert at[INF] == INF
    assert numpy.all(numpy.isnan(mine[numpy.isnan(x)]))
    assert numpy.all(mine[x < -745.14] == 0.0), x[(x < -745.14) & (mine != 0.0)]
    assert numpy.all(mine[x > 709.79] == INF), x[(x > 709.79) & (mine != INF)]
    assert numpy.all(mine[x == 0.0] == 1.0)
    assert not diff.any()
    assert numpy.array_equal(numpy.isfinite(mine[fin]), numpy.isfinite(ref))
    assert u.max() <= 1


# -------------------------------------------------------------------------------------------
# fma_k
# -------------------------------------------------------------------------------------------
def test_fma_k(dc):
    """fma_k(a, b, C) -- v_fma_f64 with the addend in scalar registers -- is fma(a, b, C): the
    same bits as the compiler's fma in the same kernel, and the correctly rounded a b + C."""
    nc = dc.dc_fma_k_count()
    C = numpy.empty(nc)
    dc.dc_fma_k_constants(ptr(C))
    rng = numpy.random.default_rng(3)
    a, b = [], []
    for c in C:
        bb = rng.uniform(0.5, 2.0, 200) * 10.0 ** rng.uniform(-3, 3, 200)
        # a b cancels C to its last bits, to half its bits and not at all
        for scale in (1e-16, 1e-8, 1.0):
            a.append(-c / bb * (1.0 + scale * rng.uniform(-4, 4, 200)))
            b.append(bb)
    # results in the subnormal range and on the overflow threshold, wide dynamic range
    a.append(rng.uniform(-1, 1, 400) * 10.0 ** rng.uniform(-160, -150, 400))
    b.append(rng.uniform(-1, 1, 400) * 10.0 ** rng.uniform(-160, -150, 400))
    a.append(rng.uniform(-1, 1, 400) * 10.0 ** rng.uniform(-300, 300, 400))
    b.append(rng.uniform(-1, 1, 400) * 10.0 ** rng.uniform(-8, 8, 400))
    a.append(numpy.array([0.0, -0.0, 1.0, 5e-324, 1e154, -1e154, 1e150]))
    b.append(numpy.array([3.0, 3.0, -0.0, 0.5, 1e154, 1e154, -1e150]))
    a, b = _odd(numpy.concatenate(a)), _odd(numpy.concatenate(b))
    n = a.size
    out_k, out_f = numpy.empty(nc * n), numpy.empty(nc * n)
    call(dc, "dc_fma_k", ptr(a), ptr(b), n, ptr(out_k), ptr(out_f))
    out_k, out_f = out_k.reshape(nc, n), out_f.reshape(nc, n)
    sub = numpy.sum((numpy.abs(out_f) < 2.2250738585072014e-308) & (out_f != 0))
    print("fma_k: %d x %d cases, %d subnormal results" % (nc, n, sub))
    assert sub > 100
    assert numpy.array_equal(_bits(out_k), _bits(out_f))
    for k, c in enumerate(C):
        for i in range(n):
            exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c))
            try:
                want = float(exact)               # (correctly rounded, subnormals included)
            except OverflowError:
                want = INF if exact > 0 else -INF
            assert out_k[k, i] == want, (c, a[i], b[i], out_k[k, i], want)


# -------------------------------------------------------------------------------------------
# fast_sincos, fast_sincos_pm, tophat_numer_pm
# -------------------------------------------------------------------------------------------
def _sincos_inputs():
    rng = numpy.random.default_rng(11)
    k = numpy.arange(0, 2000) * numpy.pi / 4
    edges = numpy.concatenate([k, numpy.nextafter(k, INF), numpy.nextafter(k, -INF), -k[1:400]])
    return _odd(numpy.concatenate([
        numpy.logspace(-12, numpy.log10(3.3e9), 6001), -numpy.logspace(-8, 5, 2001),
        rng.uniform(0, 1e4, 4000), rng.uniform(-3.3e9, 3.3e9, 500), edges,
        [0.0, numpy.pi / 2, numpy.pi, 1e8, 3.3e9, -3.3e9]]))


@pytest.fixture(scope="module")
def sincos(dc):
    x = _sincos_inputs()
    assert x.size <= 20000 and x.size % 64 != 0
    out = numpy.empty(7 * x.size)
    call(dc, "dc_sincos", ptr(x), x.size, ptr(out))
    return (x,) + tuple(out.reshape(7, x.size))


def test_fast_sincos(dc, sincos):
    """Bound: test_hostmath.test_fast_sincos, 2.3e-16 absolute (relative where sin x ~ x)."""
    x, s, c = sincos[:3]
    rs, rc = _ref(mp.sin, x), _ref(mp.cos, x)
    es, ec = numpy.abs(s - rs), numpy.abs(c - rc)
    print("fast_sincos: max |sin error| %.3g at x = %r, max |cos error| %.3g at x = %r"
          % (es.max(), x[es.argmax()], ec.max(), x[ec.argmax()]))
    assert es.max() < 2.3e-16
    assert ec.max() < 2.3e-16
    small = numpy.abs(x) < 1e-3
    rel = numpy.abs(s[small] - rs[small]) / numpy.maximum(numpy.abs(x[small]), 1e-300)
    print("fast_sincos: max relative sin error for |x| < 1e-3: %.3g" % rel.max())
    assert rel.max() < 2.3e-16
    # degrades gracefully, stays in [-1, 1] (the host test's trio)
    big = _odd(numpy.array([1e12, 7.7e14, -3e13]))
    out = numpy.empty(7 * big.size)
    call(dc, "dc_sincos", ptr(big), big.size, ptr(out))
    sb, cb = out.reshape(7, big.size)[:2]
    assert numpy.all(numpy.abs(sb) <= 1.0 + 1e-15) and numpy.all(numpy.abs(cb) <= 1.0 + 1e-15)
    assert numpy.max(numpy.abs(sb - _ref(mp.sin, big))) < 1e-15 * 1e15 * 1e-15 + 1e-3


def test_fast_sincos_pm_and_tophat(sincos):
    """fast_sincos_pm is fast_sincos up to ONE sign for the pair; tophat_numer_pm is
    +-(sin x - x cos x) of fast_sincos's pair, bit for bit up to the sign, in both call forms."""
    x, s, c, spm, cpm, th_ref, th_default, th_lead = sincos
    same = (spm == s) & (cpm == c)
    flipped = (spm == -s) & (cpm == -c)
    print("fast_sincos_pm: %d as fast_sincos, %d with both signs flipped, of %d"
          % (same.sum(), (flipped & ~same).sum(), x.size))
    assert numpy.all(same | flipped), x[~(same | flipped)][:10]
    assert flipped.sum() > x.size // 10 and same.sum() > x.size // 10
    assert numpy.array_equal(_bits(th_default), _bits(th_lead))
    assert numpy.array_equal(_bits(numpy.abs(th_default)), _bits(numpy.abs(th_ref)))


# -------------------------------------------------------------------------------------------
# fast_log
# -------------------------------------------------------------------------------------------
def test_fast_log(dc):
    """Bounds: test_hostmath.test_fast_log, 4e-16 relative and 4e-19 absolute near 1."""
    rng = numpy.random.default_rng(7)
    p2 = 2.0 ** numpy.arange(-1022, 1024, 7)
    r2 = numpy.sqrt(2.0) * 2.0 ** numpy.arange(-1000, 1000, 17)
    x = _odd(numpy.concatenate([
        numpy.logspace(-300, 300, 6001), 1.0 + rng.uniform(-1e-3, 1e-3, 3000),
        rng.uniform(0.5, 2.0, 6000), p2, numpy.nextafter(p2, INF), numpy.nextafter(p2[1:], 0),
        r2, numpy.nextafter(r2, INF), numpy.nextafter(r2, 0),
        _around(numpy.sqrt(0.5), 5), _around(numpy.sqrt(2.0), 5), _around(1.0, 5), [2.0, 0.5]]))
    assert x.size <= 20000
    out = numpy.empty_like(x)
    call(dc, "dc_fast_log", ptr(x), x.size, ptr(out))
    ref = _ref(mp.log, x)
    big = numpy.abs(ref) > 1e-3
    rel = numpy.abs(out - ref)[big] / numpy.abs(ref)[big]
    ab = numpy.abs(out - ref)[~big]
    print("fast_log: max relative error %.3g at x = %r; max absolute error near 1 %.3g at x = %r"
          % (rel.max(), x[big][rel.argmax()], ab.max(), x[~big][ab.argmax()]))
    assert rel.max() < 4e-16
    assert ab.max() < 4e-19


# -------------------------------------------------------------------------------------------
# Si, Ci
# -------------------------------------------------------------------------------------------
# Ci against mpmath: the host test's 3e-15 holds against SciPy's Ci only, which is itself one unit
# of the last place off the true value where |Ci| is in [16, 32): 3.553e-15 = ulp(17.69) at
# x = 1.1605855066056662e-08, Ci = gamma + ln x + ... rounded once in that binade.  The host build
# (g++) and SciPy return the same double there as the device: no host / device difference.
# Measured maximum against mpmath (MI355X and host alike) 3.553e-15, times 2 (finite sample).
CI_BOUND = 2 * 3.553e-15


def test_sici(dc):
    """Bounds: test_hostmath.test_sici, 1.6e-15 for Si and 3e-15 for Ci (absolute; Ci against the
    true value: CI_BOUND above)."""
    seams = numpy.concatenate([_around(32.0 / j, 2) for j in range(1, 9)])    # Chebyshev panels
    x = _odd(numpy.concatenate([
        numpy.logspace(-8, numpy.log10(4), 400)[:-1], numpy.linspace(4, 40, 2000),
        numpy.logspace(1.6, 5, 500), seams, _around(4.0, 4), [32.0 / 7, 8.0, 16.0, 1e6]]))
    assert x.size <= 4000
    ln_x = _ref(mp.log, x)
    out = numpy.empty(4 * x.size)
    call(dc, "dc_sici", ptr(x), ptr(ln_x), x.size, ptr(out))
    si, ci, si_ln, ci_ln = out.reshape(4, x.size)
    rsi, rci = _ref(mp.si, x), _ref(mp.ci, x)
    esi, eci = numpy.abs(si - rsi), numpy.abs(ci - rci)
    print("sici: max |Si error| %.3g at x = %r, max |Ci error| %.3g at x = %r"
          % (esi.max(), x[esi.argmax()], eci.max(), x[eci.argmax()]))
    print("sici_sc_ln: max |Si - sici's| %.3g, max |Ci - sici's| %.3g; against the true values "
          "%.3g, %.3g" % (numpy.abs(si_ln - si).max(), numpy.abs(ci_ln - ci).max(),
                          numpy.abs(si_ln - rsi).max(), numpy.abs(ci_ln - rci).max()))
    assert esi.max() < 4e-16 * 4
    assert numpy.abs(ci - special.sici(x)[1]).max() < 3e-15      # the host test's own assertion
    assert eci.max() < CI_BOUND
    assert numpy.abs(si_ln - si).max() < 4e-16 * 4
    assert numpy.abs(ci_ln - ci).max() < 3e-15
    assert numpy.abs(si_ln - rsi).max() < 4e-16 * 4
    assert numpy.abs(ci_ln - rci).max() < CI_BOUND


# -------------------------------------------------------------------------------------------
# J0, J2
# -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 2])
def test_bessel(dc, order):
    """Bounds: test_hostmath.test_bessel, 2e-15 absolute up to x = 200 and 2e-17 x beyond."""
    edges = numpy.concatenate([_around(4.0 * j, 3) for j in range(1, 9)])     # 4-wide panels, 32
    x = _odd(numpy.concatenate([
        numpy.linspace(0, 32, 1801), edges, numpy.linspace(32, 200, 1500),
        numpy.logspace(2.3, 5, 200), [0.0, 1e5]]))
    assert x.size <= 4000
    out = numpy.empty_like(x)
    call(dc, "dc_bessel", order, ptr(x), x.size, ptr(out))
    ref = _ref(lambda v: mp.besselj(order, v), x)
    small = x <= 200.0
    e_small = numpy.abs(out - ref)[small]
    e_big = (numpy.abs(out - ref) / numpy.maximum(x, 1.0))[~small]
    print("J%d: max |error| %.3g at x = %r (x <= 200); max |error| / x %.3g at x = %r beyond"
          % (order, e_small.max(), x[small][e_small.argmax()], e_big.max(),
             x[~small][e_big.argmax()]))
    assert e_small.max() < 2e-15
    assert e_big.max() < 2e-17


# -------------------------------------------------------------------------------------------
# not-a-knot spline, built and evaluated on the device
# -------------------------------------------------------------------------------------------
def test_notaknot_spline(dc):
    """Bound: test_hostmath.test_notaknot_spline, 2e-13 against FITPACK (the spline's definition:
    SciPy is the reference here, as there)."""
    rng = numpy.random.default_rng(7)
    for uniform in (0, 1):
        if uniform:
            x = numpy.linspace(numpy.log(1e-3), numpy.log(1e2), 50)
        else:
            x = numpy.cumsum(rng.uniform(0.05, 2.0, 50))
        y = numpy.sin(x) * numpy.exp(0.1 * x) + 3
        ref = InterpolatedUnivariateSpline(x, y)
        xe = numpy.concatenate([numpy.linspace(x[0] - 1.0, x[-1] + 1.0, 1001), x])
        out = numpy.empty_like(xe)
        call(dc, "dc_spline", ptr(x), ptr(y), x.size, ptr(xe), xe.size, ptr(out), uniform)
        err = numpy.max(numpy.abs(out - ref(xe)) / (1 + numpy.abs(ref(xe))))
        print("spline (%s knots): max error %.3g" % ("uniform" if uniform else "graded", err))
        assert err < 2e-13


# -------------------------------------------------------------------------------------------
# reductions
# -------------------------------------------------------------------------------------------
def _wave_sum_ref(v):
    """wave_sum's documented order in IEEE double: quad xor-1, xor-2, row-rotate 4, row-rotate 8
    (a lane of a 16-lane row takes the lane 4, then 8, below it, cyclically), then
    (r0 + r16) + (r32 + r48).  v: [..., 64]; the value every lane returns."""
    lane = numpy.arange(64)
    v = v + v[..., lane ^ 1]
    v = v + v[..., lane ^ 2]
    row, pos = lane & ~15, lane & 15
    v = v + v[..., row | ((pos - 4) & 15)]
    v = v + v[..., row | ((pos - 8) & 15)]
    return (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])


def _wide(rng, shape):
    """Mixed signs, 30 orders of magnitude: another order of summation changes the bits."""
    return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-15, 15, shape)


def test_wave_sums(dc):
    rng = numpy.random.default_rng(5)
    nw = 96
    v = _wide(rng, (nw, 64))
    v[0] = numpy.arange(64.0)                       # (a plain one)
    v[1] = 2.0 ** -numpy.arange(64.0)               # (exact in any order: lanes only)
    # the documented order is not just any order on these inputs
    assert numpy.mean(_wave_sum_ref(v) != numpy.sum(v, axis=-1)) > 0.5
    out = numpy.empty_like(v)
    call(dc, "dc_wave_sum", 0, ptr(v), nw, ptr(out))
    want = _wave_sum_ref(v)
    assert numpy.array_equal(_bits(out), _bits(numpy.repeat(want[:, None], 64, axis=1)))
    # wave_sum32 / wave_sum16: lanes 32.. / 16.. hold garbage (NaN, inf, huge) that must not count
    garbage = numpy.array([numpy.nan, INF, -INF, 1e308, -1e308, 7.0])
    for mode, keep in ((1, 32), (2, 16)):
        g = v.copy()
        g[:, keep:] = rng.choice(garbage, (nw, 64 - keep))
        z = v.copy()
        z[:, keep:] = 0.0
        call(dc, "dc_wave_sum", mode, ptr(g), nw, ptr(out))
        want = _wave_sum_ref(z)
        # ... and the same bits from wave_sum itself with those lanes zeroed
        full = numpy.empty_like(v)
        call(dc, "dc_wave_sum", 0, ptr(z), nw, ptr(full))
        assert numpy.array_equal(_bits(full), _bits(numpy.repeat(want[:, None], 64, axis=1)))
        assert numpy.array_equal(_bits(out), _bits(full)), keep


@pytest.mark.parametrize("nw", [2, 4, 8, 16])
def test_group_sum(dc, nw):
    """group_sum<NW>: the wavefront totals added left to right, every thread the same value;
    twice in a row (the second call takes the other half of the exchange buffer)."""
    rng = numpy.random.default_rng(nw)
    ng = 5
    a, b = _wide(rng, (ng, nw, 64)), _wide(rng, (ng, nw, 64))
    oa, ob = numpy.empty_like(a), numpy.empty_like(b)
    call(dc, "dc_group_sum", nw, ptr(a), ptr(b), ng, ptr(oa), ptr(ob))
    for v, o in ((a, oa), (b, ob)):
        tot = _wave_sum_ref(v)                       # [ng, nw]
        t = numpy.zeros(ng)
        for w in range(nw):
            t = t + tot[:, w]
        assert numpy.array_equal(_bits(o), _bits(numpy.broadcast_to(t[:, None, None], o.shape)))
