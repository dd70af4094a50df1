"""chomp_romberg.h driven directly on the device (tests/devcheck): romberg_group<NW, NF>,
romberg_wave6, romberg1, the dump -> RombergResume hand-over, RombergLoose and gauss_panels, with
integrands whose answer AND stopping level are known independently.

Reference: oracle/romberg.py (SciPy's rule, pinned by tests/test_oracle.py) in float64 with each
integrand restated in NumPy, operation for operation (the harness compiles its integrands without
FMA contraction); mpmath keeps the oracle honest.  Value and stopping level are compared."""
import math
import warnings

import mpmath
import numpy
import pytest

import devcheck_build as dcb
from devcheck_build import SHAPE, call, ptr
from oracle.romberg import AccuracyWarning, romberg

gpu = pytest.mark.gpu

mp = mpmath.mp.clone()
mp.dps = 50
EPS = 2.0 ** -52
TOL = 1.48e-8
RTOLS = (1.48e-8, 1e-5, 1e-10)
DIVMAXES = (1, 2, 5, 6, 7, 8, 9, 10, 16)
DMAX = max(DIVMAXES)

# Value bound: |device - oracle| <= K eps |b - a| mean|f| (the mean over the nodes used).
# Measured on the MI355X over all cases and all execution shapes: the largest ratio is 4.537
# (e^{1.5x} / (1 + e^{2x})^2 on [-9, 9], rtol 1.48e-8, divmax 7, the same in every shape: the
# device's exp against NumPy's at the nodes, not the order of summation).  K is twice that,
# rounded up to a power of two.
K = 16.0


# -------------------------------------------------------------------------------------------
# the integrands of the harness's menu, restated (tests/devcheck/devcheck.hip, struct Menu)
# -------------------------------------------------------------------------------------------
def f_np(ident, x):
    x = numpy.asarray(x, dtype=numpy.float64)
    if ident == 0:
        return x * x * x - 2.0 * x + 1.0
    if ident == 1:
        return numpy.exp(x)
    if ident == 2:
        return numpy.sin(10.0 * x)
    if ident == 3:
        return 1.0 + numpy.sin(40.0 * x)
    if ident == 4:
        return numpy.exp(-200.0 * ((x - 0.37) * (x - 0.37)))
    if ident == 5:
        return numpy.sqrt(x)
    if ident == 6:
        return numpy.where(x < 0.3, 1.0, 0.25)
    if ident == 7:
        return 1.0 / (1e-4 + (x - 0.5) * (x - 0.5))
    if ident == 8:
        d = 1.0 + numpy.exp(2.0 * x)
        return numpy.exp(1.5 * x) / (d * d)
    if ident == 9:
        return numpy.cos(x)
    if ident == 10:
        return numpy.zeros_like(x)
    if ident == 11:
        p = numpy.full_like(x, 1.0 / 32.0)
        for k in range(30, -1, -1):
            p = p * x + 1.0 / float(k + 1)
        return p
    if ident == 12:
        x2 = x * x
        x4 = x2 * x2
        x8 = x4 * x4
        x16 = x8 * x8
        return (((x16 * x8) * x4) * x2) * x
    if ident == 13:
        return (x * x) * (x * x) * x + 3.0 * (x * x) + 0.5
    raise ValueError(ident)


def exact_integral(ident, a, b):
    """The integral to 50 digits (mpmath)."""
    a, b = mp.mpf(a), mp.mpf(b)
    prim = {
        0: lambda x: x ** 4 / 4 - x ** 2 + x,
        1: mp.exp,
        2: lambda x: -mp.cos(10 * x) / 10,
        3: lambda x: x - mp.cos(40 * x) / 40,
        4: lambda x: mp.sqrt(mp.pi / 200) / 2 * mp.erf(mp.sqrt(200) * (x - mp.mpf("0.37"))),
        5: lambda x: 2 * x ** mp.mpf(1.5) / 3,
        6: lambda x: x if x < mp.mpf(0.3) else mp.mpf(0.3) + (x - mp.mpf(0.3)) / 4,
        7: lambda x: 100 * mp.atan(100 * (x - mp.mpf("0.5"))),
        9: mp.sin,
        10: lambda x: mp.mpf(0),
        11: lambda x: sum(mp.mpf(1.0 / float(k + 1)) * x ** (k + 1) / (k + 1) for k in range(32)),
        12: lambda x: x ** 32 / 32,
        13: lambda x: x ** 6 / 6 + x ** 3 + x / 2,
    }
    if ident == 8:
        return mp.quad(lambda x: mp.exp(1.5 * x) / (1 + mp.exp(2 * x)) ** 2,
                       numpy.linspace(float(a), float(b), 19).tolist())
    return prim[ident](b) - prim[ident](a)


# (integrand, a, b): the table of the issue.  The constants 1e-4, 0.37 of the device integrands
# are the doubles; the exact integrals take the decimal values (the difference is far below the
# tolerances they are compared at).
INTEGRALS = [
    (0, 0.0, 2.0), (1, 0.0, 1.0), (2, 0.0, 3.0), (3, 0.0, 3.0), (4, 0.0, 1.0), (5, 0.0, 1.0),
    (6, 0.0, 1.0), (7, 0.0, 1.0), (8, -9.0, 9.0), (9, 2.0, 0.5), (10, -1.0, 2.0), (1, 0.7, 0.7),
]
# NF = 2: two integrands on the same nodes that stop at different levels, in both positions
PAIRS = [(1, 4, 0.0, 1.0), (4, 1, 0.0, 1.0), (5, 6, 0.0, 1.0), (7, 1, 0.0, 1.0), (1, 7, 0.0, 1.0),
         (2, 3, 0.0, 3.0), (3, 2, 0.0, 3.0), (10, 1, 0.0, 1.0)]


class Oracle(object):
    """One integral on the CPU: the diagonal R[i][i], i = 0 .. DMAX, from oracle.romberg run with
    tol = rtol = 0 to each divmax (the same arithmetic as any run with other tolerances), the
    mean |f| over the nodes of each level's grid, and the exact value."""

    def __init__(self, ident, a, b):
        self.ident, self.a, self.b = ident, a, b
        f = lambda x: f_np(ident, x)                     # noqa: E731
        self.diag = [(b - a) * (0.5 * (float(f(a)) + float(f(b))))]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", AccuracyWarning)
            for i in range(1, DMAX + 1):
                self.diag.append(float(romberg(f, a, b, tol=0.0, rtol=0.0, divmax=i,
                                               vec_func=True)))
        self.mean_abs = []
        for i in range(DMAX + 1):
            x = a + (b - a) * numpy.arange(2 ** i + 1) / float(2 ** i)
            self.mean_abs.append(float(numpy.mean(numpy.abs(f(x)))))
        self.exact = float(exact_integral(ident, a, b))
        self._runs = {}

    def run(self, tol, rtol, divmax):
        """(value, level, converged) of oracle.romberg itself (computed once)."""
        key = (tol, rtol, divmax)
        if key not in self._runs:
            self._runs[key] = self._run(*key)
        return self._runs[key]

    def _run(self, tol, rtol, divmax):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            value, level = romberg(lambda x: f_np(self.ident, x), self.a, self.b, tol=tol,
                                   rtol=rtol, divmax=divmax, vec_func=True, return_level=True)
        return float(value), level, not any(issubclass(x.category, AccuracyWarning) for x in w)

    def walk(self, tol, rtol, divmax, loose_rtol=None, min_level=8):
        """The rows the rule walks, from the diagonal: (level, converged, the err / threshold
        ratios of every row walked [, the same for the loose rule from min_level on])."""
        ratios, loose_ratios = [], []
        for i in range(1, divmax + 1):
            err = abs(self.diag[i] - self.diag[i - 1])
            ratios.append(err / max(tol, rtol * abs(self.diag[i])))
            if err < tol or err < rtol * abs(self.diag[i]):
                return i, True, ratios, loose_ratios
            if loose_rtol is not None and i >= min_level:
                den = loose_rtol * abs(self.diag[i])
                loose_ratios.append(err / den if den > 0 else numpy.inf)
                if err < den:
                    return i, True, ratios, loose_ratios
        return divmax, False, ratios, loose_ratios

    def bound(self, level):
        return K * EPS * abs(self.b - self.a) * self.mean_abs[level]


def _marginal(ratios):
    return [r for r in ratios if 0.9 <= r <= 1.1]


@pytest.fixture(scope="module")
def oracles():
    return {key: Oracle(*key) for key in set(INTEGRALS) | {(p[0], p[2], p[3]) for p in PAIRS} |
            {(p[1], p[2], p[3]) for p in PAIRS}}


@pytest.fixture(scope="module")
def dc():
    return dcb.load()


def _cases(rows):
    """rows of dictionaries -> the harness's case array."""
    stride = 16
    c = numpy.zeros((len(rows), stride))
    for r, row in zip(c, rows):
        r[0], r[1], r[2], r[3] = row["a"], row["b"], row.get("tol", TOL), row.get("rtol", RTOLS[0])
        r[4], r[5], r[6] = row["divmax"], row["id0"], row.get("id1", row["id0"])
        if "loose" in row:
            r[7] = 1.0
            r[8:13] = row["loose"]
        r[13] = row.get("d", 0)
    return c


def _quad(dc, shape, rows, entry="dc_quad"):
    c = _cases(rows)
    assert dc.dc_case_stride() == c.shape[1]
    out = numpy.full((len(rows), dc.dc_out_stride()), numpy.nan)
    call(dc, entry, shape if isinstance(shape, int) else SHAPE[shape], ptr(c), len(rows), ptr(out))
    assert numpy.all(out[:, 6] == 0.0), "threads of one group disagree in value or level"
    return out


SINGLE_SHAPES = ["group1", "group2", "group4", "group8", "group16", "group4_unroll4",
                 "group4_fast4", "wave6", "romberg1_1", "romberg1_4"]
NW_SHAPES = ["group1", "group2", "group4", "group8", "group16"]


def _single_rows(shape):
    return [dict(a=a, b=b, id0=ident, rtol=rtol, divmax=dm)
            for (ident, a, b) in INTEGRALS for rtol in RTOLS for dm in DIVMAXES
            if not (shape.startswith("wave6") and dm < 6)]


@pytest.fixture(scope="module")
def singles(dc):
    """Every single-integrand execution shape on every case: shape -> (rows, output)."""
    return {shape: (_single_rows(shape), _quad(dc, shape, _single_rows(shape)))
            for shape in SINGLE_SHAPES}


def test_cases_are_admissible(oracles):
    """A property of the inputs, on the CPU: no stopping decision the oracle takes is marginal
    (err / max(tol, rtol |result|) outside [0.9, 1.1] at every row walked), the levels cover both
    sides of every NW's fused first round, and the walk from the diagonal is the oracle's."""
    levels, closest = set(), numpy.inf
    for row in _single_rows("group1"):
        o = oracles[(row["id0"], row["a"], row["b"])]
        level, conv, ratios, _ = o.walk(TOL, row["rtol"], row["divmax"])
        assert not _marginal(ratios), (row, ratios)
        closest = min([closest] + [abs(math.log(r)) for r in ratios if r > 0])
        value, olevel, oconv = o.run(TOL, row["rtol"], row["divmax"])
        assert (olevel, oconv) == (level, conv) and value == o.diag[level], row
        levels.add(level if conv else -1)
    print("stopping levels covered: %s (-1: divmax exhausted); smallest |ln(err / threshold)| %.2f"
          % (sorted(levels), closest))
    assert {1, 2, 3, 4, 8, 9, 10, 12, 13, -1} <= levels


def test_oracle_against_mpmath(oracles):
    """Wherever the oracle says converged it is within 10 max(tol, rtol |I|) of the integral."""
    for row in _single_rows("group1"):
        o = oracles[(row["id0"], row["a"], row["b"])]
        value, level, conv = o.run(TOL, row["rtol"], row["divmax"])
        if conv:
            assert abs(value - o.exact) <= 10 * max(TOL, row["rtol"] * abs(o.exact)), (row, value)


@gpu
@pytest.mark.parametrize("shape", SINGLE_SHAPES)
def test_level_and_value(oracles, singles, shape):
    rows, out = singles[shape]
    worst = (0.0, None)
    for row, got in zip(rows, out):
        o = oracles[(row["id0"], row["a"], row["b"])]
        value, level, conv = o.run(TOL, row["rtol"], row["divmax"])
        assert int(got[2]) == level, (row, got, level)
        if got[4] >= 0:
            assert bool(got[4]) == conv, (row, got)
        scale = EPS * abs(o.b - o.a) * o.mean_abs[level]
        if scale == 0.0:
            assert got[0] == 0.0 and value == 0.0, (row, got)
        else:
            worst = max(worst, (abs(got[0] - value) / scale, str(row)), key=lambda t: t[0])
        if conv:
            assert abs(got[0] - o.exact) <= 10 * max(TOL, row["rtol"] * abs(o.exact)), (row, got)
    print("%s: %d cases, largest |device - oracle| / (eps |b - a| mean|f|) = %.3f at %s"
          % ((shape, len(rows)) + worst))
    assert worst[0] <= K


@gpu
def test_shape_independence(oracles, singles):
    """All NW, UNROLL 1 / 4 (with and without fast()), romberg1 and romberg_wave6 agree in level
    exactly and in value within the K bound; how many agree bit for bit is reported."""
    base_rows, base = singles["group1"]
    index = {(r["id0"], r["a"], r["b"], r["rtol"], r["divmax"]): i for i, r in enumerate(base_rows)}
    for shape in SINGLE_SHAPES[1:]:
        rows, out = singles[shape]
        same = 0
        for row, got in zip(rows, out):
            ref = base[index[(row["id0"], row["a"], row["b"], row["rtol"], row["divmax"])]]
            o = oracles[(row["id0"], row["a"], row["b"])]
            assert got[2] == ref[2], (shape, row)
            assert abs(got[0] - ref[0]) <= o.bound(int(ref[2])), (shape, row, got[0], ref[0])
            same += got[0] == ref[0]
        print("%s: %d of %d values bit-identical to romberg_group<1, 1>" % (shape, same, len(rows)))
    # the wrappers are the same code: bit for bit
    for a_, b_ in (("romberg1_1", "group1"), ("romberg1_4", "group4"), ("group4_unroll4", "group4"),
                   ("group4_fast4", "group4")):
        assert numpy.array_equal(singles[a_][1][:, 0], singles[b_][1][:, 0]), (a_, b_)
    allnw = numpy.all([singles[s][1][:, 0] == base[:, 0] for s in NW_SHAPES], axis=0)
    print("bit-identical across NW = 1, 2, 4, 8, 16: %d of %d cases" % (allnw.sum(), len(base_rows)))


@gpu
@pytest.mark.parametrize("shape", ["group1_nf2", "group4_nf2", "wave6_nf2"])
def test_two_integrands(dc, oracles, shape):
    """NF = 2: each integrand stops at its own level with its own value, in either position."""
    rows = [dict(a=a, b=b, id0=i0, id1=i1, rtol=rtol, divmax=dm)
            for (i0, i1, a, b) in PAIRS for rtol in RTOLS for dm in DIVMAXES
            if not (shape.startswith("wave6") and dm < 6)]
    out = _quad(dc, shape, rows)
    differ = 0
    for row, got in zip(rows, out):
        for q, ident in enumerate((row["id0"], row["id1"])):
            o = oracles[(ident, row["a"], row["b"])]
            value, level, conv = o.run(TOL, row["rtol"], row["divmax"])
            assert int(got[2 + q]) == level and bool(got[4 + q]) == conv, (row, q, got)
            assert abs(got[q] - value) <= o.bound(level), (row, q, got[q], value)
        differ += got[2] != got[3]
    print("%s: %d cases, the two integrands stop at different levels in %d" % (shape, len(rows), differ))
    assert differ > len(rows) // 4


HANDOVER = ((6, 10), (7, 12), (9, 16))


@gpu
@pytest.mark.parametrize("stage", [0, 1])
def test_hand_over(dc, oracles, stage):
    """Stopped by divmax = d with its state dumped, then RombergResume to D: the straight run to
    D in level; bit for bit in value where the level sums are formed the same way (from
    romberg_group<4, 1> at d >= 7: the same fused grid and the same strided sums), within the K
    bound otherwise.  An integral that converged before d is not resumed."""
    rows = [dict(a=a, b=b, id0=ident, rtol=rtol, divmax=D, d=d)
            for (ident, a, b) in INTEGRALS for rtol in RTOLS for (d, D) in HANDOVER]
    out = _quad(dc, stage, rows, entry="dc_resume")
    straight = _quad(dc, "group4" if stage == 0 else "wave6", rows)
    first = _quad(dc, "group4" if stage == 0 else "wave6", [dict(r, divmax=r["d"]) for r in rows])
    resumed = untouched = 0
    for row, got, ref, alone in zip(rows, out, straight, first):
        o = oracles[(row["id0"], row["a"], row["b"])]
        value, level, conv = o.run(TOL, row["rtol"], row["divmax"])
        assert int(got[2]) == level == int(ref[2]) and bool(got[4]) == conv, (row, got, ref)
        before = o.walk(TOL, row["rtol"], row["d"])
        if before[1]:                               # converged before d: nothing to carry on,
            assert got[7] == 0 and numpy.array_equal(got[:6], alone[:6]), (row, got, alone)   # unchanged
            untouched += 1
        else:
            assert got[7] == level - row["d"], (row, got)
            resumed += got[7] > 0
        if stage == 0 and row["d"] >= 7:
            assert got[0] == ref[0], (row, got[0], ref[0])
        else:
            assert abs(got[0] - ref[0]) <= o.bound(level), (row, got[0], ref[0])
        assert abs(got[0] - value) <= o.bound(level), (row, got[0], value)
    print("hand-over from %s: %d carried on, %d already converged"
          % ("romberg_group<4, 1>" if stage == 0 else "romberg_wave6<1>", resumed, untouched))
    assert resumed > 10 and untouched > 10


@gpu
@pytest.mark.parametrize("shape", ["group1", "group4", "wave6"])
def test_loose_rule(dc, oracles, shape):
    rtol_loose, far = 1e-3, [1e30, 2e30, -2e30, -1e30]
    base = [dict(a=a, b=b, id0=ident, rtol=rtol, divmax=dm)
            for (ident, a, b) in INTEGRALS for rtol in RTOLS for dm in (7, 8, 10, 16)]
    outside = [dict(r, loose=[rtol_loose] + far) for r in base]
    inside = [dict(r, loose=[rtol_loose, -1e300, 1e300, -1e300, 1e300]) for r in base]
    plain, got_out, got_in = _quad(dc, shape, base), _quad(dc, shape, outside), _quad(dc, shape, inside)
    # a window that contains the result: the regular rule alone, bit for bit
    assert numpy.array_equal(plain, got_in)
    earlier = 0
    for row, got, reg in zip(base, got_out, plain):
        o = oracles[(row["id0"], row["a"], row["b"])]
        level, conv, ratios, loose_ratios = o.walk(TOL, row["rtol"], row["divmax"], rtol_loose)
        assert not _marginal(ratios) and not _marginal(loose_ratios), row
        assert int(got[2]) == level and bool(got[4]) == conv, (row, got, level)
        assert abs(got[0] - o.diag[level]) <= o.bound(level), (row, got)
        if got[2] < reg[2]:                          # the loose rule decided: never below level 8
            earlier += 1
            assert got[2] >= 8, (row, got)
    print("%s: the loose rule stopped %d of %d integrals earlier" % (shape, earlier, len(base)))
    assert earlier > 5


@gpu
@pytest.mark.parametrize("shape", [0, 1, 2, 3, 4, 5])
def test_node_indexing(dc, shape):
    """An integrand that returns (j, level, 1 if x is node (level, j) of [a, b]): the dumped
    trapezoid estimates T_m = (b - a) sum_{l <= m} S_l / 2^m hold the exact sum of j, the exact
    level-weighted node counts and the node counts of every level (all integers in a double)."""
    divmaxes = [d for d in DIVMAXES if not (shape == 5 and d < 6)]
    rows = [dict(a=0.0, b=1.0, id0=0, divmax=d) for d in divmaxes]
    c = _cases(rows)
    stride = dc.dc_index_out_stride()
    out = numpy.full((len(rows), stride), numpy.nan)
    call(dc, "dc_index", shape, ptr(c), len(rows), ptr(out))
    for d, o in zip(divmaxes, out):
        assert o[3 * 34] == d and o[3 * 34 + 1] == 0.0
        sums = numpy.zeros((3, 32))                  # the running node sums after level m
        run = numpy.array([0.5 * (0 + 1), 0.0, 0.5 * (1 + 1)])
        for m in range(32):
            if 1 <= m <= d:
                n = 2 ** (m - 1)
                run = run + numpy.array([n * (n - 1) / 2.0, m * float(n), float(n)])
            sums[:, m] = run
        for q in range(3):
            T = o[34 * q:34 * q + 32]
            want = numpy.where(numpy.arange(32) <= d, sums[q] / 2.0 ** numpy.arange(32), 0.0)
            assert numpy.array_equal(T, want), (shape, d, q, T, want)
            assert o[34 * q + 32] == sums[q, d], (shape, d, q)


@gpu
@pytest.mark.parametrize("nw", [1, 4])
def test_gauss_panels(dc, nw):
    """16-node Gauss-Legendre panels: exact on polynomials of degree <= 31 and on exp, to
    8 eps sum |w f| against mpmath."""
    xw = numpy.empty(32)
    dc.dc_gl16(ptr(xw))
    cases = [(11, 0.0, 1.0, 1), (11, 0.0, 1.0, 5), (12, 0.0, 1.0, 1), (12, -1.0, 1.0, 1),
             (12, 0.25, 1.5, 3), (13, 0.0, 2.0, 1), (13, 0.0, 2.0, 8), (13, 0.5, 3.0, 17),
             (1, 0.0, 1.0, 1), (1, 0.0, 1.0, 3), (1, 0.0, 1.0, 8), (1, -2.0, 3.0, 8)]
    rows = [dict(a=a, b=b, id0=ident, divmax=npanel) for (ident, a, b, npanel) in cases]
    c = _cases(rows)
    out = numpy.full(len(rows), numpy.nan)
    call(dc, "dc_gauss", nw, ptr(c), len(rows), ptr(out))
    worst = 0.0
    for (ident, a, b, npanel), got in zip(cases, out):
        w = (b - a) / npanel
        mid = a + w * (numpy.arange(npanel)[:, None] + 0.5)
        x = mid + 0.5 * w * xw[None, :16]
        scale = 0.5 * w * numpy.sum(numpy.abs(xw[None, 16:] * f_np(ident, x)))
        err = abs(got - float(exact_integral(ident, a, b)))
        worst = max(worst, err / (EPS * scale))
        print("gauss_panels<%d>: integrand %d on [%g, %g], %d panels: error %.3f eps sum|w f|"
              % (nw, ident, a, b, npanel, err / (EPS * scale)))
    assert worst <= 8.0
