"""The projection and covariance layers of chomp_proj_kernels.h / chomp_cov_kernels.h AS COMPILED
FOR THE DEVICE (tests/devcheck/devproj.hip, the product's compiler flags and launch shapes),
piece by piece against long-double restatements: the moment route of w(theta) (segment
arithmetic, prefix-moment records, segment totals, the level sums k_wtheta_fast recombines from
them, the exact knot and range rules, the epoch forms), the bicubic tables (SscSpline, SscRow,
NgSpline) and HaloFit's quintic derivatives (quintic_derivs_wave, quintic_derivs_inv).  The
w(theta) work buffer is filled with NaN bytes before the moment kernel runs: a value the fast
kernel uses but the moment kernel never wrote poisons the result.

Every tolerance is one of three kinds, named beside it: [project] a bound the suite already
asserts for the same routine; [derived] a rounding bound written out where it is used;
[measured] sized IN THE TEST from the error of an fp64 reference solver (SciPy / FITPACK) against
the same high-precision restatement, never from the device.  Each test prints what it measured
before it asserts."""
import ctypes

import numpy
import pytest
from scipy.interpolate import InterpolatedUnivariateSpline, RectBivariateSpline

import devcheck_build as dcb
import hostcheck_build
from devcheck_build import call, ptr

pytestmark = pytest.mark.gpu

LD = numpy.longdouble
EPS = 2.0 ** -52
ITEMS, PARTS, TILE = 8, 8, 256 * 8          # kWthItems, kWthParts, a tile of k_wtheta_moments
LT = 17
LN_A, LN_B = numpy.log(1e-3), numpy.log(1e2)
NAN_BITS = numpy.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def dj():
    L = dcb.load("devproj")
    assert L.dj_wth_items() == ITEMS and L.dj_wth_parts() == PARTS
    return L


def _d(x):
    return ctypes.c_double(float(x))


# -------------------------------------------------------------------------------------------
# the index arithmetic of the moment route, restated with Python integers
# -------------------------------------------------------------------------------------------
def seg_start(m, lev, nseg):
    """WthSeg::start: the first node of segment m, ceil((m 2^lev - nseg) / (2 nseg)), >= 0."""
    p = (m << lev) - nseg
    return 0 if p <= 0 else -((-p) // (2 * nseg))


def seg_starts(lev, nseg):
    return numpy.array([seg_start(m, lev, nseg) for m in range(nseg + 1)], dtype=numpy.int64)


def seg_of(j, lev, nseg):
    """wth_seg_of"""
    return ((2 * j + 1) * nseg) >> lev


def part_count(length):
    return min(PARTS, -(-length // TILE))


def part_bounds(j0, j1):
    """[p0, p1) of every part of a segment, as wth_moments_body cuts it."""
    length = j1 - j0
    parts = part_count(length)
    if parts == 0:
        return []
    plen = -(-length // parts)
    return [(j0 + plen * p, min(j0 + plen * (p + 1), j1)) for p in range(parts)
            if j0 + plen * p < j1]


def sizes(L, lt, nseg, E):
    out = numpy.zeros(4)
    call(L, "dj_wth_sizes", lt, nseg, E, ptr(out))
    return [int(v) for v in out]


def level_nodes(nodes, lev):
    n = 1 << (lev - 1)
    return nodes[1 + n:1 + 2 * n]


def exact_abscissa(a, b, lev):
    """x_j = a + (b - a)(j + 1/2) / n of the level, in long double from the doubles a, b."""
    n = 1 << (lev - 1)
    j = numpy.arange(n, dtype=LD)
    return LD(a) + (LD(b) - LD(a)) * (j + LD(0.5)) / LD(n)


# -------------------------------------------------------------------------------------------
# a. segment arithmetic and prefix moments
# -------------------------------------------------------------------------------------------
# (5 is the one count with segments of seven parts; 31 and 33 put a segment just above and
# just below a tile)
NSEGS = (1, 2, 3, 5, 7, 19, 31, 33, 50, 64)
MOMENT_SHAPES = [(ns, LN_A, LN_B) for ns in NSEGS] + [(3, -8.0, 8.0), (64, -8.0, 8.0)]


def _moment_reference(nodes, a, b, nseg):
    """Per level: (starts, pre[q][j]: the long-double sum of g u^q over the nodes from the start
    of j's segment through j, u about the exact origin a + m (b - a) / nseg, the same of
    |g| |u|^q).  The sums restart at every segment, as the device's do."""
    ref = {}
    for lev in range(1, LT + 1):
        n = 1 << (lev - 1)
        st = seg_starts(lev, nseg)
        m_of = numpy.repeat(numpy.arange(nseg), numpy.diff(st))
        origin = LD(a) + LD(m_of) * (LD(b) - LD(a)) / LD(nseg)
        u = exact_abscissa(a, b, lev) - origin
        g = level_nodes(nodes, lev).astype(LD)
        pre = numpy.zeros((4, n), dtype=LD)
        prea = numpy.zeros((4, n), dtype=LD)
        for q in range(4):
            t, ta = g * u ** q, numpy.abs(g) * numpy.abs(u) ** q
            for m in range(nseg):
                pre[q, st[m]:st[m + 1]] = numpy.cumsum(t[st[m]:st[m + 1]])
                prea[q, st[m]:st[m + 1]] = numpy.cumsum(ta[st[m]:st[m + 1]])
        ref[lev] = (st, pre, prea)
    return ref


def _moment_bound(prea, count, a, b):
    """[derived] for the moments q = 0..3 of a prefix of c = count nodes, prea its sums of
    |g| |u|^q: (c + 8) 2^-52 sum |g| |u|^q (any order of summation plus forming each term)
    + q d sum |g| |u|^(q - 1), d = 4 2^-53 max(|a|, |b|) (the rounding of the abscissa and of
    the origin, whether or not lox + h j is contracted).  The second term is the first order of
    |(u + d)^q - u^q| <= sum_k C(q, k) d^k |u|^(q - k); the higher orders are kept, because a
    node can lie exactly on its segment's origin (u = 0: level 2 at nseg = 64), where they are
    all there is."""
    c = numpy.asarray(count).astype(LD)
    d = LD(4 * 2.0 ** -53 * max(abs(a), abs(b)))
    binom = ((1,), (1, 1), (1, 2, 1), (1, 3, 3, 1))
    return numpy.array([(c + 8) * LD(EPS) * prea[q] +
                        sum(binom[q][k] * d ** k * prea[q - k] for k in range(1, q + 1))
                        for q in range(4)])


def _check_moments(L, nodes, nseg, a, b, exact0):
    tot, rec_at, tot_at, _ = sizes(L, LT, nseg, 0)
    work = numpy.zeros(tot)
    call(L, "dj_moments", ptr(nodes), LT, nseg, _d(numpy.exp(a)), _d(numpy.exp(b)), 0, ptr(work))
    assert numpy.log(numpy.exp(a)) == a and numpy.log(numpy.exp(b)) == b
    n_nodes = (1 << LT) + 1
    assert numpy.array_equal(work[:n_nodes], nodes)
    rec = work[rec_at:tot_at].reshape(-1, 4)
    segtot = work[tot_at:tot_at + 4 * (LT + 1) * nseg].reshape(LT + 1, nseg, 4)
    ref = _moment_reference(nodes, a, b, nseg)
    # what was written, and only that: the records 2 .. 2^LT / 8 of the heap, the totals of the
    # non-empty segments of the levels 1..LT; NaN bytes everywhere else
    written = numpy.zeros(rec.shape[0], dtype=bool)
    written[2:(1 << LT) // ITEMS + 1] = True
    assert numpy.array_equal(~numpy.isnan(rec).any(axis=1), written)
    assert numpy.all(rec[~written].view(numpy.uint64) == NAN_BITS)
    assert numpy.all(work[n_nodes:rec_at].view(numpy.uint64) == NAN_BITS)
    assert numpy.all(work[tot_at + segtot.size:].view(numpy.uint64) == NAN_BITS)
    assert numpy.all(segtot[0].view(numpy.uint64) == NAN_BITS)
    worst = numpy.zeros(4)
    n_checked = 0
    for lev in range(1, LT + 1):
        n = 1 << (lev - 1)
        st, pre, prea = ref[lev]
        full = numpy.diff(st) > 0
        assert numpy.array_equal(~numpy.isnan(segtot[lev]).any(axis=1), full), lev
        assert numpy.all(segtot[lev][~full].view(numpy.uint64) == NAN_BITS)
        # the totals of every segment
        lo, hi = st[:-1][full], st[1:][full]
        want = pre[:, hi - 1]
        got = segtot[lev][full].T
        bound = _moment_bound(prea[:, hi - 1], hi - lo, a, b)
        if exact0:
            assert numpy.array_equal(got[0], want[0].astype(float)), ("segtot", lev)
        err = numpy.abs(got.astype(LD) - want)
        assert numpy.all(err <= bound), ("segtot", lev, float(numpy.max(err - bound)))
        worst = numpy.maximum(worst, numpy.max(err / numpy.maximum(bound, LD(1e-300)), axis=1))
        # every record: the prefix from the start of the segment of its node j = 8 k - 1
        if n >= ITEMS:
            j = numpy.arange(ITEMS - 1, n, ITEMS)
            js = st[seg_of(j, lev, nseg)]
            want = pre[:, j]
            got = rec[(n + j + 1) // ITEMS].T
            bound = _moment_bound(prea[:, j], j + 1 - js, a, b)
            if exact0:
                assert numpy.array_equal(got[0], want[0].astype(float)), ("rec", lev)
            err = numpy.abs(got.astype(LD) - want)
            assert numpy.all(err <= bound), ("rec", lev, float(numpy.max(err - bound)))
            worst = numpy.maximum(worst, numpy.max(err / numpy.maximum(bound, LD(1e-300)), axis=1))
        # chosen prefix ends, rebuilt from the records as k_wtheta_fast does: the record at or
        # before the node, plus the nodes behind it (here in long double about the exact origin).
        # Every record and every total was compared above, so this pass launches nothing and
        # adds no coverage of the device: it re-reads records through the index arithmetic of
        # the consumer (which record serves which node), and the fixed stride below may thin
        # one category of ends at a shape without loss.
        ends = set()
        for m in numpy.nonzero(full)[0]:
            j0, j1 = int(st[m]), int(st[m + 1])
            cuts = {j0, j1 - 1}
            for p0, p1 in part_bounds(j0, j1):
                cuts |= {p0 - 1, p0, p1 - 1, p0 + TILE - 1, p0 + TILE}
            for c in cuts:
                for jj in range(c - ITEMS, c + ITEMS + 1):
                    if j0 <= jj < j1 and ((jj + 1) % ITEMS in (0, 1, 7) or jj in cuts):
                        ends.add((int(m), jj))
        ends = sorted(ends)[::max(1, len(ends) // 400)]
        g = level_nodes(nodes, lev).astype(LD)
        x = exact_abscissa(a, b, lev)
        for m, jl in ends:
            js = int(st[m])
            jb = ((jl + 1) // ITEMS) * ITEMS
            from_rec = jb > js
            i0 = jb if from_rec else js
            P = rec[(n + jb) // ITEMS].astype(LD) if from_rec else numpy.zeros(4, dtype=LD)
            assert not numpy.isnan(P).any(), (lev, m, jl)
            u = x[i0:jl + 1] - (LD(a) + LD(m) * (LD(b) - LD(a)) / LD(nseg))
            P = P + numpy.array([numpy.sum(g[i0:jl + 1] * u ** q) for q in range(4)])
            want = pre[:, jl]
            bound = _moment_bound(prea[:, jl], jl + 1 - js, a, b)
            if exact0:
                assert float(P[0]) == float(want[0]), ("prefix", lev, m, jl)
            assert numpy.all(numpy.abs(P - want) <= bound), ("prefix", lev, m, jl)
            n_checked += 1
    return worst, n_checked


@pytest.mark.parametrize("nseg,a,b", MOMENT_SHAPES)
def test_prefix_moments(dj, nseg, a, b):
    """k_wtheta_moments at LT = 17: every segment total, every record and a few hundred prefix
    ends per shape (segment first and last nodes, nodes j with (j + 1) % 8 in {0, 1, 7}, part
    and tile boundaries) against long-double sums about the exact origin a + m (b - a) / nseg.
    Integer node values: the zeroth moment bit-exact (any order of summation is exact).  Generic
    values: moments 0..3 within the [derived] bound of _moment_bound.  The record heap and the
    totals hold NaN bytes wherever nothing is to be written."""
    rng = numpy.random.default_rng(1000 * nseg + int(b))
    n_nodes = (1 << LT) + 1
    ints = rng.integers(-8, 9, n_nodes).astype(float)
    w_i, n_i = _check_moments(dj, ints, nseg, a, b, True)
    gen = rng.choice([-1.0, 1.0], n_nodes) * 10.0 ** rng.uniform(-1.5, 1.5, n_nodes)
    w_g, n_g = _check_moments(dj, gen, nseg, a, b, False)
    print("nseg %d [%g, %g]: worst error / bound, q = 0..3: integer %s generic %s; %d + %d "
          "prefix ends" % (nseg, a, b, numpy.round(w_i, 3), numpy.round(w_g, 3), n_i, n_g))


# -------------------------------------------------------------------------------------------
# b. level sums of k_wtheta_fast
# -------------------------------------------------------------------------------------------
def kernel_rule(pp, nkt, lo, hi, x):
    """KernelView: K(lo) below the range, the piece polynomial on [lo, hi] (hi inside), 0 above.
    pp: [NKT - 1][4] coefficients in rising powers of x - X_i; x: long double."""
    x = numpy.asarray(x, dtype=LD)
    dx = (LD(hi) - LD(lo)) / LD(nkt - 1)
    i = numpy.clip(numpy.floor((x - LD(lo)) / dx).astype(numpy.int64), 0, nkt - 2)
    d = x - (LD(lo) + dx * i.astype(LD))
    c = pp.astype(LD)[i]
    v = ((c[..., 3] * d + c[..., 2]) * d + c[..., 1]) * d + c[..., 0]
    return numpy.where(x < LD(lo), LD(pp[0, 0]), numpy.where(x <= LD(hi), v, LD(0)))


def romberg_rows_value(rng_, end, sums):
    """oracle/romberg.py's rows on level sums, in long double: R[L][L] after the levels given."""
    ordsum = LD(end)
    last = [LD(rng_) * ordsum]
    n = 1
    for i, s in enumerate(sums, 1):
        n *= 2
        ordsum = ordsum + LD(s)
        row = [LD(rng_) * ordsum / LD(n)]
        for k in range(i):
            t = LD(4) ** (k + 1)
            row.append((t * row[k] - last[k]) / (t - LD(1)))
        last = row
    return last[-1]


def _unit_weights(rng_, lt):
    """d value / d S_l, l = 1..lt, of the rows after lt levels (the value is linear in the sums)."""
    return [romberg_rows_value(rng_, 0.0, [1.0 if l == k else 0.0 for l in range(lt)])
            for k in range(lt)]


def _run_wtheta(L, nodes, lt, nseg, a, b, pp, lo, hi, theta, runs, E=0, want_work=False):
    nkt = pp.shape[0] + 1
    theta = numpy.ascontiguousarray(theta, dtype=float)
    n_out = theta.size * (E if E else len(runs))
    out = numpy.zeros(n_out)
    logs = numpy.zeros(2 + theta.size)
    lt_run = (ctypes.c_int * len(runs))(*runs)
    work = numpy.zeros(sizes(L, lt, nseg, E)[0]) if want_work else None
    call(L, "dj_wtheta", ptr(nodes), lt, nseg, _d(numpy.exp(a)), _d(numpy.exp(b)), E, nkt,
         ptr(numpy.ascontiguousarray(pp).ravel()), _d(lo), _d(hi), ptr(theta), theta.size, lt_run,
         len(runs), _d(0.0), _d(0.0), ptr(out), ptr(logs), ptr(work) if want_work else None)
    return out.reshape(-1, theta.size), logs, work


K_LO, K_HI = -6.0, 4.0
# ln theta: the kernel's range (i) strictly inside [a + s, b + s], (ii) overhanging below,
# (iii) above, (iv) missing the integration range on either side, (v) generic shifts of the
# pieces against the segments (whole segments inside one piece, pieces over two segments)
SHIFTS = (0.3, 2.5, -2.5, 12.0, -12.0, 0.123456, -0.777, 1.0 / 3.0)
_level_ref_cache = {}


def _level_reference(nkt):
    """The node table, the kernel pieces and, per level and theta, the long-double level sum
    sum_j g_j K(x_j + ln theta), sum_j |g_j| -- computed once per NKT."""
    if nkt in _level_ref_cache:
        return _level_ref_cache[nkt]
    rng = numpy.random.default_rng(100 + nkt)
    n_nodes = (1 << LT) + 1
    nodes = rng.choice([-1.0, 1.0], n_nodes) * 10.0 ** rng.uniform(-1.0, 1.0, n_nodes)
    dxk = (K_HI - K_LO) / (nkt - 1)
    # a random piecewise cubic (no continuity: it need not be a spline), every term O(1)
    pp = rng.uniform(-1.0, 1.0, (nkt - 1, 4)) / dxk ** numpy.arange(4)
    A = float(numpy.max(numpy.sum(numpy.abs(pp) * (3.0 * dxk) ** numpy.arange(4), axis=1)))
    theta = numpy.exp(numpy.array(SHIFTS))
    s = numpy.log(theta).astype(LD)
    S = numpy.zeros((LT + 1, theta.size), dtype=LD)
    G = numpy.zeros(LT + 1, dtype=LD)
    ends = 0.5 * (LD(nodes[0]) * kernel_rule(pp, nkt, K_LO, K_HI, LD(LN_A) + s) +
                  LD(nodes[1]) * kernel_rule(pp, nkt, K_LO, K_HI, LD(LN_B) + s))
    for lev in range(1, LT + 1):
        x = exact_abscissa(LN_A, LN_B, lev)
        g = level_nodes(nodes, lev).astype(LD)
        for t in range(theta.size):
            S[lev, t] = numpy.sum(g * kernel_rule(pp, nkt, K_LO, K_HI, x + s[t]))
        G[lev] = numpy.sum(numpy.abs(g))
    _level_ref_cache[nkt] = (nodes, pp, A, theta, ends, S, G)
    return _level_ref_cache[nkt]


@pytest.mark.parametrize("nkt", (4, 33, 50, 63))
def test_level_sums(dj, nkt):
    """k_wtheta_fast with global_precision = corr_precision = 0 (no level stops early), run with
    LT' = 1..17 on the tables of one k_wtheta_moments launch at LT = 17, so that every level is
    once the deepest of its call, at the product's nseg = floor((b - a) / dxK), one less and half
    of it (NKT = 4: 3, 2, 1).
    Reference: the rows of oracle/romberg.py on the long-double level sums
    sum_j g_j K(x_j + ln theta).
    [derived] a level sum may be off by (n_lev + 64) 2^-52 sum_j |g_j| A, A the largest over the
    pieces of sum_p |c_p| (3 dxK)^p (the recombination shifts by at most two piece widths); the
    end points by 64 2^-52 (|g_0| + |g_1|) A / 2.  The value is linear in the level sums, so
    its bound is sum_l |d value / d S_l| bound_l, plus 64 2^-52 of the largest |T_i| for the
    rows' own arithmetic.  One misplaced node is |g| |K|: 2^20 times the bound at the deepest
    level, more at the others.
    That A is asserted at every nseg.  Where a segment is wider than two pieces (half the
    product's nseg; NKT = 4, nseg = 1) the recombination's shift can exceed what (3 dxK)^p
    allows for (a moment about a far origin: |u| < seg_w and a shift |dl| <= seg_w), and the
    route is by design worse conditioned; at the widths tested here, up to 3.45 pieces a
    segment, the device stays within the same bound, so no wider one is taken.
    [derived] the device's logs of the range and of theta are the test's to 2 ulp (each log is
    good to one)."""
    nodes, pp, A, theta, ends, S, G = _level_reference(nkt)
    rng_ = LN_B - LN_A
    dxk = (K_HI - K_LO) / (nkt - 1)
    product_nseg = int(numpy.floor(rng_ / dxk))
    assert product_nseg * dxk <= rng_
    runs = list(range(1, LT + 1))
    for nseg in sorted({product_nseg, max(1, product_nseg // 2), max(1, product_nseg - 1)}):
        seg_w = rng_ / nseg
        lev_bound = numpy.array([LD(0)] + [((1 << (l - 1)) + 64) * LD(EPS) * G[l] * A
                                           for l in range(1, LT + 1)])
        end_bound = 64 * LD(EPS) * (abs(nodes[0]) + abs(nodes[1])) * A / 2
        out, logs, _ = _run_wtheta(dj, nodes, LT, nseg, LN_A, LN_B, pp, K_LO, K_HI, theta, runs)
        assert not numpy.isnan(out).any(), "an unwritten record or total reached the result"
        # the device's log is the test's (the range and the shifts of the reference)
        assert abs(logs[0] - LN_A) <= 2 * EPS * abs(LN_A) and abs(logs[1] - LN_B) <= 2 * EPS * LN_B
        assert numpy.all(numpy.abs(logs[2:] - numpy.log(theta)) <= 2 * EPS * numpy.abs(logs[2:]))
        worst = 0.0
        for r, lt in enumerate(runs):
            w = _unit_weights(rng_, lt)
            tmax = max(LD(rng_) * (abs(nodes[0]) + abs(nodes[1]) + numpy.sum(G[1:i + 1])) * A /
                       LD(2 ** i) for i in range(lt + 1))
            bound = (sum(abs(w[l - 1]) * lev_bound[l] for l in range(1, lt + 1)) +
                     abs(romberg_rows_value(rng_, 1.0, [0.0] * lt)) * end_bound +
                     64 * LD(EPS) * tmax)
            for t in range(theta.size):
                want = romberg_rows_value(rng_, ends[t], S[1:lt + 1, t])
                err = abs(LD(out[r, t]) - want)
                worst = max(worst, float(err / bound))
                assert err <= bound, (nseg, lt, SHIFTS[t], float(out[r, t]), float(want),
                                      float(err / bound))
        print("NKT %d nseg %d (%.2f pieces a segment): worst error / bound over %d levels x %d "
              "theta: %.3g" % (nkt, nseg, seg_w / dxk, LT, theta.size, worst))


# -------------------------------------------------------------------------------------------
# c. exact knot and range semantics
# -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkt,lo,hi", ((5, -4.0, 4.0), (9, -4.0, 4.0), (5, -6.0, 2.0),
                                       (9, -2.0, 6.0), (3, -8.0, 8.0)))
def test_knot_and_range_rules_exact(dj, nkt, lo, hi):
    """theta = 1 (ln theta = 0 exactly), [a, b] = [-8, 8], dyadic knots, a piecewise CONSTANT
    kernel with distinct non-zero integer values and non-zero integer node values: every level
    sum is an integer, exact in fp64 in any order.  At the levels 1..4 nodes fall exactly on
    knots, on lo and on hi.  Pins: a node on a knot belongs to the piece that starts there; a
    node on hi is inside; a node below lo takes K(lo); a node above hi takes 0.  The level sum is
    recovered from the value of the call in which the level is the deepest (the value is linear
    in it, with weight w) as reference + (value - reference) / w.  Only c_0 of the pieces is
    non-zero, so the device's level sum is itself an integer, and two integers less than 1e-6
    apart are equal: |(value - reference) / w| < 1e-6 IS the equality of the level sums, seen
    through the rows' arithmetic [derived: the sums are integers below 2^12 and the rows are good
    to 1e-13 of them; one misplaced node moves a sum by an integer >= 1].  k_kernel_eval at the
    same abscissae: exactly the rule's integers."""
    lt = 6
    a, b = -8.0, 8.0
    rng = numpy.random.default_rng(nkt * 10 + int(hi))
    n_nodes = (1 << lt) + 1
    nodes = rng.choice([-1.0, 1.0], n_nodes) * rng.integers(1, 9, n_nodes)
    pp = numpy.zeros((nkt - 1, 4))
    pp[:, 0] = (numpy.arange(nkt - 1) + 2.0) * numpy.where(numpy.arange(nkt - 1) % 2, -1.0, 1.0)
    dxk = (hi - lo) / (nkt - 1)

    def K(x):
        out = numpy.zeros(x.size)
        for i, xv in enumerate(x):
            if xv < lo:
                out[i] = pp[0, 0]
            elif xv <= hi:
                out[i] = pp[min(int((xv - lo) // dxk), nkt - 2), 0]
        return out

    xs, S = [numpy.array([a, b])], []
    for lev in range(1, lt + 1):
        n = 1 << (lev - 1)
        x = a + (b - a) * (numpy.arange(n) + 0.5) / n           # exact: dyadic
        xs.append(x)
        S.append(float(numpy.sum(level_nodes(nodes, lev) * K(x))))
    on_knot = sum(int(numpy.sum((x >= lo) & (x <= hi) & ((x - lo) % dxk == 0))) for x in xs[1:5])
    assert on_knot >= 1
    end = 0.5 * (nodes[0] * K(xs[0][:1])[0] + nodes[1] * K(xs[0][1:])[0])
    xe = numpy.concatenate(xs + [numpy.array([lo, hi, numpy.nextafter(lo, -9.0),
                                              numpy.nextafter(hi, 9.0)])])
    got = numpy.zeros(xe.size)
    call(dj, "dj_kernel_eval", nkt, ptr(pp.ravel()), _d(lo), _d(hi), ptr(xe), xe.size, ptr(got))
    assert numpy.array_equal(got, K(xe))
    theta = numpy.array([1.0])
    runs = list(range(1, lt + 1))
    product_nseg = int((b - a) // dxk)
    # (a segment is never narrower than a piece: nseg <= (b - a) / dxK)
    for nseg in sorted(ns for ns in {product_nseg, 1, 3, max(1, product_nseg // 2)}
                       if ns <= product_nseg):
        out, logs, _ = _run_wtheta(dj, nodes, lt, nseg, a, b, pp, lo, hi, theta, runs)
        assert logs[0] == a and logs[1] == b and logs[2] == 0.0
        for r, lev in enumerate(runs):
            want = romberg_rows_value(b - a, end, S[:lev])
            w = _unit_weights(b - a, lev)[lev - 1]
            off = float((LD(out[r, 0]) - want) / w)
            print("NKT %d [%g, %g] nseg %d level %d: sum %g, implied error %.3g"
                  % (nkt, lo, hi, nseg, lev, S[lev - 1], off))
            assert abs(off) < 1e-6, (nseg, lev, off)


# -------------------------------------------------------------------------------------------
# d. epoch forms
# -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lt", (3, 17))
def test_epoch_forms_are_the_single_epoch_launch(dj, lt):
    """k_wtheta_moments_epochs / k_wtheta_fast_epochs on three node tables at wth_epoch_stride
    (LT = 3: 9 nodes, odd padding, a record heap of 3 entries none of which is written; LT = 17):
    every epoch's values, records and totals are bit for bit those of the single-epoch launch on
    its table, and the NaN fill stays in place between and behind the epochs."""
    nkt, E = 50, 3
    rng = numpy.random.default_rng(lt)
    n_nodes = (1 << lt) + 1
    nodes = rng.choice([-1.0, 1.0], (E, n_nodes)) * 10.0 ** rng.uniform(-1.0, 1.0, (E, n_nodes))
    dxk = (K_HI - K_LO) / (nkt - 1)
    pp = rng.uniform(-1.0, 1.0, (nkt - 1, 4)) / dxk ** numpy.arange(4)
    nseg = int(numpy.floor((LN_B - LN_A) / dxk))
    theta = numpy.exp(numpy.array(SHIFTS[:4]))
    tot1, rec_at, tot_at, _ = sizes(dj, lt, nseg, 0)
    totE, rec_atE, tot_atE, stride = sizes(dj, lt, nseg, E)
    assert (rec_at, tot_at) == (rec_atE, tot_atE) and stride % 2 == 0 and totE == E * stride
    used = tot_at + 4 * (lt + 1) * nseg
    assert used <= tot1 <= stride
    outE, _, workE = _run_wtheta(dj, nodes.ravel(), lt, nseg, LN_A, LN_B, pp, K_LO, K_HI, theta,
                                 [lt], E=E, want_work=True)
    assert not numpy.isnan(outE).any()
    for e in range(E):
        out1, _, work1 = _run_wtheta(dj, nodes[e], lt, nseg, LN_A, LN_B, pp, K_LO, K_HI, theta,
                                     [lt], want_work=True)
        assert numpy.array_equal(out1[0].view(numpy.uint64), outE[e].view(numpy.uint64)), e
        chunk = workE[e * stride:(e + 1) * stride]
        assert numpy.array_equal(chunk[:used].view(numpy.uint64), work1[:used].view(numpy.uint64))
        assert numpy.all(chunk[used:].view(numpy.uint64) == NAN_BITS), e
        assert numpy.all(chunk[n_nodes:rec_at].view(numpy.uint64) == NAN_BITS), e
    assert not numpy.array_equal(outE[0], outE[1])


# -------------------------------------------------------------------------------------------
# e. bicubic
# -------------------------------------------------------------------------------------------
def nak_pp(x, y):
    """The not-a-knot cubic spline through (x, y[:, k]) for every column k in long double: the
    slope system of chomp_math.h's spline_build restated (rows 0 and n - 1 the not-a-knot
    conditions) and solved by elimination; pp[i, p, k] in rising powers of x - x_i."""
    x = numpy.asarray(x, dtype=LD)
    y = numpy.asarray(y, dtype=LD)
    n = x.size
    h = numpy.diff(x)
    d = numpy.diff(y, axis=0) / h[:, None]
    sub, dia, sup = (numpy.zeros(n, dtype=LD) for _ in range(3))
    r = numpy.zeros_like(y)
    dia[0], sup[0] = h[1], h[0] + h[1]
    r[0] = ((3 * h[0] + 2 * h[1]) * h[1] * d[0] + h[0] * h[0] * d[1]) / (h[0] + h[1])
    for i in range(1, n - 1):
        sub[i], dia[i], sup[i] = h[i], 2 * (h[i - 1] + h[i]), h[i - 1]
        r[i] = 3 * (h[i] * d[i - 1] + h[i - 1] * d[i])
    sub[-1], dia[-1] = h[-1] + h[-2], h[-2]
    r[-1] = (h[-1] ** 2 * d[-2] + (2 * h[-2] + 3 * h[-1]) * h[-2] * d[-1]) / (h[-2] + h[-1])
    for i in range(1, n):
        m = sub[i] / dia[i - 1]
        dia[i] = dia[i] - m * sup[i - 1]
        r[i] = r[i] - m * r[i - 1]
    s = numpy.zeros_like(y)
    s[-1] = r[-1] / dia[-1]
    for i in range(n - 2, -1, -1):
        s[i] = (r[i] - sup[i] * s[i + 1]) / dia[i]
    pp = numpy.zeros((n - 1, 4) + y.shape[1:], dtype=LD)
    pp[:, 0] = y[:-1]
    pp[:, 1] = s[:-1]
    pp[:, 2] = (3 * d - 2 * s[:-1] - s[1:]) / h[:, None]
    pp[:, 3] = (s[:-1] + s[1:] - 2 * d) / (h ** 2)[:, None]
    return pp


def bicubic_ref(x, tab):
    """Two passes: along b for every row, then along a for every (interval, power) of the row
    pieces.  bic[ia, jb, p, q] of sum_pq bic (a - x_ia)^p (b - x_jb)^q, tab[i, j] at (x_i, x_j)."""
    n = x.size
    rows = nak_pp(x, numpy.asarray(tab, dtype=LD).T)            # [jb, q, i]
    cols = nak_pp(x, rows.reshape(-1, n).T)                     # [ia, p, (jb, q)]
    return cols.reshape(n - 1, 4, n - 1, 4).transpose(0, 2, 1, 3)


def cell_of(x, v):
    """The piece a point belongs to: a knot starts its piece, hi is inside the last one."""
    return numpy.clip(numpy.searchsorted(x, v, side="right") - 1, 0, x.size - 2)


def bicubic_eval(x, bic, a, b, magnitude=False):
    """sum_pq bic[ia, jb, p, q] da^p db^q in the points' cells; magnitude: of |bic|, |da|, |db|."""
    ia, jb = cell_of(x, a), cell_of(x, b)
    da = (numpy.asarray(a, dtype=LD) - x[ia].astype(LD))[:, None]
    db = (numpy.asarray(b, dtype=LD) - x[jb].astype(LD))[:, None]
    c = bic[ia, jb]
    if magnitude:
        c, da, db = numpy.abs(c), numpy.abs(da), numpy.abs(db)
    pw = numpy.arange(4)
    return numpy.einsum("npq,np,nq->n", c, da ** pw, db ** pw)


def ssc_rule(x, bic, a, b):
    """SscSpline: clamp at and below lo, exactly 0 for either argument above hi or NaN."""
    lo, hi = x[0], x[-1]
    a = numpy.asarray(a, dtype=float)
    b = numpy.asarray(b, dtype=float)
    zero = ~((a <= hi) & (b <= hi))
    ac = numpy.where(zero, lo, numpy.maximum(a, lo))
    bc = numpy.where(zero, lo, numpy.maximum(b, lo))
    return numpy.where(zero, LD(0), bicubic_eval(x, bic, ac, bc)), zero


def _knots(n, kind):
    x = numpy.linspace(numpy.log(1e-3), numpy.log(1e2), n)
    if kind == "perturbed":
        # interval() corrects a uniform guess by one: below half a spacing
        rng = numpy.random.default_rng(n)
        x[1:-1] += rng.uniform(-0.3, 0.3, n - 2) * (x[1] - x[0])
    return x


def _points(x):
    """All knot pairs, one ulp either side of the knots in each argument, cell centres, points
    between a knot and its uniform place, lo and hi exactly, below lo, above hi and NaN; as 1-D
    lists for a cross product."""
    centres = 0.5 * (x[1:] + x[:-1])
    if centres.size > 40:                   # N = 50: every fifth cell's centre
        centres = centres[::5]
    inner = numpy.concatenate([x, numpy.nextafter(x, -1e9)[1:], numpy.nextafter(x, 1e9)[:-1],
                               centres])
    outer = numpy.array([x[0] - 1.0, numpy.nextafter(x[0], -1e9), numpy.nextafter(x[-1], 1e9),
                         x[-1] + 1.0, numpy.nan])
    # half-way between every knot and its place on the uniform grid: where interval()'s uniform
    # guess is one off and must be corrected (a spline is continuous, so an ulp from a knot the
    # neighbouring cell's polynomial would do as well)
    uni = numpy.linspace(x[0], x[-1], x.size)
    gap = 0.5 * (x + uni)[numpy.abs(x - uni) > 0]
    return numpy.concatenate([inner, gap, outer])


def _tables(x, rng):
    n = x.size
    X, Y = numpy.meshgrid(x, x, indexing="ij")
    c = rng.integers(-3, 4, (4, 4)).astype(float)
    c[3, 2] += 5.0                                               # (not symmetric)
    u, v = (X - x[0]) / (x[-1] - x[0]), (Y - x[0]) / (x[-1] - x[0])
    poly = sum(c[p, q] * u ** p * v ** q for p in range(4) for q in range(4))
    smooth = numpy.sin(0.7 * X + 0.2) * numpy.exp(0.1 * Y) + 0.3 * X * Y / 10.0 + 2.0
    rough = rng.choice([-1.0, 1.0], (n, n)) * 10.0 ** rng.uniform(-1.0, 1.0, (n, n))
    return {"poly": (poly, c), "smooth": (smooth, None), "rough": (rough, None)}


def _poly_exact(x, c, a, b):
    u = (numpy.asarray(a, dtype=LD) - LD(x[0])) / (LD(x[-1]) - LD(x[0]))
    v = (numpy.asarray(b, dtype=LD) - LD(x[0])) / (LD(x[-1]) - LD(x[0]))
    return sum(LD(c[p, q]) * u ** p * v ** q for p in range(4) for q in range(4))


def _run_ssc(L, x, tab, pa, pb, ra, rb):
    n = x.size
    bic = numpy.zeros(16 * (n - 1) ** 2)
    ev = numpy.zeros(pa.size)
    row = numpy.zeros(ra.size * rb.size)
    call(L, "dj_ssc", n, ptr(x), ptr(numpy.ascontiguousarray(tab).ravel()), _d(x[0]), _d(x[-1]),
         ptr(pa), ptr(pb), pa.size, ptr(ra), ra.size, ptr(rb), rb.size, ptr(bic), ptr(ev),
         ptr(row))
    return bic.reshape(n - 1, n - 1, 4, 4), ev, row.reshape(ra.size, rb.size)


@pytest.mark.parametrize("kind", ("linspace", "perturbed"))
@pytest.mark.parametrize("n", (4, 5, 8, 50))
def test_bicubic(dj, n, kind):
    """k_ssc_bicubic / k_ssc_eval / SscRow at N = 4 (the smallest spline_build accepts), 5, 8, 50
    on the product's linspace knots and on slightly non-uniform ones, for samples of a bicubic
    polynomial with small integer coefficients (reference: the polynomial itself), a smooth and
    a rough random table (reference: two passes of long-double not-a-knot solves, cross-checked
    against RectBivariateSpline(kx = ky = 3, s = 0)).
    [project] 2e-13 (1 + |ref|) is the bar of test_notaknot_spline for one pass; two passes:
    4e-13 (scale + |ref|), scale = max |table|.  [measured] on the rough tables the bar is the
    larger of that and 4 x the error of fp64 FITPACK against the same long-double reference on
    the same input (the device runs the same algorithm in the same precision); both are printed
    (FITPACK: at most 7.9e-16 on these shapes, so the bar is 4e-13 everywhere; the MI355X: at
    most 8.2e-15, the rough table at N = 50 on perturbed knots; row against spline at most
    1.4 2^-52 mag).
    The cross-check of the restatement against FITPACK is held to 1e-12 (1e-9 on the rough
    tables) [project: five times test_notaknot_spline's bar; FITPACK is measured far inside it].
    [derived] SscRow against SscSpline: both are two nested cubic Horner passes in fma over the
    same 16 coefficients and the same da, db, summed in the other order: six roundings each, so
    each is within 6 2^-53 of mag = sum_pq |c_pq| |da|^p |db|^q of the exact sum and the two
    within 6 2^-52 mag of each other; 8 2^-52 mag is asserted at every point.
    The coefficients bic[ia][jb][p][q] are checked against the restatement's cell polynomials on
    these non-symmetric tables, each scaled by the cell's widths: a transposition or a wrong
    cell at a knot is an error of the order of the table.  [derived from the [project] bar] 4 x the
    bar of the values: taking the one-pass bar 2e-13 as the budget e of a solved slope times its
    spacing, a scaled coefficient carries at most 3 e per pass (c_1 h = s h, c_2 h^2 = 3 dy -
    (2 s_i + s_{i+1}) h, c_3 h^3 = (s_i + s_{i+1}) h - 2 dy; the data are exact), two passes
    6 e = 1.2e-12 of the table's scale, within 4 x 4e-13."""
    x = _knots(n, kind)
    rng = numpy.random.default_rng(n)
    p = _points(x)
    A, B = numpy.meshgrid(p, p, indexing="ij")
    pa, pb = numpy.ascontiguousarray(A.ravel()), numpy.ascontiguousarray(B.ravel())
    inside = ~(numpy.isnan(pa) | numpy.isnan(pb) | (pa > x[-1]) | (pb > x[-1]))
    hw = numpy.diff(x)
    for name, (tab, c) in _tables(x, rng).items():
        scale = float(numpy.max(numpy.abs(tab)))
        ref_bic = bicubic_ref(x, tab)
        ref, zero = ssc_rule(x, ref_bic, pa, pb)
        assert numpy.array_equal(zero, ~inside)
        sp = RectBivariateSpline(x, x, tab, kx=3, ky=3, s=0)
        ac, bc = numpy.maximum(pa[inside], x[0]), numpy.maximum(pb[inside], x[0])
        scipy_err = float(numpy.max(numpy.abs(sp.ev(ac, bc) - ref[inside]) /
                                    (scale + numpy.abs(ref[inside]))))
        assert scipy_err < 1e-12 if name != "rough" else scipy_err < 1e-9   # (the cross-check)
        bar = 4e-13 if name != "rough" else max(4e-13, 4 * scipy_err)
        if c is not None:
            exact = _poly_exact(x, c, ac, bc)
            # (the samples are the polynomial's to half an ulp: the restatement reproduces it)
            assert float(numpy.max(numpy.abs(ref[inside] - exact) / (scale + abs(exact)))) < 1e-14
            ref[inside] = exact
        bic, ev, row = _run_ssc(dj, x, tab, pa, pb, p, p)
        assert numpy.all(ev[~inside] == 0.0) and not numpy.isnan(ev).any()
        err = float(numpy.max(numpy.abs(ev - ref) / (scale + numpy.abs(ref))))
        # SscRow: the same rules, the same values to rounding
        assert numpy.all(row.ravel()[~inside] == 0.0) and not numpy.isnan(row).any()
        err_row = float(numpy.max(numpy.abs(row.ravel() - ref) / (scale + numpy.abs(ref))))
        mag = numpy.zeros(pa.size, dtype=LD)
        mag[inside] = bicubic_eval(x, ref_bic, ac, bc, magnitude=True)
        row_diff = numpy.abs(row.ravel() - ev)
        rows_vs_spline = float(numpy.max(row_diff[inside] / (LD(EPS) * mag[inside])))
        # the coefficients, each scaled to its contribution over the cell
        w = (hw[:, None, None, None] ** numpy.arange(4)[None, None, :, None] *
             hw[None, :, None, None] ** numpy.arange(4)[None, None, None, :])
        err_bic = float(numpy.max(numpy.abs(bic - ref_bic) * w) / scale)
        print("bicubic N %d %s %s: SscSpline %.3g SscRow %.3g (row vs spline %.3g eps mag) "
              "coefficients %.3g; bar %.3g (FITPACK fp64 against the reference: %.3g)"
              % (n, kind, name, err, err_row, rows_vs_spline, err_bic, bar, scipy_err))
        assert err <= bar and err_row <= bar
        assert numpy.all(row_diff <= 8 * LD(EPS) * mag)
        assert err_bic <= 4 * bar


@pytest.mark.parametrize("n", (4, 8, 50))
def test_ng_spline(dj, n):
    """k_ng_bicubic / k_ng_eval: the min scalar (a NaN entry gives NaN, and with it every
    value inside the range; so does a positive minimum, whose log(table - 10 min) is NaN at the
    minimum), the bicubic of log(table - 10 min) and exp(poly) + 10 min with SscSpline's range
    rules for tables with a negative minimum.
    [project] the bicubic of the log table to 4e-13 (scale + |ref|) as test_bicubic; through exp
    that is a relative 4e-13 (scale + |poly|) of exp(poly), plus 4 2^-52 for exp and the sum
    [derived]; the device's own log of the table entries adds 4 2^-52 (scale + |poly|) to the
    bicubic's bar, and 10 min is held to 2 ulp [derived].  The coefficients: 4 x the bar of
    the values as in test_bicubic, with scale + |ref| <= 2 scale [derived from [project]]."""
    x = _knots(n, "linspace")
    rng = numpy.random.default_rng(50 + n)
    p = _points(x)
    A, B = numpy.meshgrid(p, p, indexing="ij")
    pa, pb = numpy.ascontiguousarray(A.ravel()), numpy.ascontiguousarray(B.ravel())
    inside = ~(numpy.isnan(pa) | numpy.isnan(pb) | (pa > x[-1]) | (pb > x[-1]))
    X, Y = numpy.meshgrid(x, x, indexing="ij")
    base = numpy.exp(0.3 * numpy.sin(0.5 * X) + 0.1 * Y) * rng.uniform(0.9, 1.1, (n, n))
    for name, tab in (("positive", base + 0.5), ("negative", base - base.max() - 0.25),
                      ("negative2", 0.01 * base - 7.0), ("nan", base + 0.5)):
        tab = tab.copy()
        if name == "nan":
            tab[n // 2, 1] = numpy.nan
        mn = numpy.zeros(1)
        bic = numpy.zeros(16 * (n - 1) ** 2)
        ev = numpy.zeros(pa.size)
        call(dj, "dj_ng", n, ptr(x), ptr(tab.ravel()), _d(x[0]), _d(x[-1]), ptr(pa), ptr(pb),
             pa.size, ptr(mn), ptr(bic), ptr(ev))
        assert numpy.all(ev[~inside] == 0.0)
        if name == "nan":
            assert numpy.isnan(mn[0]) and numpy.all(numpy.isnan(ev[inside]))
            continue
        assert mn[0] == tab.min() and (mn[0] > 0) == (name == "positive")
        if name == "positive":
            # table - 10 min < 0 at the minimum itself: log gives NaN there and nothing is
            # guarded (kernel.py:1026-1029 does the same), so the whole spline is NaN
            assert numpy.all(numpy.isnan(ev[inside]))
            continue
        off = 10.0 * mn[0]
        ltab = numpy.log(tab.astype(LD) - LD(off))
        ref_bic = bicubic_ref(x, ltab)
        poly, _ = ssc_rule(x, ref_bic, pa, pb)
        want = numpy.exp(poly[inside]) + LD(off)
        lscale = float(numpy.max(numpy.abs(ltab)))
        # (the device's log of the table entries: 2 ulp of |ltab| on the knots' values)
        tol = ((4e-13 + 4 * EPS) * (lscale + numpy.abs(poly[inside])) + 4 * EPS) * \
            numpy.exp(poly[inside]) + 2 * EPS * abs(off)
        err = numpy.abs(ev[inside] - want)
        print("kernel_NG N %d %s minimum: min %.6g, worst error / bound %.3g"
              % (n, name, mn[0], float(numpy.max(err / tol))))
        assert numpy.all(err <= tol)
        w = numpy.diff(x)[0] ** (numpy.arange(4)[:, None] + numpy.arange(4)[None, :])
        err_bic = float(numpy.max(numpy.abs(bic.reshape(n - 1, n - 1, 4, 4) - ref_bic) * w))
        assert err_bic <= 4 * (4e-13 + 4 * EPS) * 2 * lscale


# -------------------------------------------------------------------------------------------
# f. quintic derivatives
# -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hc():
    """tests/hostcheck: the serial quintic_derivs of chomp_math.h, compiled for the host."""
    return hostcheck_build.load()


def _basis(t, m, p, xv):
    """B_{m-p+r,p}(xv), r = 0..p, in knot span m (Cox - de Boor), long double."""
    N = [LD(1)] + [LD(0)] * p
    left, right = [LD(0)] * (p + 1), [LD(0)] * (p + 1)
    for j in range(1, p + 1):
        left[j] = xv - t[m + 1 - j]
        right[j] = t[m + j] - xv
        saved = LD(0)
        for r in range(j):
            temp = N[r] / (right[r + 1] + left[j - r])
            N[r] = saved + right[r + 1] * temp
            saved = left[j - r] * temp
        N[j] = saved
    return N


def _span(t, n, xv):
    m = 5
    while m < n - 1 and xv >= t[m + 1]:
        m += 1
    return m


def quintic_ref(x, y, xq):
    """d1, d2 of the quintic interpolating spline with FITPACK's knots for s = 0 (6-fold end
    knots, the data sites x[3] .. x[n - 4] inside): the collocation system solved in long
    double with partial pivoting, the derivatives from the B-spline derivative formula."""
    n = x.size
    xl = x.astype(LD)
    t = numpy.concatenate([[xl[0]] * 6, xl[3:n - 3], [xl[-1]] * 6])
    M = numpy.zeros((n, n + 1), dtype=LD)
    for i in range(n):
        m = _span(t, n, xl[i])
        M[i, m - 5:m + 1] = _basis(t, m, 5, xl[i])
    M[:, n] = y.astype(LD)
    for col in range(n):
        piv = col + int(numpy.argmax(numpy.abs(M[col:, col])))
        if piv != col:
            M[[col, piv]] = M[[piv, col]]
        M[col] = M[col] / M[col, col]
        f = M[:, col].copy()
        f[col] = 0
        M -= f[:, None] * M[col][None, :]
    c = M[:, n]
    d1, d2 = numpy.zeros(xq.size, dtype=LD), numpy.zeros(xq.size, dtype=LD)
    for k, v in enumerate(xq.astype(LD)):
        m = _span(t, n, v)
        c1 = {j: 5 * (c[j] - c[j - 1]) / (t[j + 5] - t[j]) for j in range(m - 4, m + 1)}
        c2 = {j: 4 * (c1[j] - c1[j - 1]) / (t[j + 4] - t[j]) for j in range(m - 3, m + 1)}
        N4, N3 = _basis(t, m, 4, v), _basis(t, m, 3, v)
        d1[k] = sum(c1[m - 4 + r] * N4[r] for r in range(5))
        d2[k] = sum(c2[m - 3 + r] * N3[r] for r in range(4))
    return d1, d2


@pytest.mark.parametrize("n", (6, 7, 50, 63, 64, 65, 100))
def test_quintic_derivatives(dj, hc, n):
    """quintic_derivs_wave and quintic_derivs_inv (ainv_t from halofit_collocation_inverse_host)
    on HaloFit's grid linspace(ln 0.1, ln 10, n) at n = 6 (the smallest the knot construction
    t[6 + i] = x[3 + i], i < n - 6, allows: no interior knot, the lane-strided knot loop is empty
    and the tail knots follow the head knots at once), n = 7 (one interior knot) and across the
    64 lanes of the set-up loops, for a quintic polynomial (reference: its exact derivatives; the
    spline reproduces it) and the HaloFit-like curve of test_hostmath.test_quintic_derivatives
    (reference: the long-double collocation solve), at 500 points across the range, every knot
    and both ends; and against the serial quintic_derivs of tests/hostcheck.
    [measured] in the test: the error of SciPy's InterpolatedUnivariateSpline(k = 5) derivatives
    against the same reference on the same inputs; the device forms and the serial routine may
    have 4 x that, floor 1e-13 (they solve the same banded system in fp64).  [derived] any two
    of the three forms then differ by at most twice the bar (each is within it of the
    reference).  Every figure is printed; the MI355X's are in DESIGN.md section 3."""
    x = numpy.zeros(n)
    dj.dj_quintic_grid(n, ptr(x))
    assert numpy.allclose(x, numpy.linspace(numpy.log(0.1), numpy.log(10.0), n), rtol=0, atol=1e-15)
    xq = numpy.concatenate([numpy.linspace(x[0], x[-1], 500), x, x[:1], x[-1:]])
    co = numpy.array([0.4, -1.3, -0.21, 0.05, 0.02, -0.01])
    xl = x.astype(LD)
    ql = xq.astype(LD)
    poly_y = sum(LD(co[k]) * xl ** k for k in range(6))
    datasets = {
        "polynomial": poly_y.astype(float),
        "halofit": -1.3 * x - 0.21 * x ** 2 + 0.01 * numpy.sin(2 * x) + 0.4,
    }
    for name, y in datasets.items():
        r1, r2 = quintic_ref(x, y, xq)
        if name == "polynomial":
            # The reference is the polynomial's exact derivatives, for the device, the serial
            # routine and SciPy's bar alike.  The samples are the polynomial's to half an ulp, so
            # the restatement (the spline through the ROUNDED samples) reproduces them only as
            # far as that rounding carries into a derivative (its noise gain grows as 1 / h and
            # 1 / h^2, h ~ 5 / n).  The two asserts below only check the restatement, which the
            # other data set relies on; they bound nothing of the code under test.
            e1 = sum(k * LD(co[k]) * ql ** (k - 1) for k in range(1, 6))
            e2 = sum(k * (k - 1) * LD(co[k]) * ql ** (k - 2) for k in range(2, 6))
            amp = 1e3 if n > 7 else 1e2
            assert float(numpy.max(numpy.abs(r1 - e1))) < amp * n * EPS
            assert float(numpy.max(numpy.abs(r2 - e2))) < amp * n * n * EPS
            r1, r2 = e1, e2
        sp = InterpolatedUnivariateSpline(x, y, k=5)
        sd = numpy.array([sp.derivatives(v)[1:3] for v in xq]).T
        s_err = [float(numpy.max(numpy.abs(sd[0] - r1))), float(numpy.max(numpy.abs(sd[1] - r2)))]
        bar = [max(1e-13, 4 * e) for e in s_err]
        out = numpy.zeros(4 * xq.size)
        call(dj, "dj_quintic", ptr(y), n, ptr(xq), xq.size, ptr(out))
        wave, inv = out[:2 * xq.size].reshape(2, -1), out[2 * xq.size:].reshape(2, -1)
        ser = numpy.zeros((2, xq.size))
        d = numpy.zeros(2)
        hc.hc_quintic.restype = None
        for k, v in enumerate(xq):
            hc.hc_quintic(ptr(x), ptr(y), n, ctypes.c_double(v), ptr(d))
            ser[:, k] = d
        ref = (r1, r2)
        for q in range(2):
            errs = {nm: float(numpy.max(numpy.abs(v[q] - ref[q])))
                    for nm, v in (("wave", wave), ("inv", inv), ("serial", ser))}
            cross = {"wave-inv": float(numpy.max(numpy.abs(wave[q] - inv[q]))),
                     "wave-serial": float(numpy.max(numpy.abs(wave[q] - ser[q]))),
                     "inv-serial": float(numpy.max(numpy.abs(inv[q] - ser[q])))}
            print("quintic n %d %s d%d: SciPy %.3g -> bar %.3g; %s; %s"
                  % (n, name, q + 1, s_err[q], bar[q], errs, cross))
            assert not numpy.isnan(wave[q]).any() and not numpy.isnan(inv[q]).any()
            assert all(e <= bar[q] for e in errs.values()), (errs, bar[q])
            assert all(e <= 2 * bar[q] for e in cross.values()), (cross, bar[q])
