"""The host-side reference tests/test_gpu_devpower.py measures the device against, and the k grids
it runs: no GPU, no harness.  tests/test_devpower_cpu.py checks this module by itself.

The in-range value of every halo-model spectrum is  A shape h_a(ln k) h_b(ln k) + pp(ln k)
(halo.py:277-439; the super-sample codes: halo.py:1136-1169), the three cubic pieces evaluated in
long double (eps 1.1e-19) at ln k taken in long double from the double k.  The knot tables are
deliberately discontinuous: each piece of each family is an independent cubic with non-negative
coefficients (positive and increasing over its interval, condition number 1), values differing by
tens of percent across a knot, so that a lane that reads a neighbouring piece is grossly wrong.
A second family of tables holds C2 splines of smooth functions (SciPy's not-a-knot CubicSpline)."""
import numpy

LD = numpy.longdouble
EPS = 2.0 ** -52
U = 2.0 ** -53
FAST_LOG_REL = 4e-16            # [project] tests/test_gpu_devmath.py::test_fast_log

LIN, MM, GM, GG, SSC_RESPONSE, MM_SSC = range(6)
HALOFIT, EXTRAPOLATE = 16, 32
F_HM, F_PPMM, F_HG, F_PPGM, F_PPGG, F_I12 = range(6)
SSC_BEAT = 68.0 / 21.0
K_MIN, K_MAX = 1e-3, 1e2
GROUP = 128                     # k of one wavefront (two per lane)
BLOCK = 512                     # k of one block of the grid kernels


def families(w):
    """power_families (chomp_power_kernels.h)."""
    if w == GM:
        return F_HG, F_HM, F_PPGM
    if w == GG:
        return F_HG, F_HG, F_PPGG
    if w in (SSC_RESPONSE, MM_SSC):
        return F_HM, F_I12, F_PPMM
    return F_HM, F_HM, F_PPMM


class Knots:
    """The uniform knots x_i = x0 + dx i over [x0, x1] as doubles (x0, x1: the logarithms the
    evaluator takes of k_min, k_max; the device's are handed in by the GPU test)."""

    def __init__(self, NK, x0=None, x1=None):
        self.NK = NK
        self.x0 = float(numpy.log(K_MIN)) if x0 is None else float(x0)
        self.x1 = float(numpy.log(K_MAX)) if x1 is None else float(x1)
        self.dx = (self.x1 - self.x0) / (NK - 1)
        self.x = self.x0 + self.dx * numpy.arange(NK)          # (two roundings; an fma: one)

    def delta(self, lnk, j):
        """How far the evaluator's own ln k - x_j may be from the exact one: [project] fast_log's
        relative bound (the library log is within it), one ulp of x0 + dx j (formed with or
        without an fma), and [derived] the three roundings of the index expression
        floor((ln k - x0) / dx) -- difference, quotient or reciprocal, product -- each U of
        |x_j - x0| at the knot, times two."""
        xj = self.x[j]
        return (FAST_LOG_REL * numpy.abs(numpy.asarray(lnk, dtype=float)) +
                (numpy.nextafter(numpy.abs(xj), numpy.inf) - numpy.abs(xj)) +
                3 * EPS * numpy.abs(xj - self.x0) + U * self.dx)

    def locate(self, k):
        """Per k: ln k (long double), the interval index of the exact ln k (clamped to
        0 .. NK - 2), in_range, and `alt`: the other adjacent interval where the exact ln k lies
        within delta of an interior knot (the knot band), else the same index."""
        k = numpy.asarray(k, dtype=float)
        ok = numpy.isfinite(k) & (k > 0)
        lnk = numpy.log(numpy.where(ok, k, 1.0).astype(LD))
        idx = numpy.clip(numpy.floor((lnk - LD(self.x0)) / LD(self.dx)).astype(int), 0, self.NK - 2)
        # (the division above is in long double; a knot x_i is a double: settle idx against it)
        idx = numpy.where((idx < self.NK - 2) & (lnk >= self.x[numpy.minimum(idx + 1, self.NK - 1)].astype(LD)),
                          idx + 1, idx)
        idx = numpy.where((idx > 0) & (lnk < self.x[idx].astype(LD)), idx - 1, idx)
        in_range = ok & (k >= K_MIN) & (k <= K_MAX)
        alt = idx.copy()
        lo = (idx > 0) & (numpy.abs(lnk - self.x[idx].astype(LD)) <= self.delta(lnk, idx))
        hi = (idx < self.NK - 2) & (numpy.abs(lnk - self.x[idx + 1].astype(LD)) <=
                                    self.delta(lnk, idx + 1))
        alt[lo] = idx[lo] - 1
        alt[hi] = idx[hi] + 1
        return lnk, idx, in_range, alt


# -------------------------------------------------------------------------------------------
# knot tables
# -------------------------------------------------------------------------------------------
SCALE = {F_HM: 1.0, F_PPMM: 40.0, F_HG: 1.6, F_PPGM: 90.0, F_PPGG: 150.0, F_I12: 25.0}


def random_pieces(NK, seed, dx):
    """pp[f][i] = (c0, c1, c2, c3) of family f on interval i: non-negative coefficients, the rise
    over an interval 10 .. 60 %, and c0 at least 20 % off the previous piece's end value."""
    rng = numpy.random.default_rng(seed)
    pp = numpy.empty((6, NK - 1, 4))
    for f in range(6):
        end = None
        for i in range(NK - 1):
            while True:
                c0 = SCALE[f] * rng.uniform(0.5, 2.0)
                if end is None or abs(c0 / end - 1.0) > 0.2:
                    break
            r = rng.uniform(0.2, 1.0, 3)
            c = numpy.array([c0, 0.3 * r[0] * c0 / dx, 0.2 * r[1] * c0 / dx ** 2,
                             0.1 * r[2] * c0 / dx ** 3])
            pp[f, i] = c
            end = c[0] + c[1] * dx + c[2] * dx ** 2 + c[3] * dx ** 3
    return pp


def smooth_pieces(kn):
    """C2 not-a-knot splines of smooth positive functions of ln k on the knots (SciPy)."""
    from scipy.interpolate import CubicSpline
    x = kn.x
    t = (x - kn.x0) / (kn.x1 - kn.x0)
    fs = {F_HM: 1.0 + 0.4 * numpy.cos(2.0 * t), F_PPMM: 40.0 * numpy.exp(-1.5 * t),
          F_HG: 1.6 + 0.5 * numpy.sin(3.0 * t), F_PPGM: 90.0 * numpy.exp(-2.0 * t * t),
          F_PPGG: 150.0 / (1.0 + 4.0 * t * t), F_I12: 25.0 * numpy.exp(-t)}
    pp = numpy.empty((6, kn.NK - 1, 4))
    for f, y in fs.items():
        pp[f] = CubicSpline(x, y, bc_type="not-a-knot").c[::-1].T
    return pp


def knot_values(pp, dx):
    """off_knot[f]: the value of each piece at its own left knot, and of the last piece at the
    last knot."""
    last = pp[:, -1, :]
    end = last[:, 0] + dx * (last[:, 1] + dx * (last[:, 2] + dx * last[:, 3]))
    return numpy.concatenate([pp[:, :, 0], end[:, None]], axis=1)


def poly(c, d):
    """The cubic pieces c[..., 4] at d, in long double (Horner)."""
    c = c.astype(LD)
    return c[..., 0] + d * (c[..., 1] + d * (c[..., 2] + d * c[..., 3]))


def poly_abs(c, d):
    """sum |c_j| |d|^j."""
    c, d = numpy.abs(c).astype(LD), numpy.abs(d)
    return c[..., 0] + d * (c[..., 1] + d * (c[..., 2] + d * c[..., 3]))


# -------------------------------------------------------------------------------------------
# the in-range restatement
# -------------------------------------------------------------------------------------------
# [derived] first-order rounding bounds, in units of U = 2^-53, of what the evaluators do with
# exact cubic values (each cubic is three fma: 3 U of its value, all terms positive):
#   T1 = A shape h_a h_b: A shape 1, h_a 3, h_b 3, two products 2, the closing fma / sum 1 = 10
#   pp: 3 and the closing sum 1 = 4
# asserted at twice that (EPS = 2 U).
K_T1, K_PP = 10, 4
# ssc_in_range: h^2 = 3 + 3 + 1 = 7; P_mm = fma(As, h^2, pp): 1 + 7 + 1 = 9 (positive terms);
# numerator fma(beat As, h^2, I12): beat 1, its product 1, As 1, h^2 7, fma 1 = 11 (I12: 3 + 1);
# the quotient 11 + 9 + 1 = 21; P_mm (1 + resp delta_b): fma 21 + 1, product 9 + 22 + 1 = 32
K_RESP, K_MM_SSC = 21, 32


def in_range(w, A, shape, pp, kn, lnk, idx, delta_b=0.0):
    """(value, bound) per sample, long double / double: the spectrum of code w from the pieces of
    interval idx at the exact ln k; bound = twice the [derived] rounding bound plus the change of
    the value when ln k - x_idx moves by delta (see Knots.delta), taken by differences."""
    fa, fb, fp = families(w)
    A = numpy.asarray(A).astype(LD)
    shape = numpy.asarray(shape).astype(LD)

    def at(d):
        ha, hb, p = poly(pp[fa][idx], d), poly(pp[fb][idx], d), poly(pp[fp][idx], d)
        if w in (SSC_RESPONSE, MM_SSC):
            As, h2 = A * shape, ha * ha
            pmm = As * h2 + p
            resp = (LD(SSC_BEAT) * As * h2 + hb) / pmm
            if w == SSC_RESPONSE:
                return resp, K_RESP * numpy.abs(resp)
            # (a negative delta_b: the bound is of the terms' magnitudes, not of their sum)
            return pmm * (1 + resp * LD(delta_b)), K_MM_SSC * pmm * (1 + numpy.abs(resp * LD(delta_b)))
        # (a cubic's 3 U are of sum |c_j| |d|^j: its value where the coefficients are non-negative)
        sa, sb, sp = poly_abs(pp[fa][idx], d), poly_abs(pp[fb][idx], d), poly_abs(pp[fp][idx], d)
        t1 = A * shape * ha * hb
        return t1 + p, (numpy.abs(A * shape) * (3 * sa * numpy.abs(hb) + 3 * sb * numpy.abs(ha)) +
                        (K_T1 - 6) * numpy.abs(t1) + 3 * sp + (K_PP - 3) * numpy.abs(p))

    if w in (SSC_RESPONSE, MM_SSC):          # (their bounds take every term positive)
        assert min(pp[f].min() for f in (fa, fb, fp)) >= 0.0
    d = lnk - kn.x[idx].astype(LD)
    dl = kn.delta(lnk, idx).astype(LD)
    v, r = at(d)
    moved = numpy.maximum(numpy.abs(at(d + dl)[0] - v), numpy.abs(at(d - dl)[0] - v))
    return v, (EPS * r + 1.01 * moved).astype(float)


# -------------------------------------------------------------------------------------------
# how a wavefront's k sit on the knots (classify_wave restated from reference indices)
# -------------------------------------------------------------------------------------------
def classify(kn, k, w=MM, n_groups=None, use_alt=False):
    """Per group of 128 consecutive k: (idxu, fast, two).  Lanes past nk hold k = 1 (load_k_lanes);
    a group is fast when every k is present, in range and in interval idxu or idxu + 1, idxu the
    interval of its first k; `two` when any interval differs from idxu.  use_alt: the knot-band
    samples take their other interval."""
    k = numpy.asarray(k, dtype=float)
    nk = k.size
    ng = (nk + GROUP - 1) // GROUP if n_groups is None else n_groups
    pad = numpy.ones(ng * GROUP)
    pad[:nk] = k
    present = numpy.arange(ng * GROUP) < nk
    _, idx, inr, alt = kn.locate(pad)
    if use_alt:
        idx = alt
    idx, inr, present = (a.reshape(ng, GROUP) for a in (idx, inr, present))
    idxu = idx[:, 0]
    near = (idx == idxu[:, None]) | (idx == idxu[:, None] + 1)
    fast = numpy.all(present & inr & near, axis=1) & (w != LIN)
    two = numpy.any(idx != idxu[:, None], axis=1)
    return idxu, fast, two


def band_count(kn, k):
    _, idx, inr, alt = kn.locate(k)
    return int(numpy.sum(inr & (alt != idx)))


# -------------------------------------------------------------------------------------------
# k grids of the grid and streaming cases, built group by group
# -------------------------------------------------------------------------------------------
KINDS = ("in", "two", "slow2", "shuffled", "oor_hi", "oor_lo", "nan")


def group_k(kn, kind, j, m, rng):
    """m k of one wavefront.  in: inside interval j; two: across knot j + 1 only; slow2: across
    knots j + 1 and j + 2; shuffled: `slow2` in random order; oor_hi / oor_lo / nan: `in` with
    one k (not the first) above k_max / below k_min / NaN.  ln k stays 5 % of dx off every knot."""
    j = j % (kn.NK - 3)
    a, dx = kn.x[j], kn.dx
    if kind == "two":
        lo, hi = a + 0.55 * dx, a + 1.45 * dx
    elif kind in ("slow2", "shuffled"):
        lo, hi = a + 0.55 * dx, a + 2.45 * dx
    else:
        lo, hi = a + 0.05 * dx, a + 0.95 * dx
    x = numpy.linspace(lo, hi, m) if m > 1 else numpy.array([0.5 * (lo + hi)])
    # keep 5 % of dx off the knots inside the span
    for q in (1, 2):
        knot = a + q * dx
        close = numpy.abs(x - knot) < 0.05 * dx
        x[close] = knot + numpy.where(x[close] >= knot, 0.05, -0.05) * dx
    k = numpy.exp(x)
    if kind == "shuffled":
        k = rng.permutation(k)
    if m > 1 and kind in ("oor_hi", "oor_lo", "nan"):
        at = 1 + int(rng.integers(m - 1))
        k[at] = {"oor_hi": 2.0 * K_MAX, "oor_lo": 0.5 * K_MIN, "nan": numpy.nan}[kind]
    return k


def make_grid(kn, nk, pattern, seed=0):
    """nk k, the kinds of `pattern` cycled over the groups of 128, the interval advancing with the
    group (so that consecutive blocks sit on different pieces)."""
    rng = numpy.random.default_rng(seed)
    out = []
    for g in range((nk + GROUP - 1) // GROUP):
        m = min(GROUP, nk - g * GROUP)
        out.append(group_k(kn, pattern[g % len(pattern)], g, m, rng))
    return numpy.concatenate(out)


def sorted_grid(kn, nk):
    """Log-spaced over the open range, ascending."""
    return numpy.exp(numpy.linspace(kn.x0 + 0.013 * kn.dx, kn.x1 - 0.017 * kn.dx, nk))


GRID_NKS = (1, 2, 127, 128, 129, 512, 514, 2562)
GRID_PATTERNS = {
    "dense": ("in",),
    "one_knot": ("two",),
    "two_knots": ("slow2",),
    "shuffled": ("shuffled",),
    "ragged": ("in", "oor_hi", "two", "nan", "in", "oor_lo"),
    "mixed": ("in", "two", "slow2", "two", "in", "shuffled", "in"),
}


def grid(kn, name, nk, seed=0):
    if name == "sorted":
        return sorted_grid(kn, nk)
    return make_grid(kn, nk, GRID_PATTERNS[name], seed)


# the streaming shape's parity sequence: many slow groups, few, none, many again (equal nk, a
# multiple of 128 so that `none` is possible)
STREAM_NK = 2560
STREAM_SEQUENCE = ("mixed", "few", "dense_two", "shuffled")


def stream_grid(kn, name, nk=STREAM_NK):
    if name == "few":
        pat = ["in", "two"] * ((nk // GROUP + 1) // 2 + 1)
        pat[3] = "oor_hi"
        pat[11] = "slow2"
        return make_grid(kn, nk, tuple(pat[:(nk + GROUP - 1) // GROUP]), 3)
    if name == "dense_two":
        return make_grid(kn, nk, ("in", "two", "in"), 4)
    return make_grid(kn, nk, GRID_PATTERNS[name], 5)


def start_rows(kn, k, cnt, w=MM):
    """The start rows blockIdx.x % cnt that a fast wavefront of the grid takes (k_power_grid)."""
    _, fast, _ = classify(kn, k, w)
    return {(g // (BLOCK // GROUP)) % cnt for g in numpy.nonzero(fast)[0]}


# -------------------------------------------------------------------------------------------
# the 6-point stencil (CellTabIntegrand::from_table)
# -------------------------------------------------------------------------------------------
def lagrange6(q, t):
    """Exact (long double) 6-point Lagrange value on nodes -2 .. 3 at t, and sum |q_m L_m(t)|."""
    t = LD(t)
    nodes = [LD(m) for m in range(-2, 4)]
    v, s = LD(0), LD(0)
    for m, xm in enumerate(nodes):
        L = LD(1)
        for n_, xn in enumerate(nodes):
            if n_ != m:
                L *= (t - xn) / (xm - xn)
        v += LD(q[m]) * L
        s += abs(LD(q[m]) * L)
    return v, s


# [derived] per term of the stencil: five factors t + c (1 U each), four products among them, the
# constant and its product (2), the product with q (1) = 12 U; five sums or fma more = 17 U of
# sum |q_m L_m(t)|; asserted at twice that
K_STENCIL = 17


def stencil_index(u, N):
    """from_table's interval choice."""
    inside = (u >= 0.0) and (u <= N)
    i = int(u) if inside else 2
    i = min(i, N - 3) if (inside and i > 2) else 2
    return inside, i
