"""The layer that turns the knot tables into P(k), AS COMPILED FOR THE DEVICE
(tests/devcheck/devpower.hip, the product's compiler flags), piece by piece against the long
double / mpmath restatement of tests/devpower_ref.py: PowerEval::eval_t (k_power) on every
branch, PowerEval::at_ln and its agreement with eval_t, halofit_mm / halofit_mm_ln, power_tail,
k_power_extrap, the Stage E launch shapes (k_power_grid with explicit epochs_per_y; k_power_prep +
k_power_stream + k_power_grid_lanes with their parity sequence), k_cell_ptab and the 6-point
stencil CellTabIntegrand::from_table.

The knot tables are handed in and deliberately discontinuous (devpower_ref.random_pieces): a lane
that reads a neighbouring cubic piece, a wrong knot offset or a wrong `two` flag is a gross error
here, where on a C2 spline it would hide below any golden bound.  A k whose exact ln k lies
within delta of an interior knot (the knot band, Knots.delta) may match either adjacent piece;
tests/test_devpower_cpu.py caps such samples at 2 % of a grid and shows from the reference alone
that the grids reach the fast, `two` and slow paths and every start-row rotation.

Every tolerance is one of three kinds, named beside it: [project] a bound the suite already
asserts (fast_log 4e-16 relative, test_gpu_devmath.py; linear power 2e-13, 1e-12 with wiggles,
test_gpu_devphys.py); [derived] a first-order rounding bound written out where it is used, times
two; [measured] sized in the test from a reference-side error against the high-precision
restatement, never from the device.  Each test prints what it measured before it asserts; the
maxima are in DESIGN.md."""
import ctypes

import numpy
import pytest

import devcheck_build as dcb
from devcheck_build import call, ptr
import devpower_ref as r
from devpower_ref import (EPS, U, LD, LIN, MM, GM, GG, SSC_RESPONSE, MM_SSC, HALOFIT, EXTRAPOLATE,
                          K_MIN, K_MAX)
from test_gpu_devphys import COSMOS, COSMO_KEYS, M, mp, mp_eh, mp_eh_bao, mp_delta_k

pytestmark = pytest.mark.gpu

INF = numpy.inf
CODES = (LIN, MM, GM, GG, SSC_RESPONSE, MM_SSC)
NAMES = {LIN: "lin", MM: "mm", GM: "gm", GG: "gg", SSC_RESPONSE: "ssc_response", MM_SSC: "mm_ssc"}
# HaloFit constants of plausible size (halo.py:1261-1319), one set per epoch of a case
HF_KEYS = ("k_s", "a_n", "b_n", "c_n", "alpha_n", "beta_n", "gamma_n", "mu_n", "nu_n", "f1", "f2", "f3")
HF_SETS = ((0.71, 1.52, 0.43, 2.1, 3.1, 1.9, 0.35, 0.0, 2.5, 1.03, 1.06, 0.93),
           (0.33, 2.7, 0.61, 1.4, 5.2, 2.3, 0.21, 0.02, 4.9, 1.01, 1.02, 0.97))
P_LIN_BOUND = {0: 2e-13, 1: 1e-12}     # [project] test_gpu_devphys.py::test_transfer_and_power
_MAXIMA = {}


def _note(key, value):
    _MAXIMA[key] = max(_MAXIMA.get(key, 0.0), float(value))


@pytest.fixture(scope="module")
def dw():
    return dcb.load("devpower")


@pytest.fixture(scope="module")
def fields():
    return dcb.epoch_fields(dcb.load("devphys"))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


class Ep:
    """One Epoch record read back from the device."""

    def __init__(self, buf, fields, hf):
        self.buf, self._fields = buf, fields
        for key, v in zip(HF_KEYS, hf):
            setattr(self, "hf_" + key, float(v))

    def __getattr__(self, name):
        try:
            off, is_int = self.__dict__["_fields"][name]
        except KeyError:
            raise AttributeError(name)
        return (int(self.buf[off:off + 4].view(numpy.int32)[0]) if is_int
                else float(self.buf[off:off + 8].view(numpy.float64)[0]))


class Case:
    """Epochs, table blocks and scalars handed to the harness.  cosmos / zs: per epoch; pieces:
    per epoch the (6, NK - 1, 4) coefficients; flags: misc[2]; tails: misc[3..7] per epoch."""

    def __init__(self, dw, fields, NK, bao, cosmos, zs, pieces, flags=None, tails=None, delta_b=None):
        self.dw, self.NK, self.bao, self.n = dw, NK, int(bao), len(zs)
        raw = numpy.zeros(14, dtype=numpy.int32)
        call(dw, "dw_layout", NK, _ip(raw))
        self.off_knot, self.off_kpp = raw[0:6], raw[6:12]
        self.off_misc, self.stride = int(raw[12]), int(raw[13])
        logs = numpy.empty(2)
        call(dw, "dw_logs", K_MIN, K_MAX, ptr(logs))
        self.kn = r.Knots(NK, logs[0], logs[1])
        nin = dw.dw_epoch_inputs()
        self.ein = numpy.zeros((self.n, nin))
        self.hf = []
        for e in range(self.n):
            c = COSMOS[cosmos[e]]
            v = self.ein[e]
            v[:8] = [c[key] for key in COSMO_KEYS]
            v[8:14] = [zs[e], 1.48e-8, K_MIN, K_MAX, self.bao, 0.93]
            v[14:20] = [0, 0.3, 0.707, 0.3222, 1.0, 200.0]
            v[20:25] = 1.0
            v[25:29] = [2.1e12, 9.0, -0.13, -1.0]
            v[29:36] = [0, 12.14, 0.15, 12.14, 13.43, 1.0, 0.0]
            hf = HF_SETS[0 if cosmos[e] == cosmos[0] else 1]
            v[37:49] = hf
            self.hf.append(hf)
        self.pieces = pieces
        self.tab = numpy.full((self.n, self.stride), numpy.nan)
        for e in range(self.n):
            kv = r.knot_values(pieces[e], self.kn.dx)
            for f in range(6):
                self.tab[e, self.off_knot[f]:self.off_knot[f] + NK] = kv[f]
                self.tab[e, self.off_kpp[f]:self.off_kpp[f] + 4 * (NK - 1)] = pieces[e][f].ravel()
            self.tab[e, self.off_misc + 2] = 0.0 if flags is None else flags[e]
            if tails is not None:
                self.tab[e, self.off_misc + 3:self.off_misc + 8] = tails[e]
        self.db = numpy.zeros(self.n) if delta_b is None else numpy.asarray(delta_b, dtype=float)
        buf = numpy.zeros(self.n * dw.dw_sizeof_epoch(), dtype=numpy.uint8)
        self.A = numpy.empty(self.n)
        call(dw, "dw_epochs", *self.head(), buf.ctypes.data_as(ctypes.c_void_p), ptr(self.A))
        size = dw.dw_sizeof_epoch()
        self.ep = [Ep(buf[e * size:(e + 1) * size], fields, self.hf[e]) for e in range(self.n)]
        self._shapes = {}

    def head(self, n=None):
        n = self.n if n is None else n
        return (n, ptr(self.ein), ptr(self.tab), self.NK, K_MIN, K_MAX)

    def eval(self, which, k, n=None):
        n = self.n if n is None else n
        out = numpy.empty((n, k.size))
        call(self.dw, "dw_eval", *self.head(n), ptr(self.db), self.bao, which, ptr(k), k.size, ptr(out))
        return out

    def at_ln(self, which, e, k):
        """at_ln, log(k), shape(log k), fast_log(k), shape(fast_log k) per sample."""
        out = numpy.empty((5, k.size))
        call(self.dw, "dw_at_ln", *self.head(), ptr(self.db), self.bao, which, e, ptr(k), k.size,
             ptr(out))
        return out

    def grid(self, w, extrap, epy, k, n=None):
        n = self.n if n is None else n
        out = numpy.empty((n, k.size))
        call(self.dw, "dw_grid", *self.head(n), ptr(self.db), self.bao, w, int(extrap), epy, ptr(k),
             k.size, ptr(out))
        return out

    def stream(self, w, extrap, blocks, ks, n=None):
        n = self.n if n is None else n
        ks = numpy.ascontiguousarray(ks)
        n_call, nk = ks.shape
        gx8 = (((nk + 511) // 512) + 7) // 8 * 8
        out = numpy.empty((n_call, n, nk))
        winfo = numpy.zeros((n_call, gx8 * 4), dtype=numpy.int32)
        slow = numpy.zeros((n_call, 2), dtype=numpy.int32)
        call(self.dw, "dw_stream", *self.head(n), ptr(self.db), self.bao, w, int(extrap), blocks,
             ptr(ks), n_call, nk, ptr(out), _ip(winfo), _ip(slow))
        return out, winfo, slow

    def extrap(self, w):
        out = numpy.empty((self.n, 5))
        call(self.dw, "dw_extrap", *self.head(), self.bao, w, ptr(out))
        return out

    def shapes(self, k, key):
        """Per epoch: (shape at log k, shape at fast_log k), as the device returned them."""
        if key not in self._shapes:
            got = [self.at_ln(MM, e, k) for e in range(self.n)]
            self._shapes[key] = (numpy.array([g[2] for g in got]), numpy.array([g[4] for g in got]))
        return self._shapes[key]


def make_case(dw, fields, NK, bao, cosmos=("default", "alt"), zs=(0.0, 0.5), smooth=False, seed=1,
              **kw):
    logs = numpy.empty(2)
    call(dw, "dw_logs", K_MIN, K_MAX, ptr(logs))
    kn = r.Knots(NK, logs[0], logs[1])
    if smooth:
        pieces = [r.smooth_pieces(kn) * (1.0 + 0.1 * e) for e in range(len(zs))]
    else:
        pieces = [r.random_pieces(NK, seed + 17 * e, kn.dx) for e in range(len(zs))]
    return Case(dw, fields, NK, bao, cosmos, zs, pieces, **kw)


def special_k(kn):
    """About 1500 k (so that the 3 (NK - 2) samples on and beside the interior knots stay under
    the 2 % cap at NK = 11): log-spaced 1e-5 .. 1e4, the ends of the range and every knot with one
    ulp either side, and 1e-17, 0, -1, inf, NaN."""
    pts = [K_MIN, K_MAX] + [float(numpy.exp(x)) for x in kn.x[1:-1]]
    sp = []
    for v in pts:
        sp += [numpy.nextafter(v, 0.0), v, numpy.nextafter(v, INF)]
    return numpy.concatenate([numpy.logspace(-5, 4, 1460), sp, [1e-17, 1e-16, 0.0, -1.0, INF, numpy.nan]])


def _same(a, b):
    """Bit for bit (NaN equal to NaN)."""
    return numpy.array_equal(numpy.asarray(a), numpy.asarray(b), equal_nan=True)


def _ratio(got, val, bound, alt_val=None, alt_bound=None, band=None):
    """max |got - val| / bound over the samples; a knot-band sample may match its other piece."""
    err = numpy.abs(got.astype(LD) - val).astype(float) / bound
    if alt_val is not None and band is not None and band.any():
        err_alt = numpy.abs(got.astype(LD) - alt_val).astype(float) / alt_bound
        err = numpy.where(band, numpy.minimum(err, err_alt), err)
    return float(numpy.max(err)) if err.size else 0.0


def c_lo_candidates(pp, w, plin_kmin):
    """c_lo = h_a(k_min) h_b(k_min) + pp(k_min) / P_lin(k_min) in double, the sum with or without
    an fma (the compiler's choice): both exactly."""
    fa, fb, fp = r.families(w)
    if w in (SSC_RESPONSE, MM_SSC):
        fb = fa
    ha, hb, q = float(pp[fa][0, 0]), float(pp[fb][0, 0]), float(pp[fp][0, 0]) / float(plin_kmin)
    fused = float(M(ha) * M(hb) + M(q))
    return {fused, ha * hb + q}


# -------------------------------------------------------------------------------------------
# mpmath: HaloFit and the tail (halo.py:1339-1360, 341-367)
# -------------------------------------------------------------------------------------------
def mp_halofit(e, k, dk):
    k, dk = M(k), M(dk) if not isinstance(dk, mp.mpf) else dk
    y = k / M(e.hf_k_s)
    d2q = dk * ((1 + dk) ** M(e.hf_beta_n) / (1 + M(e.hf_alpha_n) * dk) * mp.exp(-(y / 4 + y * y / 8)))
    d2h = (M(e.hf_a_n) * y ** (3 * M(e.hf_f1)) /
           (1 + M(e.hf_b_n) * y ** M(e.hf_f2) + (M(e.hf_c_n) * M(e.hf_f3) * y) ** (3 - M(e.hf_gamma_n)))) / \
        (1 + M(e.hf_mu_n) / y + M(e.hf_nu_n) / (y * y))
    return 2 * mp.pi ** 2 / k ** 3 * (d2q + d2h)


def halofit_bound(e, k, dk, dk_rel):
    """[derived] relative bound of either device form of halofit_mm given its Delta^2 to dk_rel:
    d2q moves by at most (1 + beta) dk_rel with dk; every power is an exp (or pow) whose argument
    X = c L carries U |X| from its product, c (2 U |L| + fast_log's 4e-16 |ln k|) from the logarithm
    L inside and 2 U of its own; 16 U for the remaining products, sums and quotients; times two."""
    lk, ly = abs(float(numpy.log(k))), abs(float(numpy.log(k / e.hf_k_s)))
    y = k / e.hf_k_s
    args = 0.0
    for c, L in ((e.hf_beta_n, abs(float(numpy.log1p(dk)))), (1.0, y / 4 + y * y / 8),
                 (e.hf_f2, ly), (3.0 - e.hf_gamma_n, ly + abs(numpy.log(e.hf_c_n * e.hf_f3))),
                 (3.0 * e.hf_f1, ly)):
        args += abs(c) * (3 * U * L + r.FAST_LOG_REL * lk) + 2 * U
    return 2 * ((1 + abs(e.hf_beta_n)) * dk_rel + args + 16 * U)


def mp_plin(e, k, bao):
    T = mp_eh_bao(e, k) if bao else mp_eh(e, k)
    return 2 * mp.pi ** 2 * mp_delta_k(e, k, T) / M(k) ** 3


# -------------------------------------------------------------------------------------------
# a. eval_t, every branch; b. at_ln against the same reference and against eval_t
# -------------------------------------------------------------------------------------------
TAILS = ((1.37, 310.0, -1.31, 520.0, -2.07), (0.83, 95.0, -0.77, 1400.0, -1.63))
# [derived] eval_t multiplies the cubics by P_lin = 2 pi^2 Delta^2 / k^3 taken from the CHOMP_P_LIN
# launch of the same function: the two instances of that expression (8 roundings) may contract
# differently, 8 U of the term, times two
K_PLIN = 8


def _reference(C, e, w, extrap, k, plin, factor, loc):
    """Per sample of epoch e: value and bound where the knot tables answer (the spectrum's
    factor -- P_lin, A shape, or HaloFit's P_mm -- handed in), and the masks of the branches."""
    lnk, idx, inr, alt = loc
    ssc = w in (SSC_RESPONSE, MM_SSC)
    mid = inr & (k < K_MAX) if (extrap and not ssc) else inr
    val, bound = r.in_range(w, 1.0, factor, C.pieces[e], C.kn, lnk, idx, C.db[e])
    val2, bound2 = r.in_range(w, 1.0, factor, C.pieces[e], C.kn, lnk, alt, C.db[e])
    return mid, (val, bound, val2, bound2, alt != idx)


@pytest.mark.parametrize("smooth", [0, 1])
@pytest.mark.parametrize("NK", [8, 11])
@pytest.mark.parametrize("bao", [0, 1])
def test_eval_and_at_ln_every_branch(dw, fields, bao, NK, smooth):
    """k_power<BAO> (eval_t) and at_ln<false, BAO> for every code, with and without extrapolate,
    over special_k.  In range: [derived] the bound of devpower_ref.in_range (10 U of the 2-halo
    term, 4 U of the 1-halo term, the super-sample forms 21 U / 32 U, times two, plus the move of
    ln k - x_i by delta), the factor taken from the device (P_lin of the CHOMP_P_LIN launch for
    eval_t, plus K_PLIN; A times the shape at_ln's kernel returned for at_ln) and checked by
    itself against mpmath at the [project] bound.  The exact rules are asserted exactly: 1e-16 for
    k <= 1e-16, P_lin c_lo below k_min (0 for the response), 0 above k_max without extrapolation
    (and for NaN), P_lin misc[3] above k_max for P_mm with it; the power-law tails against mpmath:
    [derived] (|slope| + 3) U -- the quotient's rounding through the power, pow's 2 U, the product
    -- times two.  at_ln and eval_t agree within the sum of their two bounds in range and bit for
    bit on the constant branches.  smooth: the C2 spline tables instead of the discontinuous ones
    (the halo-model codes: the super-sample bounds take non-negative coefficients)."""
    C = make_case(dw, fields, NK, bao, tails=TAILS, delta_b=(0.013, -0.021), smooth=smooth)
    kn = C.kn
    k = special_k(kn)
    loc = kn.locate(k)
    lnk, idx, inr, alt = loc
    nband = int(numpy.sum(inr & (alt != idx)))
    print("knot-band samples: %d of %d" % (nband, k.size))
    assert nband <= 0.02 * k.size
    pos = numpy.isfinite(k) & (k > 1e-16)
    lin = C.eval(LIN, k)
    kmm = numpy.array([K_MIN, K_MAX])
    lin_ends = C.eval(LIN, kmm)
    sh_log, _ = C.shapes(k, "special")
    for e in range(C.n):
        # the factor by itself: linear power against mpmath on a thinned set
        sel = numpy.nonzero(pos)[0][::7]
        ref = numpy.array([float(mp_plin(C.ep[e], k[i], bao)) for i in sel])
        _note("eval_t LIN vs mpmath / [project] bound", numpy.max(numpy.abs(lin[e, sel] / ref - 1)) / P_LIN_BOUND[bao])
        assert numpy.max(numpy.abs(lin[e, sel] / ref - 1)) < P_LIN_BOUND[bao]
        assert numpy.all(lin[e, ~(k > 1e-16)] == 1e-16)       # k <= 1e-16, 0, -1, NaN
        ash = C.A[e] * sh_log[e]
        _note("A shape vs P_lin / [project] bound",
              numpy.max(numpy.abs(ash[pos] / lin[e, pos] - 1)) / (2 * P_LIN_BOUND[bao]))
        assert numpy.max(numpy.abs(ash[pos] / lin[e, pos] - 1)) < 2 * P_LIN_BOUND[bao]
    at_lin = numpy.array([C.at_ln(LIN, e, k)[0] for e in range(C.n)])
    assert _same(at_lin, lin)
    for w in (CODES[1:4] if smooth else CODES[1:]):
        ssc = w in (SSC_RESPONSE, MM_SSC)
        for extrap in (0, 1):
            which = w | (EXTRAPOLATE if extrap else 0)
            got = C.eval(which, k)
            for e in range(C.n):
                g = got[e]
                factor = C.A[e] * sh_log[e] if ssc else lin[e]
                mid, (val, bound, val2, bound2, band) = _reference(C, e, w, extrap, k, lin[e], factor, loc)
                slack = 0.0 if ssc else K_PLIN * EPS * numpy.abs(val).astype(float)
                key = "eval_t %s in range / [derived] bound" % ("ssc" if ssc else "halo")
                ratio = _ratio(g[mid], val[mid], (bound + slack)[mid], val2[mid], (bound2 + slack)[mid], band[mid])
                _note(key, ratio)
                assert ratio <= 1.0, (NAMES[w], extrap, e, ratio)
                below = ~numpy.isnan(k) & (k < K_MIN)
                if w == SSC_RESPONSE:
                    assert numpy.all(g[below] == 0.0)
                else:
                    cands = c_lo_candidates(C.pieces[e], w, lin_ends[e, 0])
                    assert any(_same(g[below], lin[e, below] * c) for c in cands), (NAMES[w], e)
                above = ~mid & ~below
                if not extrap or ssc:
                    assert numpy.all(g[above] == 0.0), (NAMES[w], e)       # k > k_max, NaN
                elif w == MM:
                    assert _same(g[above], lin[e, above] * TAILS[e][0])
                else:
                    v0, slope = TAILS[e][1:3] if w == GM else TAILS[e][3:5]
                    fin = above & numpy.isfinite(k)
                    assert numpy.isnan(g[numpy.isnan(k)]).all()
                    ref = numpy.array([float((M(kv) / M(K_MAX)) ** M(slope) * M(v0)) for kv in k[fin]])
                    ratio = float(numpy.max(numpy.abs(g[fin] / ref - 1)) / (2 * (abs(slope) + 3) * U))
                    _note("power_tail vs mpmath / [derived] bound", ratio)
                    assert ratio <= 1.0
                    assert g[k == INF][0] == 0.0              # (a negative slope)
                if ssc:
                    continue
                # at_ln: the factor is A times the shape its own kernel returned
                a = C.at_ln(which, e, k)
                assert _same(a[2], sh_log[e])
                midv = r.in_range(w, C.A[e], sh_log[e], C.pieces[e], kn, lnk, idx)
                midv2 = r.in_range(w, C.A[e], sh_log[e], C.pieces[e], kn, lnk, alt)
                ratio = _ratio(a[0][mid], midv[0][mid], midv[1][mid], midv2[0][mid], midv2[1][mid], band[mid])
                _note("at_ln in range / [derived] bound", ratio)
                assert ratio <= 1.0, (NAMES[w], extrap, e, ratio)
                # the constant branches, bit for bit (but a NaN k with extrapolate: eval_t hands it
                # to the tail, at_ln returns 0)
                cb = ~mid & ~numpy.isnan(k)
                assert _same(a[0][cb], g[cb]), (NAMES[w], extrap, e)
                assert numpy.all(a[0][numpy.isnan(k)] == 0.0)
                # "agrees with operator() to rounding": within the sum of the two bounds, the
                # factors' difference included ([project] twice the linear power's bound)
                both = bound + slack + midv[1] + 2 * P_LIN_BOUND[bao] * numpy.abs(val).astype(float)
                agree = numpy.abs(a[0][mid] - g[mid]) / both[mid]
                # (a knot-band sample may sit on different pieces in the two: compare each to its own)
                agree = agree[~band[mid]]
                _note("at_ln vs eval_t / sum of bounds", agree.max())
                assert agree.max() <= 1.0


@pytest.mark.parametrize("bao", [0, 1])
def test_halofit_both_forms(dw, fields, bao):
    """halofit_mm (eval_t: pow) and halofit_mm_ln (at_ln<true>: exp of linear forms in ln k)
    against mpmath on the device's own Delta^2 -- P_lin of the CHOMP_P_LIN launch times
    k^3 / 2 pi^2 for the pow form (4 U), A shape k^3 / 2 pi^2 for the ln form (5 U) -- within
    halofit_bound ([derived]); the two forms within the sum of their bounds plus [project] twice
    the linear power's bound for their different Delta^2.  The cross spectra: P_mm of the same
    launch times the cubic pieces ([derived] in_range), exactly 0 outside [k_min, k_max] for every
    finite positive k (HaloFit's range rule) and, in at_ln, for every k; extrapolate is ignored."""
    C = make_case(dw, fields, 11, bao, tails=TAILS)
    kn = C.kn
    k = special_k(kn)
    loc = kn.locate(k)
    lnk, idx, inr, alt = loc
    band = alt != idx
    pos = numpy.isfinite(k) & (k > 1e-16)
    lin = C.eval(LIN, k)
    sh_log, _ = C.shapes(k, "special")
    pmm = C.eval(MM | HALOFIT, k)
    assert _same(pmm, C.eval(MM | HALOFIT | EXTRAPOLATE, k))
    sel = numpy.nonzero(pos)[0][::5]
    for e in range(C.n):
        E = C.ep[e]
        a_mm = C.at_ln(MM | HALOFIT, e, k)[0]
        worst = [0.0, 0.0, 0.0]
        for i in sel:
            kv = float(k[i])
            dk_pow = M(lin[e, i]) * M(kv) ** 3 / (2 * mp.pi ** 2)
            dk_ln = M(C.A[e]) * M(sh_log[e, i]) * M(kv) ** 3 / (2 * mp.pi ** 2)
            b_pow = halofit_bound(E, kv, float(dk_pow), 4 * U)
            b_ln = halofit_bound(E, kv, float(dk_ln), 5 * U)
            r_pow, r_ln = mp_halofit(E, kv, dk_pow), mp_halofit(E, kv, dk_ln)
            worst[0] = max(worst[0], abs(float(M(pmm[e, i]) / r_pow - 1)) / b_pow)
            worst[1] = max(worst[1], abs(float(M(a_mm[i]) / r_ln - 1)) / b_ln)
            both = b_pow + b_ln + 2 * (1 + abs(E.hf_beta_n)) * 2 * P_LIN_BOUND[bao]
            worst[2] = max(worst[2], abs(a_mm[i] / pmm[e, i] - 1) / both)
        _note("halofit_mm vs mpmath / [derived] bound", worst[0])
        _note("halofit_mm_ln vs mpmath / [derived] bound", worst[1])
        _note("halofit ln form vs pow form / sum of bounds", worst[2])
        assert max(worst) <= 1.0, worst
        for w in (GM, GG):
            g = C.eval(w | HALOFIT, k)[e]
            a = C.at_ln(w | HALOFIT | EXTRAPOLATE, e, k)[0]
            a_pmm = a_mm
            for got, factor, key in ((g, pmm[e], "eval_t"), (a, a_pmm, "at_ln")):
                v, b = r.in_range(w, 1.0, factor, C.pieces[e], kn, lnk, idx)
                v2, b2 = r.in_range(w, 1.0, factor, C.pieces[e], kn, lnk, alt)
                s, s2 = K_PLIN * EPS * numpy.abs(v).astype(float), K_PLIN * EPS * numpy.abs(v2).astype(float)
                ratio = _ratio(got[inr], v[inr], (b + s)[inr], v2[inr], (b2 + s2)[inr], band[inr])
                _note("HaloFit cross spectra in range / [derived] bound", ratio)
                assert ratio <= 1.0, (key, NAMES[w], e, ratio)
            assert numpy.all(g[pos & ~inr] == 0.0) and numpy.all(a[~inr] == 0.0)


# -------------------------------------------------------------------------------------------
# c. k_power_extrap, and k == k_max with extrapolate in every shape
# -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NK", [8, 11])
@pytest.mark.parametrize("bao", [0, 1])
def test_extrap_constants_and_k_max(dw, fields, bao, NK):
    """misc[3] = h_a h_b + pp / P_lin(k_max), the value P_lin h_a h_b + pp at k_max and the mean of
    the five log-slopes over knots -7 .. -1, against mpmath on the knot values handed in and
    mpmath's linear power.  [project] P_lin's bound B, and [derived]: value and misc[3] 2 (B + 4 U);
    a log-slope is a difference of two logarithms, each off by B + 4 U, over dx: 2 (B + 4 U) / dx,
    times two.  (The knot values differ by tens of percent from knot to knot: a mean over four
    slopes, or over other knots, is far off.)  The kernel writes only its own spectrum's slots.
    Then k == k_max with extrapolate: eval_t and at_ln take the tail (k < k_max fails: the value
    slot, P_lin misc[3] for P_mm), k_power_grid -- fast path and per-lane path alike -- takes the
    spline's last piece at its right end (in1 = k <= k_max); they agree within in_range's
    [derived] bound plus [project] twice P_lin's bound (the tail's P_lin against A shape) and 8 U."""
    C = make_case(dw, fields, NK, bao, tails=TAILS)
    kn = C.kn
    B = P_LIN_BOUND[bao]
    kv = r.knot_values
    kmax = numpy.array([K_MAX])
    for w in (MM, GM, GG):
        got = C.extrap(w)
        fa, fb, fp = r.families(w)
        for e in range(C.n):
            kn_v = kv(C.pieces[e], kn.dx)
            plin = mp_plin(C.ep[e], K_MAX, bao)
            ha, hb, p = M(kn_v[fa][-1]), M(kn_v[fb][-1]), M(kn_v[fp][-1])
            if w == MM:
                ref = ha * hb + p / plin
                err = abs(float(M(got[e, 0]) / ref - 1)) / (2 * (B + 4 * U))
                _note("k_power_extrap misc[3] / bound", err)
                assert err <= 1.0 and numpy.isnan(got[e, 1:]).all()
                continue
            lv, lx = [], []
            for j in range(NK - 7, NK - 1):
                x = M(kn.x0) + (M(kn.x1) - M(kn.x0)) * j / (NK - 1)
                lx.append(x)
                lv.append(mp.log(mp_plin(C.ep[e], float(mp.exp(x)), bao) * M(kn_v[fa][j]) * M(kn_v[fb][j]) +
                                 M(kn_v[fp][j])))
            slope = sum((lv[m + 1] - lv[m]) / (lx[m + 1] - lx[m]) for m in range(5)) / 5
            four = sum((lv[m + 1] - lv[m]) / (lx[m + 1] - lx[m]) for m in range(4)) / 4
            at = 1 if w == GM else 3
            err_v = abs(float(M(got[e, at]) / (plin * ha * hb + p) - 1)) / (2 * (B + 4 * U))
            tol_s = 2 * 2 * (B + 4 * U) / kn.dx
            err_s = abs(float(M(got[e, at + 1]) - slope)) / tol_s
            _note("k_power_extrap value at k_max / bound", err_v)
            _note("k_power_extrap mean log-slope / bound", err_s)
            assert abs(float(four - slope)) > 100 * tol_s       # (the test can tell them apart)
            assert err_v <= 1.0 and err_s <= 1.0, (NAMES[w], e, err_v, err_s)
            others = [j for j in range(5) if j not in (at, at + 1)]
            assert numpy.isnan(got[e, others]).all()
    # k == k_max with the constants k_power_extrap wrote
    for e in range(C.n):
        C.tab[e, C.off_misc + 3] = C.extrap(MM)[e, 0]
        C.tab[e, C.off_misc + 4:C.off_misc + 6] = C.extrap(GM)[e, 1:3]
        C.tab[e, C.off_misc + 6:C.off_misc + 8] = C.extrap(GG)[e, 3:5]
    kfull = numpy.full(128, K_MAX)                              # a fast wavefront of k_max
    lnk, idx, inr, alt = kn.locate(kmax)
    assert inr[0] and idx[0] == NK - 2 == alt[0]
    lin = C.eval(LIN, kmax)
    for w in (MM, GM, GG):
        which = w | EXTRAPOLATE
        ev = C.eval(which, kmax)
        lanes = C.grid(w, 1, 1, kmax)                           # one k: the per-lane path
        fast = C.grid(w, 1, C.n, kfull)
        assert numpy.all(fast == fast[:, :1])
        for e in range(C.n):
            al = C.at_ln(which, e, kmax)
            assert al[0][0] == ev[e, 0]                         # both take the tail
            tail = lin[e, 0] * C.tab[e, C.off_misc + 3] if w == MM else C.tab[e, C.off_misc + (4 if w == GM else 6)]
            assert ev[e, 0] == tail
            v, b = r.in_range(w, C.A[e], al[4], C.pieces[e], kn, lnk, idx)
            tol = b[0] + (2 * B + 8 * U) * abs(float(v[0]))
            for name, g in (("per-lane", lanes[e, 0]), ("fast", fast[e, 0])):
                ratio = abs(float(LD(g) - v[0])) / b[0]
                _note("grid at k_max (spline) / [derived] bound", ratio)
                assert ratio <= 1.0, (name, NAMES[w], e)
                ratio = abs(g - ev[e, 0]) / tol
                _note("tail vs spline at k_max / bound", ratio)
                assert ratio <= 1.0, (name, NAMES[w], e)


# -------------------------------------------------------------------------------------------
# d. k_power_grid
# -------------------------------------------------------------------------------------------
# two cosmologies interleaved A A B B A with the same-cosmology flags of k_halo_knots; and a
# second arrangement, A B B A A, in which a block of two rows (B, A) starts at a row whose flag
# is set: the rotated walk A -> B must take B's shape afresh
EPOCH_SETS = {
    "AABBA": (("default", "default", "alt", "alt", "default"), (0, 1, 0, 1, 0)),
    "ABBAA": (("default", "alt", "alt", "default", "default"), (0, 0, 1, 0, 1)),
}
ZS5 = (0.0, 0.3, 0.3, 1.1, 2.0)
DB5 = (0.013, -0.021, 0.034, 0.0, -0.008)
N_EPY = [(n, epy) for n in (1, 2, 3, 5) for epy in sorted({1, 2, n}) if epy <= n]


def grid_reference(C, w, extrap, k, key):
    """Per epoch (value, bound, alt value, alt bound), the band mask and the in-range mask: the
    grid kernels take ln k by fast_log and the shape at it, in range is k_min <= k <= k_max."""
    loc = C.kn.locate(k)
    lnk, idx, inr, alt = loc
    _, sh_fl = C.shapes(k, key)
    rows = []
    for e in range(C.n):
        v, b = r.in_range(w, C.A[e], sh_fl[e], C.pieces[e], C.kn, lnk, idx, C.db[e])
        v2, b2 = r.in_range(w, C.A[e], sh_fl[e], C.pieces[e], C.kn, lnk, alt, C.db[e])
        rows.append((v, b, v2, b2))
    return rows, alt != idx, inr


def check_grid(got, C, w, extrap, k, ref, ev, what):
    rows, band, inr = ref
    worst = 0.0
    for e in range(got.shape[0]):
        v, b, v2, b2 = rows[e]
        assert not numpy.isnan(got[e][inr]).any(), (what, e, "a sample never written")
        worst = max(worst, _ratio(got[e][inr], v[inr], b[inr], v2[inr], b2[inr], band[inr]))
        assert _same(got[e][~inr], ev[e][~inr]), (what, e, "outside the knots: not eval_t's bits")
    return worst


@pytest.mark.parametrize("name", list(r.GRID_PATTERNS) + ["sorted"])
@pytest.mark.parametrize("bao", [0, 1])
def test_power_grid(dw, fields, bao, name):
    """k_power_grid<BAO, SSC> for every non-LIN code over the row counts GRID_NKS (NK alternating
    8, 11), n in {1, 2, 3, 5} with epochs_per_y in {1, 2, n}, both epoch arrangements: in range
    against in_range ([derived] bound, shape at fast_log k as the device returned it, A = misc[1]);
    outside the knots bit for bit k_power's eval_t.  Every launch of one (grid, code) must also
    return the same bits whatever n and epochs_per_y."""
    worst = 0.0
    for inx, nk in enumerate(r.GRID_NKS):
        NK = (8, 11)[inx % 2]
        for set_name, (cosmos, flags) in EPOCH_SETS.items():
            if set_name == "ABBAA" and nk < 512:
                continue
            C = make_case(dw, fields, NK, bao, cosmos=cosmos, zs=ZS5, flags=flags, tails=[TAILS[0]] * 5,
                          delta_b=DB5, seed=3 + inx)
            k = r.grid(C.kn, name, nk, seed=inx)
            for w in CODES[1:]:
                for extrap in ((0, 1) if name in ("ragged", "sorted") else (inx % 2,)):
                    ref = grid_reference(C, w, extrap, k, (name, nk))
                    ev = C.eval(w | (EXTRAPOLATE if extrap else 0), k)
                    first = None
                    for n, epy in (N_EPY if set_name == "AABBA" else [(5, 2), (4, 2), (5, 5), (3, 2)]):
                        got = C.grid(w, extrap, epy, k, n)
                        worst = max(worst, check_grid(got, C, w, extrap, k, ref, ev,
                                                      (name, nk, NAMES[w], extrap, n, epy, set_name)))
                        if first is None or first.shape[0] < n:
                            first = got if first is None else numpy.concatenate([first, got[first.shape[0]:]])
                        assert _same(got, first[:n]), (name, nk, NAMES[w], n, epy, set_name)
    print("k_power_grid %s: %.3f of the [derived] bound" % (name, worst))
    _note("k_power_grid in range / [derived] bound", worst)
    assert worst <= 1.0


def test_power_grid_linear(dw, fields):
    """CHOMP_P_LIN through k_power_grid: never the fast path; every sample linear_power_t's bits."""
    C = make_case(dw, fields, 8, 0, cosmos=EPOCH_SETS["AABBA"][0], zs=ZS5, flags=EPOCH_SETS["AABBA"][1])
    for nk in (129, 2562):
        k = r.grid(C.kn, "ragged", nk)
        assert _same(C.grid(LIN, 0, 2, k), C.eval(LIN, k))


# -------------------------------------------------------------------------------------------
# e. k_power_prep + k_power_stream + k_power_grid_lanes
# -------------------------------------------------------------------------------------------
def expected_winfo(kn, k, n_groups, bits):
    """winfo per k group, restated twice: the knot-band samples on either side."""
    mask, slow_bit, two_bit = bits
    out = []
    for use_alt in (False, True):
        idxu, fast, two = r.classify(kn, k, MM, n_groups, use_alt)
        out.append(idxu | numpy.where(two, two_bit, 0) | numpy.where(fast, 0, slow_bit))
    return out


@pytest.mark.parametrize("blocks", [1, 2, 1024])
@pytest.mark.parametrize("bao", [0, 1])
def test_power_stream(dw, fields, bao, blocks):
    """The streaming shape on one set of buffers over the four k grids of STREAM_SEQUENCE (many slow
    groups, few, none, many), n in {1, 2, 3, 4} (PER = 1 and 2), the lanes kernel on `blocks`
    blocks (chunks = 1, clamped, n_epoch): winfo is the restatement (either index only where a
    group holds a knot-band sample), slow[parity] the restated count and slow[parity ^ 1] zero
    after every call, no NaN byte survives in range, and every sample carries k_power_grid's bits.
    Then single calls on the even row counts of GRID_NKS."""
    bits = numpy.zeros(3, dtype=numpy.int32)
    dw.dw_wave_bits(_ip(bits))
    assert list(bits) == [0xffff, 1 << 16, 1 << 17]
    for n in (1, 2, 3, 4):
        NK = (8, 11)[n % 2]
        C = make_case(dw, fields, NK, bao, cosmos=("default",) * n, zs=ZS5[:n],
                      flags=(0, 1, 1, 1)[:n], tails=[TAILS[0]] * n, delta_b=DB5[:n], seed=40 + n)
        ks = numpy.array([r.stream_grid(C.kn, nm) for nm in r.STREAM_SEQUENCE])
        for w, extrap in ((MM, 0), (GM, 1), (GG, 0), (SSC_RESPONSE, 0), (MM_SSC, 1))[(n - 1) % 2::2] + ((GM, 0),):
            out, winfo, slow = C.stream(w, extrap, blocks, ks)
            for c in range(ks.shape[0]):
                lo, hi = expected_winfo(C.kn, ks[c], winfo.shape[1], bits)
                groups = (ks.shape[1] + r.GROUP - 1) // r.GROUP
                finite = numpy.all(numpy.isfinite(numpy.pad(ks[c], (0, winfo.shape[1] * r.GROUP - ks.shape[1]),
                                                            constant_values=1.0).reshape(-1, r.GROUP)), axis=1)
                cmp_mask = numpy.where(finite, -1, ~bits[2])               # (`two` of a NaN: unspecified)
                ok = ((winfo[c] & cmp_mask) == (lo & cmp_mask)) | ((winfo[c] & cmp_mask) == (hi & cmp_mask))
                assert ok.all(), (n, NAMES[w], c, numpy.nonzero(~ok)[0][:5])
                count = int(numpy.sum((lo[:groups] & bits[1]) != 0))
                assert numpy.array_equal(lo[:groups] & bits[1], hi[:groups] & bits[1])
                assert slow[c, c & 1] == count and slow[c, (c & 1) ^ 1] == 0, (n, c, slow[c], count)
                want = C.grid(w, extrap, 1, ks[c])
                assert not numpy.isnan(out[c][:, numpy.isfinite(ks[c])]).any()
                assert _same(out[c], want), (n, NAMES[w], extrap, c)
            counts = slow[numpy.arange(4), numpy.arange(4) & 1]
            assert counts[0] >= 5 and 1 <= counts[1] <= 2 and counts[2] == 0 and counts[3] >= 10
        for nk in [v for v in r.GRID_NKS if v % 2 == 0]:
            for name in ("dense", "one_knot", "ragged", "sorted", "two_knots"):
                k1 = r.grid(C.kn, name, nk)[None, :]
                out, winfo, slow = C.stream(GG, 1, blocks, k1)
                assert _same(out[0], C.grid(GG, 1, 1, k1[0])), (n, nk, name)


# -------------------------------------------------------------------------------------------
# f. k_cell_ptab and from_table
# -------------------------------------------------------------------------------------------
def _ptab_x(kn, N):
    return kn.x0 + (kn.x1 - kn.x0) * (numpy.arange(N + 1) / N)


@pytest.mark.parametrize("NK", [8, 11])
def test_cell_ptab(dw, fields, NK):
    """k_cell_ptab<HF, false>: the table of kPTabN + 1 values is at_ln at x_i = x0 + (x1 - x0) i / N,
    k = exp(x_i) -- compared with the reference at the k the device's at_ln kernel is then given
    (numpy's exp of the same x_i; a 1-ulp difference of k moves the value by |dP/dln k| ulp, inside
    delta) -- and its end points are exactly k_min and k_max: entry 0 and entry N equal at_ln at
    those k bit for bit.  [derived] in_range's bound; HaloFit P_mm: halofit_bound."""
    N = dw.dw_ptab_n()
    assert N == 8192
    C = make_case(dw, fields, NK, 0, cosmos=("alt",), zs=(0.4,), tails=TAILS[:1])
    kn = C.kn
    x = _ptab_x(kn, N)
    k = numpy.exp(x)
    k[0], k[-1] = K_MIN, K_MAX
    lnk, idx, inr, alt = kn.locate(k)
    # ln k of the table is x_i itself (handed to at_ln), not log(exp(x_i)): locate on x_i
    lnk = x.astype(LD)
    idx = numpy.clip(numpy.floor((x - kn.x0) / kn.dx).astype(int), 0, NK - 2)
    near = numpy.minimum(numpy.abs(x - kn.x[idx]), numpy.abs(x - kn.x[numpy.minimum(idx + 1, NK - 1)]))
    band = (near <= kn.delta(x, idx)) & (numpy.arange(N + 1) > 0) & (numpy.arange(N + 1) < N)
    alt = numpy.where(band, numpy.where(numpy.abs(x - kn.x[idx]) <= kn.delta(x, idx),
                                        numpy.maximum(idx - 1, 0), numpy.minimum(idx + 1, NK - 2)), idx)
    print("knot-band samples of the table: %d of %d" % (band.sum(), N + 1))
    assert band.sum() <= 0.02 * (N + 1)
    sh = C.at_ln(MM, 0, k)[2]
    out = numpy.empty(N + 1)
    for w in (LIN, MM, GM, GG):
        for extrap in (0, EXTRAPOLATE):
            which = w | extrap
            call(dw, "dw_ptab", *C.head()[1:], which, ptr(out))
            assert not numpy.isnan(out).any()
            ends = C.at_ln(which, 0, numpy.array([K_MIN, K_MAX]))[0]
            assert out[0] == ends[0] and out[N] == ends[1], (NAMES[w], extrap)
            if w == LIN:
                ref = C.eval(LIN, k)[0]
                ratio = float(numpy.max(numpy.abs(out / ref - 1))) / (2 * P_LIN_BOUND[0])
                _note("k_cell_ptab LIN vs linear_power_t / [project] bound", ratio)
                assert ratio <= 1.0
                continue
            inside = numpy.arange(N + 1) < (N if extrap else N + 1)     # (k_max with extrapolate: the tail)
            # the shape carries exp(ns x_i) against exp(ns log k): [derived] ns (U |x_i| + delta)
            v, b = r.in_range(w, C.A[0], sh, C.pieces[0], kn, lnk, idx)
            v2, b2 = r.in_range(w, C.A[0], sh, C.pieces[0], kn, lnk, alt)
            s = 2 * (EPS * numpy.abs(x) + kn.delta(x, idx)) * numpy.abs(v).astype(float)
            ratio = _ratio(out[inside], v[inside], (b + s)[inside], v2[inside], (b2 + s)[inside], band[inside])
            _note("k_cell_ptab in range / [derived] bound", ratio)
            assert ratio <= 1.0, (NAMES[w], extrap, ratio)
    for w in (MM, GM, GG):
        call(dw, "dw_ptab", *C.head()[1:], w | HALOFIT, ptr(out))
        ends = C.at_ln(w | HALOFIT, 0, numpy.array([K_MIN, K_MAX]))[0]
        assert out[0] == ends[0] and out[N] == ends[1] and not numpy.isnan(out).any()
        ref = C.at_ln(w | HALOFIT, 0, k)[0]
        E = C.ep[0]
        sel = numpy.arange(0, N + 1, 97)
        tol = numpy.array([halofit_bound(E, float(k[i]), float(C.A[0] * sh[i] * k[i] ** 3 / (2 * numpy.pi ** 2)),
                                         2 * (EPS * abs(x[i]) + kn.delta(x[i], idx[i])))
                           for i in sel]) * 2
        ok = ~band[sel]
        ratio = float(numpy.max((numpy.abs(out[sel] / ref[sel] - 1) / tol)[ok]))
        _note("k_cell_ptab HaloFit vs at_ln / [derived] bound", ratio)
        assert ratio <= 1.0, (NAMES[w], ratio)


def _stencil(dw, C, which, table, lk, k):
    out = numpy.empty((3, lk.size))
    call(dw, "dw_stencil", *C.head()[1:], which, ptr(table), ptr(lk), ptr(k), lk.size, ptr(out))
    return out


def _stencil_points(kn, N):
    pdx = (kn.x1 - kn.x0) / N
    inv = 1.0 / pdx
    us = [0.0, 0.5, numpy.nextafter(2.0, 0.0), 2.0, 2.5, numpy.nextafter(N - 3.0, 0.0), N - 3.0,
          numpy.nextafter(N - 3.0, INF), N - 0.5, float(N), 3.0, 2.999, 17.25, 4000.5, N - 2.5, N - 1.0]
    lk = [kn.x0 + u * pdx for u in us]
    lk[9] = kn.x1
    lk += [kn.x0 - 1e-12, kn.x0 - 1.0, kn.x1 + 1e-12, kn.x1 + 2.0, numpy.nan]     # (just outside: ~1e-9 of a step)
    lk = numpy.array(lk)
    u = (lk - kn.x0) * inv                                      # (from_table's own expression)
    return lk, u


def test_stencil_on_a_handed_in_table(dw, fields):
    """from_table on a random positive table, and on the table k_cell_ptab fills from the C2 spline
    tables, against exact 6-point Lagrange at from_table's own
    u = (lk - x0) / pdx (double): [derived] K_STENCIL U sum |q_m L_m(t)|, times two.  At
    u = kPTabN the last entry exactly, at u = 0 the first; just outside both ends and for NaN the
    value is 0."""
    N = dw.dw_ptab_n()
    C = make_case(dw, fields, 8, 0, cosmos=("default",), zs=(0.2,), tails=TAILS[:1])
    kn = C.kn
    rng = numpy.random.default_rng(11)
    table = rng.uniform(0.5, 2.0, N + 1) * numpy.exp(-numpy.arange(N + 1) / 2000.0)
    # ... and the table k_cell_ptab fills from the C2 spline tables (P_gm)
    S = make_case(dw, fields, 11, 0, cosmos=("default",), zs=(0.2,), tails=TAILS[:1], smooth=True)
    spline_table = numpy.empty(N + 1)
    call(dw, "dw_ptab", *S.head()[1:], GM, ptr(spline_table))
    lk, u = _stencil_points(kn, N)
    k = numpy.exp(lk)
    worst = 0.0
    seen = set()
    for tab_ in (spline_table, table):
        out = _stencil(dw, C, MM, tab_, lk, k)
        for j in range(lk.size):
            inside, i = r.stencil_index(u[j], N) if not numpy.isnan(u[j]) else (False, 2)
            if not inside:
                assert out[0, j] == 0.0, (j, u[j])
                continue
            seen.add(i)
            v, s = r.lagrange6(tab_[i - 2:i + 4], LD(u[j]) - i)
            worst = max(worst, abs(float(LD(out[0, j]) - v)) / float(2 * r.K_STENCIL * U * s))
    print("stencil against exact Lagrange: %.3f of the [derived] bound; intervals %s" % (worst, sorted(seen)))
    _note("from_table vs exact Lagrange / [derived] bound", worst)
    assert worst <= 1.0
    assert {2, 3, N - 4, N - 3} <= seen
    # at u = kPTabN the last entry exactly -- for any last entry: sixteen of them
    assert u[9] == N and u[0] == 0.0
    last = []
    for j in range(16):
        table[N] = rng.uniform(0.5, 2.0)
        last.append((_stencil(dw, C, MM, table, lk[9:10], k[9:10])[0, 0], table[N]))
    print("at u = kPTabN: device - last entry, in ulps:",
          [round((g - t) / (numpy.nextafter(t, INF) - t)) for g, t in last])
    assert all(g == t for g, t in last)


@pytest.mark.parametrize("halofit", [0, 1])
def test_stencil_truth_table(dw, fields, halofit):
    """ok and the zeroing for every code, with and without extrapolate, and for HaloFit: inside the
    table ok and the stencil's value; outside it the value is 0, and ok only where the spectrum is
    identically zero there -- above k_max without extrapolate for the halo-model codes but LIN; on
    both sides for the HaloFit cross spectra.  Where ok is false operator() falls back to at_ln
    (bit for bit the at_ln kernel's value at the same ln k and k); where it is true it returns
    the table's value (times the node's factor 1)."""
    N = dw.dw_ptab_n()
    C = make_case(dw, fields, 8, 0, cosmos=("default",), zs=(0.2,), tails=TAILS[:1])
    kn = C.kn
    table = numpy.linspace(3.0, 1.0, N + 1)
    lk, u = _stencil_points(kn, N)
    lk, u = lk[:-1], u[:-1]                                       # (NaN: in the test above)
    k = numpy.exp(lk)
    k[numpy.argmax(u == N)] = K_MAX
    inside = (u >= 0.0) & (u <= N)
    assert (~inside & (u < 0)).sum() == 2 and (~inside & (u > N)).sum() == 2
    for w in ((MM, GM, GG) if halofit else (LIN, MM, GM, GG)):
        for extrap in (0, EXTRAPOLATE):
            which = w | extrap | (HALOFIT if halofit else 0)
            out = _stencil(dw, C, which, table, lk, k)
            if halofit:
                zero_out = numpy.full(u.shape, w != MM)
            else:
                zero_out = (u > 0.0) & (not extrap) & (w != LIN)
            ok = inside | zero_out
            assert numpy.array_equal(out[1] != 0.0, ok), (NAMES[w], extrap, halofit)
            assert numpy.all(out[0][~inside] == 0.0)
            direct = C.at_ln(which, 0, k)
            # (the at_ln kernel takes its own log(k); operator() the ln k handed in: compare where
            # the two logarithms are the same bits, which includes every point outside the table
            # unless the library's log(exp(x)) is not x)
            same_lk = direct[1] == lk
            fb = ~ok
            assert numpy.all(out[2][ok] == out[0][ok])
            assert (fb & same_lk).any() or not fb.any()
            assert _same(out[2][fb & same_lk], direct[0][fb & same_lk]), (NAMES[w], extrap, halofit)
            # outside [k_min, k_max] at_ln does not use ln k at all (but in the tail's power law,
            # which takes k): there the fall-back is at_ln's value whatever the logarithm
            if not halofit or w != MM:
                assert _same(out[2][fb], direct[0][fb]), (NAMES[w], extrap, halofit)


def test_interpolation_claim(dw, fields):
    """"~1e-16 relative at this spacing": on a table filled from a smooth analytic spectrum
    (a power law bent by a Gaussian bump, in long double, rounded to double) the exact Lagrange
    value against the exact function is the [measured, reference side] interpolation error; the
    device must be within that error plus the stencil's [derived] rounding bound.  The measured
    error itself is printed: it is the claim."""
    N = dw.dw_ptab_n()
    C = make_case(dw, fields, 8, 0, cosmos=("default",), zs=(0.2,), tails=TAILS[:1])
    kn = C.kn
    pdx = (kn.x1 - kn.x0) / N
    inv = 1.0 / pdx

    def f(x):
        x = numpy.asarray(x).astype(LD)
        return LD(3.0e3) * numpy.exp(-LD(1.3) * x - LD(0.05) * x * x) * (1 + LD(0.3) * numpy.exp(-(x + 2) ** 2))

    xi = LD(kn.x0) + LD(pdx) * numpy.arange(N + 1)
    table = f(xi).astype(float)
    rng = numpy.random.default_rng(5)
    u_try = numpy.concatenate([rng.uniform(0.0, N, 2000), rng.uniform(0.0, 3.0, 50), rng.uniform(N - 3.0, N, 50)])
    lk = kn.x0 + u_try * pdx
    u = (lk - kn.x0) * inv
    keep = (u >= 0) & (u <= N)
    lk, u = lk[keep], u[keep]
    out = _stencil(dw, C, MM, table, lk, numpy.exp(lk))
    interp, worst = 0.0, 0.0
    for j in range(lk.size):
        _, i = r.stencil_index(u[j], N)
        v, s = r.lagrange6(table[i - 2:i + 4], LD(u[j]) - i)
        exact = f(LD(kn.x0) + LD(u[j]) * LD(pdx))
        e_int = abs(float(v - exact))
        interp = max(interp, e_int / abs(float(exact)))
        worst = max(worst, abs(float(LD(out[0, j]) - exact)) / (e_int + float(2 * r.K_STENCIL * U * s)))
    print("6-point interpolation of a smooth spectrum: %.2e relative (reference side); the device "
          "at %.3f of that plus its rounding bound" % (interp, worst))
    _note("interpolation error of the stencil, relative (reference side)", interp)
    _note("from_table vs the exact function / (interpolation + rounding)", worst)
    assert worst <= 1.0
    # the claim itself, on the reference side.  [derived] the table's entries are rounded to double,
    # U each, and sum |L_m(t)| < 8 over the whole span of six equispaced points (their Lebesgue
    # constant is 3.1); the polynomial's own error at this spacing is below that: 8 U, times two
    assert interp < 8 * EPS


def test_print_maxima():
    """(last in the file) what the tests above measured, for DESIGN.md."""
    for key in sorted(_MAXIMA):
        print("%-66s %.3g" % (key, _MAXIMA[key]))
