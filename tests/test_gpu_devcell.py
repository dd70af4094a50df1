"""The C_l route -- the chi-only node table, k_cell, k_cell4, the hand-over of Romberg states,
k_cell_deep and the _epochs / _sets forms -- and the parallel not-a-knot spline build, AS COMPILED
FOR THE DEVICE (tests/devcheck/devcell.hip, the product's compiler flags), against the long-double
restatement of tests/devcell_ref.py.  The spectrum evaluator, k_cell_ptab and from_table are
test_gpu_devpower.py's: they are used here, not tested again.

Every tolerance is one of three kinds, named beside it, as in test_gpu_devpower.py: [project] a
bound the suite already asserts; [derived] a first-order rounding bound written out where it is
formed (devcell_ref.py), times two; [measured] sized in the test from a reference-side fp64
computation against the long-double one, never from the device.  Each test prints measured / bound
before it asserts; the maxima are in DESIGN.md."""
import ctypes

import mpmath
import numpy
import pytest
from scipy.interpolate import InterpolatedUnivariateSpline

import devcheck_build as dcb
import hostcheck_build
from devcheck_build import call, ptr
import devcell_ref as c
from devcell_ref import LD
from devpower_ref import FAST_LOG_REL

pytestmark = pytest.mark.gpu

NAN_BITS = numpy.uint64(0xFFFFFFFFFFFFFFFF)
NAN_INT = numpy.int32(-1)               # an int of NaN bytes
D_Z = 0.77


@pytest.fixture(scope="module")
def dl():
    return dcb.load("devcell")


@pytest.fixture(scope="module")
def projs():
    return c.proj_cases()


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _bits(a):
    return numpy.ascontiguousarray(a).view(numpy.uint64)


# -------------------------------------------------------------------------------------------
# 1. k_cell_nodes, k_cell_nodes_sets
# -------------------------------------------------------------------------------------------
_LOGS = {}


def _mp_log(chi):
    """ln of the doubles chi by mpmath (30 digits), as long double; cached per value."""
    out = numpy.empty(chi.size, dtype=LD)
    for i, v in enumerate(chi):
        v = float(v)
        if v not in _LOGS:
            _LOGS[v] = LD(mpmath.nstr(mpmath.log(mpmath.mpf(v)), 25))
        out[i] = _LOGS[v]
    return out


def _check_table(P, D_z, LT, nodes, tag):
    """One node table (3 N doubles) against the restatement: chi within 1 ulp of the exact node
    formula under the index map, ln chi within the device log's [project] bound of mpmath at the
    chi the device stored, F within the [derived] bound at that chi."""
    N = (1 << LT) + 1
    F, lnchi, chi = nodes[:N], nodes[N:2 * N], nodes[2 * N:3 * N]
    exact, lev, j = c.node_chi(P.chi_min, P.chi_max, LT)
    assert chi[0] == P.chi_min and chi[1] == P.chi_max
    for i in (2, 3, N - 1):                                 # the index map, spelt out
        if i < N:
            assert c.node_index(int(lev[i]), int(j[i])) == i
    err_chi = float(numpy.max(numpy.abs(chi.astype(LD) - exact) / c.ulp(exact.astype(float))))
    # thin the mpmath logarithms of a large table (every 16th node and both ends of every level)
    sel = numpy.arange(N) if N <= 1025 else numpy.unique(numpy.concatenate(
        [numpy.arange(0, N, 16), numpy.arange(1030), [N - 1]]))
    ref_log = _mp_log(chi[sel])
    err_log = float(numpy.max(numpy.abs(lnchi[sel].astype(LD) - ref_log) / numpy.abs(ref_log)) /
                    FAST_LOG_REL)
    ref, bound, (both, ig, _) = P.F(chi, D_z)
    zero = ref == 0
    assert numpy.all(F[zero] == 0.0), tag                   # outside a window: exactly 0
    nz = ~zero
    assert nz.any(), tag
    err_F = float(numpy.max(numpy.abs(F[nz].astype(LD) - ref[nz]) / bound[nz]))
    print("k_cell_nodes %s LT %d: chi %.3g ulp, ln chi %.3g of [project] %.1e, F %.3g of [derived] "
          "bound (bound / |F|: median %.2g max %.2g); nodes outside a window %d, growth outside its "
          "table %d of %d" % (tag, LT, err_chi, err_log, FAST_LOG_REL, err_F,
                              float(numpy.median(bound[nz] / numpy.abs(ref[nz]))),
                              float(numpy.max(bound[nz] / numpy.abs(ref[nz]))), int(zero.sum()),
                              int((~ig).sum()), N))
    assert err_chi <= 1.0, tag
    assert err_log <= 1.0, tag
    assert err_F <= 1.0, tag
    return err_chi, err_log, err_F


NODE_RUNS = [("equal", 1, 1, 2), ("equal", 6, 3, 7), ("inside", 9, 1, 2), ("overhang", 9, 3, 1000),
             ("narrow", 6, 1, 2), ("growth_ends", 9, 3, 64), ("overhang", 16, 1, 2),
             ("growth_ends", 16, 3, 4097)]


@pytest.mark.parametrize("name,LT,n_lists,stride", NODE_RUNS)
def test_cell_nodes(dl, projs, name, LT, n_lists, stride):
    """k_cell_nodes at LT in {1, 6, 9, 16} with 1 and 3 lists: the table (see _check_table), the
    lists' count and head zeroed and nothing else of the list buffer, nothing behind the table."""
    P = projs[name]
    N, extra = (1 << LT) + 1, 64
    nodes = numpy.zeros(3 * N + extra)
    deep = numpy.zeros((n_lists - 1) * stride + 2 + extra, dtype=numpy.int32)
    call(dl, "dl_nodes", P.NC, P.NWp, ptr(P.pdv), ptr(P.tab), D_Z, LT, n_lists, stride, extra,
         ptr(nodes), _ip(deep))
    assert numpy.all(_bits(nodes[3 * N:]) == NAN_BITS)      # entries behind 3 (2^LT + 1): untouched
    assert not numpy.isnan(nodes[:3 * N]).any()
    want = numpy.full(deep.size, NAN_INT)
    for q in range(n_lists):
        want[q * stride:q * stride + 2] = 0
    assert numpy.array_equal(deep, want)
    _check_table(P, D_Z, LT, nodes, name)
    if name == "narrow":                                    # nodes 0, 1 and the midpoint see zero
        assert numpy.all(nodes[:3] == 0.0) and numpy.any(nodes[3:N] != 0.0)


@pytest.mark.parametrize("LT,n", [(6, 17), (9, 40)])
def test_cell_nodes_sets(dl, projs, LT, n):
    """k_cell_nodes_sets with 3 sets of different chi ranges, windows and D_z, in rows of
    cell_set_stride: each row's table as the single launch's (same bits), its list's count and
    head zeroed, and every other double of the buffer -- spectrum table, states, the list's
    entries, what lies between the rows -- keeps its NaN bytes."""
    sets = [projs["inside"], projs["growth_ends"], projs["overhang"]]
    D = numpy.array([0.77, 0.61, 0.93])
    stride = c.set_stride(n, LT)
    N = (1 << LT) + 1
    deep_at = 3 * N + c.PTAB_N + 1 + n * c.ROMBERG_DUMP
    pdv = numpy.concatenate([P.pdv for P in sets])
    tab = numpy.concatenate([P.tab for P in sets])
    buf = numpy.zeros(3 * stride)
    call(dl, "dl_nodes_sets", 50, 100, 3, ptr(pdv), ptr(tab), ptr(D), LT, n, ptr(buf))
    for y, P in enumerate(sets):
        row = buf[y * stride:(y + 1) * stride]
        _check_table(P, D[y], LT, row[:3 * N], "set %d" % y)
        single = numpy.zeros(3 * N)
        one = numpy.zeros(2, dtype=numpy.int32)
        call(dl, "dl_nodes", 50, 100, ptr(P.pdv), ptr(P.tab), float(D[y]), LT, 1, 2, 0, ptr(single),
             _ip(one))
        assert numpy.array_equal(_bits(row[:3 * N]), _bits(single)), y
        rest = _bits(row[3 * N:]).copy()
        head = row[deep_at:deep_at + 1].view(numpy.int32)
        assert list(head) == [0, 0], y
        rest[deep_at - 3 * N] = NAN_BITS
        assert numpy.all(rest == NAN_BITS), y
    assert stride == 3 * N + c.epoch_stride(n)


# -------------------------------------------------------------------------------------------
# 8. spline_build_pcr, spline_build_staged
# -------------------------------------------------------------------------------------------
BAR = 2e-13                             # [project] test_hostmath.py::test_notaknot_spline


@pytest.fixture(scope="module")
def hc():
    return hostcheck_build.load()


_FAMILY = {}


def _family(name, n):
    """(x, y, reference pieces, 500 points, reference values, scale, bar), computed once."""
    if (name, n) not in _FAMILY:
        x, y = c.family(name, n)
        x, y = numpy.ascontiguousarray(x, dtype=float), numpy.ascontiguousarray(y, dtype=float)
        pp = c.nak_pp(x, y)
        xe = numpy.linspace(x[0], x[-1], 500)
        ref = c.pp_eval(x, pp, xe)
        scale = float(numpy.max(numpy.abs(y)))
        if name == "cubic":             # the reference: the polynomial itself
            t = (xe.astype(LD) - LD(x[0])) / (LD(x[-1]) - LD(x[0]))
            exact = LD(c.CUBIC[0]) + t * (LD(c.CUBIC[1]) + t * (LD(c.CUBIC[2]) + t * LD(c.CUBIC[3])))
            assert float(numpy.max(numpy.abs(ref - exact))) / scale < 1e-14
            ref = exact
        fit = InterpolatedUnivariateSpline(x, y, k=3)(xe)
        fit_err = float(numpy.max(numpy.abs(fit.astype(LD) - ref))) / scale
        # [measured] 4 x FITPACK's fp64 error against the same reference, floor the [project] bar
        _FAMILY[(name, n)] = (x, y, pp, xe, ref, scale, max(BAR, 4 * fit_err), fit_err)
    return _FAMILY[(name, n)]


def _spline_errors(x, coef, pp, xe, ref, scale):
    """Of device coefficients [n - 1, 4]: the 500 values (evaluated in long double) and the
    coefficients, each scaled by its interval's width to its contribution, over the scale."""
    ev = float(numpy.max(numpy.abs(c.pp_eval(x, coef, xe) - ref))) / scale
    h = numpy.diff(x).astype(LD)[:, None] ** numpy.arange(4)[None, :]
    return ev, float(numpy.max(numpy.abs(coef.astype(LD) - pp) * h)) / scale


def _run_spline(dl, staged, xs, ys, mask, threads):
    n_sys, n = xs.shape
    out = numpy.zeros((n_sys, n - 1, 4))
    call(dl, "dl_spline", staged, ptr(numpy.ascontiguousarray(xs)), ptr(numpy.ascontiguousarray(ys)),
         n, n_sys, mask, threads, ptr(out))
    return out


@pytest.mark.parametrize("n", c.SPLINE_NS)
def test_spline_build_pcr(dl, hc, n):
    """spline_build_pcr, one system on 64 threads (rows strided by 64 beyond n = 64; 5, 31, 50, 63,
    65, 100: no power of two, so the last reduction step reaches past both ends), for every knot
    family: the 500 values within the bar -- [measured] 4 x FITPACK's fp64 error against the same
    long-double solve, floor [project] 2e-13 of the table's scale -- and so are the coefficients,
    each scaled by its interval's width to its contribution.  The host emulation
    hc_spline_pcr is printed beside the device.  A block of 256 threads gives the same bits."""
    worst = 0.0
    for name in c.FAMILIES:
        x, y, pp, xe, ref, scale, bar, fit_err = _family(name, n)
        coef = _run_spline(dl, 0, x[None, :], y[None, :], 1, 64)[0]
        assert not numpy.isnan(coef).any(), name
        ev, ce = _spline_errors(x, coef, pp, xe, ref, scale)
        host = numpy.empty(xe.size)
        hc.hc_spline_pcr(ptr(x), ptr(y), n, ptr(xe), xe.size, ptr(host))
        host_err = float(numpy.max(numpy.abs(host.astype(LD) - ref))) / scale
        print("spline_build_pcr n %d %s: values %.3g coefficients %.3g (host emulation %.3g, "
              "FITPACK fp64 %.3g); bar %.3g" % (n, name, ev, ce, host_err, fit_err, bar))
        assert ev <= bar and ce <= bar, name
        worst = max(worst, ev / bar, ce / bar)
    wide = _run_spline(dl, 0, x[None, :], y[None, :], 1, 256)[0]
    assert numpy.array_equal(_bits(wide), _bits(coef))
    print("spline_build_pcr n %d: largest measured / bound %.3g" % (n, worst))


@pytest.mark.parametrize("n,n_sys,mask", [(8, 3, 0b101), (50, 3, 0b111), (50, 3, 0b011),
                                          (100, 3, 0b110), (128, 3, 0b101), (100, 2, 0b11),
                                          (5, 2, 0b10), (65, 4, 0b1011)])
def test_spline_build_staged(dl, n, n_sys, mask):
    """spline_build_staged with one system per wavefront in lockstep: three in a 192-thread block
    (k_proj_me_splines), two in a 128-thread block (k_proj_window_splines), four in 256; a
    wavefront with `mine` false takes part in the barriers and writes nothing (its output keeps its
    NaN bytes).  Different families side by side, so that a wavefront reading another's LDS carve
    is a gross error; each system as the single build of it (same bits) and within its bar."""
    names = ("z_chi", "chi_z", "ln_k", "nu_lnm")[:n_sys]
    fams = [_family(nm, n) for nm in names]
    xs = numpy.array([f[0] for f in fams])
    ys = numpy.array([f[1] for f in fams])
    out = _run_spline(dl, 1, xs, ys, mask, 64 * n_sys)
    for s, (x, y, pp, xe, ref, scale, bar, _) in enumerate(fams):
        if not (mask >> s) & 1:
            assert numpy.all(_bits(out[s]) == NAN_BITS), s
            continue
        ev, ce = _spline_errors(x, out[s], pp, xe, ref, scale)
        print("spline_build_staged n %d system %d of %d (%s): values %.3g coefficients %.3g; bar %.3g"
              % (n, s, n_sys, names[s], ev, ce, bar))
        assert ev <= bar and ce <= bar, s
        single = _run_spline(dl, 0, x[None, :], y[None, :], 1, 64)[0]
        assert numpy.array_equal(_bits(out[s]), _bits(single)), s


# -------------------------------------------------------------------------------------------
# 2. - 6. the C_l chain: k_cell, k_cell4, the hand-over, k_cell_deep; the _epochs and _sets forms
# -------------------------------------------------------------------------------------------
from test_gpu_devpower import Case                               # noqa: E402
from devpower_ref import MM, GM, LIN, HALOFIT, EXTRAPOLATE, Knots                   # noqa: E402
import devpower_ref as r                                         # noqa: E402

_MAXIMA = {}


def _note(key, value):
    _MAXIMA[key] = max(_MAXIMA.get(key, 0.0), float(value))
    return _MAXIMA[key]


@pytest.fixture(scope="module")
def dw():
    return dcb.load("devpower")


@pytest.fixture(scope="module")
def fields():
    return dcb.epoch_fields(dcb.load("devphys"))


_POWER = {}


def _power(dw, fields, NK, bao, n_epoch=1, mode="mm"):
    """The spectrum side: test_gpu_devpower.py's Case on cell_pieces (epoch e's scaled by
    1 + 0.1 (e % 2): epochs A B A of two HODs on two cosmologies)."""
    key = (NK, bao, n_epoch, mode == "mm_ext")
    if key not in _POWER:
        logs = numpy.empty(2)
        call(dw, "dw_logs", r.K_MIN, r.K_MAX, ptr(logs))
        kn = Knots(NK, logs[0], logs[1])
        pieces = [c.cell_pieces(kn) * c.row_scale(e) for e in range(n_epoch)]
        cosmos = list(c.ROW_COSMOS[:n_epoch])
        tails = None
        if mode == "mm_ext":            # misc[3]: the continuous tail (the other four: GM / GG, unused)
            tails = [(c.Spec(kn, pieces[e], mode).tail0, 1.0, -1.0, 1.0, -1.0) for e in range(n_epoch)]
        _POWER[key] = Case(dw, fields, NK, bao, cosmos, [0.0] * n_epoch, pieces, tails=tails)
    return _POWER[key]


def _check_amplitude(C, spec, e=0):
    """The amplitude the references of P_lin h_a h_b, HaloFit and the tails rest on: the device's linear spectrum (k_power,
    CHOMP_P_LIN) against devcell_ref.PLIN_KMIN times the oracle's ratio, at twice the [project]
    bound (the device's and the oracle's)."""
    k = numpy.array([r.K_MIN, 0.03, 1.0, r.K_MAX, 3.0 * r.K_MAX])
    got = C.eval(LIN, k)[e]
    bound = 2 * c.P_LIN_BOUND[spec.bao]
    worst = float(numpy.max(numpy.abs(got / spec.plin(k).astype(float) - 1.0))) / bound
    print("linear spectrum against the recorded amplitude: %.3g of 2 x [project] %.1e"
          % (worst, c.P_LIN_BOUND[spec.bao]))
    assert worst <= 1.0


def _device_logs(dl, x):
    x = numpy.ascontiguousarray(x, dtype=float)
    out = numpy.empty(x.size)
    call(dl, "dl_logs", ptr(x), x.size, ptr(out))
    return out


def _run(dl, C, L, ell, projs, D, form=0, rows=1):
    """dl_cell of one launch: (out1, buf1, out2, buf2, layout)."""
    n, N = ell.size, (1 << L["LT"]) + 1
    stride = c.set_stride(n, L["LT"]) if form == 2 else c.epoch_stride(n)
    total = (0 if form == 2 else 3 * N) + stride * rows
    out1, out2 = numpy.full(n * rows, numpy.nan), numpy.full(n * rows, numpy.nan)
    buf1, buf2 = numpy.full(total, numpy.nan), numpy.full(total, numpy.nan)
    which = {"mm": MM, "mm_ext": MM | EXTRAPOLATE, "hf_gm": GM | HALOFIT, "hf_mm": MM | HALOFIT}[L["mode"]]
    pdv = numpy.concatenate([P.pdv for P in projs])
    tab = numpy.concatenate([P.tab for P in projs])
    D = numpy.ascontiguousarray(D, dtype=float)
    call(dl, "dl_cell", *C.head(max(rows, 1)), which, int(L["bao"]), projs[0].NC, projs[0].NWp,
         len(projs), ptr(pdv), ptr(tab), ptr(D), ptr(ell), n, c.TOL, L["rtol"], L["divmax"], L["LT"],
         L["split"], L["kind"], int(L["use_ptab"]), form, rows, L["blocks"], ptr(out1), ptr(buf1),
         ptr(out2), ptr(buf2))
    return out1, buf1, out2, buf2, (n, N, stride)


def _row(buf, lay, form, y):
    """Row y of a work buffer: (node table, P(k), states [n, 34], list ints, what lies behind)."""
    n, N, stride = lay
    if form == 2:
        row = buf[y * stride:(y + 1) * stride]
        nodes, slab = row[:3 * N], row[3 * N:]
    else:
        nodes, slab = buf[:3 * N], buf[3 * N + y * stride:3 * N + (y + 1) * stride]
    pk = slab[:c.PTAB_N + 1]
    state = slab[c.PTAB_N + 1:c.PTAB_N + 1 + n * c.ROMBERG_DUMP].reshape(n, c.ROMBERG_DUMP)
    ints = slab[c.PTAB_N + 1 + n * c.ROMBERG_DUMP:].view(numpy.int32)
    return nodes, pk, state, ints


def _over(got, ref, bound):
    """|got - ref| / bound; a bound of 0 (all-zero nodes) asks for the value exactly."""
    if bound == 0:
        assert LD(got) == ref, (got, ref)
        return 0.0
    return abs(float(LD(got) - ref)) / bound


def _check_row(case, L, T, out1, row1, out2, row2, tag):
    """One row of one launch against the reference (see the module's tests for what is held)."""
    n, split, divmax = case.ell.size, L["split"], L["divmax"]
    hand = split < divmax
    full = [case.reference(T, il) for il in range(n)]
    first = [case.reference(T, il, upto=split) for il in range(n)]
    worst = 0.0
    for il in range(n):
        ref = first[il]
        worst = max(worst, _over(out1[il], ref["value"], ref["bound"]))   # (all-zero nodes: exactly 0)
    _, _, state, ints = row1
    want = sorted(il for il in range(n) if not first[il]["converged"])
    w_state = w_sum = 0.0
    if hand:
        assert ints[0] == len(want) and ints[1] == 0, (tag, ints[:2], len(want))
        assert sorted(ints[2:2 + ints[0]].tolist()) == want, tag
        assert numpy.all(ints[2 + ints[0]:] == NAN_INT), tag      # behind the count: NaN bytes
        for il in want:
            ref, st = first[il], state[il]
            for m in range(split + 1):
                w_state = max(w_state, _over(st[m], ref["T"][m], ref["T_bounds"][m]))
            assert numpy.all(st[split + 1:32] == 0.0), (tag, il)
            w_sum = max(w_sum, _over(st[32], ref["ordsum"][split], ref["ordsum_bounds"][split]))
            w_state = max(w_state, _over(st[33], ref["rows"][split], ref["row_bounds"][split]))
    else:
        assert list(ints[:2]) == [0, 0] and numpy.all(ints[2:] == NAN_INT), tag
        assert numpy.all(_bits(state) == NAN_BITS), tag           # no hand-over: no state written
    w_deep = 0.0
    if hand and L["blocks"]:
        ints2 = row2[3]
        for il in range(n):
            if il in want:
                ref = full[il]
                w_deep = max(w_deep, _over(out2[il], ref["value"], ref["bound"]))
            else:                                                 # unlisted: unchanged, bit for bit
                assert _bits(out2[il:il + 1])[0] == _bits(out1[il:il + 1])[0], (tag, il)
        assert ints2[0] == len(want) and len(want) <= ints2[1] <= len(want) + L["blocks"], (tag, ints2[:2])
        assert numpy.array_equal(ints2[2:], ints[2:]), tag
        assert numpy.array_equal(_bits(row2[2]), _bits(state)), tag   # the states: read only
    print("%s: first kernel %.3g of its bound, states %.3g, node sums %.3g, k_cell_deep %.3g; listed "
          "%d of %d; levels %s" % (tag, worst, w_state, w_sum, w_deep, len(want), n,
                                   " ".join(("%d" if f["converged"] else "X%d") % f["level"] for f in full)))
    assert worst <= 1.0 and w_state <= 1.0 and w_sum <= 1.0 and w_deep <= 1.0, tag
    for key, v in (("value", worst), ("state rows", w_state), ("node sum", w_sum), ("k_cell_deep", w_deep)):
        _note(key, v)
    print("maxima so far, measured / bound: %s" % ", ".join("%s %.3g" % kv for kv in sorted(_MAXIMA.items())))


def _tables(dl, case, nodes, pk):
    N = (1 << case.LT) + 1
    x = _device_logs(dl, numpy.concatenate([[r.K_MIN, r.K_MAX], case.ell]))
    return c.Tables(case.LT, nodes[:N], nodes[N:2 * N], nodes[2 * N:3 * N],
                    pk if case.use_ptab else None, x[0], x[1], x[2:])


@pytest.mark.parametrize("name", list(c.LAUNCHES))
def test_cell_launch(dl, dw, fields, projs, name):
    """One launch of devcell_ref.LAUNCHES: k_cell<HF, BAO, DIRECT> or k_cell4<HF, BAO> to `split`
    and, with a hand-over, k_cell_deep on the listed multipoles.  The reference replays
    scipy.integrate.romberg's rows in long double on node values formed from the tables read back
    -- lagrange6 of the spectrum table at the device's own u_j times F_j; at_ln's restatement where
    from_table declines; eval_t's restatement times the restated windows and growth beyond LT --
    so an error in k_cell_nodes or k_cell_ptab is the first tests' and test_gpu_devpower.py's, and
    this one isolates the integration, the indexing and the hand-over.  Held, per multipole:
    the first kernel's value at the reference's level (or at `split`); with a hand-over the list's
    count and set, NaN bytes behind the count, every listed state row (T_m for m <= split, exactly
    0 above, the node sum, the last row's value); after k_cell_deep the listed values at the
    reference's level, the unlisted bit for bit as before, count <= head <= count + blocks, the
    list and the states unchanged.  Bounds: [derived] 2 x 17 U sum |q_m L_m(t)| |F_j| per table
    node, [project] at_ln's and eval_t's bounds elsewhere, carried through the rows by
    sum_m |C[i][m]|, plus [project] 16 eps |b - a| mean |f| for the rows.  test_devcell_cpu.py
    shows that the value pins the level for every multipole here."""
    L = dict(zip(c.FIELDS, c.LAUNCHES[name]))
    C = _power(dw, fields, L["NK"], L["bao"], mode=L["mode"])
    case, L = c.launch(name, kn=C.kn, pieces=C.pieces[0], projs=projs)
    _check_amplitude(C, case.spec)
    out1, buf1, out2, buf2, lay = _run(dl, C, L, case.ell, [case.proj], [case.D_z])
    row1, row2 = _row(buf1, lay, 0, 0), _row(buf2, lay, 0, 0)
    if not case.use_ptab:
        assert numpy.all(_bits(row1[1]) == NAN_BITS)              # no spectrum table was built
    T = _tables(dl, case, row1[0], row1[1])
    _check_row(case, L, T, out1, row1, out2, row2, name)


@pytest.mark.parametrize("form,name", c.ROW_RUNS)
def test_cell_rows(dl, dw, fields, projs, form, name):
    """The _epochs (form 1) and _sets (form 2) kernels with 3 rows -- epochs A B A of two
    cosmologies and HODs; sets of different chi ranges, windows and D_z -- against three single
    launches: the values bit for bit after both kernels, the lists as sets, the listed states bit
    for bit; and row y against the reference as the single launches are."""
    L = dict(zip(c.FIELDS, c.LAUNCHES[name]))
    C = _power(dw, fields, L["NK"], 0, n_epoch=3)
    cases = [c.row_case(form, name, y, kn=C.kn, pieces=C.pieces[y], projs=projs)[0] for y in range(3)]
    ell = cases[0].ell
    sets = [cs.proj for cs in cases] if form == 2 else [cases[0].proj]
    Ds = [cs.D_z for cs in cases] if form == 2 else [cases[0].D_z]
    out1, buf1, out2, buf2, lay = _run(dl, C, L, ell, sets, Ds, form=form, rows=3)
    n = ell.size
    for y, case in enumerate(cases):
        _check_amplitude(C, case.spec, y)
        one = Case(dw, fields, L["NK"], 0, [c.ROW_COSMOS[y]], [0.0], [C.pieces[y]])
        s1, sb1, s2, sb2, slay = _run(dl, one, L, ell, [case.proj], [case.D_z])
        a1, a2 = _row(buf1, lay, form, y), _row(buf2, lay, form, y)
        b1, b2 = _row(sb1, slay, 0, 0), _row(sb2, slay, 0, 0)
        assert numpy.array_equal(_bits(out1[y * n:(y + 1) * n]), _bits(s1)), (form, name, y)
        assert numpy.array_equal(_bits(out2[y * n:(y + 1) * n]), _bits(s2)), (form, name, y)
        assert numpy.array_equal(_bits(a1[0]), _bits(b1[0]))      # the node table
        assert numpy.array_equal(_bits(a1[1]), _bits(b1[1]))      # P(k)
        assert a1[3][0] == b1[3][0] and sorted(a1[3][2:2 + a1[3][0]]) == sorted(b1[3][2:2 + b1[3][0]])
        assert numpy.all(a1[3][2 + a1[3][0]:] == NAN_INT)
        for il in a1[3][2:2 + a1[3][0]]:
            assert numpy.array_equal(_bits(a1[2][il]), _bits(b1[2][il])), (form, name, y, il)
        T = _tables(dl, case, a1[0], a1[1])
        _check_row(case, L, T, out1[y * n:(y + 1) * n], a1, out2[y * n:(y + 1) * n], a2, case.name)
    assert not numpy.array_equal(out2[:n], out2[n:2 * n])
    if form == 1:                                                 # A B A: rows 0 and 2 alike
        assert numpy.array_equal(_bits(out2[:n]), _bits(out2[2 * n:]))
