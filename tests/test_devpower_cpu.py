"""tests/devpower_ref.py checked without a GPU: the k grids test_gpu_devpower.py runs meet the cap
on knot-band samples and reach every mechanism they advertise (from the reference's interval
indices alone: the GPU test cannot pass by never reaching a path), and the in-range restatement,
fed the oracle's knot tables of the default halo, is the oracle's power_gm / power_gg."""
import numpy
import pytest

import devpower_ref as r
from oracle import chomp_oracle as o

NKS = (8, 11)


def _all_grids(kn):
    for name in list(r.GRID_PATTERNS) + ["sorted"]:
        for nk in r.GRID_NKS:
            yield "%s/%d" % (name, nk), r.grid(kn, name, nk)
    for name in r.STREAM_SEQUENCE:
        yield "stream/" + name, r.stream_grid(kn, name)


@pytest.mark.parametrize("NK", NKS)
def test_grids_meet_the_band_cap(NK):
    """At most 2 % of a grid's samples lie within delta of an interior knot (where the test
    accepts either adjacent piece); the built grids keep 5 % of an interval off every knot, so
    only the log-spaced `sorted` grids can have any."""
    kn = r.Knots(NK)
    worst = 0.0
    for name, k in _all_grids(kn):
        n = r.band_count(kn, k)
        worst = max(worst, n / k.size)
        assert n <= 0.02 * k.size, (name, n)
        if not name.startswith("sorted"):
            assert n == 0, (name, n)
    print("largest share of knot-band samples: %.4f" % worst)


@pytest.mark.parametrize("NK", NKS)
def test_grids_reach_every_mechanism(NK):
    kn = r.Knots(NK)
    got = {}
    for name, k in _all_grids(kn):
        idxu, fast, two = r.classify(kn, k)
        got[name] = (int(numpy.sum(fast & ~two)), int(numpy.sum(fast & two)), int(numpy.sum(~fast)))
    # whole wavefronts in one interval; across exactly one knot; across two (off the fast path)
    for nk in (128, 512, 2562):
        full = nk // r.GROUP
        assert got["dense/%d" % nk][:2] == (full, 0)
        assert got["one_knot/%d" % nk][:2] == (0, full)
        assert got["two_knots/%d" % nk][:2] == (0, 0) and got["shuffled/%d" % nk][:2] == (0, 0)
        assert got["two_knots/%d" % nk][2] == (nk + r.GROUP - 1) // r.GROUP
    # a partial wavefront is never fast; odd and even row counts both occur
    for nk in (1, 2, 127, 129, 514):
        assert got["dense/%d" % nk][2] >= 1
    assert {nk % 2 for nk in r.GRID_NKS} == {0, 1}
    # one out-of-range or NaN k in an otherwise fast wavefront
    a, b, c = got["ragged/2562"]
    assert a >= 5 and b >= 3 and c >= 10
    k = r.grid(kn, "ragged", 2562)
    assert numpy.isnan(k).sum() >= 3 and (k > r.K_MAX).sum() >= 3 and (k < r.K_MIN).sum() >= 3
    # the log-spaced grid at 2562: fast wavefronts with and without a knot
    a, b, c = got["sorted/2562"]
    assert a >= 5 and b >= 5
    # every rotation of the start row, for every count of rows a block can walk
    for name in ("dense", "one_knot", "mixed", "sorted"):
        k = r.grid(kn, name, 2562)
        for cnt in (2, 3, 5):
            assert r.start_rows(kn, k, cnt) == set(range(cnt)), (name, cnt)
    # the linear spectrum never takes the fast path
    assert not r.classify(kn, r.grid(kn, "dense", 512), w=r.LIN)[1].any()
    # the parity sequence: many, few, none, many
    counts = [got["stream/" + n][2] for n in r.STREAM_SEQUENCE]
    print("slow groups per streaming call", counts, "of", r.STREAM_NK // r.GROUP)
    assert counts[0] >= 5 and 1 <= counts[1] <= 2 and counts[2] == 0 and counts[3] >= 10
    assert got["stream/dense_two"][1] >= 5 and got["stream/dense_two"][0] >= 5


def test_locate_and_band():
    """Knots.locate on the knots themselves and one ulp either side: the exact interval, and the
    band flags the interior ones (and only ln k within delta of a knot)."""
    kn = r.Knots(11)
    for j in range(1, kn.NK - 1):
        k0 = float(numpy.exp(kn.x[j]))
        for k in (numpy.nextafter(k0, 0.0), k0, numpy.nextafter(k0, numpy.inf)):
            lnk, idx, inr, alt = kn.locate([k])
            assert inr[0] and idx[0] in (j - 1, j) and {idx[0], alt[0]} == {j - 1, j}
        for k in (k0 * (1 - 1e-13), k0 * (1 + 1e-13)):
            lnk, idx, inr, alt = kn.locate([k])
            assert alt[0] == idx[0] == (j - 1 if k < k0 else j)
    lnk, idx, inr, alt = kn.locate([r.K_MIN, r.K_MAX, 0.5 * r.K_MIN, 2 * r.K_MAX, numpy.nan, 0.0, -1.0])
    assert list(inr) == [True, True, False, False, False, False, False]
    assert idx[0] == alt[0] == 0 and idx[1] == alt[1] == kn.NK - 2


def test_restatement_is_the_oracles_power():
    """in_range, fed the oracle's h_g, h_m, pp_gm, pp_gg splines of the default halo as piecewise
    cubics on the oracle's knots, against o.halo_power (halo.py:322-439) inside the range.  The
    oracle evaluates FITPACK B-splines in double and multiplies in double; [measured, reference
    side] its own rounding is sized as the largest difference between the double piecewise-cubic
    form and the B-spline form of the same splines, relative to the terms' sum, plus the [derived]
    bound in_range returns."""
    from scipy.interpolate import PPoly
    t = o.halo_table(families=("gm", "gg"))
    NK = t.ln_k.size
    kn = r.Knots(NK, t.ln_k[0], t.ln_k[-1])
    assert numpy.max(numpy.abs(kn.x - t.ln_k)) < 8 * r.EPS * abs(t.ln_k[0])
    kn.x = t.ln_k.copy()
    pp = numpy.zeros((6, NK - 1, 4))
    own = 0.0
    k = numpy.exp(numpy.linspace(t.ln_k[0] + 1e-3, t.ln_k[-1] - 1e-3, 397))
    for f, s in ((r.F_HM, t.h_m_spline), (r.F_HG, t.h_g_spline), (r.F_PPGM, t.pp_gm_spline),
                 (r.F_PPGG, t.pp_gg_spline)):
        P = PPoly.from_spline(s._eval_args)
        # FITPACK's knots: not-a-knot drops x[1] and x[-2]; re-expand each piece about its own knot
        for i in range(NK - 1):
            j = numpy.searchsorted(P.x, t.ln_k[i], side="right") - 1
            j = min(max(j, 3), P.c.shape[1] - 4)
            c = P.c[::-1, j].astype(r.LD)
            h = r.LD(t.ln_k[i]) - r.LD(P.x[j])
            pp[f, i] = [c[0] + h * (c[1] + h * (c[2] + h * c[3])), c[1] + h * (2 * c[2] + 3 * h * c[3]),
                        c[2] + 3 * h * c[3], c[3]]
        _, idx, _, _ = kn.locate(k)
        mine = r.poly(pp[f][idx], numpy.log(k.astype(r.LD)) - t.ln_k[idx].astype(r.LD))
        own = max(own, float(numpy.max(numpy.abs(mine - s(numpy.log(k))) / numpy.abs(s(numpy.log(k))))))
    print("piecewise-cubic form against the B-spline form: %.2e relative" % own)
    lnk, idx, inr, _ = kn.locate(k)
    assert inr.all()
    plin = o.linear_power(t.e, k)
    for w, name in ((r.GM, "gm"), (r.GG, "gg")):
        ref = o.halo_power(t, name, k)
        v, bound = r.in_range(w, 1.0, plin, pp, kn, lnk, idx)
        fa, fb, fp = r.families(w)
        terms = numpy.abs(plin * r.poly(pp[fa][idx], lnk - t.ln_k[idx]) *
                          r.poly(pp[fb][idx], lnk - t.ln_k[idx])) + \
            numpy.abs(r.poly(pp[fp][idx], lnk - t.ln_k[idx]))
        err = numpy.abs(v - ref).astype(float)
        tol = bound + 3 * own * terms.astype(float)
        print("P_%s: restatement against the oracle %.2e relative, %.3f of its bound"
              % (name, float(numpy.max(err / numpy.abs(ref))), float(numpy.max(err / tol))))
        assert numpy.all(err <= tol)
