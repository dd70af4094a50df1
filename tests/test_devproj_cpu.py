"""The host-side restatements tests/test_gpu_devproj.py measures the device against, checked
without a GPU: the index arithmetic of the w(theta) moment route over the shapes the GPU tests
use (every part count and the segment lengths they are meant to reach), and the Romberg rows
against oracle/romberg.py itself."""
import warnings

import numpy

import test_gpu_devproj as t
from oracle import romberg as oracle_romberg


def test_shapes_cover_every_part_count():
    """The shapes of the moment tests reach every part count 0 (empty: shallow levels with
    nseg > n) .. 8 (capped) and segment lengths on both sides of multiples of kWthItems and of a
    tile of 256 kWthItems nodes (restated index arithmetic; no launch)."""
    counts, lengths = set(), set()
    for nseg in t.NSEGS:
        for lev in range(1, t.LT + 1):
            st = t.seg_starts(lev, nseg)
            assert st[0] == 0 and st[-1] == 1 << (lev - 1) and numpy.all(numpy.diff(st) >= 0)
            # the two statements of membership agree on every segment's first and last node
            for m in range(nseg):
                if st[m + 1] > st[m]:
                    assert t.seg_of(int(st[m]), lev, nseg) == m
                    assert t.seg_of(int(st[m + 1]) - 1, lev, nseg) == m
            for length in numpy.diff(st):
                counts.add(t.part_count(int(length)))
                lengths.add(int(length))
                assert sum(p1 - p0 for p0, p1 in t.part_bounds(0, int(length))) == length
    print("part counts", sorted(counts))
    assert {0, 1, 2, 8} <= counts
    assert counts == set(range(t.PARTS + 1)), counts
    assert {l % t.ITEMS for l in lengths} == set(range(t.ITEMS))
    assert t.TILE in lengths and 2 * t.TILE in lengths
    assert any(t.TILE < l < t.TILE + 128 for l in lengths)
    assert any(t.TILE - 128 < l < t.TILE for l in lengths)
    assert any(l > t.PARTS * t.TILE and l % t.TILE for l in lengths)      # (capped, ragged tiles)


def test_rows_restatement_is_the_oracles():
    """t.romberg_rows_value against oracle/romberg.py itself, fed the same level sums (no launch):
    with tol = rtol = 0 its stopping test `err < tol or err < rtol |result|` never holds -- a zero
    error does not count as converged, as in RombergRows2::advance -- and all levels are run.
    [derived] 64 2^-52 of range x sum |S_l|: nine rows of at most nine extrapolations each, in
    fp64 on the oracle's side."""
    rng = numpy.random.default_rng(5)
    sums = rng.normal(size=9)
    e0, e1 = 0.3, -1.1
    it = iter(sums)

    def f(x):
        if numpy.isscalar(x):
            return e0 if x == -2.0 else e1
        out = numpy.zeros(len(x))
        out[0] = next(it)
        return out

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", oracle_romberg.AccuracyWarning)
        v, level = oracle_romberg.romberg(f, -2.0, 3.0, tol=0.0, rtol=0.0, divmax=9, vec_func=True,
                                          return_level=True)
    mine = float(t.romberg_rows_value(5.0, 0.5 * (e0 + e1), sums))
    assert level == 9 and abs(v - mine) <= 64 * t.EPS * numpy.sum(numpy.abs(sums)) * 5.0
