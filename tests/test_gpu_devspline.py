"""The one-wavefront not-a-knot build (spline_build_pcr_wave, chomp_mass_kernels.h) against the
block builder it replaces where a table has at most 64 knots (spline_build_pcr): the same
spline_row / pcr_step / spline_coef calls per row in the same order, so the coefficients must
agree byte for byte -- no tolerance.  tests/devcheck/devspline.hip launches both on the same
knots: the knot families of tests/devcell_ref.py at n = 5, 31, 50, 63, 64 (one step of the
reduction; an odd size; the product's default; one short of a wavefront; a full wavefront), with
one and with two systems in the block, against both shapes the product calls the block builder
in (a system per wavefront; a system per 128 threads).  test_gpu_devcell.py holds the block
builder itself to the long-double solve.
"""
import ctypes

import numpy
import pytest

import devcheck_build as dcb
from devcheck_build import call, ptr
import devcell_ref as ref

_i, _p = ctypes.c_int, dcb.c_double_p
dcb.HARNESSES.setdefault("devspline", dcb.Harness("devspline"))
dcb.ALL_ENTRY_POINTS.setdefault("devspline", {"ds_wave_max": [], "ds_build": [_p, _p, _i, _i, _i, _p, _p]})
dcb.VOID.setdefault("devspline", ())

NS = (5, 31, 50, 63, 64)
# two systems in one block: the pairs the mass tables build side by side, and two unlike ones
PAIRS = (("lnm_nu", "nu_lnm"), ("ln_k", "cubic"), ("z_chi", "chi_z"), ("window", "de_ln_a"))


@pytest.fixture(scope="module")
def lib():
    return dcb.load("devspline")


@pytest.fixture(scope="module")
def knots():
    """{(family, n): (x, y)}, computed once."""
    return {(f, n): ref.family(f, n) for f in ref.FAMILIES for n in NS}


def _both(lib, systems, tps):
    n = systems[0][0].size
    x = numpy.ascontiguousarray(numpy.concatenate([s[0] for s in systems]), dtype=numpy.float64)
    y = numpy.ascontiguousarray(numpy.concatenate([s[1] for s in systems]), dtype=numpy.float64)
    cb = numpy.zeros(len(systems) * 4 * (n - 1))
    cw = numpy.zeros_like(cb)
    call(lib, "ds_build", ptr(x), ptr(y), n, len(systems), tps, ptr(cb), ptr(cw))
    return cb, cw


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_wave_build_is_the_block_build(lib, knots, n):
    assert lib.ds_wave_max() == 64
    for tps in (64, 128):
        for f in ref.FAMILIES:
            cb, cw = _both(lib, [knots[f, n]], tps)
            assert numpy.all(numpy.isfinite(cb)), (f, n, tps)
            assert cb.tobytes() == cw.tobytes(), (f, n, tps)
        for fa, fb in PAIRS:
            cb, cw = _both(lib, [knots[fa, n], knots[fb, n]], tps)
            assert numpy.all(numpy.isfinite(cb)), (fa, fb, n, tps)
            assert cb.tobytes() == cw.tobytes(), (fa, fb, n, tps)
            # a system's coefficients do not depend on its neighbour
            one = _both(lib, [knots[fb, n]], tps)[1]
            assert cw[4 * (n - 1):].tobytes() == one.tobytes(), (fa, fb, n, tps)
