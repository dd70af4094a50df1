"""tests/devcheck/devspline.hip without a GPU: it compiles for the device with the product's flags
(hipcc cross-compiles, nothing is launched), and its entry point refuses what its buffers and the
one-wavefront builder are not sized for before it touches the device.  The builder's
host-callable parts (spline_row, pcr_step, spline_coef) are run under the sanitizers by
tests/hostcheck/hostcheck.cpp; the builder itself is device code only."""
import ctypes

import pytest

import devcheck_build as dcb

dcb.HARNESSES.setdefault("devspline", dcb.Harness("devspline"))
needs_hipcc = pytest.mark.skipif(not dcb.have_hipcc(), reason="hipcc is not installed")


@needs_hipcc
def test_harness_builds_and_refuses():
    L = ctypes.CDLL(dcb.build(harness="devspline"))
    assert L.ds_wave_max() == 64
    _p = dcb.c_double_p
    L.ds_build.argtypes = [_p, _p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _p, _p]
    null = _p()
    for n, n_sys, tps in ((3, 1, 64), (65, 1, 64), (50, 0, 64), (50, 3, 64), (50, 1, 32)):
        assert L.ds_build(null, null, n, n_sys, tps, null, null) == -1, (n, n_sys, tps)
