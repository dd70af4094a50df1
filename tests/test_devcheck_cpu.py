"""The device harness of the fp64 primitives and the wavefront Romberg (tests/devcheck) compiles
for gfx950 against the current headers and exports every entry point the GPU tests
(test_gpu_devmath.py, test_gpu_romberg.py) use.  No GPU is needed: hipcc cross-compiles.  This
keeps the harness from rotting when a header's signature changes in a change developed without
a GPU."""
import ctypes

import pytest

import devcheck_build


@pytest.mark.skipif(not devcheck_build.have_hipcc(), reason="hipcc is not installed")
def test_devcheck_compiles_and_exports():
    path = devcheck_build.build()
    assert devcheck_build.build() == path                     # (second call: nothing to do)
    with open(devcheck_build.HASH) as f:
        assert f.read().strip() == devcheck_build.source_hash()
    L = ctypes.CDLL(path)
    for name in devcheck_build.ENTRY_POINTS:
        assert hasattr(L, name), name
    # the getters run on the host
    L.dc_case_stride.restype = ctypes.c_int
    assert L.dc_case_stride() == 16 and L.dc_out_stride() == 8
    assert L.dc_index_out_stride() == 3 * 34 + 2
    assert L.dc_fma_k_count() == 6
    # the flags are the product's, not a copy
    from chomp_amd import _lib
    assert devcheck_build.flags() == _lib.HIPCC_FLAGS + _lib.NO_LICM
