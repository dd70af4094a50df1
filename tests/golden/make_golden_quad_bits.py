#!/usr/bin/env python3
"""Generate tests/golden/g27_i_0_4_quad_bits.npz: the values and Romberg levels that
HaloTrispectrumOneHalo's quadruple kernel (k_tri1h_quad) gave on the MI355X at the G24 quadruples
BEFORE the kernel took its arity parameter -- run with the package of the commit that precedes
HaloTrispectrum, on the device.  tests/test_gpu_trispectrum.py asserts the same bits since.

    python tests/golden/make_golden_quad_bits.py
"""
import os
import sys

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CASES = (("z000_mmmm", 0.0, "power_mmmm"), ("z050_mmmm", 0.5, "power_mmmm"),
         ("z030_gggg", 0.3, "power_gggg"))


def main():
    from chomp_amd import _lib, halo_trispectrum
    quads = numpy.load(os.path.join(HERE, "g24_trispectrum_one_halo.npz"))["quads"]
    out = {"quads": quads}
    for tag, z, spec in CASES:
        h = halo_trispectrum.HaloTrispectrumOneHalo(z, power_spec=spec)
        v, lev = h._sync(0).tri1h_quad(_lib.TRI_MOMENT[spec], quads, 0, levels=True)
        out[tag + "_value"], out[tag + "_level"] = v, lev
    numpy.savez(os.path.join(HERE, "g27_i_0_4_quad_bits.npz"), **out)


if __name__ == "__main__":
    main()
