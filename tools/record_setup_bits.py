#!/usr/bin/env python
"""Record tests/golden/setup_bits.npz: what the set-ups of tests/test_gpu_setup_bits.py hand
back through the C API, on the commit whose bits are to be kept (run it there, on the GPU):

    python tools/record_setup_bits.py [out.npz]

Digests for the large arrays, values for the small ones; see the test for what is taken.
"""
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import test_gpu_setup_bits as t
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    rec = {}
    for name in sorted(t.CASES):
        got = t.measure(name)
        t.check_shape(name, got)
        again = t.measure(name)
        for key, v in got.items():
            same = v == again[key] if isinstance(v, str) else v.tobytes() == again[key].tobytes()
            assert same, "%s/%s differs between two runs" % (name, key)
            rec[name + "/" + key] = numpy.array(v)
        print(name, "status", got["status"][:4], "deep", got["deep_stats"], flush=True)
    numpy.savez(out, **rec)
    print("wrote", out, len(rec), "entries")


if __name__ == "__main__":
    main()
