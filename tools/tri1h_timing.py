#!/usr/bin/env python3
"""Workload for timing HaloTrispectrumOneHalo on the device: one I_0^4 table set-up
(k_tri1h_table + k_tri1h_bicubic) for 1 and for 64 epochs, and N = 2^16 quadruples
(k_tri1h_quad) already in HBM.  Run it under the profiler, with a time limit, e.g.

    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \\
        python tools/tri1h_timing.py

and read k_tri1h_table, k_tri1h_bicubic and k_tri1h_quad from the kernel statistics (each
timed launch runs REPEATS times after one warm-up).  Also prints the host-timed cost of each
(events around the launches)."""
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from chomp_amd import _lib, cosmology, defaults, hod  # noqa: E402

N = 1 << 16
REPEATS = 5


def timed(ctx, fn):
    fn()                                                 # (warm-up)
    ctx.sync()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr)
    t0.record(stream)
    for _ in range(REPEATS):
        out = fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / REPEATS, out


def main():
    torch.cuda.init()
    prof = defaults.default_halo_dict
    ctx = cosmology._context()
    for n_epoch in (1, 64):
        ctx.epochs_set(defaults.default_cosmo_dict, numpy.linspace(0.0, 2.0, n_epoch))
        ctx.stage_k(prof, _lib.MF_ST, prof, hod.HODZheng(), 0)
        ms, _ = timed(ctx, lambda: ctx.tri1h_setup(_lib.TRI_MOMENT["power_mmmm"], 0, n_epoch))
        tab, lev = ctx.tri1h_setup(0, 0, n_epoch, copy_out=True)
        print("table set-up  epochs %3d  %.3f ms  (%.3f ms per epoch)  levels %d..%d  status %s"
              % (n_epoch, ms, ms / n_epoch, lev.min(), lev.max(),
                 numpy.unique(ctx.status(0, n_epoch)).tolist()))
    rng = numpy.random.default_rng(1)
    k = torch.from_numpy(10.0 ** rng.uniform(-3, 2, (N, 4))).cuda()
    ms, out = timed(ctx, lambda: ctx.tri1h_quad(0, k, 0))
    print("quadruples    N %d  %.3f ms  %.3g quadruples / s  finite %.3f"
          % (N, ms, N / (ms * 1e-3), float(torch.isfinite(out).double().mean())))


if __name__ == "__main__":
    main()
