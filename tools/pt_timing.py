#!/usr/bin/env python3
"""Workload for timing PerturbationTheory (k_pt) and the MassFunctionSecondOrder set-up
(k_mass_b2) on the device.  Run it under the profiler, e.g.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/pt_timing.py

and read k_pt (one instance per form) and k_mass_b2 from the kernel statistics.  The PT launches
take N = 2^20 configurations already in HBM (torch tensors, no host copies) for 1 and 64 epochs
of one cosmology, for bispectrum_len, trispectrum_parallelogram and trispectrum, each REPEATS
times.  Also prints the host-timed rate of each (events around the launches)."""
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from chomp_amd import cosmology, defaults, mass_function  # noqa: E402

N = 1 << 20
REPEATS = 10
FORMS = ("bispectrum_len", "trispectrum_parallelogram", "trispectrum")


def configs(form, rng):
    if form == "bispectrum_len":
        a = numpy.concatenate([10.0 ** rng.uniform(-3, 1, (N, 3)), rng.uniform(-1, 1, (N, 3))], 1)
    elif form == "trispectrum_parallelogram":
        a = numpy.stack([10.0 ** rng.uniform(-3, 1, N), 10.0 ** rng.uniform(-3, 1, N),
                         rng.uniform(-1, 1, N)], 1)
    else:
        a = rng.normal(size=(N, 12)) * 0.3
    return torch.from_numpy(numpy.ascontiguousarray(a)).cuda()


def main():
    torch.cuda.init()
    rng = numpy.random.default_rng(1)
    ctx = cosmology._context()
    for n_epoch in (1, 64):
        ctx.epochs_set(defaults.default_cosmo_dict, numpy.linspace(0.0, 2.0, n_epoch))
        for form in FORMS:
            args = configs(form, rng)
            ctx.pt_eval(form, args, 0, n_epoch)          # (warm-up)
            ctx.sync()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream = torch.cuda.ExternalStream(ctx.stream_ptr)
            t0.record(stream)
            for _ in range(REPEATS):
                out = ctx.pt_eval(form, args, 0, n_epoch)
            t1.record(stream)
            t1.synchronize()
            ms = t0.elapsed_time(t1) / REPEATS
            print("%-26s epochs %3d  %.3f ms  %.3g configurations x epochs / s  finite %.3f" % (
                form, n_epoch, ms, N * n_epoch / (ms * 1e-3),
                float(torch.isfinite(out).double().mean())))
    # the second-order set-up: MassFunction vs MassFunctionSecondOrder, same cosmology
    for cls in (mass_function.MassFunction, mass_function.MassFunctionSecondOrder):
        for z in (0.0, 0.5, 1.0):
            mf = cls(z, cosmology.SingleEpoch(z))
            mf.f_norm
    print("bias_2_norm at z = 1:", mf.bias_2_norm, "level", mf._bias_2_level)


if __name__ == "__main__":
    main()
