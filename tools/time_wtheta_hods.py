"""Measurement aid (GPU box): w(theta) at the 33 binned theta of the G6 set-up (galaxy x galaxy
windows, power_gg) for N seeded HODs, by Correlation.correlation_hods (one batch) and by the loop
set_hod + correlation over the same HODs (the route that existed before the batch) -- in one
process, alternating the two, each window a host clock around calls that end with their results
on the host (a device synchronise).

    python tools/time_wtheta_hods.py [--n 64 512] [--repeats 5] [--window 0.5] [--chunk E] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_wtheta_hods.py --count batched --n 64
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_wtheta_hods.py --count loop --n 64

--count MODE runs MODE exactly once over N HODs and nothing else.  The launches per point are not
counted here: they are the dispatches in that trace's kernel_stats.csv, less those of --count
setup (the same process without the evaluation), over N.  Prints one JSON line; --out also writes
it to a file.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D2R = numpy.pi / 180.0


def hods(n, seed=20):
    """n Zheng HODs around the Zehavi values, M_0 tied to M_min."""
    rng = numpy.random.RandomState(seed)
    out = []
    for _ in range(n):
        m = rng.uniform(11.9, 12.4)
        out.append({"log_M_min": m, "sigma": rng.uniform(0.1, 0.4), "log_M_0": m,
                    "log_M_1p": rng.uniform(13.1, 13.8), "alpha": rng.uniform(0.9, 1.2)})
    return out


def correlation_object():
    from chomp_amd import correlation, cosmology, halo, kernel
    cm = cosmology.MultiEpoch(0.0, 5.0)
    wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    wb = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    kern = kernel.Kernel(1e-6 * D2R, 100.0 * D2R, wa, wb, cm)
    return correlation.Correlation(0.001, 1.0, kern, input_halo=halo.Halo(0.0), power_spec="power_gg")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--chunk", type=int, help="CHOMP_TUNE_WTHETA_EPOCH_CHUNK of the batched call")
    ap.add_argument("--count", choices=["batched", "loop", "setup"])
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    warnings.simplefilter("ignore")
    theta = numpy.logspace(-3, 0, 33) * D2R
    batch, loop = correlation_object(), correlation_object()

    def run_batched(hs):
        return batch.correlation_hods(theta, hs)

    def run_loop(hs):
        rows = []
        for h in hs:
            loop.set_hod(h)
            rows.append(loop.correlation(theta))
        return numpy.array(rows)

    if args.count:
        hs = hods(args.n[0])
        if args.count == "setup":
            batch.kernel._setup_on(batch.halo._context())
            batch.halo._context().sync()
        else:
            (run_batched if args.count == "batched" else run_loop)(hs)
        print(json.dumps({"count": args.count, "n_hod": len(hs)}))
        return
    result = {"what": "host seconds of w(theta) at 33 theta for n_hod HODs, results on the host",
              "device": torch.cuda.get_device_name(0), "n_theta": int(theta.size),
              "epoch_chunk": args.chunk or "default", "runs": []}
    for n in args.n:
        hs = hods(n)
        t0 = time.perf_counter(); a = run_batched(hs); tb = time.perf_counter() - t0   # warm-up
        if args.chunk:        # (the grid of this n exists from here on: set the knob once)
            from chomp_amd import _lib
            batch._hods_grid[1].ctx.set_tuning(_lib.TUNE_WTHETA_EPOCH_CHUNK, args.chunk)
            a = run_batched(hs)
        t0 = time.perf_counter(); b = run_loop(hs); tl = time.perf_counter() - t0
        t0 = time.perf_counter(); run_batched(hs); tb = time.perf_counter() - t0       # warm
        t0 = time.perf_counter(); run_loop(hs); tl = time.perf_counter() - t0
        inner = {"batched": max(1, int(numpy.ceil(args.window / tb))),
                 "loop": max(1, int(numpy.ceil(args.window / tl)))}
        times = {"batched": [], "loop": []}
        for _ in range(args.repeats):                     # alternating
            for name, fn in (("batched", run_batched), ("loop", run_loop)):
                t0 = time.perf_counter()
                for _ in range(inner[name]):
                    fn(hs)
                times[name].append((time.perf_counter() - t0) / inner[name])
        run = {"n_hod": n, "calls_per_window": inner,
               "max_rel_diff_batched_vs_loop": float(numpy.max(numpy.abs(a / b - 1)))}
        for name in ("batched", "loop"):
            t = numpy.array(times[name])
            run[name] = {"seconds_per_call_median": float(numpy.median(t)),
                         "seconds_per_call_min": float(t.min()), "seconds_per_call_max": float(t.max()),
                         "microseconds_per_point_median": float(numpy.median(t) / n * 1e6),
                         "all": [float(x) for x in t]}
        run["loop_over_batched"] = run["loop"]["seconds_per_call_median"] / run["batched"]["seconds_per_call_median"]
        result["runs"].append(run)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
