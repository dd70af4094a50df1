"""Measurement aid (GPU box): xi(r) at the separations of Correlation3d(0.1, 50) (logspace(-1,
log10(50), n_r), default precision, the halo's own k range, power_gg, z = 0) for N seeded HODs on
ONE context -- a HaloGrid of one epoch per HOD, no projection set-up -- three ways, HIP-event
timed with device buffers:

    single  chomp_xi3d of epoch 0 (the call the batch reproduces bit for bit)
    loop    N chomp_xi3d calls, one per epoch
    batch   one chomp_xi3d_epochs call over the N epochs

    timeout -k 10 300 python tools/time_xi_hods.py [--n-hod 16] [--n-r 50] [--rounds 7] [--out FILE.json]
    timeout -k 10 300 python tools/time_xi_hods.py --tree build_exp/parent ...   (another checkout of
        the project, built; one without chomp_xi3d_epochs times single and loop only)
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_xi_hods.py --count batch

Every run is one process and one GPU step: give each its own time limit, as above, and start the
next only after the one before has ended well.

The modes alternate round by round; each figure is the median over the rounds, with the least and
the largest beside it (the spread a difference has to exceed).  --count MODE runs MODE once after
the set-up and nothing else (for a kernel trace).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import warnings

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hods(n, seed=20):
    """n Zheng HODs around the Zehavi values, M_0 tied to M_min (those of time_wtheta_hods.py)."""
    rng = numpy.random.RandomState(seed)
    out = []
    for _ in range(n):
        m = rng.uniform(11.9, 12.4)
        out.append({"log_M_min": m, "sigma": rng.uniform(0.1, 0.4), "log_M_0": m,
                    "log_M_1p": rng.uniform(13.1, 13.8), "alpha": rng.uniform(0.9, 1.2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-hod", type=int, default=16)
    ap.add_argument("--n-r", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=4, help="calls per timed window (single: x 4)")
    ap.add_argument("--tree", help="another checkout of the project, built, to time instead")
    ap.add_argument("--count", choices=["single", "loop", "batch"])
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.tree:                                # (another checkout, built: its package, its library)
        sys.path[0] = os.path.abspath(args.tree)
    from chomp_amd import _lib
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    warnings.simplefilter("ignore")
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    from chomp_amd import correlation, defaults, grid
    n = args.n_hod
    hg = grid.HaloGrid(numpy.zeros(n), hod_dict=hods(n))
    ctx = hg.ctx
    hg.setup("power_gg")
    flagged = int(numpy.count_nonzero(hg.status()))      # (set-ups that exhausted their divmax)
    code = correlation._POWER["power_gg"][0]
    k_min, k_max = defaults.default_limits["k_min"], defaults.default_limits["k_max"]
    r = torch.logspace(-1, float(numpy.log10(50.0)), args.n_r, dtype=torch.float64, device="cuda")
    have_batch = "chomp_xi3d_epochs" in _lib.EXPORTS

    modes = {"single": lambda: ctx.xi3d(code, 0, k_min, k_max, r),
             "loop": lambda: [ctx.xi3d(code, e, k_min, k_max, r) for e in range(n)]}
    if have_batch:
        modes["batch"] = lambda: ctx.xi3d_epochs(code, 0, n, k_min, k_max, r)
    if args.count:
        modes[args.count]()
        torch.cuda.synchronize()
        print(json.dumps({"count": args.count, "n_hod": n, "n_r": args.n_r}))
        return

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3          # microseconds per call

    result = {"what": "device microseconds per call (HIP events), xi(r) of n_r separations, power_gg",
              "device": torch.cuda.get_device_name(0), "tree": args.tree or "this one",
              "n_hod": n, "n_r": args.n_r, "rounds": args.rounds, "divmax": ctx.config.divmax,
              "hods_with_a_status_word": flagged}
    loop_rows = torch.stack(modes["loop"]())
    if have_batch:
        result["batch_equals_loop"] = bool(torch.equal(modes["batch"](), loop_rows))
    reps = {"single": 4 * args.reps, "loop": max(1, args.reps // 4), "batch": args.reps}
    for name, fn in modes.items():                        # warm-up
        window(fn, 1)
    times = {name: [] for name in modes}
    for _ in range(args.rounds):                          # alternating
        for name, fn in modes.items():
            times[name].append(window(fn, reps[name]))
    for name, t in times.items():
        t = numpy.array(t)
        result[name] = {"median_us": float(numpy.median(t)), "min_us": float(t.min()),
                        "max_us": float(t.max()), "all_us": [float(x) for x in t]}
    if have_batch:
        result["loop_over_batch"] = result["loop"]["median_us"] / result["batch"]["median_us"]
        result["batch_us_per_hod"] = result["batch"]["median_us"] / n
    result["loop_us_per_hod"] = result["loop"]["median_us"] / n
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
