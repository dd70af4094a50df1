"""Measurement aid (GPU box): w(theta) at n_theta angles (logspace(-3, 0, n_theta) degrees) of the
G6 set-up (galaxy x galaxy windows, power_gg) for N cosmologies of a seeded flat-universe design
(omega_m0, sigma_8 and h drawn, omega_l0 = 1 - omega_m0 - omega_r0), two ways, HIP-event timed
around work that ends in a synchronise (host theta, host result):

    loop    set_cosmology + correlation per point on one Correlation
    batch   one Correlation.correlation_cosmologies call over the N points

    python tools/time_wtheta_cosmologies.py [--n-cosmo 64] [--n-theta 1024] [--rounds 7] [--out F.json]
    python tools/time_wtheta_cosmologies.py --tree build_exp/parent ...   (another checkout of the
        project, built; one without correlation_cosmologies times the loop only)
    python tools/time_wtheta_cosmologies.py --merge A.json B.json ... --out profiles/wtheta_cosmologies_timing.json

The modes alternate round by round; each figure is the median over the rounds, with the least and
the largest beside it.  Whether the single-call path pays for the set axis is read off the loop of
two builds run alternately in separate processes (--merge: the runs side by side, the loop's
medians per tree, and this tree's loop against the parent's beside the spread of the repeats).
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import warnings

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D2R = numpy.pi / 180.0
PROJ_RTOL = 1e-9


def cosmologies(n, seed=34):
    """n points of a flat-universe design around the default cosmology."""
    from chomp_amd import defaults
    rng = numpy.random.RandomState(seed)
    out = []
    for _ in range(n):
        c = dict(defaults.default_cosmo_dict, omega_m0=rng.uniform(0.25, 0.35),
                 sigma_8=rng.uniform(0.7, 0.9), h=rng.uniform(0.65, 0.75))
        c["omega_l0"] = 1.0 - c["omega_m0"] - c["omega_r0"]
        out.append(c)
    return out


def merge(paths, out):
    runs = []
    for p in paths:
        with open(p) as f:
            runs.append(json.load(f))
    result = {"what": runs[0]["what"], "device": runs[0]["device"], "n_cosmo": runs[0]["n_cosmo"],
              "n_theta": runs[0]["n_theta"], "rounds": runs[0]["rounds"], "runs": runs}
    mine = [r for r in runs if r["tree"] == "this one"]
    other = [r for r in runs if r["tree"] != "this one"]
    n = runs[0]["n_cosmo"]
    if mine:
        loop = [r["loop"]["median_us"] for r in mine]
        batch = [r["batch"]["median_us"] for r in mine]
        result["loop_us_per_point"] = float(numpy.median(loop)) / n
        result["batch_us_per_point"] = float(numpy.median(batch)) / n
        result["loop_over_batch"] = float(numpy.median(loop)) / float(numpy.median(batch))
        result["batch_equals_loop"] = all(r["batch_equals_loop"] for r in mine)
        result["loop_spread_between_repeats"] = (max(loop) - min(loop)) / min(loop)
    if mine and other:
        ploop = [r["loop"]["median_us"] for r in other]
        result["parent_loop_us_per_point"] = float(numpy.median(ploop)) / n
        result["parent_loop_spread_between_repeats"] = (max(ploop) - min(ploop)) / min(ploop)
        result["loop_over_parent_loop"] = float(numpy.median(loop)) / float(numpy.median(ploop))
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}))
    with open(out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-cosmo", type=int, default=64)
    ap.add_argument("--n-theta", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tree", help="another checkout of the project, built, to time instead")
    ap.add_argument("--merge", nargs="+", help="result files of earlier runs to put side by side")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    if args.tree:                                # (another checkout, built: its package, its library)
        sys.path[0] = os.path.abspath(args.tree)
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    warnings.simplefilter("ignore")
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    from chomp_amd import correlation, cosmology, halo, kernel
    cm = cosmology.MultiEpoch(0.0, 5.0)
    wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    wb = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    kern = kernel.Kernel(1e-6 * D2R, 100.0 * D2R, wa, wb, cm)
    corr = correlation.Correlation(0.001, 1.0, kern, input_halo=halo.Halo(0.0), power_spec="power_gg")
    n = args.n_cosmo
    points = cosmologies(n)
    theta = numpy.logspace(-3, 0, args.n_theta) * D2R
    have_batch = hasattr(corr, "correlation_cosmologies")

    def loop():
        rows = []
        for c in points:
            corr.set_cosmology(c)
            rows.append(corr.correlation(theta))
        return numpy.array(rows)
    modes = {"loop": loop}
    if have_batch:
        batch_corr = correlation.Correlation(0.001, 1.0, kern, input_halo=halo.Halo(0.0),
                                             power_spec="power_gg")
        modes["batch"] = lambda: batch_corr.correlation_cosmologies(theta, points)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()                                     # (ends in a synchronise: the result is on the host)
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3         # microseconds per call

    result = {"what": "microseconds per call (HIP events around host-synchronous work), w(theta) of "
                      "n_theta angles for n_cosmo cosmologies, power_gg",
              "device": torch.cuda.get_device_name(0), "tree": args.tree or "this one",
              "n_cosmo": n, "n_theta": args.n_theta, "rounds": args.rounds}
    loop_rows = modes["loop"]()                  # warm-up
    if have_batch:
        rows, words = batch_corr.correlation_cosmologies(theta, points, with_status=True)   # warm-up
        err = float(numpy.max(numpy.abs(rows / loop_rows - 1.0)))
        result["batch_against_loop_max_rel"] = err
        result["batch_equals_loop"] = bool(err < 2 * PROJ_RTOL)
        result["points_with_a_status_word"] = int(numpy.count_nonzero(words))
    times = {name: [] for name in modes}
    for _ in range(args.rounds):                 # alternating
        for name, fn in modes.items():
            times[name].append(window(fn))
    for name, t in times.items():
        t = numpy.array(t)
        result[name] = {"median_us": float(numpy.median(t)), "min_us": float(t.min()),
                        "max_us": float(t.max()), "all_us": [float(x) for x in t]}
    result["loop_us_per_point"] = result["loop"]["median_us"] / n
    if have_batch:
        result["batch_us_per_point"] = result["batch"]["median_us"] / n
        result["loop_over_batch"] = result["loop"]["median_us"] / result["batch"]["median_us"]
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
