"""Measurement aid (GPU box): tools/time_kernels_batch.py with the bins a survey brings -- the 15
galaxy-galaxy kernels of five TABULATED lens bins (dNdzInterpolation through 33 points of a
Gaussian of width 0.1 around z0 = 0.3 .. 0.7 with a ripple on it), power_gg, w(theta) at n_theta
angles and C_l at n_ell multipoles -- two ways.  Every step rescales the ripple of one bin, so
that bin's table, every projection set-up that reads it, its z_bar and its halo epochs are
rebuilt:

    loop    per kernel: chomp_kernel_setup (the table rides behind the single set-up's slab),
            chomp_kernel_info (a synchronising read-back of z_bar and D(z_bar)), the halo set-up of
            one epoch at z_bar, chomp_wtheta / chomp_cell
    batch   chomp_kernel_setup_pairs behind chomp_set_sets_scope (five tables in the sets' arena),
            chomp_kernel_info_sets (ONE read-back), the grid set-up of 15 epochs,
            chomp_wtheta_sets / chomp_cell_sets

    python tools/time_kernels_tabulated.py [--n-theta 1024] [--n-ell 2048] [--rounds 7] [--out F.json]
    python tools/time_kernels_tabulated.py --root OTHER_TREE --modes loop-w,loop-cl
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_kernels_tabulated.py --count batch-w
    ... --analytic       the bins as dNdzGaussian(0, 2, z0, 0.1): what tools/time_kernels_batch.py times

--root: import the package from another checkout (a tree of the commit before the batch took
tables has the loop only: name the modes).  Timed as tools/time_kernels_batch.py times: HIP events
on the contexts' stream around the step, warm, the modes alternating round by round; each figure
is the median over the rounds with the least and the largest beside it.  Prints one JSON line.
"""
import argparse
import itertools
import json
import os
import sys
import warnings

import numpy

D2R = numpy.pi / 180.0
Z0 = (0.3, 0.4, 0.5, 0.6, 0.7)
MODES = ("loop-w", "batch-w", "loop-cl", "batch-cl")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-theta", type=int, default=1024)
    ap.add_argument("--n-ell", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3, help="steps per timed window")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--count", choices=MODES)
    ap.add_argument("--analytic", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    warnings.simplefilter("ignore")
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    from chomp_amd import correlation, defaults, grid, kernel, cosmology
    names = [m for m in args.modes.split(",") if m]
    assert all(m in MODES for m in names), names

    def bins_of(scale):
        """The five bins: scale[i] is the ripple of bin i."""
        if args.analytic:
            return [kernel.dNdzGaussian(0.0, 2.0, z0 + 1e-4 * (s - 0.2), 0.1)
                    for z0, s in zip(Z0, scale)]
        out = []
        for z0, s in zip(Z0, scale):
            z = numpy.linspace(max(z0 - 0.4, 0.0), z0 + 0.4, 33)
            p = numpy.exp(-0.5 * ((z - z0) / 0.1) ** 2) * (1.0 + s * numpy.sin(25.0 * z)) + 1e-3
            out.append(kernel.dNdzInterpolation(z, p))
        return out

    def kernels_of(scale):
        """The 15 pairs (i <= j) of the five bins, each a fresh Kernel on one shared MultiEpoch."""
        me = cosmology.MultiEpoch(0.0, 5.0)
        bins = bins_of(scale)
        return [kernel.Kernel(1e-6 * D2R, 100.0 * D2R, kernel.WindowFunctionGalaxy(bins[i], me),
                              kernel.WindowFunctionGalaxy(bins[j], me), me)
                for i, j in itertools.combinations_with_replacement(range(len(bins)), 2)]

    n = len(kernels_of([0.2] * 5))
    hg1 = grid.HaloGrid(numpy.zeros(1))                  # (the loop's context: one epoch)
    hgn = grid.HaloGrid(numpy.zeros(n))                  # (the batch's: one epoch per kernel)
    code = correlation._POWER["power_gg"][0]
    k_lim = (defaults.default_limits["k_min"], defaults.default_limits["k_max"])
    theta = torch.logspace(-3, 0, args.n_theta, dtype=torch.float64, device="cuda") * D2R
    ell = torch.logspace(1, 4, args.n_ell, dtype=torch.float64, device="cuda")
    step = [0]

    def shifted():
        """The kernels of the next step: one bin's ripple rescaled by a new amount."""
        step[0] += 1
        scale = [0.2] * 5
        scale[step[0] % 5] += 1e-4 * step[0]
        return kernels_of(scale)

    def loop(what):
        rows, ctx = [], hg1.ctx
        for k in shifted():
            ctx.kernel_setup(k.cosmo.cosmo_dict, k.cosmo.z_min, k.cosmo.z_max, k._ktheta[0],
                             k._ktheta[1], k.window_function_a._struct(),
                             k.window_function_b._struct(), k._order)
            info = ctx.kernel_info()
            hg1.set_parameters(z=info["z_bar"])
            hg1.setup("power_gg")
            rows.append(ctx.wtheta(code, 0, k_lim[0], k_lim[1], info["D_zbar"], theta) if what == "w"
                        else ctx.cell(code, 0, info["D_zbar"], ell))
        return torch.stack(rows)

    def batch(what):
        ctx = hgn.ctx
        kernel.Kernel._setup_pairs_on(ctx, shifted())
        info = ctx.kernel_info_sets()
        hgn.set_parameters(z=info["z_bar"])
        hgn.setup("power_gg")
        if what == "w":
            return ctx.wtheta_sets(code, 0, n, k_lim[0], k_lim[1], info["D_zbar"], theta)
        return ctx.cell_sets(code, 0, n, info["D_zbar"], ell)

    modes = {"loop-w": lambda: loop("w"), "batch-w": lambda: batch("w"),
             "loop-cl": lambda: loop("cl"), "batch-cl": lambda: batch("cl")}
    if args.count:
        modes[args.count]()
        torch.cuda.synchronize()
        print(json.dumps({"count": args.count, "kernels": n, "analytic": args.analytic}))
        return
    modes = {name: modes[name] for name in names}

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3          # microseconds per step

    result = {"what": "microseconds per chain step (HIP events around the step, read-backs "
                      "included), 15 kernels of five %s bins, power_gg"
                      % ("analytic" if args.analytic else "tabulated"),
              "device": torch.cuda.get_device_name(0), "kernels": n, "n_theta": args.n_theta,
              "n_ell": args.n_ell, "rounds": args.rounds, "steps_per_window": args.reps,
              "root": os.path.basename(os.path.abspath(args.root))}
    for what in ("w", "cl"):                             # (the same step both ways)
        if "loop-" + what in modes and "batch-" + what in modes:
            at = step[0]
            a = loop(what)
            step[0] = at
            b = batch(what)
            # (the loop's halo set-up is a one-epoch grid's, the batch's a 15-epoch grid's)
            result["batch_against_loop_max_rel_" + what] = float(((b - a).abs() / a.abs()).max())
            result["not_finite_" + what] = int((~torch.isfinite(b)).sum())
            result["rows_with_a_status_word"] = int(numpy.count_nonzero(hgn.status()))
    for fn in modes.values():                             # warm-up
        window(fn, 1)
    times = {name: [] for name in modes}
    for _ in range(args.rounds):                          # alternating
        for name, fn in modes.items():
            times[name].append(window(fn, args.reps))
    for name, t in times.items():
        t = numpy.array(t)
        result[name] = {"median_us": float(numpy.median(t)), "min_us": float(t.min()),
                        "max_us": float(t.max()), "all_us": [float(x) for x in t]}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
