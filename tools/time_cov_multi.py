"""Measurement aid (GPU box): the Gaussian covariance of a tomographic analysis -- five Gaussian
lens bins (dNdzGaussian(0, 2, z0, 0.1), z0 = 0.3 .. 0.7), their 15 galaxy-galaxy correlations
(each on its own halo.Halo), 120 blocks, 10 angular bins (bins_per_decade=5 over 0.01-1 deg, 55 bin
pairs) -- two ways:

    loop    CovarianceMulti.get_covariance(): per cross block two set-ups, two snapshots
            (chomp_covariance_cross_stage), chomp_covariance_table_cross and
            chomp_covariance_gaussian_cross; a block keeps its tables until something it was
            built from changes
    batch   CovarianceMulti.get_covariance_batched(): chomp_kernel_setup_pairs, ONE read-back of
            z_bar, the grid set-up of 15 epochs, chomp_covariance_blocks; keeps no tables

    python tools/time_cov_multi.py [--rounds 5] [--modes loop,batch] [--ssc] [--ng] [--out FILE.json]

--ssc: the same analysis with the super-sample term, CovarianceMulti(ssc_cov=True,
cross_terms=True): per cross block the loop adds kernel_ssc (a read-back of the chi range, a host
sigma_r call, the 1275 integrals of the table, its bicubic) and covariance_ssc; the batch adds one
read-back of every block's range, one sigma_r call per row of blocks and
chomp_covariance_ssc_blocks.

--ng: the same analysis with the one-halo trispectrum term, CovarianceMulti(nongaussian_cov=True,
cross_terms=True, input_halo_trispectrum=HaloTrispectrumOneHalo(0.5)), one trispectrum object at
one fixed redshift for all blocks: per cross block the loop adds the kernel_ssc scalars (a
read-back of the chi range, a host sigma_r call), kernel_NG (the 1275 integrals of the table, a
read-back of it, its bicubic) and covariance_NG (the upload and bicubic of the I_0^4 table, the
k_b and outer integrals); the batch, get_covariance_batched(trispectrum=True), adds
chomp_covariance_ng_blocks alone.  --ng --ssc: all three terms.

Timed, host clock around calls that end with their result on the host (so synchronised):
    loop_first / batch_first   the first call on fresh objects (contexts, buffers, code objects)
    loop_all                   get_covariance() after set_hod on EVERY correlation: all 120
                               blocks rebuilt -- the work the batch always does
    loop_one                   ... after set_hod on ONE correlation: its 15 blocks rebuilt, 105
                               served from their kept tables
    batch_one                  get_covariance_batched() after set_hod on one correlation
Warm figures alternate round by round; each is the median over the rounds with the least and the
largest beside it.  --modes loop runs on a tree that has no get_covariance_batched (the parent
commit's loop in the same session).  Prints one JSON line.
"""
import argparse
import itertools
import json
import os
import sys
import time
import warnings

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D2R = numpy.pi / 180.0
Z0 = (0.3, 0.4, 0.5, 0.6, 0.7)


def correlations():
    """The 15 pairs (i <= j) of the five bins: a Correlation each, on its own Halo."""
    from chomp_amd import correlation, cosmology, halo, kernel
    me = cosmology.MultiEpoch(0.0, 5.0)
    win = [kernel.WindowFunctionGalaxy(kernel.dNdzGaussian(0.0, 2.0, z0, 0.1), me) for z0 in Z0]
    out = []
    for i, j in itertools.combinations_with_replacement(range(len(Z0)), 2):
        kern = kernel.Kernel(1e-6 * D2R, 100.0 * D2R, win[i], win[j], me)
        out.append(correlation.Correlation(0.01, 1.0, kern, input_halo=halo.Halo(0.0),
                                           power_spec="power_mm"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--modes", default="loop,batch")
    ap.add_argument("--ssc", action="store_true")
    ap.add_argument("--ng", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    warnings.simplefilter("ignore")
    from chomp_amd import covariance, defaults, halo_trispectrum
    modes = args.modes.split(",")
    step = [0]

    def build():
        corrs = correlations()
        kws = dict(nongaussian_cov=False)
        if args.ssc:
            kws.update(ssc_cov=True, cross_terms=True)
        if args.ng:
            kws.update(nongaussian_cov=True, cross_terms=True,
                       input_halo_trispectrum=halo_trispectrum.HaloTrispectrumOneHalo(0.5))
        return corrs, covariance.CovarianceMulti(corrs, bins_per_decade=5,
                                                 survey_area_deg2=25.0, **kws)

    def batched(cm):
        # (the keyword only where it is needed: the Gaussian and --ssc runs also serve trees
        #  whose get_covariance_batched does not have it)
        return cm.get_covariance_batched(trispectrum=True) if args.ng else cm.get_covariance_batched()

    def move(corrs, which):
        """A new HOD on the correlations `which`."""
        step[0] += 1
        hod = dict(defaults.default_hod_dict)
        hod["log_M_min"] = hod["log_M_min"] + 1e-4 * step[0]
        for c in which:
            corrs[c].set_hod(hod)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out    # milliseconds

    result = {"what": "milliseconds per covariance matrix (host clock, result on the host), 15 "
                      "correlations, 120 blocks, 10 angular bins, power_mm"
                      + (", Gaussian + super-sample terms (ssc_cov, cross_terms)" if args.ssc else "")
                      + (", + one-halo trispectrum term (nongaussian_cov, cross_terms)" if args.ng else ""),
              "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "modes": modes}
    state, warm = {}, {}
    if "loop" in modes:
        corrs, cm = build()
        result["loop_first_ms"], w = clock(cm.get_covariance)
        state["loop"] = (corrs, cm, w.copy())
        warm["loop_all"] = lambda: (move(corrs, range(len(corrs))), cm.get_covariance())[1]
        warm["loop_one"] = lambda: (move(corrs, [step[0] % len(corrs)]), cm.get_covariance())[1]
    if "batch" in modes:
        corrs_b, cm_b = build()
        result["batch_first_ms"], w = clock(lambda: batched(cm_b))
        state["batch"] = (corrs_b, cm_b, w.copy())
        warm["batch_one"] = lambda: (move(corrs_b, [step[0] % len(corrs_b)]),
                                     batched(cm_b))[1]
        result["correlations_with_a_status_word"] = int(numpy.count_nonzero(cm_b.blocks_status))
    if "loop" in state and "batch" in state:
        a, b = state["loop"][2], state["batch"][2]
        result["shape"] = list(b.shape)
        result["batch_equals_loop"] = bool(numpy.array_equal(a, b))
        result["batch_against_loop_max_rel"] = float(numpy.max(numpy.abs(b - a) / numpy.abs(a)))
        result["not_finite"] = int(numpy.count_nonzero(~numpy.isfinite(b)))
    for fn in warm.values():                                 # warm-up
        clock(fn)
    times = {name: [] for name in warm}
    for _ in range(args.rounds):                             # alternating
        for name, fn in warm.items():
            times[name].append(clock(fn)[0])
    for name, t in times.items():
        t = numpy.array(t)
        result[name] = {"median_ms": float(numpy.median(t)), "min_ms": float(t.min()),
                        "max_ms": float(t.max()), "all_ms": [float(x) for x in t]}
    if "loop_all" in result and "batch_one" in result:
        for name in ("loop_all", "loop_one"):
            result[name + "_over_batch_one"] = (result[name]["median_ms"]
                                                / result["batch_one"]["median_ms"])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
