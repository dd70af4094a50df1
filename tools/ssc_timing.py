#!/usr/bin/env python3
"""Workload for timing the super-sample covariance of w(theta) on the device: the kernel_ssc
table set-up and a C4-sized get_covariance() (6 bins, 21 pairs; G and SSC together), on G12's
galaxy x convergence windows.  Run it under the profiler, e.g.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ssc_timing.py

and read k_ssc_prep / k_ssc_table / k_ssc_bicubic (set-up), k_cov_* (G) and k_ssc_kb /
k_ssc_outer (SSC) from the kernel statistics.  Prints the host wall time of each step."""
import os
import sys
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chomp_amd import correlation, cosmology, covariance, halo, kernel  # noqa: E402

deg_to_rad = numpy.pi / 180.0


def main():
    cm = cosmology.MultiEpoch(0.0, 5.0)
    wa = kernel.WindowFunctionGalaxy(kernel.dNdzMagLim(0.0, 2.0, 2.0, 0.3, 2.0), cm)
    wb = kernel.WindowFunctionConvergence(kernel.dNdzGaussian(0.0, 2.0, 1.0, 0.2), cm)
    kern = kernel.Kernel(1e-6 * deg_to_rad, 100.0 * deg_to_rad, wa, wb, cm)
    corr = correlation.Correlation(0.01, 1.0, kern, input_halo=halo.Halo(0.0),
                                   power_spec="power_mm")
    cv = covariance.Covariance(corr, corr, bins_per_decade=3.0, survey_area_deg2=25.0,
                               nongaussian_cov=False, ssc_cov=True)
    t0 = time.time()
    cv.kernel._ssc()
    t1 = time.time()
    cov = cv.get_covariance()
    t2 = time.time()
    print("bins %d  table set-up %.2f ms  get_covariance %.2f ms  finite %s" % (
        len(cv.annular_bins), 1e3 * (t1 - t0), 1e3 * (t2 - t1), numpy.isfinite(cov).all()))


if __name__ == "__main__":
    main()
