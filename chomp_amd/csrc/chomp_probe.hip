// chomp_probe.hip -- the translation unit of k_epoch_probe (compiled with machine LICM; the
// rest of the library without: chomp_amd/_lib.py).
#include <hip/hip_runtime.h>

#include "../../include/chomp_mi355x.h"
#include "chomp_probe_kernel.h"

namespace chomp {

void launch_epoch_probe(bool bao, unsigned n_epoch, hipStream_t stream, const chomp_config& cfg,
                        Epoch* epochs, double* search, const double* cand, const double* snodes,
                        double* probe, int* count, unsigned* status) {
  // A large batch: probed by the caller (k_epoch_probe<., 1, 1>, instantiated in chomp_capi.hip,
  // the unit without machine LICM, capped at 128 registers: 120), certified here, behind the
  // kernel boundary.
  const bool large = n_epoch >= (unsigned)kProbeLargeBatch;
  const dim3 grid = large ? dim3(n_epoch) : dim3(n_epoch, 2 * kProbes);
  with_flag(bao, large, [&](auto BAO, auto LARGE) {
    hipLaunchKernelGGL((k_epoch_probe<BAO, LARGE ? 2 : 0>), grid, dim3(64 * kInitNW), 0, stream,
                       cfg, epochs, search, cand, snodes, probe, count, status);
  });
}

}  // namespace chomp
