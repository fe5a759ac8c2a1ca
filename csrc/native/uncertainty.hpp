// The /uncertainty group of a solution file (--replicas; docs/FORMATS.md): per composite frame the per-voxel mean and
// unbiased standard deviation over the noisy replicas that counted, how many counted, and every column's status and
// update count (column 0: the nominal, unperturbed solve); with keep, every column's solution too.
#pragma once

#include <cstdint>
#include <string>

#include "h5.hpp"

namespace sart {

#ifdef SART_HAVE_HDF5
// The file is created (truncated) with the group and its pre-sized datasets for `frames` composite frames of `nrep`
// replicas; /solution is added to it afterwards (SolutionWriter with into_existing). A frame is written when its last
// column has arrived; the file is opened and closed by every write_frame, under the HDF5 lock, so the solution writer's
// background flushes of the same file never meet an open handle.
class UncertaintyWriter {
   public:
    UncertaintyWriter(const std::string& filename, uint64_t frames, uint64_t nrep, uint64_t nvoxel, const double noise[3],
                      uint64_t seed, bool keep);
    // mean[k, :], std[k, :], count[k], status[k, :], iterations[k, :] (nrep + 1 entries each), and with keep
    // value[k, :, :] from columns [nrep + 1][nvoxel]
    void write_frame(uint64_t k, const double* mean, const double* std_dev, int32_t count, const int32_t* status,
                     const int32_t* iterations, const double* columns);

   private:
    std::string filename_;
    uint64_t frames_, nrep_, nvox_;
    bool keep_;
};
#endif

}  // namespace sart
