// L-curve corner of a Laplacian-weight scan (--beta_scan): the point of largest positive Menger curvature of the
// curve (log residual norm, log roughness norm) over the weights in increasing order. Plain sequential fp64.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "h5.hpp"

namespace sart {

struct LcurveCorner {
    int selected = 0;               // index of the corner, or the fallback rule's index when none was found
    int found = 0;                  // 1: some point has a curvature > 0
    std::vector<double> curvature;  // [nb], NaN where undefined
};

// rho, eta: residual and roughness norms of nb points in increasing-weight order; ok[i] != 0: frame i did not stop on a
// non-finite iterate. A point is valid when ok is set and rho and eta are finite and > 0. With p_i = (log rho_i,
// log eta_i), a valid point b between its nearest valid neighbours a (before) and c (after) gets
//   cross = (p_b - p_a).x (p_c - p_b).y - (p_b - p_a).y (p_c - p_b).x,
//   kappa = 2 cross / (|p_b - p_a| |p_c - p_b| |p_c - p_a|), or 0 when one of the three lengths is 0
// (the curve runs down and to the right as the weight grows, so its corner has cross > 0). selected is the index of
// the largest kappa if that is > 0 (ties to the smaller index; found = 1). Otherwise found = 0 and selected is
// `fallback` if that point is valid, else the valid index nearest to it (ties to the smaller), else `fallback`.
LcurveCorner lcurve_corner(const double* rho, const double* eta, const uint8_t* ok, int nb, int fallback);

#ifdef SART_HAVE_HDF5
// The /beta_scan group of a solution file (docs/FORMATS.md): the file is created (truncated) with the group and its
// pre-sized datasets for `frames` composite frames x `nb` weights; /solution is added to it afterwards (SolutionWriter
// with into_existing). Columns are written as they finish, so the scan's solutions are never held in host memory. The
// file stays open between column writes until close().
class ScanWriter {
   public:
    ScanWriter(const std::string& filename, uint64_t frames, uint64_t nb, uint64_t nvoxel, const double* beta);
    // value[k, i], status[k, i], iterations[k, i]
    void write_column(uint64_t k, uint64_t i, const double* x, int32_t status, int32_t iterations);
    // rows [j0, j0 + n) of value seen as [frames nb][nvoxel] (row j = k nb + i) into out
    void read_columns(uint64_t j0, uint64_t n, double* out);
    // residual_norm[k, :], roughness_norm[k, :], curvature[k, :], selected[k], corner_found[k]
    void write_frame(uint64_t k, const double* rho, const double* eta, const double* curvature, int32_t selected,
                     uint8_t found);
    void close();

   private:
    hid_t file();
    std::string filename_;
    uint64_t frames_, nb_, nvox_;
    H5Id file_;
};
#endif

}  // namespace sart
