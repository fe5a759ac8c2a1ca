// Fit diagnostics (--fit, --fit_only, SARTSolver.fit): the fp64 forward projection f = A x of stored solutions on the
// host (the --use_cpu path; the GPU paths use csrc/kernels/fit64.hip), the residual statistics against the measured
// composite frame, and the /fit group of the solution file (docs/FORMATS.md).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "h5.hpp"
#include "sparse_csr.hpp"

namespace sart {

// F[j][p] = sum_v A[p][v] X[j][v] for j < nv in fp64: products and sums rounded separately (the native sources are
// built with contraction off, by the in-tree build and by CMake alike), each row summed in column order (OpenMP over
// rows: the values do not depend on the thread count, on nv or on a vector's position). A: row-major fp32 [P][ld];
// X: [nv][ldx], read below V only; F: [nv][ldf]
void cpu_fit_forward(const float* A, int64_t P, int64_t V, int64_t ld, const double* X, int64_t ldx, int nv, double* F,
                     int64_t ldf);
// the same on CSR rows, each row summed in its entries' order
void cpu_fit_forward(const HostCsr& rows, const double* X, int64_t ldx, int nv, double* F, int64_t ldf);

// Residual statistics of one fitted image f against the measured frame g over the pixels
// S = {p : g[p] >= 0 and ell[p] > threshold} (negative pixels are saturated, docs/FORMATS.md), for the whole image and
// for each camera's pixel range (camera_pixels: pixels per camera in composite order, summing to npixel). Plain
// sequential fp64 loops in pixel order: the numbers do not depend on a thread count.
struct FitStats {
    double residual_norm = 0, measurement_norm = 0, residual_max = 0;  // sqrt sum (g - f)^2, sqrt sum g^2, max |g - f|
    int64_t pixels = 0;                                                // |S|
    std::vector<double> residual_norm_camera, measurement_norm_camera;
    std::vector<int64_t> pixels_camera;
};
FitStats fit_statistics(const double* f, const double* g, const double* ell, int64_t npixel, double threshold,
                        const std::vector<int64_t>& camera_pixels);

#ifdef SART_HAVE_HDF5
// The /fit group of a finished solution file: opened read-write, an existing /fit group removed and rebuilt with
// `frames` rows (row k belongs to row k of /solution/*).
class FitWriter {
   public:
    FitWriter(const std::string& filename, uint64_t frames, uint64_t npixel, uint64_t ncamera);
    void write(uint64_t k, const double* image, const FitStats& s);
    uint64_t frames() const { return frames_; }

   private:
    std::string filename_;
    uint64_t frames_, npix_, ncam_;
};

// /solution/time of a solution file (empty when the file is missing, not HDF5 or holds no solution) and rows
// [k0, k0 + n) of /solution/value (n x nvoxel doubles)
std::vector<double> read_solution_times(const std::string& filename);
std::vector<double> read_solution_rows(const std::string& filename, uint64_t k0, uint64_t n, uint64_t nvoxel);
#endif

}  // namespace sart
