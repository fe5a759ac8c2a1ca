// Hold-out cross-validation (--holdout, models/holdout.py): the fold of a pixel, the masked columns, the scores of a
// composite frame from the scoring kernel's sums (csrc/kernels/holdout64.hip) and the /holdout group of the output
// file. utils/holdout.py restates the folds, the masks and the scores in NumPy bit for bit.
//
// Folds. Pixel mode: w = philox4x32_10(global pixel, 0, 0x484F4C44, 0; key = seed low word, seed high word)
// (csrc/kernels/philox.hpp), fold(p) = (uint64(w[0]) K) >> 32: a function of (seed, global pixel) alone. Camera mode:
// fold(p) = the index of p's camera in composite order.
// Columns. Column 0 of a frame is the frame as measured; column c >= 1 has g_p = -1 (the solver's exclusion marker)
// where fold(p) = c - 1 and g_p >= 0.
// Sums [K + 1][ncam][6] per ladder entry, over S = {p : g_p >= 0 and ray length > threshold}: for column c and camera
// m with H = S n camera m n {fold = c - 1} (empty for c = 0) and Kp = (S n camera m) \ H:
//   sum_H (g - f)^2, sum_H g^2, |H|, sum_Kp (g - f)^2, sum_Kp g^2, |Kp|.
// Scores per ladder entry i (each operation correctly rounded, sums over c = 1 .. K outer and cameras inner, in index
// order; a zero denominator gives NaN):
//   cv_error = sqrt(sum_c sum_m s0 / sum_c sum_m s2), cv_relative = sqrt(sum_c sum_m s0 / sum_c sum_m s1),
//   cv_error_camera[m] = sqrt(sum_c s0[c][m] / sum_c s2[c][m]), train_error = sqrt(sum_m s3[0][m] / sum_m s5[0][m]),
//   eligible = none of the K + 1 columns stopped on a non-finite iterate and cv_error is finite.
// selected: the first i with the smallest cv_error among the eligible ones (found = 1); with none eligible the
// fallback entry (found = 0).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "h5.hpp"

namespace sart {

constexpr int kHoldoutSumCount = 6;
constexpr uint32_t kHoldoutCounterTag = 0x484F4C44u;  // "HOLD"

// out[i] = fold of global pixel pixel0 + i for i < n; K within 2 .. 32, pixel0 + n <= 2^32
void holdout_pixel_folds(uint64_t seed, int K, uint64_t pixel0, uint64_t n, int32_t* out);
// camera mode: camera_pixels [ncam] pixels per camera in composite order; pixel0 + n <= their sum
void holdout_camera_folds(const int64_t* camera_pixels, int ncam, uint64_t pixel0, uint64_t n, int32_t* out);
// column held + 1 of a frame: out[p] = -1 where fold[p] == held and g[p] >= 0, else g[p] (held < 0: a copy)
void holdout_mask(const double* g, const int32_t* fold, int64_t n, int held, double* out);
// the ladder entry nearest to beta (ties to the smaller index); nb >= 1
int holdout_fallback(const double* betas, int nb, double beta);

struct HoldoutScores {
    std::vector<double> cv_error, cv_relative, train_error;  // [nb]
    std::vector<double> cv_error_camera;                     // [nb][ncam]
    std::vector<uint8_t> eligible;                           // [nb]
    int32_t selected = 0;
    uint8_t found = 0;
};
// sums [nb][K + 1][ncam][6], ok [nb][K + 1] (ok != 0: the column did not stop on a non-finite iterate)
HoldoutScores holdout_scores(const double* sums, const uint8_t* ok, int nb, int K, int ncam, int fallback);

#ifdef SART_HAVE_HDF5
// The /holdout group of a solution file (docs/FORMATS.md): the file is created (truncated) with the group and its
// pre-sized datasets for `frames` composite frames x nb weights x K + 1 columns; /solution is added to it afterwards
// (SolutionWriter with into_existing). Columns are written as they finish; the file stays open between column writes
// until close().
class HoldoutWriter {
   public:
    HoldoutWriter(const std::string& filename, uint64_t frames, uint64_t nb, uint64_t K, uint64_t ncam, uint64_t nvoxel,
                  bool cameras, const int32_t* folds, uint64_t npixel, uint64_t seed, const double* beta);
    // value[k, i, c], status[k, i, c], iterations[k, i, c]
    void write_column(uint64_t k, uint64_t i, uint64_t c, const double* x, int32_t status, int32_t iterations);
    // rows [j0, j0 + n) of value seen as [frames nb (K + 1)][nvoxel] into out
    void read_columns(uint64_t j0, uint64_t n, double* out);
    // sums[k] ([nb][K + 1][ncam][6]) and the scores derived from them
    void write_frame(uint64_t k, const double* sums, const HoldoutScores& s);
    void close();

   private:
    hid_t file();
    std::string filename_;
    uint64_t frames_, nb_, nc_, ncam_, nvox_;
    H5Id file_;
};
#endif

}  // namespace sart
