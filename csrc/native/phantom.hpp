// --phantom: the phantom file's reader (known emissivities, docs/FORMATS.md), the scores of a reconstructed column
// against its truth from the ten values of csrc/kernels/phantom64.hip, and the /phantom group of a solution file.
// Plain sequential fp64.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "h5.hpp"

namespace sart {

// The ten values per column, in the kernel's order
enum PhantomSum { kSumT = 0, kSumX, kSumTT, kSumXX, kSumXT, kSumDD, kSumIn, kMaxD, kMaxT, kMaxX, kPhantomSumCount };

constexpr int kPhantomScoreCount = 6;
// the score datasets of /phantom, in the order of PhantomScores' members
extern const char* const kPhantomScoreNames[kPhantomScoreCount];

struct PhantomScores {
    double rel_l2;           // sqrt(s_dd / s_tt)
    double cosine;           // s_xt / sqrt(s_xx s_tt)
    double total_ratio;      // s_x / s_t
    double peak_ratio;       // m_x / m_t
    double max_error;        // m_d / m_t
    double inside_fraction;  // s_in / s_x
};
// Each score is one correctly rounded division (cosine: a product, a square root and a division) of the sums as
// given; a zero denominator gives NaN.
PhantomScores phantom_scores(const double sums[kPhantomSumCount]);

#ifdef SART_HAVE_HDF5
// /phantom/value [n][nvoxel] (fp32 or fp64; finite, >= 0) and the optional /phantom/time [n] (strictly increasing;
// default 0, 1, ...). The constructor validates every entry and throws an Error that names the dataset; rows are
// read on demand. Every call holds the HDF5 lock: a reader thread and a sink may share one object.
class PhantomFile {
   public:
    PhantomFile(const std::string& filename, uint64_t nvoxel);
    uint64_t count() const { return n_; }
    const std::vector<double>& times() const { return time_; }
    // rows [k0, k0 + n) into out [n][nvoxel]
    void read_rows(uint64_t k0, uint64_t n, double* out) const;

   private:
    std::string filename_;
    uint64_t n_ = 0, nvox_;
    std::vector<double> time_;
};

// A phantom file from value [n][nvoxel] (stored fp32 with as_f32) and, unless null, time [n]. Nothing is validated:
// the tests write the files the reader must refuse with it.
void write_phantom_file(const std::string& filename, const double* value, uint64_t n, uint64_t nvoxel,
                        const double* time, bool as_f32);

// The /phantom group of a solution file: image [n][npixel], time [n], sums [n][nc][10], one dataset [n][nc] per score,
// status and iterations [n][nc], and the phantom file's name as the group's attribute "file". The file is created
// (truncated) with the pre-sized group, or with into_existing the group is added to the file an UncertaintyWriter made;
// /solution is added afterwards. The file is opened and closed by every write, under the HDF5 lock.
class PhantomWriter {
   public:
    PhantomWriter(const std::string& filename, uint64_t n, uint64_t nc, uint64_t npixel, const std::string& source,
                  const double* time, bool into_existing);
    // phantom k: sums [nc][10], status and iterations [nc]; the scores are taken here
    void write_phantom(uint64_t k, const double* sums, const int32_t* status, const int32_t* iterations);
    void write_images(const double* image);  // [n][npixel]

   private:
    std::string filename_;
    uint64_t n_, nc_, npix_;
};
#endif

}  // namespace sart
