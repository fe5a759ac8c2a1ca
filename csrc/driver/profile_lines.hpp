// --profile: one JSON object per line. JsonLine appends "key": value pairs to a stream with the stream's default
// formatting (six significant digits, true / false literals, strings escaped); one function per line kind
// (docs/FORMATS.md). Host code only.
#pragma once
#include <cstdint>
#include <ostream>
#include <string>
#include <type_traits>

#include "../native/solver_params.hpp"

namespace sart {

inline std::string json_escape(const std::string& s) {
    std::string o;
    for (char c : s) o += (c == '"' || c == '\\') ? std::string("\\") + c : std::string(1, c);
    return o;
}

class JsonLine {
   public:
    explicit JsonLine(std::ostream& os) : os_(os) { os_ << '{'; }
    template <class T>
    JsonLine& operator()(const char* key, const T& v) {
        this->key(key);
        if constexpr (std::is_same_v<T, bool>)
            os_ << (v ? "true" : "false");
        else if constexpr (std::is_convertible_v<const T&, std::string>)
            os_ << '"' << json_escape(v) << '"';
        else
            os_ << v;
        return *this;
    }
    JsonLine& open(const char* key) {  // a nested object: pairs up to close() go into it
        this->key(key);
        os_ << '{';
        first_ = true;
        return *this;
    }
    JsonLine& close() {
        os_ << '}';
        return *this;
    }
    void end() { os_ << "}\n"; }

   private:
    void key(const char* k) {
        os_ << (first_ ? "\"" : ", \"") << k << "\": ";
        first_ = false;
    }
    std::ostream& os_;
    bool first_ = true;
};

struct LoadStats;
class MultiFrameEngine;

// The load line: the load's figures over the ranks (each group is one host all-reduce of doubles), rank 0's own
// LoadStats, what was loaded and how it is solved. fp64_semantics: empty unless the fp64 engine runs.
struct LoadLine {
    struct Max { double load_s, rss_growth_mb, setup_s, shard_bytes; } max;       // slowest / largest rank
    struct Sum { double bytes, read_s, h2d_s, wait_read_s, wait_copy_s; } sum;    // over the ranks
    struct F16 { double flushed, nonzeros; } f16;  // --rtm_f16, summed: stored as zero / subnormal, all non-zeros
    int ranks = 1;
    bool parallel_read = false, has_sparse = false;
    const char *format = "dense", *storage = "fp32";
    std::string solver_path, fp64_semantics;
    int64_t nnz = 0;
};
void write_load_line(std::ostream& os, const LoadLine& l, const LoadStats& rank0);

// The frame records: which composite frame, its time and its "Processed in" time
struct FrameId {
    uint64_t frame;
    double time, ms;
};
// frame by frame: the solve's throughput model (pv = pixels x voxels) and this frame's host times
struct FrameCosts {
    bool gpu;
    double pv, elem_bytes, writer_ms, wait_frame_ms;
    int ranks;
    std::string comm, device_comm;
};
void write_frame_line(std::ostream& os, const FrameId& f, const SolveInfo& info, const FrameCosts& c);
void write_lead_line(std::ostream& os, const FrameId& f, const SolveInfo& info, int batch);  // a series' lead frame
// a frame of a batch; warm_from: the composite frame whose iterate started it (-1: none)
void write_batched_line(std::ostream& os, const FrameId& f, const SolveInfo& info, int batch, int64_t warm_from);
void write_series_line(std::ostream& os, const MultiFrameEngine& mf, double reader_ms, double sink_ms);
// --replicas: the noise definition's parameters and the total kernel times (device events) of the noise and moments
// kernels over the run
struct UncertaintyLine {
    int replicas;
    uint64_t seed;
    double noise_abs, noise_shot, noise_rel, noise_kernel_ms, moments_kernel_ms;
    uint64_t frames;
};
void write_uncertainty_line(std::ostream& os, const UncertaintyLine& u);
// --phantom: the counts and the total kernel times (device events) of the projection and scoring kernels over the run
struct PhantomLine {
    uint64_t phantoms;
    int replicas;
    uint64_t groups;  // projection passes over the shard
    double projection_kernel_ms, scoring_kernel_ms;
};
void write_phantom_line(std::ostream& os, const PhantomLine& p);
// --holdout: the run's shape, the projection groups of the hold-out pass, the scoring kernel's total time (device events
// around rank 0's launches) and the pass's wall time on rank 0
struct HoldoutLine {
    const char* mode;
    int folds;
    uint64_t seed;
    uint64_t betas, frames, columns, groups;
    double scoring_kernel_ms, ms;
};
void write_holdout_line(std::ostream& os, const HoldoutLine& h);
void write_fit_line(std::ostream& os, uint64_t frames, uint64_t groups, double ms, const char* storage,
                    const char* format, int ranks);

}  // namespace sart
