// What the native driver's units share: what main() sets up once (Driver, Solvers), the skeleton of a run over
// MultiFrameEngine::solve_series (SeriesRun) and the runs that run() starts.
#pragma once
#include <array>
#include <fstream>
#include <iostream>

#include "../engine/comm.hpp"
#include "../engine/engine64.hpp"
#include "../engine/multiframe.hpp"
#include "../native/cpu_solver.hpp"
#include "../native/frames.hpp"
#include "../native/holdout.hpp"
#include "../native/lcurve.hpp"
#include "frame_readahead.hpp"
#include "profile_lines.hpp"
#include "series_order.hpp"
#include "shard_load.hpp"

namespace sart {

using Clock = std::chrono::steady_clock;

struct Driver {
    Config cfg;
    std::vector<std::array<double, 4>> intervals;
    InputSet in;
    std::unique_ptr<Communicator> dcomm;  // GPU runs: the device communicator (host: its host side)
    std::unique_ptr<HostComm> hcomm;      // --use_cpu
    HostComm* host = nullptr;
    int rank = 0, size = 1, device = 0;
    bool gpu = true, cols = false;  // cols: --partition_voxels (every rank holds all pixels of a block of voxels)
    Block blk, vblk;                // this rank's pixels and voxels
    std::unique_ptr<CompositeImage> image;
    std::unique_ptr<SolutionWriter> writer;  // rank 0
    std::ofstream profile;                   // rank 0, --profile
};

// the single-frame engine (frame by frame; with --batch_frames it solves a cold time series' first frame), the fp64
// engine, the multi-frame engine or the CPU solver
struct Solvers {
    std::unique_ptr<Engine> engine, lead_engine;
    std::unique_ptr<Engine64> engine64;
    std::unique_ptr<MultiFrameEngine> mf;
    std::unique_ptr<CpuSolver> cpu;
    // the lead frame stops at lead_tol x the tolerance and hands its iterate to the batch, where it finishes next
    // to the frames chained from it (1: it finishes on the single-frame engine; SART_MF_LEAD_TOL)
    double lead_tol = 1.0;
    void reset() { engine.reset(), lead_engine.reset(), engine64.reset(), mf.reset(); }
};

// One run of n series frames through MultiFrameEngine::solve_series. A reader thread keeps up to 4 N frames of `frame`
// (series index -> this rank's pixels) read ahead; the engine stages them into its device queue while earlier frames
// sweep and delivers finished columns out of order. No host collective in a column callback: the series thread
// interleaves staging and delivery differently on different ranks.
class SeriesRun {
   public:
    SeriesRun(Driver& d, MultiFrameEngine& mf, int64_t n, FrameReadahead::Source frame)
        : d_(d), mf_(mf), n_(n), ra_(n, 4 * (int64_t)d.cfg.batch_frames, std::move(frame)) {}
    FrameReadahead& readahead() { return ra_; }  // (the lead frame is taken before the series starts)
    // Solves frames off .. n - 1 (x0, chain, frame_beta: solve_series'; frame_beta[0] is frame off's). Rank 0:
    // column(k, x, info) for every finished frame k, which calls tick() where a "Processed in" line is due; then the
    // --profile series line.
    template <class Column>
    void solve(int64_t off, const double* x0, bool chain, const float* frame_beta, Column&& column) {
        const size_t npix = (size_t)mf_.nrows();
        auto src = [&](int64_t j, double* dst) {  // series index j = frame off + j
            const std::vector<double> f = ra_.take(j + off);
            if (f.size() != npix) throw std::runtime_error("frame size does not match the shard's pixels");
            std::copy(f.begin(), f.end(), dst);
        };
        double sink_ms = 0.0;  // (--profile: rank 0's writes)
        prev_ = Clock::now();
        auto sink = [&](int64_t j, const double* xs, const SolveInfo& info) {
            if (d_.rank != 0) return;
            const auto tsk = Clock::now();
            column(j + off, xs, info);
            sink_ms += ms_since(tsk);
        };
        mf_.solve_series(n_ - off, src, sink, x0, chain, frame_beta);
        if (d_.rank == 0 && d_.profile.is_open()) write_series_line(d_.profile, mf_, ra_.reader_ms(), sink_ms);
    }
    double tick() {  // prints "Processed in": the time since the previous line (the first: since solve() began)
        const auto now = Clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - prev_).count();
        prev_ = now;
        std::cout << "Processed in: " << ms << " ms" << std::endl;
        return ms;
    }

   private:
    Driver& d_;
    MultiFrameEngine& mf_;
    const int64_t n_;
    FrameReadahead ra_;
    Clock::time_point prev_;
};

// --beta_scan: what rank 0 keeps of the columns between the series and the scan pass (the solutions are in the file)
struct ScanColumns {
    std::unique_ptr<ScanWriter> file;         // rank 0
    std::vector<int32_t> status, iterations;  // [T nb], rank 0
    std::vector<uint8_t> ok;                  // [T nb], rank 0: the column did not stop on a non-finite iterate
};

// --holdout: what the run shares between the series and the hold-out pass. K, the fold table over all pixels and the
// cameras' pixel ranges are the same on every rank; the columns' solutions are in the file
struct HoldoutColumns {
    int K = 0;                                // folds: --holdout K, or the number of cameras
    std::vector<double> betas;                // [nb]: --holdout_betas, or -b alone
    std::vector<int32_t> folds;               // [npixel]
    std::vector<int64_t> cam_start;           // [ncam + 1]
    std::unique_ptr<HoldoutWriter> file;      // rank 0
    std::vector<int32_t> status, iterations;  // [T nb (K + 1)], rank 0
    std::vector<uint8_t> ok;                  // [T nb (K + 1)], rank 0: the column did not stop on a non-finite iterate
    int64_t nb() const { return (int64_t)betas.size(); }
    int64_t ncam() const { return (int64_t)cam_start.size() - 1; }
};

// frames: the composite frames to solve; warm: the resumed solution (all voxels) or empty
void run_frames(Driver& d, Solvers& s, const std::vector<uint64_t>& frames, std::vector<double> warm);
void run_series(Driver& d, Solvers& s, const std::vector<uint64_t>& frames, const std::vector<double>& warm);
void run_scan_series(Driver& d, Solvers& s, const std::vector<uint64_t>& frames, ScanColumns& sc);
void run_replica_series(Driver& d, Solvers& s, const std::vector<uint64_t>& frames);
void run_holdout_series(Driver& d, Solvers& s, const std::vector<uint64_t>& frames, HoldoutColumns& hc);
// --phantom: the frames are projections of the phantom file's rows on this rank's shard; the number of phantoms
uint64_t run_phantom_series(Driver& d, Solvers& s, const Shard& sh);
// after the frames, main thread, collective; the engines released (their device buffers)
void run_fit_pass(Driver& d, const Shard& sh);
void run_scan_pass(Driver& d, const Shard& sh, const Csr& lap, const std::vector<uint64_t>& frames, ScanColumns& sc);
void run_holdout_pass(Driver& d, const Shard& sh, const std::vector<uint64_t>& frames, HoldoutColumns& hc);

}  // namespace sart
