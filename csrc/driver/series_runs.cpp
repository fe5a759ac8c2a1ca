// The native driver's frame loops over the measured frames: frame by frame (run_frames) and --batch_frames
// (run_series with its lead frame).
#include <cmath>
#include <future>

#include "driver.hpp"

namespace sart {
namespace {

// A cold time series: its first frame is solved alone by the single-frame engine (the fused sweep, half the time of a
// batched sweep) and starts the chain as a converged source -- frames chained from a cold start's young iterates
// would carry its error for ~100 frames (profiles/series_r6_*). SART_MF_LEAD_ENGINE=0: the multi-frame engine's own
// lead frame instead (MfQueue::lead). off: the first frame the batch solves; iters: the lead's update count (-1: no
// lead); bwarm: the batch's start value (a resumed series starts from the stored solution instead).
struct Lead {
    int64_t off = 0;
    int iters = -1;
    std::vector<double> bwarm;
};
Lead solve_lead_frame(Driver& d, Solvers& s, FrameReadahead& ra, const std::vector<uint64_t>& frames,
                      std::vector<double> bwarm) {
    Lead lead{0, -1, std::move(bwarm)};
    if (!s.lead_engine || !lead.bwarm.empty() || frames.empty()) return lead;
    const auto t0 = Clock::now();
    std::vector<double> x0s(d.in.nvoxel);
    // frame 0 from the reader thread (which goes on reading the next frames meanwhile)
    const std::vector<double> g0 = ra.take(0);
    const SolveInfo info = s.lead_engine->solve(g0.data(), nullptr, x0s.data());
    s.lead_engine.reset();
    const double ms = ms_since(t0);
    const bool handover = s.lead_tol > 1.0;
    if (d.rank == 0 && !handover) {
        const double time = d.image->frame_time(frames[0]);
        d.writer->add(x0s, info.status, time, d.image->camera_frame_time(frames[0]), info.iterations);
        std::cout << "Processed in: " << ms << " ms" << std::endl;
        if (d.profile.is_open()) write_lead_line(d.profile, {frames[0], time, ms}, info, d.cfg.batch_frames);
    }
    if (std::all_of(x0s.begin(), x0s.end(), [](double v) { return std::isfinite(v); })) lead.bwarm = x0s;
    lead.iters = info.iterations;
    // handover: frame 0 is solved on in the batch from this iterate (its reported update count includes the lead's),
    // as are the first frames chained from it; else the lead is frame 0.
    // ADVICE.md (lead frame lost): a handover whose iterate is non-finite gives off = 1 with frame 0 never written
    lead.off = (handover && !lead.bwarm.empty()) ? 0 : 1;
    return lead;
}

}  // namespace

// --batch_frames N: N slots on the matrix cores, refilled on the device (MultiFrameEngine::solve_series): the sweep in
// which a frame finishes admits the next staged frame into its slot. The whole series is one stream (SeriesRun);
// finished frames (out of order) are written in time order. Without --no_guess the frames form a warm-started time
// series -- each starts from the current iterate of the newest frame in flight, rescaled (the resumed solution starts
// the first ones); with --no_guess every frame cold-starts.
void run_series(Driver& d, Solvers& s, const std::vector<uint64_t>& frames, const std::vector<double>& warm) {
    const Config& cfg = d.cfg;
    const CompositeImage& image = *d.image;
    SeriesRun run(d, *s.mf, (int64_t)frames.size(), [&](int64_t k) { return d.image->frame(frames[k]); });
    const Lead lead = solve_lead_frame(d, s, run.readahead(), frames, cfg.no_guess ? std::vector<double>() : warm);
    s.lead_engine.reset();
    const int64_t off = lead.off;
    InOrder<std::pair<std::vector<double>, SolveInfo>> done(off);  // rank 0: finished frames, written in time order
    const double* x0 = lead.bwarm.empty() ? nullptr : lead.bwarm.data();
    run.solve(off, x0, !cfg.no_guess, nullptr, [&](int64_t k, const double* xs, const SolveInfo& info) {
        SolveInfo fi = info;
        if (fi.warm_from >= 0) {
            fi.warm_from += (int)off;
        } else if (lead.iters >= 0 && k == 0) {  // the lead frame, finished in the batch (handover)
            fi.iterations += lead.iters;
        } else if (lead.iters >= 0) {  // started from the lead frame's solution / handed-over iterate
            fi.warm_from = 0;
            fi.warm_iter = lead.iters;
            fi.warm_live = false;
        }
        done.put(k, std::make_pair(std::vector<double>(xs, xs + d.in.nvoxel), fi));
        done.drain([&](int64_t w, std::pair<std::vector<double>, SolveInfo>&& it) {
            const uint64_t cur = frames[w];
            const SolveInfo& fi = it.second;
            d.writer->add(it.first, fi.status, image.frame_time(cur), image.camera_frame_time(cur), fi.iterations);
            const double ms = run.tick();
            if (fi.nonfinite) std::cerr << "warning: frame " << cur << ": non-finite iterate, stopped" << std::endl;
            if (d.profile.is_open())
                write_batched_line(d.profile, {cur, image.frame_time(cur), ms}, fi, cfg.batch_frames,
                                   fi.warm_from >= 0 ? (int64_t)frames[fi.warm_from] : -1);
        });
    });
}

// Frame by frame on the single-frame engine, the fp64 engine or the CPU solver; the next composite frame is read on a
// helper thread during the solve. warm: the resumed solution (all voxels) or empty.
void run_frames(Driver& d, Solvers& s, const std::vector<uint64_t>& frames, std::vector<double> warm) {
    const Config& cfg = d.cfg;
    CompositeImage& image = *d.image;
    const Block& vblk = d.vblk;
    if (d.cols && !warm.empty())  // this rank's voxels of the stored solution
        warm = std::vector<double>(warm.begin() + vblk.offset, warm.begin() + vblk.offset + vblk.size);
    std::vector<double> solution = warm, x(vblk.size), xfull(d.cols ? d.in.nvoxel : 0);
    const char* wd = std::getenv("SART_WARM_ON_DEVICE");
    const bool warm_dev = !(wd && *wd && std::atoi(wd) == 0);
    std::future<std::vector<double>> fut;
    if (!frames.empty()) fut = std::async(std::launch::async, [&image, i = frames[0]]() { return image.frame(i); });
    for (size_t k = 0; k < frames.size(); ++k) {
        const uint64_t cur = frames[k];
        const auto tf = Clock::now();
        std::vector<double> frame = fut.get();
        const double wait_frame_ms = ms_since(tf);
        if (k + 1 < frames.size())  // prefetch the next composite frame during the solve
            fut = std::async(std::launch::async, [&image, i = frames[k + 1]]() { return image.frame(i); });
        const auto t0 = Clock::now();
        const double* x0 = (cfg.no_guess || solution.empty()) ? nullptr : solution.data();
        // from frame 1 on, a warm start is the engine's own previous solution: rescaled on the device
        // (SART_WARM_ON_DEVICE=0: through the host copy, for A/B runs)
        const SolveInfo info = s.engine64 ? s.engine64->solve(frame.data(), x0, x.data())
                               : d.gpu    ? s.engine->solve(frame.data(), x0, x.data(), k > 0 && x0 != nullptr && warm_dev)
                                          : s.cpu->solve(frame.data(), x0, x.data());
        if (info.fallbacks) std::cerr << "warning: fused sweep fell back " << info.fallbacks << " time(s)" << std::endl;
        if (info.comm_fallbacks && d.rank == 0)
            std::cerr << "warning: frame " << cur << ": device all-reduce timed out; re-solved on "
                      << (d.dcomm ? d.dcomm->backend() : "the base communicator") << std::endl;
        if (info.nonfinite) std::cerr << "warning: frame " << cur << ": non-finite iterate, stopped" << std::endl;
        solution = x;
        if (d.cols) {  // gather the voxel blocks (zero-filled sum over ranks)
            std::fill(xfull.begin(), xfull.end(), 0.0);
            std::copy(x.begin(), x.end(), xfull.begin() + vblk.offset);
            d.host->all_reduce_host(xfull.data(), xfull.size(), ReduceOp::kSum);
        }
        if (d.rank == 0) {
            const auto tw = Clock::now();
            d.writer->add(d.cols ? xfull : x, info.status, image.frame_time(cur), image.camera_frame_time(cur),
                          info.iterations);
            const auto t1 = Clock::now();
            const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
            std::cout << "Processed in: " << ms << " ms" << std::endl;  // reference main.cpp:132-137
            if (d.profile.is_open()) {
                const double elem = d.gpu && (cfg.rtm_bf16 || cfg.rtm_f16) ? 2.0 : 4.0;  // bytes per stored RTM element
                const double writer_ms = std::chrono::duration<double, std::milli>(t1 - tw).count();
                write_frame_line(d.profile, {cur, image.frame_time(cur), ms}, info,
                                 {d.gpu, (double)d.in.npixel * (double)d.in.nvoxel, elem, writer_ms, wait_frame_ms,
                                  d.size, d.host->backend(), d.dcomm ? d.dcomm->describe() : "none"});
            }
        }
        // --no_guess, or a frame whose iterate stayed non-finite (the NaN/Inf guard returned the last finite
        // iterate when there was one): the next frame cold-starts instead of inheriting NaN
        if (cfg.no_guess ||
            (info.nonfinite && !std::all_of(x.begin(), x.end(), [](double v) { return std::isfinite(v); })))
            solution.clear();
    }
}

}  // namespace sart
