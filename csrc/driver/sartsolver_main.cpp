// sartsolver -- native driver binary: same CLI, input validation, frame loop, output file
// and console output as the reference binary (reference main.cpp:25-151), MI355X-first:
//
//   * one process per GPU, any launcher that sets RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR /
//     MASTER_PORT (torchrun --no-python, mpirun via OMPI_COMM_WORLD_*, or bin/sartsolver); one process
//     runs without any launcher. Rank -> GPU = LOCAL_RANK % device count (reference: rank % count,
//     sartsolver_cuda.cpp:96-98).
//   * per-iteration reductions on device buffers (csrc/engine/comm.cpp): the one-shot P2P all-reduce over
//     xGMI or RCCL; host scalars over the TCP or MPI bootstrap (mpiexec launches use MPI_COMM_WORLD); the
//     --use_cpu path uses the host communicator alone.
//   * every rank streams only its pixel rows from HDF5 straight into HBM through two pinned staging
//     buffers (the reference keeps the whole shard in host RAM, raytransfer.hpp:20); with
//     --parallel_read all ranks read at once, otherwise in turn (reference main.cpp:78-86).
//   * the next composite frame is read on a helper thread while the current one is solved.
//   * a fatal error on any rank aborts the communicators instead of leaving peers blocked in a
//     collective (the reference calls std::exit on one rank).
// Extensions: --resume, --two_pass, --profile FILE (JSON lines per frame: iterations, convergence, it/s,
// GFLOPS, RTM GB/s, GPU time in the all-reduces, communicators), --batch_frames N (N
// frames solved together by the multi-frame MFMA engine; batches warm-start from the previous batch), --fit / --fit_only
// (after the frames: fp64 fitted images and residuals of every stored solution into the output's /fit group),
// --beta_scan B0,B1,... (every frame at each Laplacian weight as columns of the multi-frame engine; the L-curve into
// the output's /beta_scan group, its corner's solution into /solution), --replicas N (every frame and N noisy replicas
// of it as columns of the multi-frame engine; per-voxel mean and spread into the output's /uncertainty group).
// This file: main()'s sequence and the runs it starts (run_series, run_frames, run_fit_pass, run_scan,
// run_replica_series). The shard and its loaders: shard_load.{hpp,cpp}; the series' frame reader:
// frame_readahead.hpp; the --profile lines: profile_lines.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <future>
#include <iostream>
#include <limits>
#include <map>
#include <sstream>
#include <tuple>
#include <sys/prctl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <csignal>
#include <cstdlib>
#include <cstring>

#include "../engine/comm.hpp"
#include "../engine/engine64.hpp"
#include "../engine/multiframe.hpp"
#include "../kernels/launchers.hpp"
#include "../native/cpu_solver.hpp"
#include "../native/fit.hpp"
#include "../native/frames.hpp"
#include "../native/lcurve.hpp"
#include "../native/uncertainty.hpp"
#include "frame_readahead.hpp"
#include "profile_lines.hpp"
#include "shard_load.hpp"

using namespace sart;

namespace {

using Clock = std::chrono::steady_clock;

// What main() sets up once and the runs share
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

Solvers build_solvers(const Driver& d, Shard& sh, const SolverParams& params, const Csr& lap) {
    const Config& cfg = d.cfg;
    Solvers s;
    EngineConfig base;
    static_cast<SolverParams&>(base) = params;
    auto single = [&](double tol_factor) {
        EngineConfig ec = base;
        ec.conv_tolerance *= tol_factor;
        // f16 shards: the two-pass kernels unless --rtm_f16_fused opts in to the fused f16 sweep
        ec.f16_fused = cfg.rtm_f16_fused;
        ec.use_fused = !cfg.two_pass && (!cfg.rtm_f16 || cfg.rtm_f16_fused);
        ec.fused_min_bytes = fused_min_bytes_from_env();
        if (const char* v = std::getenv("SART_FUSED_VARIANT"); v && *v) ec.fused_variant = std::atoi(v);
        ec.time_collectives = !cfg.profile_file.empty();  // --profile: GPU time in the all-reduces per frame
        if (d.cols) {
            ec.column_shard = true;
            ec.col_offset = (int64_t)d.vblk.offset;
            ec.nvoxel_total = (int64_t)d.in.nvoxel;
        }
        return make_engine<Engine>(sh, d.device, d.dcomm.get(), ec, lap);
    };
    if (d.gpu && cfg.batch_frames > 1) {
        // batch width 16, 32, 64 or 128 (rounded up; 128: bf16 storage and f16-pair split-A); sparse shards: fp32 SpMM
        // projections of the CSR / CSC; bf16 / f16 shards: MFMA projections
        base.mf_frames = cfg.batch_frames;
        base.mf_frame_beta = !cfg.beta_scan.empty();  // the scan brings a weight per column: keep the Laplacian
        s.mf = make_engine<MultiFrameEngine>(sh, d.device, d.dcomm.get(), base, lap);
        // a cold time series' first frame: the single-frame engine, built with the set-up (before the frame loop's
        // clock, like the frame-by-frame engine); dropped after that frame (SART_MF_LEAD_ENGINE=0: none)
        const char* le = std::getenv("SART_MF_LEAD_ENGINE");
        if (const char* lt = std::getenv("SART_MF_LEAD_TOL"); lt && *lt) s.lead_tol = std::max(1.0, std::atof(lt));
        if (!cfg.no_guess && !(le && *le && std::atoi(le) == 0)) s.lead_engine = single(s.lead_tol);
    } else if (d.gpu && cfg.fp64) {  // the double-precision engine, frame by frame
        s.engine64 = make_engine<Engine64>(sh, d.device, d.dcomm.get(), base, lap, cfg.fp64_semantics == "gpu");
    } else if (d.gpu && !cfg.fit_only) {
        s.engine = single(1.0);
    } else if (!cfg.fit_only) {
        if (sh.csr_format)
            s.cpu = std::make_unique<CpuSolver>(std::move(sh.csr), d.host, params, false);
        else
            s.cpu = std::make_unique<CpuSolver>(sh.host.data(), (int64_t)d.blk.size, (int64_t)d.in.nvoxel,
                                                (int64_t)d.in.nvoxel, d.host, params, false);
        if (lap.nnz()) s.cpu->set_laplacian(lap);
    }
    return s;
}

// first profile line: the HDF5 -> HBM load (slowest rank's wall time; totals over ranks). Collective.
void profile_load(Driver& d, const Shard& sh, const LoadStats& ls, const Solvers& s) {
    LoadLine l{{ls.wall_s, ls.rss_hwm_after_mb - ls.rss_hwm_before_mb, ls.setup_s, (double)ls.bytes},
               {(double)ls.bytes, ls.read_s, ls.h2d_s, ls.wait_read_s, ls.wait_copy_s},
               {(double)ls.f16_flushed, (double)ls.f16_nonzeros}};
    static_assert(sizeof(l.max) == 4 * sizeof(double) && sizeof(l.sum) == 5 * sizeof(double) &&
                  sizeof(l.f16) == 2 * sizeof(double), "each group is reduced as an array of doubles");
    d.host->all_reduce_host(&l.max.load_s, 4, ReduceOp::kMax);
    d.host->all_reduce_host(&l.sum.bytes, 5, ReduceOp::kSum);
    d.host->all_reduce_host(&l.f16.flushed, 2, ReduceOp::kSum);
    if (!d.profile.is_open()) return;
    l.ranks = d.size;
    l.parallel_read = d.cfg.parallel_read || d.size == 1;
    l.has_sparse = d.in.has_sparse;
    l.format = sh.format, l.storage = sh.storage;
    l.solver_path = d.cfg.fit_only ? "none (fit only)" : "cpu";
    if (s.mf)
        l.solver_path = "multi-frame " + s.mf->forward_split() + " / " + s.mf->backproject_split();
    else if (s.engine64)
        l.solver_path = "fp64-two-pass", l.fp64_semantics = d.cfg.fp64_semantics;
    else if (s.engine)
        l.solver_path = sh.csr_format ? "sparse two-pass" : (s.engine->use_fused() ? "fused" : "two-pass");
    l.nnz = sh.nnz;
    write_load_line(d.profile, l, ls);
}

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

// --batch_frames N: N slots on the matrix cores, refilled on the device (MultiFrameEngine::solve_series): the sweep in
// which a frame finishes admits the next staged frame into its slot. The whole series is one stream: a reader thread
// keeps up to 4 N frames read ahead, the engine stages them into its device queue while earlier frames sweep, and
// finished frames (out of order) are written in time order. Without --no_guess the frames form a warm-started time
// series -- each starts from the current iterate of the newest frame in flight, rescaled (the resumed solution starts
// the first ones); with --no_guess every frame cold-starts.
void run_series(Driver& d, Solvers& s, const std::vector<uint64_t>& frames, const std::vector<double>& warm) {
    const Config& cfg = d.cfg;
    const CompositeImage& image = *d.image;
    const int64_t nfr = (int64_t)frames.size();
    FrameReadahead ra(nfr, 4 * (int64_t)cfg.batch_frames, [&](int64_t k) { return d.image->frame(frames[k]); });
    const Lead lead = solve_lead_frame(d, s, ra, frames, cfg.no_guess ? std::vector<double>() : warm);
    s.lead_engine.reset();
    const int64_t off = lead.off;
    const size_t npix = (size_t)s.mf->nrows();
    auto src = [&](int64_t j, double* dst) {  // series index j = frame off + j
        const std::vector<double> f = ra.take(j + off);
        if (f.size() != npix) throw std::runtime_error("frame size does not match the shard's pixels");
        std::copy(f.begin(), f.end(), dst);
    };
    // rank 0: finished frames written in time order
    std::map<int64_t, std::pair<std::vector<double>, SolveInfo>> done;
    int64_t written = off;
    double sink_ms = 0.0;  // (--profile: rank 0's writes)
    auto t_prev = Clock::now();
    auto sink = [&](int64_t j, const double* xs, const SolveInfo& info) {
        if (d.rank != 0) return;
        const auto tsk = Clock::now();
        SolveInfo fi = info;
        if (fi.warm_from >= 0) {
            fi.warm_from += (int)off;
        } else if (lead.iters >= 0 && j + off == 0) {  // the lead frame, finished in the batch (handover)
            fi.iterations += lead.iters;
        } else if (lead.iters >= 0) {  // started from the lead frame's solution / handed-over iterate
            fi.warm_from = 0;
            fi.warm_iter = lead.iters;
            fi.warm_live = false;
        }
        done.emplace(j + off, std::make_pair(std::vector<double>(xs, xs + d.in.nvoxel), fi));
        for (auto it = done.find(written); it != done.end(); it = done.find(written)) {
            const uint64_t cur = frames[written];
            const SolveInfo& fi = it->second.second;
            d.writer->add(it->second.first, fi.status, image.frame_time(cur), image.camera_frame_time(cur),
                          fi.iterations);
            const auto now = Clock::now();
            const double ms = std::chrono::duration<double, std::milli>(now - t_prev).count();
            t_prev = now;
            std::cout << "Processed in: " << ms << " ms" << std::endl;
            if (fi.nonfinite) std::cerr << "warning: frame " << cur << ": non-finite iterate, stopped" << std::endl;
            if (d.profile.is_open())
                write_batched_line(d.profile, {cur, image.frame_time(cur), ms}, fi, cfg.batch_frames,
                                   fi.warm_from >= 0 ? (int64_t)frames[fi.warm_from] : -1);
            done.erase(it);
            ++written;
        }
        sink_ms += ms_since(tsk);
    };
    s.mf->solve_series(nfr - off, src, sink, lead.bwarm.empty() ? nullptr : lead.bwarm.data(), !cfg.no_guess);
    if (d.rank == 0 && d.profile.is_open()) write_series_line(d.profile, *s.mf, ra.reader_ms(), sink_ms);
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

// solutions per pass over the shard: the width at which a frame costs least for the storage (8; 4 on 16-bit shards)
int fit_group(const Shard& sh) {
    const DeviceShard* dn = sh.dense.get();
    int group = fit64_group(dn && dn->bf16, dn && dn->f16, !dn);
    if (const char* e = std::getenv("SART_FIT_GROUP"); e && *e) {  // (an A/B knob: the file does not depend on it)
        group = std::atoi(e);
        if (group < 1 || group > 8) throw Error(std::string("SART_FIT_GROUP must be within 1 .. 8, not '") + e + "'");
    }
    return group;
}

// The fit projection of this rank's shard (run_fit_pass, run_scan_pass): device operands X [group][ldx], F [group][ldf]
// and the sparse kernel's voxel-major copy of X
struct FitProjector {
    const Driver& d;
    const Shard& sh;
    const int group;
    DeviceArray<double> dX, dF, dXt;
    int64_t ldx = 0, ldf = 0;
    SparseRtm view;
    FitProjector(const Driver& d_, const Shard& sh_, int group_) : d(d_), sh(sh_), group(group_) {
        const DeviceShard* dn = sh.dense.get();
        if (dn) {
            ldx = dn->ld;
            ldf = dn->nrows_pad;
        } else if (sh.sparse) {
            ldx = (sh.sparse->nvoxel + 63) / 64 * 64;
            ldf = (sh.sparse->nrows + 63) / 64 * 64;
            dXt.resize((size_t)ldx * 8);
            view = sh.sparse->view();
        }
        if (sh.gpu) {
            dX.resize((size_t)group * ldx);
            dF.resize((size_t)group * ldf);
        }
    }
    // out [n][npixel] += this rank's part of A X^T for X [n][nvoxel] (out zero-filled by the caller); on a GPU shard
    // dX keeps this rank's voxels of the n solutions afterwards
    void project(const double* X, int n, double* out) {
        const uint64_t npixel = d.in.npixel, nvoxel = d.in.nvoxel;
        const Block &blk = d.blk, &vblk = d.vblk;
        const DeviceShard* dn = sh.dense.get();
        if (sh.gpu) {
            for (int j = 0; j < n; ++j)
                hip_ok(hipMemcpy(dX.get() + (size_t)j * ldx, X + (size_t)j * nvoxel + vblk.offset,
                                 vblk.size * sizeof(double), hipMemcpyHostToDevice), "H2D fit solutions");
            if (dn)
                launch_fit64(dn->A, dn->bf16, dn->f16, dn->rsc.get(), dn->ld, dn->nrows, dn->nrows_pad, dn->nvoxel,
                             dX.get(), ldx, n, dF.get(), ldf, nullptr);
            else
                launch_fit64_csr(view, sh.sparse->nrows, sh.sparse->nvoxel, ldx, dX.get(), ldx, n, dXt.get(), dF.get(),
                                 ldf, nullptr);
            for (int j = 0; j < n; ++j)
                hip_ok(hipMemcpy(out + (size_t)j * npixel + blk.offset, dF.get() + (size_t)j * ldf,
                                 blk.size * sizeof(double), hipMemcpyDeviceToHost), "D2H fitted images");
        } else if (sh.csr_format) {
            cpu_fit_forward(sh.csr, X, (int64_t)nvoxel, n, out + blk.offset, (int64_t)npixel);
        } else {
            cpu_fit_forward(sh.host.data(), (int64_t)blk.size, (int64_t)nvoxel, (int64_t)nvoxel, X, (int64_t)nvoxel, n,
                            out + blk.offset, (int64_t)npixel);
        }
    }
};

// --fit / --fit_only: the fitted images f = A x (fp64) of every solution stored in the output file, in groups of up to
// 8 per pass over the shard (4 on bf16 / f16 shards; SART_FIT_GROUP overrides), and their residuals against the
// measured composite frames, into the file's /fit group (docs/FORMATS.md). Main thread, after the frame loop, with the
// solution writer closed. Rank 0 reads the stored solutions and broadcasts them, every rank projects on its shard (row
// shards: its rows; column shards: partial sums over its voxels for all pixels), the images are summed over the ranks
// through a zero-filled host all-reduce, rank 0 computes the statistics and writes. A value depends on its pixel row
// and solution only (csrc/kernels/fit64.hip), so the file is the same for any grouping and any number of row-shard ranks.
void run_fit_pass(Driver& d, const Shard& sh) {
    const Config& cfg = d.cfg;
    const InputSet& in = d.in;
    HostComm* host = d.host;
    const CompositeImage& image = *d.image;
    const auto t_fit = Clock::now();
    const uint64_t npixel = in.npixel, nvoxel = in.nvoxel;
    std::vector<double> times;
    if (d.rank == 0) times = read_solution_times(cfg.output_file);
    uint64_t T = times.size();
    host->broadcast_host(&T, sizeof(T), 0);
    if (T == 0)
        throw Error("Argument " + std::string(cfg.fit_only ? "fit_only" : "fit") + " needs solutions to project: " +
                    cfg.output_file + " is missing or holds none.");
    times.resize(T);
    host->broadcast_host(times.data(), T * sizeof(double), 0);
    // a stored frame belongs to the composite frame of its time (the rule of --resume)
    std::vector<uint64_t> frame_of(T);
    for (uint64_t k = 0; k < T; ++k) {
        uint64_t i = 0;
        while (i < image.nframe() && !(std::abs(image.frame_time(i) - times[k]) <= 1e-12)) ++i;
        if (i == image.nframe()) {
            std::ostringstream os;
            os.precision(17);
            os << "Stored solution time " << times[k] << " has no composite frame in the selected time range.";
            throw Error(os.str());
        }
        frame_of[k] = i;
    }
    FitProjector fp(d, sh, fit_group(sh));
    const int group = fp.group;
    // the ray lengths: the fit projection of the all-ones vector (one extra pass; any storage, no engine needed)
    std::vector<double> ell(npixel, 0.0);
    {
        const std::vector<double> ones(nvoxel, 1.0);
        fp.project(ones.data(), 1, ell.data());
        host->all_reduce_host(ell.data(), ell.size(), ReduceOp::kSum);
    }
    std::unique_ptr<FitWriter> fw;
    std::unique_ptr<CompositeImage> full;  // rank 0: the measured frames over all pixels
    std::vector<int64_t> camera_pixels;
    if (d.rank == 0) {
        for (const auto& cam : in.camera_names) {
            const auto& mask = in.frame_masks.at(cam);
            camera_pixels.push_back((int64_t)std::count_if(mask.begin(), mask.end(), [](int32_t v) { return v != 0; }));
        }
        full = std::make_unique<CompositeImage>(in.image_files, in.frame_masks, d.intervals, npixel, 0);
        full->set_max_cache_size((uint64_t)cfg.max_cached_frames);
        fw = std::make_unique<FitWriter>(cfg.output_file, T, npixel, in.camera_names.size());
    }
    std::vector<double> X((size_t)group * nvoxel), F((size_t)group * npixel);
    uint64_t groups = 0;
    for (uint64_t k0 = 0; k0 < T; k0 += group, ++groups) {
        const int n = (int)std::min<uint64_t>(group, T - k0);
        if (d.rank == 0) {
            const std::vector<double> rows = read_solution_rows(cfg.output_file, k0, n, nvoxel);
            std::copy(rows.begin(), rows.end(), X.begin());
        }
        host->broadcast_host(X.data(), (size_t)n * nvoxel * sizeof(double), 0);
        std::fill(F.begin(), F.begin() + (size_t)n * npixel, 0.0);
        fp.project(X.data(), n, F.data());
        host->all_reduce_host(F.data(), (size_t)n * npixel, ReduceOp::kSum);
        if (d.rank == 0)
            for (int j = 0; j < n; ++j) {
                const std::vector<double> g = full->frame(frame_of[k0 + j]);
                const double* f = F.data() + (size_t)j * npixel;
                fw->write(k0 + j, f, fit_statistics(f, g.data(), ell.data(), (int64_t)npixel,
                                                    cfg.ray_length_threshold, camera_pixels));
            }
    }
    host->barrier();
    if (d.rank == 0) {
        const double ms = ms_since(t_fit);
        std::cout << "Fit of " << T << " frame(s) in: " << ms << " ms" << std::endl;
        if (d.profile.is_open()) write_fit_line(d.profile, T, groups, ms, sh.storage, sh.format, d.size);
    }
}

// --beta_scan: what rank 0 keeps of the columns between the series and the scan pass (the solutions are in the file)
struct ScanColumns {
    std::unique_ptr<ScanWriter> file;       // rank 0
    std::vector<int32_t> status, iterations;  // [T nb], rank 0
    std::vector<uint8_t> ok;                  // [T nb], rank 0: the column did not stop on a non-finite iterate
};

// --beta_scan, the frame loop: run_series over T nb virtual frames, virtual frame j = k nb + i being composite frame k
// at weight i, all cold columns of the multi-frame engine with a weight per column. Rank 0's sink writes every
// finished column into /beta_scan as it arrives (no host collective in the sink: the series thread interleaves staging
// and delivery differently on different ranks); nothing goes to /solution yet.
void run_scan_series(Driver& d, Solvers& s, const std::vector<uint64_t>& frames, ScanColumns& sc) {
    const Config& cfg = d.cfg;
    const int64_t nb = (int64_t)cfg.beta_scan.size(), T = (int64_t)frames.size(), nvirt = T * nb;
    FrameReadahead ra(nvirt, 4 * (int64_t)cfg.batch_frames,
                      [&](int64_t j) { return d.image->frame(frames[j / nb]); });  // (the image caches its frames)
    const size_t npix = (size_t)s.mf->nrows();
    auto src = [&](int64_t j, double* dst) {
        const std::vector<double> f = ra.take(j);
        if (f.size() != npix) throw std::runtime_error("frame size does not match the shard's pixels");
        std::copy(f.begin(), f.end(), dst);
    };
    std::vector<float> frame_beta((size_t)nvirt);
    for (int64_t j = 0; j < nvirt; ++j) frame_beta[j] = (float)cfg.beta_scan[j % nb];
    std::vector<int64_t> left((size_t)T, nb);  // columns of each composite frame still to come
    double sink_ms = 0.0;
    auto t_prev = Clock::now();
    auto sink = [&](int64_t j, const double* xs, const SolveInfo& info) {
        if (d.rank != 0) return;
        const auto tsk = Clock::now();
        const int64_t k = j / nb, i = j % nb;
        sc.file->write_column((uint64_t)k, (uint64_t)i, xs, info.status, info.iterations);
        sc.status[j] = info.status, sc.iterations[j] = info.iterations, sc.ok[j] = info.nonfinite ? 0 : 1;
        if (info.nonfinite)
            std::cerr << "warning: frame " << frames[k] << ", beta " << cfg.beta_scan[i]
                      << ": non-finite iterate, stopped" << std::endl;
        if (--left[k] == 0) {
            const auto now = Clock::now();
            std::cout << "Processed in: " << std::chrono::duration<double, std::milli>(now - t_prev).count() << " ms"
                      << std::endl;
            t_prev = now;
        }
        sink_ms += ms_since(tsk);
    };
    s.mf->solve_series(nvirt, src, sink, nullptr, false, frame_beta.data());
    if (d.rank == 0) sc.file->close();
    if (d.rank == 0 && d.profile.is_open()) write_series_line(d.profile, *s.mf, ra.reader_ms(), sink_ms);
}

// --beta_scan, after the loop (main thread, shaped like run_fit_pass): the rows of /beta_scan/value in groups of
// fit_group() -- rank 0 reads and broadcasts a group, every rank projects it on its shard, the images are summed over
// the ranks through the zero-filled host all-reduce, rank 0 takes the residual norm against the frame's measured
// pixels (the /fit/residual_norm definition) and the roughness norm of the same device copy of the group
// (csrc/kernels/rough64.hip). A frame whose nb points are complete gets its corner (lcurve_corner); the selected
// column goes to /solution through the ordinary writer, in frame order.
void run_scan_pass(Driver& d, const Shard& sh, const Csr& lap, const std::vector<uint64_t>& frames, ScanColumns& sc) {
    const Config& cfg = d.cfg;
    HostComm* host = d.host;
    const CompositeImage& image = *d.image;
    const auto t_scan = Clock::now();
    const uint64_t npixel = d.in.npixel, nvoxel = d.in.nvoxel;
    const uint64_t nb = cfg.beta_scan.size(), T = frames.size(), nvirt = T * nb;
    // -b names the fallback: the ladder entry nearest to it (ties to the smaller)
    int fallback = 0;
    for (uint64_t i = 1; i < nb; ++i)
        if (std::abs(cfg.beta_scan[i] - cfg.beta_laplace) < std::abs(cfg.beta_scan[fallback] - cfg.beta_laplace))
            fallback = (int)i;
    FitProjector fp(d, sh, fit_group(sh));
    const int group = fp.group;
    std::vector<double> ell(npixel, 0.0);
    {
        const std::vector<double> ones(nvoxel, 1.0);
        fp.project(ones.data(), 1, ell.data());
        host->all_reduce_host(ell.data(), ell.size(), ReduceOp::kSum);
    }
    std::unique_ptr<CompositeImage> full;  // rank 0: the measured frames over all pixels
    DeviceArray<int64_t> lrp;
    DeviceArray<int32_t> lcol;
    DeviceArray<float> lval;
    DeviceArray<double> deta2, dscratch;
    if (d.rank == 0) {
        full = std::make_unique<CompositeImage>(d.in.image_files, d.in.frame_masks, d.intervals, npixel, 0);
        full->set_max_cache_size((uint64_t)cfg.max_cached_frames);
        lrp.resize(nvoxel + 1), lcol.resize((size_t)lap.nnz()), lval.resize((size_t)lap.nnz());
        hip_ok(hipMemcpy(lrp.get(), lap.row_ptr.data(), (nvoxel + 1) * sizeof(int64_t), hipMemcpyHostToDevice), "H2D");
        hip_ok(hipMemcpy(lcol.get(), lap.col.data(), (size_t)lap.nnz() * sizeof(int32_t), hipMemcpyHostToDevice), "H2D");
        hip_ok(hipMemcpy(lval.get(), lap.val.data(), (size_t)lap.nnz() * sizeof(float), hipMemcpyHostToDevice), "H2D");
        deta2.resize(8);
        dscratch.resize((size_t)rough64_scratch_elems((int64_t)nvoxel));
    }
    const std::vector<int64_t> one_camera{(int64_t)npixel};  // the norm over all pixels does not depend on the split
    std::vector<double> X((size_t)group * nvoxel), F((size_t)group * npixel), rho(nvirt), eta(nvirt), x(nvoxel), g;
    uint64_t g_frame = T, decided = 0;  // g: the measured frame g_frame; frames [0, decided) have their corner
    for (uint64_t j0 = 0; j0 < nvirt; j0 += group) {
        const int n = (int)std::min<uint64_t>(group, nvirt - j0);
        if (d.rank == 0) sc.file->read_columns(j0, n, X.data());
        host->broadcast_host(X.data(), (size_t)n * nvoxel * sizeof(double), 0);
        std::fill(F.begin(), F.begin() + (size_t)n * npixel, 0.0);
        fp.project(X.data(), n, F.data());
        host->all_reduce_host(F.data(), (size_t)n * npixel, ReduceOp::kSum);
        if (d.rank != 0) continue;
        for (int j = 0; j < n; ++j) {
            const uint64_t k = (j0 + j) / nb;
            if (k != g_frame) g = full->frame(frames[k]), g_frame = k;
            rho[j0 + j] = fit_statistics(F.data() + (size_t)j * npixel, g.data(), ell.data(), (int64_t)npixel,
                                         cfg.ray_length_threshold, one_camera).residual_norm;
        }
        double eta2[8];
        launch_rough64(lrp.get(), lcol.get(), lval.get(), (int64_t)nvoxel, fp.dX.get(), fp.ldx, n, cfg.logarithmic,
                       deta2.get(), dscratch.get(), nullptr);
        hip_ok(hipMemcpy(eta2, deta2.get(), (size_t)n * sizeof(double), hipMemcpyDeviceToHost), "D2H roughness");
        for (int j = 0; j < n; ++j) eta[j0 + j] = std::sqrt(eta2[j]);
        for (; (decided + 1) * nb <= j0 + n; ++decided) {
            const uint64_t k = decided, cur = frames[k];
            const LcurveCorner c = lcurve_corner(rho.data() + k * nb, eta.data() + k * nb, sc.ok.data() + k * nb,
                                                 (int)nb, fallback);
            sc.file->write_frame(k, rho.data() + k * nb, eta.data() + k * nb, c.curvature.data(), c.selected,
                                 (uint8_t)c.found);
            const uint64_t js = k * nb + (uint64_t)c.selected;
            sc.file->read_columns(js, 1, x.data());  // the stored row itself: /solution/value[k] is its bits
            sc.file->close();                        // the solution writer opens the file itself
            d.writer->add(x, sc.status[js], image.frame_time(cur), image.camera_frame_time(cur), sc.iterations[js]);
        }
    }
    host->barrier();
    if (d.rank == 0)
        std::cout << "Beta scan of " << T << " frame(s) x " << nb << " weights in: " << ms_since(t_scan) << " ms"
                  << std::endl;
}

// A stream of its own with two events to time a kernel on it (--replicas: the noise and the moments kernels). What the
// constructor has created is released when a later creation fails.
struct TimedStream {
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    TimedStream() {
        try {
            hip_ok(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
            hip_ok(hipEventCreate(&e0), "hipEventCreate");
            hip_ok(hipEventCreate(&e1), "hipEventCreate");
        } catch (...) {
            release();
            throw;
        }
    }
    ~TimedStream() { release(); }
    TimedStream(const TimedStream&) = delete;
    TimedStream& operator=(const TimedStream&) = delete;
    double elapsed_ms() const {  // between the two events, both reached
        float ms = 0.f;
        hip_ok(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
        return ms;
    }

   private:
    void release() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// --replicas, the frame source's device side: the noisy replicas of this rank's pixels of a composite frame, generated
// by csrc/kernels/noise.hip in chunks of up to kNoiseMaxChunk replicas on a stream of its own. A replica's bits are a
// function of (seed, frame time, global pixel, replica): they depend neither on the chunk kept here nor on the thread or
// the order of the requests. The last chunk stays on the host, one vector per replica, and a replica is handed over by
// move (the series asks for a frame's replicas in order, each once; one asked for again is generated again).
class ReplicaSource {
   public:
    ReplicaSource(const Driver& d, int64_t npix) : d_(d), cfg_(d.cfg), npix_(npix), ldo_((npix + 63) / 64 * 64) {
        dg_.resize((size_t)ldo_);
        dout_.resize((size_t)kNoiseMaxChunk * ldo_);
        rows_.resize((size_t)kNoiseMaxChunk);
    }
    ReplicaSource(const ReplicaSource&) = delete;
    ReplicaSource& operator=(const ReplicaSource&) = delete;
    // replica r >= 1 of composite frame k (series index; g: its measured pixels of this rank, time: its time)
    std::vector<double> replica(int64_t k, const std::vector<double>& g, double time, int r) {
        if ((int64_t)g.size() != npix_) throw std::runtime_error("frame size does not match the shard's pixels");
        const int r0 = 1 + (r - 1) / kNoiseMaxChunk * kNoiseMaxChunk;
        if (k != frame_ || r0 != r0_ || rows_[r - r0].empty()) {
            frame_ = -1;
            const int n = std::min(kNoiseMaxChunk, cfg_.replicas - r0 + 1);
            uint64_t bits;
            static_assert(sizeof(bits) == sizeof(time), "the frame time's IEEE-754 bits");
            std::memcpy(&bits, &time, sizeof(bits));
            hip_ok(hipSetDevice(d_.device), "hipSetDevice");  // (the reader thread's first call)
            hip_ok(hipMemcpyAsync(dg_.get(), g.data(), (size_t)npix_ * sizeof(double), hipMemcpyHostToDevice,
                                  ts_.stream), "H2D frame");
            hip_ok(hipEventRecord(ts_.e0, ts_.stream), "hipEventRecord");
            launch_noise_replicas(dg_.get(), npix_, (uint64_t)d_.blk.offset, bits, (uint32_t)r0, n, cfg_.noise_abs,
                                  cfg_.noise_shot, cfg_.noise_rel, cfg_.noise_seed, dout_.get(), ldo_, ts_.stream);
            hip_ok(hipEventRecord(ts_.e1, ts_.stream), "hipEventRecord");
            for (int i = 0; i < n; ++i) {  // every replica straight into the vector that is handed over
                rows_[i].resize((size_t)npix_);
                hip_ok(hipMemcpyAsync(rows_[i].data(), dout_.get() + (size_t)i * ldo_, (size_t)npix_ * sizeof(double),
                                      hipMemcpyDeviceToHost, ts_.stream), "D2H replicas");
            }
            hip_ok(hipStreamSynchronize(ts_.stream), "noise replicas");
            kernel_ms_ += ts_.elapsed_ms();
            frame_ = k, r0_ = r0;
        }
        std::vector<double> out = std::move(rows_[r - r0_]);
        rows_[r - r0_].clear();  // (a moved-from vector: empty by this line, whatever the library left)
        return out;
    }
    double kernel_ms() const { return kernel_ms_; }

   private:
    const Driver& d_;
    const Config& cfg_;
    const int64_t npix_, ldo_;
    DeviceArray<double> dg_, dout_;
    std::vector<std::vector<double>> rows_;  // the chunk's replicas not handed over yet
    TimedStream ts_;
    int64_t frame_ = -1;
    int r0_ = 0;
    double kernel_ms_ = 0.0;
};

// --replicas: run_series over T (N + 1) virtual frames, virtual frame j = k (N + 1) + r being composite frame k's
// replica r (r = 0: the measured frame itself), all cold columns of the multi-frame engine. Rank 0's sink keeps a
// composite frame's columns on the host until the last one has arrived (no host collective in the sink, as in the scan),
// takes the per-voxel moments of replicas 1 .. N (csrc/kernels/moments64.hip, on a stream of its own, synchronised
// before the buffer is released), writes the frame's rows of /uncertainty and hands column 0 to the ordinary solution
// writer in frame order.
void run_replica_series(Driver& d, Solvers& s, const std::vector<uint64_t>& frames) {
    const Config& cfg = d.cfg;
    const CompositeImage& image = *d.image;
    const int64_t N = cfg.replicas, nc = N + 1, T = (int64_t)frames.size(), nvirt = T * nc;
    const int64_t nvoxel = (int64_t)d.in.nvoxel;
    const size_t npix = (size_t)s.mf->nrows();
    ReplicaSource noise(d, (int64_t)npix);
    FrameReadahead ra(nvirt, 4 * (int64_t)cfg.batch_frames, [&](int64_t j) {
        const int64_t k = j / nc;
        std::vector<double> g = d.image->frame(frames[k]);  // (the image caches its frames)
        if (j % nc == 0) return g;
        return noise.replica(k, g, d.image->frame_time(frames[k]), (int)(j % nc));
    });
    auto src = [&](int64_t j, double* dst) {
        const std::vector<double> f = ra.take(j);
        if (f.size() != npix) throw std::runtime_error("frame size does not match the shard's pixels");
        std::copy(f.begin(), f.end(), dst);
    };
    // rank 0: the columns of the composite frames in flight, the moments' device operands, the output
    struct Columns {
        std::vector<double> x;  // [nc][nvoxel]
        std::vector<int32_t> status, iterations;
        std::vector<uint8_t> use;  // [N]: replica r + 1 did not stop on a non-finite iterate
        int64_t left;
    };
    std::map<int64_t, Columns> open;
    // column 0 (with its status and update count) of the completed frames not written yet, by frame
    std::map<int64_t, std::tuple<std::vector<double>, int32_t, int32_t>> done;
    int64_t written = 0;
    std::unique_ptr<UncertaintyWriter> file;
    DeviceArray<double> dX, dmean, dstd;
    DeviceArray<uint8_t> duse;
    std::unique_ptr<TimedStream> ms;
    std::vector<double> mean, sd;
    if (d.rank == 0) {
        const double triple[3] = {cfg.noise_abs, cfg.noise_shot, cfg.noise_rel};
        file = std::make_unique<UncertaintyWriter>(cfg.output_file, (uint64_t)T, (uint64_t)N, (uint64_t)nvoxel, triple,
                                                   cfg.noise_seed, cfg.replicas_keep);
        dX.resize((size_t)N * nvoxel), dmean.resize((size_t)nvoxel), dstd.resize((size_t)nvoxel);
        duse.resize((size_t)N);
        mean.resize((size_t)nvoxel), sd.resize((size_t)nvoxel);
        ms = std::make_unique<TimedStream>();
    }
    double sink_ms = 0.0, moments_ms = 0.0;
    auto t_prev = Clock::now();
    auto sink = [&](int64_t j, const double* xs, const SolveInfo& info) {
        if (d.rank != 0) return;
        const auto tsk = Clock::now();
        const int64_t k = j / nc, r = j % nc;
        auto it = open.find(k);
        if (it == open.end())
            it = open.emplace(k, Columns{std::vector<double>((size_t)nc * nvoxel), std::vector<int32_t>((size_t)nc),
                                         std::vector<int32_t>((size_t)nc), std::vector<uint8_t>((size_t)N), nc}).first;
        Columns& c = it->second;
        std::copy(xs, xs + nvoxel, c.x.begin() + (size_t)r * nvoxel);
        c.status[r] = info.status, c.iterations[r] = info.iterations;
        if (r > 0) c.use[r - 1] = info.nonfinite ? 0 : 1;
        if (info.nonfinite)
            std::cerr << "warning: frame " << frames[k] << ", replica " << r << ": non-finite iterate, stopped"
                      << std::endl;
        if (--c.left == 0) {
            hipStream_t mstream = ms->stream;
            hip_ok(hipMemcpyAsync(dX.get(), c.x.data() + nvoxel, (size_t)N * nvoxel * sizeof(double),
                                  hipMemcpyHostToDevice, mstream), "H2D replicas");
            hip_ok(hipMemcpyAsync(duse.get(), c.use.data(), (size_t)N, hipMemcpyHostToDevice, mstream), "H2D mask");
            hip_ok(hipEventRecord(ms->e0, mstream), "hipEventRecord");
            launch_moments64(dX.get(), nvoxel, nvoxel, (int)N, duse.get(), dmean.get(), dstd.get(), mstream);
            hip_ok(hipEventRecord(ms->e1, mstream), "hipEventRecord");
            hip_ok(hipMemcpyAsync(mean.data(), dmean.get(), (size_t)nvoxel * sizeof(double), hipMemcpyDeviceToHost,
                                  mstream), "D2H mean");
            hip_ok(hipMemcpyAsync(sd.data(), dstd.get(), (size_t)nvoxel * sizeof(double), hipMemcpyDeviceToHost,
                                  mstream), "D2H std");
            hip_ok(hipStreamSynchronize(mstream), "moments");
            moments_ms += ms->elapsed_ms();
            const int32_t count = (int32_t)std::count(c.use.begin(), c.use.end(), (uint8_t)1);
            file->write_frame((uint64_t)k, mean.data(), sd.data(), count, c.status.data(), c.iterations.data(),
                              cfg.replicas_keep ? c.x.data() : nullptr);
            c.x.resize((size_t)nvoxel);  // column 0 alone goes on to the solution writer
            done.emplace(k, std::make_tuple(std::move(c.x), c.status[0], c.iterations[0]));
            open.erase(it);
            const auto now = Clock::now();
            std::cout << "Processed in: " << std::chrono::duration<double, std::milli>(now - t_prev).count() << " ms"
                      << std::endl;
            t_prev = now;
            // column 0 of the completed frames to /solution, in frame order (frames complete out of order)
            for (auto dn = done.find(written); dn != done.end(); dn = done.find(written)) {
                const uint64_t cur = frames[written];
                d.writer->add(std::get<0>(dn->second), std::get<1>(dn->second), image.frame_time(cur),
                              image.camera_frame_time(cur), std::get<2>(dn->second));
                done.erase(dn);
                ++written;
            }
        }
        sink_ms += ms_since(tsk);
    };
    s.mf->solve_series(nvirt, src, sink, nullptr, false, nullptr);
    if (d.rank == 0 && d.profile.is_open()) {
        write_series_line(d.profile, *s.mf, ra.reader_ms(), sink_ms);
        write_uncertainty_line(d.profile, {cfg.replicas, cfg.noise_seed, cfg.noise_abs, cfg.noise_shot, cfg.noise_rel,
                                           noise.kernel_ms(), moments_ms, (uint64_t)T});
    }
}

// GPU runs: this rank's device and the device communicator; --use_cpu: the host communicator alone
void open_communicators(Driver& d) {
    if (d.gpu) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            throw std::runtime_error("No GPU available: run with --use_cpu or on an MI355X node.");
        d.device = env_world().local_rank % ndev;
        hip_ok(hipSetDevice(d.device), "hipSetDevice");
        d.dcomm = comm_from_env(d.device);
        d.host = &d.dcomm->host();
    } else {
        d.hcomm = host_comm_from_env();
        d.host = d.hcomm.get();
    }
    d.rank = d.host->rank(), d.size = d.host->size();
}

// --rtm_format: the single-frame GPU solver on pixel-row shards of fp32 values can keep a sparse RTM sparse (decided
// from the files' metadata: the same on every rank; --fp64 reads dense shards: auto loads the matrix dense)
bool choose_sparse(const Driver& d) {
    const Config& cfg = d.cfg;
    if (d.cols || cfg.rtm_bf16 || cfg.rtm_f16 || cfg.fp64 || cfg.rtm_format == "dense") return false;
    const double dens = rtm_sparse_density(d.in.rtm_files, d.in.rtm_name, d.in.npixel, d.in.nvoxel);
    // auto: the sparse kernels read 16 bytes per non-zero and sweep (CSR + CSC, index + value) against 4 bytes
    // per element for the dense fused sweep; measured at 32768 x 32768 (uniform random positions): sparse /
    // dense fused it/s 11268 / 1525 at 1 %, 3038 / 1532 at 4.9 %, 2031 / 1534 at 9.5 %, 1336 / 1531 at 18 %
    // (profiles/sparse_r5_density_breakeven.jsonl): auto takes the sparse path up to 10 %
    return cfg.rtm_format == "sparse" || (dens >= 0.0 && dens <= 0.10);
}

// Rank 0 owns the output (reference main.cpp:115-125, solution.cpp): opens or resumes it; every rank learns the time
// to skip up to and the stored solution to warm-start from (warm: empty without one or with --no_guess). Collective.
struct Resume {
    VoxelGrid voxelgrid;
    double skip_until = -std::numeric_limits<double>::infinity();
    std::vector<double> warm;
    bool appended = false;
};
void open_output(Driver& d, Resume& r) {
    const Config& cfg = d.cfg;
    struct stat st;
    if (d.rank == 0 && !cfg.fit_only) {
        if (cfg.resume && ::stat(cfg.output_file.c_str(), &st) == 0) {
            const StoredSolutions stored = read_solution_file(cfg.output_file);
            if (!stored.time.empty()) {
                r.appended = true;
                r.skip_until = stored.time.back();
                r.warm = stored.last_solution;
            }
        }
        // --beta_scan, --replicas: the run creates the file with its own group; /solution is added to it
        d.writer = std::make_unique<SolutionWriter>(cfg.output_file, d.in.camera_names, d.in.nvoxel,
                                                    (uint64_t)cfg.max_cached_solutions, r.appended,
                                                    !cfg.beta_scan.empty() || cfg.replicas > 0);
        r.voxelgrid.read(d.in.rtm_files.begin()->second, "rtm/voxel_map");
        for (const auto& m : r.voxelgrid.warnings) std::cerr << "warning: " << m << std::endl;
    }
    d.host->broadcast_host(&r.skip_until, sizeof(r.skip_until), 0);
    int has_warm = (!cfg.no_guess && !r.warm.empty()) ? 1 : 0;
    d.host->broadcast_host(&has_warm, sizeof(has_warm), 0);
    r.warm.resize(has_warm ? d.in.nvoxel : 0);
    if (has_warm) d.host->broadcast_host(r.warm.data(), r.warm.size() * sizeof(double), 0);
}

SolverParams solver_params(const Config& cfg) {
    SolverParams params;
    params.logarithmic = cfg.logarithmic;
    params.ray_density_threshold = cfg.ray_density_threshold;
    params.ray_length_threshold = cfg.ray_length_threshold;
    params.conv_tolerance = cfg.conv_tolerance;
    params.beta_laplace = cfg.beta_laplace;
    params.relaxation = cfg.relaxation;
    params.max_iterations = cfg.max_iterations;
    validate_params(params);
    return params;
}

// Everything after the communicators exist: an exception here aborts them (main)
void run(Driver& d) {
    const Config& cfg = d.cfg;
    const InputSet& in = d.in;
    HostComm* host = d.host;
    const int rank = d.rank, size = d.size;
    d.cols = d.gpu && cfg.partition_voxels;
    if (cfg.replicas > 0 && in.npixel >= (uint64_t)1 << 32)  // the noise counter takes the pixel index as 32 bits
        throw Error("Argument replicas applies to fewer than 2^32 pixels, " + std::to_string(in.npixel) + " given.");
    d.vblk = d.cols ? block_partition(in.nvoxel, size, rank) : Block{0, in.nvoxel};
    d.blk = d.cols ? Block{0, in.npixel} : block_partition(in.npixel, size, rank);  // reference main.cpp:67-68
    if (d.blk.size == 0 || d.vblk.size == 0)
        throw std::runtime_error("rank " + std::to_string(rank) + " owns no " + (d.cols ? "voxels" : "pixels") +
                                 ": use at most " + std::to_string(d.cols ? in.nvoxel : in.npixel) + " ranks");
    d.image = std::make_unique<CompositeImage>(in.image_files, in.frame_masks, d.intervals, d.blk.size, d.blk.offset);
    d.image->set_max_cache_size((uint64_t)cfg.max_cached_frames);
    const SolverParams params = solver_params(cfg);
    Csr lap;
    if (!cfg.laplacian_file.empty()) {
        const LaplacianCOO coo = read_laplacian(cfg.laplacian_file, in.nvoxel);
        lap = csr_from_coo((int64_t)in.nvoxel, coo.i, coo.j, coo.value);
    }

    const bool sparse = choose_sparse(d);
    LoadStats lstats;
    Shard shard;
    if (cfg.parallel_read || size == 1) {
        shard = load_shard(cfg, in, d.blk, d.vblk, sparse, d.gpu, &lstats);
    } else {
        for (int r = 0; r < size; ++r) {  // serialized reads (reference main.cpp:80-85)
            if (r == rank) shard = load_shard(cfg, in, d.blk, d.vblk, sparse, d.gpu, &lstats);
            host->barrier();
        }
    }
    if (d.gpu && rank == 0)  // the HDF5 -> HBM load of this rank's shard (all ranks: the --profile load line)
        std::cout << "RTM loaded in: " << lstats.wall_s << " s (" << lstats.bytes / 1e9 << " GB, "
                  << (lstats.wall_s > 0 ? lstats.bytes / 1e9 / lstats.wall_s : 0.0) << " GB/s"
                  << (sparse ? ", sparse: " + std::to_string(shard.nnz) + " non-zeros" : std::string()) << ")"
                  << std::endl;

    Solvers solvers = build_solvers(d, shard, params, lap);
    const bool batched = d.gpu && cfg.batch_frames > 1;
    const bool solve = !cfg.fit_only;  // --fit_only: the shard alone, for the fit pass
    // The output and the profile are closed when this function is left, also by an exception: the cached solutions and
    // the profile lines written so far are on disk before main() aborts the communicators and exits without unwinding
    struct CloseOutput {
        Driver& d;
        ~CloseOutput() {
            d.profile.close();
            d.writer.reset();
        }
    } close_output{d};
    Resume res;
    open_output(d, res);
    if (rank == 0 && !cfg.profile_file.empty()) d.profile.open(cfg.profile_file);
    if ((d.gpu || sparse) && !cfg.profile_file.empty()) profile_load(d, shard, lstats, solvers);

    std::vector<uint64_t> frames;
    for (uint64_t i = 0; i < d.image->nframe(); ++i)
        if (solve && d.image->frame_time(i) > res.skip_until + 1e-12) frames.push_back(i);
    const auto t_loop = Clock::now();
    if (!cfg.beta_scan.empty()) {
        ScanColumns sc;
        if (rank == 0) {
            const size_t nvirt = frames.size() * cfg.beta_scan.size();
            sc.file = std::make_unique<ScanWriter>(cfg.output_file, frames.size(), cfg.beta_scan.size(), in.nvoxel,
                                                   cfg.beta_scan.data());
            sc.status.resize(nvirt), sc.iterations.resize(nvirt), sc.ok.resize(nvirt);
        }
        run_scan_series(d, solvers, frames, sc);
        solvers.reset();  // the engine's device buffers, before the pass allocates its own
        run_scan_pass(d, shard, lap, frames, sc);
    } else if (cfg.replicas > 0)
        run_replica_series(d, solvers, frames);
    else if (batched)
        run_series(d, solvers, frames, res.warm);
    else
        run_frames(d, solvers, frames, res.warm);
    if (rank == 0 && solve) {
        d.writer->flush();
        if (!res.appended) res.voxelgrid.write(cfg.output_file, "voxel_map");
        // the whole frame loop (reads not hidden by the prefetch, solves, output, the final flush)
        if (!frames.empty()) {
            const double loop_s = seconds_since(t_loop);
            std::cout << "Frames processed: " << frames.size() << " in " << loop_s << " s ("
                      << frames.size() / loop_s << " frames/s)" << std::endl;
        }
    }
    host->barrier();
    if (cfg.fit || cfg.fit_only) {
        d.writer.reset();  // flushed above: the file is closed before the /fit group is added to it
        solvers.reset();
        if (!d.gpu && sparse && solvers.cpu) {  // the CPU solver took the CSR rows: read them again
            solvers.cpu.reset();
            reload_host_csr(shard, in, d.blk);
        }
        run_fit_pass(d, shard);
    }
}

}  // namespace

int main(int argc, char** argv) {
    // Started by the Python entry point (cli.py sets SART_PARENT_PID): die with it. cli.py forwards SIGTERM /
    // SIGINT / SIGHUP itself; this covers a parent killed with SIGKILL, so no orphan keeps the GPU or sits in a
    // collective. A parent that is already gone (a race with the prctl) ends the driver at once.
    if (const char* pp = std::getenv("SART_PARENT_PID"); pp && *pp) {
        (void)::prctl(PR_SET_PDEATHSIG, SIGTERM);
        if ((long)::getppid() != std::atol(pp)) return 1;
    }
    Driver d;
    try {
        d.cfg = parse_arguments(std::vector<std::string>(argv + 1, argv + argc));
        if (d.cfg.help) {
            std::cout << usage() << std::endl;
            return 0;
        }
        d.intervals = parse_time_intervals(d.cfg.time_range);
        // metadata validation on every rank, before any communicator exists (reference main.cpp:27-59)
        d.in = validate_inputs(d.cfg.input_files, d.cfg.raytransfer_name, d.cfg.wavelength_threshold);
        d.gpu = !d.cfg.use_cpu;
        open_communicators(d);
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    try {
        run(d);
    } catch (const std::exception& e) {
        std::cerr << "rank " << d.rank << ": " << e.what() << std::endl;
        if (d.dcomm) d.dcomm->abort();
        else if (d.host) d.host->abort();
        std::fflush(nullptr);
        std::_Exit(1);
    }
    return 0;
}
