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
// of it as columns of the multi-frame engine; per-voxel mean and spread into the output's /uncertainty group),
// --phantom FILE (the frames solved are the fp64 projections of known emissivities through the shard; every column
// scored against its truth into the output's /phantom group), --holdout K|cameras (every frame as measured and with
// each fold of its pixels -- or each camera -- excluded, as columns of the multi-frame engine; the prediction errors of
// the held-out pixels into the output's /holdout group, the best weight's unmasked column into /solution).
// This file: main()'s sequence up to the runs it starts (driver.hpp). The frame loops: series_runs.cpp (frame by frame,
// --batch_frames) and column_runs.cpp (--beta_scan, --replicas, --phantom, --holdout), on the series skeleton of driver.hpp with the order
// rules of series_order.hpp and the frame reader of frame_readahead.hpp; the passes after the frames: fit_pass.cpp. The
// shard and its loaders: shard_load.{hpp,cpp}; the --profile lines: profile_lines.
#include <sys/prctl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <csignal>
#include <limits>

#include "driver.hpp"

using namespace sart;

namespace {

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
        // the scan (and a hold-out ladder) brings a weight per column: keep the Laplacian
        base.mf_frame_beta = !cfg.beta_scan.empty() || !cfg.holdout_betas.empty();
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
        // --beta_scan, --replicas, --phantom, --holdout: the run creates the file with its own group; /solution is added to it
        d.writer = std::make_unique<SolutionWriter>(cfg.output_file, d.in.camera_names, d.in.nvoxel,
                                                    (uint64_t)cfg.max_cached_solutions, r.appended,
                                                    !cfg.beta_scan.empty() || cfg.replicas > 0 ||
                                                        !cfg.phantom_file.empty() || cfg.holdout_on());
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

// --holdout: the folds of all pixels and the cameras' pixel ranges (every rank: the inputs' metadata alone); rank 0: the
// output file created with its /holdout group
HoldoutColumns holdout_columns(const Driver& d, size_t T) {
    const Config& cfg = d.cfg;
    const InputSet& in = d.in;
    HoldoutColumns hc;
    std::vector<int64_t> camera_pixels;
    hc.cam_start.push_back(0);
    for (const auto& cam : in.camera_names) {
        const auto& mask = in.frame_masks.at(cam);
        camera_pixels.push_back((int64_t)std::count_if(mask.begin(), mask.end(), [](int32_t v) { return v != 0; }));
        hc.cam_start.push_back(hc.cam_start.back() + camera_pixels.back());
    }
    if ((uint64_t)hc.cam_start.back() != in.npixel) throw std::runtime_error("the cameras' masks do not add up to the pixels");
    hc.K = cfg.holdout_cameras ? (int)camera_pixels.size() : cfg.holdout;
    hc.betas = cfg.holdout_betas.empty() ? std::vector<double>{cfg.beta_laplace} : cfg.holdout_betas;
    hc.folds.resize(in.npixel);
    if (cfg.holdout_cameras)
        holdout_camera_folds(camera_pixels.data(), (int)camera_pixels.size(), 0, in.npixel, hc.folds.data());
    else
        holdout_pixel_folds(cfg.holdout_seed, hc.K, 0, in.npixel, hc.folds.data());
    if (d.rank == 0) {
        const size_t nvirt = T * hc.betas.size() * (size_t)(hc.K + 1);
        hc.file = std::make_unique<HoldoutWriter>(cfg.output_file, T, hc.betas.size(), (uint64_t)hc.K, camera_pixels.size(),
                                                  in.nvoxel, cfg.holdout_cameras, hc.folds.data(), in.npixel,
                                                  cfg.holdout_seed, hc.betas.data());
        hc.status.resize(nvirt), hc.iterations.resize(nvirt), hc.ok.resize(nvirt);
    }
    return hc;
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
    if (cfg.holdout_on() && in.npixel >= (uint64_t)1 << 32)  // the fold counter takes the pixel index as 32 bits
        throw Error("Argument holdout applies to fewer than 2^32 pixels, " + std::to_string(in.npixel) + " given.");
    if (cfg.holdout_cameras && in.camera_names.size() < 2)
        throw Error("Argument holdout cameras needs at least two cameras, " + std::to_string(in.camera_names.size()) +
                    " given.");
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
    if (!cfg.phantom_file.empty()) {  // the phantoms stand in for the measured frames (in the closing line too)
        frames.assign((size_t)run_phantom_series(d, solvers, shard), 0);
    } else if (!cfg.beta_scan.empty()) {
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
    } else if (cfg.holdout_on()) {
        HoldoutColumns hc = holdout_columns(d, frames.size());
        run_holdout_series(d, solvers, frames, hc);
        solvers.reset();  // the engine's device buffers, before the pass allocates its own
        run_holdout_pass(d, shard, frames, hc);
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
