// Command-line configuration of the sartsolver driver.
//
// Same options, short aliases, defaults and validation as the reference CLI (reference
// arguments.cpp:82-251, arguments.hpp:14-33), with an in-tree parser instead of p-ranav/argparse.
// Extensions (not in the reference) are marked: --resume, --batch_frames, --two_pass, --partition_voxels,
// --profile, --fp64, --fp64_semantics, --fit, --fit_only, --beta_scan, --replicas (with --noise_abs, --noise_shot,
// --noise_rel, --noise_seed, --replicas_keep), --phantom, --holdout (with --holdout_seed, --holdout_betas).
#pragma once

#include <array>
#include <cstdint>
#include <string>
#include <vector>

namespace sart {

struct Config {
    std::vector<std::string> input_files;
    std::string output_file = "solution.h5";
    std::string time_range;
    std::string laplacian_file;
    std::string raytransfer_name = "with_reflections";
    double wavelength_threshold = 50.0;
    double ray_density_threshold = 1e-6;
    double ray_length_threshold = 1e-6;
    double conv_tolerance = 1e-5;
    double beta_laplace = 2e-2;
    double relaxation = 1.0;
    int max_iterations = 2000;
    int max_cached_frames = 100;
    int max_cached_solutions = 100;
    bool logarithmic = false;
    bool no_guess = false;
    bool use_cpu = false;
    bool parallel_read = false;
    // extensions
    bool resume = false;        // append to an existing output file, skip frames already solved
    int batch_frames = 1;       // >1: solve independent frames together (MFMA multi-frame path, implies --no_guess)
    bool two_pass = false;      // disable the fused single-pass sweep
    bool partition_voxels = false;
    // GPU single-frame solver: keep the RTM sparse on the device (CSR + CSC, csrc/kernels/sparse.hip) instead of a
    // dense shard. "auto": when every RTM dataset is sparse COO with at most 10 % non-zeros; "dense" / "sparse".
    std::string rtm_format = "auto";
    bool rtm_f16 = false;       // GPU: store the RTM shard as row-scaled f16 (exclusive with rtm_bf16)
    bool rtm_f16_fused = false; // GPU, with rtm_f16: run the fused single-pass f16 sweep (opt-in; else two-pass)
    bool rtm_bf16 = false;      // GPU: store the RTM shard in bf16 (fp32 products and sums)  // GPU: shard the RTM by voxel columns (all pixels per rank) instead of pixel rows
    bool fp64 = false;          // GPU: solve in double precision (Engine64; fp32 dense pixel-row shards, frame by frame)
    std::string fp64_semantics = "gpu";  // with fp64: "gpu" (the default GPU path's semantics in fp64) or "cpu"
                                         // (what --use_cpu computes)
    bool fit = false;           // after the frames: fp64 fitted images f = A x and residuals into the output's /fit group
    bool fit_only = false;      // no solve: the fit pass alone over the solutions already in the output file
    // every frame at each of these Laplacian weights in one batched run (3 .. 64 increasing values >= 0): the L-curve
    // in the output's /beta_scan group, its corner's solution in /solution. Implies batch_frames >= 16 and no_guess;
    // beta_laplace only names the fallback entry
    std::vector<double> beta_scan;
    // Monte-Carlo error bars: every frame's nominal column and `replicas` (2 .. 1024) noisy replicas of it in one
    // batched run, per-voxel mean and spread into the output's /uncertainty group, the nominal column into /solution.
    // Per pixel sigma^2 = noise_abs^2 + noise_shot g + (noise_rel g)^2 (README "Replicas"). Implies batch_frames >= 16
    // and no_guess. 0: off
    int replicas = 0;
    double noise_abs = 0.0, noise_shot = 0.0, noise_rel = 0.0;
    uint64_t noise_seed = 0;
    bool replicas_keep = false;  // also store every replica's solution (/uncertainty/value)
    // Reconstruct known emissivities: the frames solved are the fp64 projections of the rows of this file's
    // /phantom/value through the RTM as stored (with `replicas`: and noisy replicas of them), scored against their truth
    // into the output's /phantom group, column 0 into /solution. Implies batch_frames >= 16 and no_guess. Empty: off
    std::string phantom_file;
    // Hold-out cross-validation: every frame as measured and with each of K folds of its pixels excluded, at every
    // weight of holdout_betas (none: at beta_laplace), in one batched run; the prediction errors of the held-out pixels
    // into the output's /holdout group, the best weight's unmasked column into /solution. holdout: K (2 .. 32) pseudo-
    // random pixel folds keyed by holdout_seed, or with holdout_cameras one fold per camera (K = the number of cameras,
    // known with the inputs). Implies batch_frames >= 16 and no_guess. 0 and false: off
    int holdout = 0;
    bool holdout_cameras = false;
    uint64_t holdout_seed = 0;
    std::vector<double> holdout_betas;
    bool holdout_on() const { return holdout > 0 || holdout_cameras; }
    std::string profile_file;  // JSON timing/telemetry sidecar
    bool help = false;
};

// Throws sart::Error with a usage message on invalid input; --help sets Config::help.
Config parse_arguments(const std::vector<std::string>& argv);
std::string usage();

// "start:stop[:step[:sync_threshold]], ..." -> {start, stop, step, threshold}; empty -> {0, inf, 0, 0}
std::vector<std::array<double, 4>> parse_time_intervals(const std::string& spec);

}  // namespace sart
