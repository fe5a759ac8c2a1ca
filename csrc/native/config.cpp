#include "config.hpp"

#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <limits>
#include <map>
#include <sstream>

#include "h5.hpp"  // sart::Error

namespace sart {

namespace {

std::string trim(const std::string& s) {
    size_t a = s.find_first_not_of(" \t\n\r"), b = s.find_last_not_of(" \t\n\r");
    return a == std::string::npos ? std::string() : s.substr(a, b - a + 1);
}

double to_double(const std::string& tok, const std::string& opt) {
    const std::string t = trim(tok);
    char* end = nullptr;
    errno = 0;
    const double v = std::strtod(t.c_str(), &end);
    if (t.empty() || end != t.c_str() + t.size() || errno == ERANGE)
        throw Error("Failed to parse '" + tok + "' as a number for " + opt + ".");
    return v;
}

int to_int(const std::string& tok, const std::string& opt) {
    const std::string t = trim(tok);
    char* end = nullptr;
    errno = 0;
    const long v = std::strtol(t.c_str(), &end, 10);
    if (t.empty() || end != t.c_str() + t.size() || errno == ERANGE || v < std::numeric_limits<int>::min() ||
        v > std::numeric_limits<int>::max())
        throw Error("Failed to parse '" + tok + "' as an integer for " + opt + ".");
    return (int)v;
}

uint64_t to_u64(const std::string& tok, const std::string& opt) {
    const std::string t = trim(tok);
    char* end = nullptr;
    errno = 0;
    const unsigned long long v = std::strtoull(t.c_str(), &end, 10);
    if (t.empty() || t[0] == '-' || t[0] == '+' || end != t.c_str() + t.size() || errno == ERANGE)
        throw Error("Failed to parse '" + tok + "' as an unsigned 64-bit integer for " + opt + ".");
    return (uint64_t)v;
}

std::string fmt(double v) {
    std::ostringstream os;
    os << v;
    return os.str();
}

// "B0,B1,...": 3 .. 64 finite values >= 0 in strictly increasing order; anything else is one error, with the text given
std::vector<double> to_beta_scan(const std::string& text, const std::string& name = "beta_scan") {
    const Error bad("Argument " + name + " must list 3 to 64 increasing values >= 0, " + text + " given.");
    std::vector<double> out;
    size_t pos = 0;
    while (true) {
        const size_t comma = text.find(',', pos);
        const std::string t = trim(text.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos));
        char* end = nullptr;
        errno = 0;
        const double v = std::strtod(t.c_str(), &end);
        if (t.empty() || end != t.c_str() + t.size() || errno == ERANGE || !std::isfinite(v) || v < 0) throw bad;
        if (!out.empty() && !(v > out.back())) throw bad;
        out.push_back(v);
        if (comma == std::string::npos) break;
        pos = comma + 1;
    }
    if (out.size() < 3 || out.size() > 64) throw bad;
    return out;
}

}  // namespace

std::string usage() {
    return "Usage: sartsolver [options] input_files...\n"
           "Impurity flux reconstruction for ITER: emissivity (MI355X-native SART solver)\n\n"
           "Positional arguments:\n"
           "  input_files                 List of ray transfer matrix and camera image hdf5 files.\n\n"
           "Optional arguments:\n"
           "  -h, --help                  shows help message and exits\n"
           "  -o, --output_file           Filename to save the solution. [default: \"solution.h5\"]\n"
           "  -t, --time_range            Time intervals in s to process in a form: start:stop:(step):(synch_threshold),\n"
           "                              e.g. '20.5:40.1, 45.2:51:15:0.05'. The step and the synchronization threshold\n"
           "                              are optional. [default: \"\"]\n"
           "  -w, --wavelength_threshold  An RTM is considered valid if its wavelength is within this threshold of the\n"
           "                              image wavelength (in nm). [default: 50]\n"
           "  -d, --ray_density_threshold Voxels with ray density lesser than this threshold are ignored. [default: 1e-06]\n"
           "  -r, --ray_length_threshold  Pixels with ray length lesser than this threshold are ignored. [default: 1e-06]\n"
           "  -m, --max_iterations        Maximum number of SART iterations. [default: 2000]\n"
           "  -c, --conv_tolerance        SART convolution relative tolerance. [default: 1e-05]\n"
           "  -l, --laplacian_file        File with laplacian regularization matrix. [default: \"\"]\n"
           "  -b, --beta_laplace          Weight of the regularization factor. [default: 0.02]\n"
           "  -R, --relaxation            Relaxation parameter. [default: 1]\n"
           "  -n, --raytransfer_name      Ray transfer matrix dataset name. [default: \"with_reflections\"]\n"
           "  -L, --logarithmic           Use logarithmic SART solver.\n"
           "  --max_cached_frames         Maximum number of cached image frames. [default: 100]\n"
           "  --max_cached_solutions      Maximum number of cached solutions. [default: 100]\n"
           "  --no_guess                  Do not use solution found on previous time moment as initial guess for the\n"
           "                              next one.\n"
           "  --use_cpu                   Perform all calculations on CPUs.\n"
           "  --parallel_read             Read RTM data in a parallel way (high-IOPS storage optimization).\n"
           "Extensions:\n"
           "  --resume                    Append to an existing output file and skip frames already solved.\n"
           "  --batch_frames N            Solve N frames together on the matrix cores (continuous batching: a\n"
           "                              finished frame's slot takes the next frame, warm-started from the\n"
           "                              latest frame finished before it; cold with --no_guess). This is NOT\n"
           "                              the reference's frame k-1 -> k warm-start chain, so results depend\n"
           "                              on N; N = 1 keeps the reference semantics. [default: 1]\n"
           "  --two_pass                  Use the two-pass projection kernels instead of the fused sweep.\n"
           "  --partition_voxels          Shard the RTM by voxel columns (every GPU holds all pixels of a voxel\n"
           "                              block; all-reduce of A x per iteration) instead of by pixel rows.\n"
           "  --rtm_bf16                  Store the RTM in bf16 on the GPU (half the memory and bytes per sweep;\n"
           "                              products and sums stay fp32).\n"
           "  --rtm_f16                   Store the RTM on the GPU as f16 with a power-of-two scale per pixel row\n"
           "                              (the same two bytes as --rtm_bf16 with 11 significant bits instead of\n"
           "                              8; two-pass kernels, and the matrix cores with --batch_frames).\n"
           "                              Exclusive with --rtm_bf16.\n"
           "  --rtm_f16_fused             With --rtm_f16: run the fused single-pass sweep on the f16 shard (one\n"
           "                              read of the RTM per iteration instead of two; opt-in, ignored with\n"
           "                              --batch_frames; --two_pass still selects the two-pass kernels).\n"
           "  --rtm_format F              auto | dense | sparse: keep a sparse RTM sparse (CSR + CSC; the GPU\n"
           "                              solvers and the CPU solver, pixel-row shards). auto: when every RTM dataset is\n"
           "                              sparse COO with at most 10 % non-zeros. [default: auto]\n"
           "  --fp64                      Solve on the GPU in double precision (fp32 RTM, every vector, product and\n"
           "                              sum fp64; two reads of the RTM per iteration): the answer to compare the\n"
           "                              other precisions against. Frame by frame, dense pixel-row shards.\n"
           "  --fp64_semantics S          gpu | cpu, with --fp64. gpu: the default GPU path (normalisation,\n"
           "                              epsilon 1e-7, fp32-rounded thresholds) evaluated in fp64; cpu: what\n"
           "                              --use_cpu computes. [default: gpu]\n"
           "  --fit                       After the frames, project every solution in the output file back through the\n"
           "                              RTM as stored (f = A x in fp64; up to 8 solutions per pass over the matrix,\n"
           "                              4 on bf16 / f16 shards) and write the fitted images and the residuals\n"
           "                              against the measured frames, in all and per camera, into the output\n"
           "                              file's /fit group.\n"
           "  --fit_only                  Solve nothing: load the RTM as the other options say and run the fit pass\n"
           "                              over the solutions already in the output file (e.g. an --rtm_bf16 solution\n"
           "                              against the fp32 matrix). Not with --resume, --batch_frames > 1 or --fp64.\n"
           "  --beta_scan B0,B1,...       Solve every frame at each of these Laplacian weights (3 to 64 increasing\n"
           "                              values >= 0) in one batched run: every weight is a column of the\n"
           "                              multi-frame engine, so the ladder costs about one batch sweep per iteration.\n"
           "                              Writes the L-curve (residual and roughness norms, curvature) and every\n"
           "                              solution into the output file's /beta_scan group and the corner's solution\n"
           "                              into /solution. Needs -l; implies --no_guess and --batch_frames >= 16;\n"
           "                              -b only names the fallback weight (the nearest entry) when no corner is\n"
           "                              found. Not with --use_cpu, --fp64, --partition_voxels, --resume, --fit or\n"
           "                              --fit_only.\n"
           "  --replicas N                Monte-Carlo error bars: solve every frame together with N (2 to 1024) noisy\n"
           "                              replicas of it in one batched run: every replica is a column of the\n"
           "                              multi-frame engine. Writes the per-voxel mean and standard deviation of the\n"
           "                              replicas into the output file's /uncertainty group and the unperturbed\n"
           "                              frame's solution into /solution. Needs a noise term; implies --no_guess and\n"
           "                              --batch_frames >= 16. Not with --use_cpu, --fp64, --partition_voxels,\n"
           "                              --resume, --fit, --fit_only or --beta_scan.\n"
           "  --noise_abs A               With --replicas: noise floor in measurement units; per pixel\n"
           "                              sigma^2 = A^2 + S g + (R g)^2. [default: 0]\n"
           "  --noise_shot S              With --replicas: shot-noise coefficient in measurement units. [default: 0]\n"
           "  --noise_rel R               With --replicas: relative noise. [default: 0]\n"
           "  --noise_seed K              With --replicas: 64-bit seed of the noise (the noise depends on the seed, the\n"
           "                              frame's time, the pixel and the replica alone). [default: 0]\n"
           "  --replicas_keep             With --replicas: also store every replica's solution (/uncertainty/value).\n"
           "  --phantom FILE              Reconstruct known emissivities: the frames solved are the fp64 projections of\n"
           "                              the rows of FILE's /phantom/value ([n][nvoxel], >= 0) through the RTM as\n"
           "                              stored, not the measured frames. The RTM and image files are given and\n"
           "                              validated as in any run (they fix the cameras and pixels); the images'\n"
           "                              frames and -t / --time_range are not used. Every column is scored against\n"
           "                              its truth into the output file's /phantom group; the noise-free column goes\n"
           "                              to /solution. With --replicas N and the --noise_* flags every phantom also\n"
           "                              gets N noisy replicas. Implies --no_guess and --batch_frames >= 16. Not with\n"
           "                              --use_cpu, --batch_frames 1, --fp64, --partition_voxels, --resume, --fit,\n"
           "                              --fit_only or --beta_scan.\n"
           "  --holdout K|cameras         Cross-validation: solve every frame as measured and with each of K (2 to 32)\n"
           "                              pseudo-random folds of its pixels excluded -- or, with 'cameras', with each\n"
           "                              camera excluded in turn (at least two cameras) -- in one batched run: every\n"
           "                              masked frame is a column of the multi-frame engine. The solutions are projected\n"
           "                              in fp64 and the prediction errors of the held-out pixels (in all, per camera)\n"
           "                              go to the output file's /holdout group with every column; the unmasked column\n"
           "                              of the weight with the smallest error goes to /solution. Implies --no_guess and\n"
           "                              --batch_frames >= 16. Not with --use_cpu, --fp64, --partition_voxels, --resume,\n"
           "                              --fit, --fit_only, --beta_scan, --replicas or --phantom.\n"
           "  --holdout_seed S            With --holdout K: 64-bit seed of the pixel folds (a pixel's fold depends on the\n"
           "                              seed and the pixel alone). [default: 0]\n"
           "  --holdout_betas B0,B1,...   With --holdout: run the folds at each of these Laplacian weights (3 to 64\n"
           "                              increasing values >= 0; needs -l) and select the weight by its cross-validation\n"
           "                              error; -b names the fallback (the nearest entry). Without it every column runs\n"
           "                              at -b.\n"
           "  --profile FILE              Write per-frame timing/iteration telemetry as JSON lines.\n";
}

Config parse_arguments(const std::vector<std::string>& argv) {
    Config c;
    bool semantics_given = false, scan_given = false, replicas_given = false, noise_given = false;
    bool batch_given = false, phantom_given = false, holdout_given = false, holdout_seed_given = false;
    bool holdout_betas_given = false;
    std::string scan_text, holdout_text, holdout_betas_text;
    using Setter = std::function<void(const std::string&, const std::string&)>;
    std::map<std::string, Setter> valued = {
        {"--output_file", [&](const std::string& v, const std::string&) { c.output_file = v; }},
        {"--time_range", [&](const std::string& v, const std::string&) { c.time_range = v; }},
        {"--wavelength_threshold", [&](const std::string& v, const std::string& o) { c.wavelength_threshold = to_double(v, o); }},
        {"--ray_density_threshold", [&](const std::string& v, const std::string& o) { c.ray_density_threshold = to_double(v, o); }},
        {"--ray_length_threshold", [&](const std::string& v, const std::string& o) { c.ray_length_threshold = to_double(v, o); }},
        {"--max_iterations", [&](const std::string& v, const std::string& o) { c.max_iterations = to_int(v, o); }},
        {"--conv_tolerance", [&](const std::string& v, const std::string& o) { c.conv_tolerance = to_double(v, o); }},
        {"--laplacian_file", [&](const std::string& v, const std::string&) { c.laplacian_file = v; }},
        {"--beta_laplace", [&](const std::string& v, const std::string& o) { c.beta_laplace = to_double(v, o); }},
        {"--relaxation", [&](const std::string& v, const std::string& o) { c.relaxation = to_double(v, o); }},
        {"--raytransfer_name", [&](const std::string& v, const std::string&) { c.raytransfer_name = v; }},
        {"--max_cached_frames", [&](const std::string& v, const std::string& o) { c.max_cached_frames = to_int(v, o); }},
        {"--max_cached_solutions", [&](const std::string& v, const std::string& o) { c.max_cached_solutions = to_int(v, o); }},
        {"--batch_frames", [&](const std::string& v, const std::string& o) { c.batch_frames = to_int(v, o); batch_given = true; }},
        {"--profile", [&](const std::string& v, const std::string&) { c.profile_file = v; }},
        {"--rtm_format", [&](const std::string& v, const std::string&) { c.rtm_format = v; }},
        {"--fp64_semantics", [&](const std::string& v, const std::string&) { c.fp64_semantics = v; semantics_given = true; }},
        {"--beta_scan", [&](const std::string& v, const std::string&) { scan_text = v; scan_given = true; }},
        {"--replicas", [&](const std::string& v, const std::string& o) { c.replicas = to_int(v, o); replicas_given = true; }},
        {"--noise_abs", [&](const std::string& v, const std::string& o) { c.noise_abs = to_double(v, o); noise_given = true; }},
        {"--noise_shot", [&](const std::string& v, const std::string& o) { c.noise_shot = to_double(v, o); noise_given = true; }},
        {"--noise_rel", [&](const std::string& v, const std::string& o) { c.noise_rel = to_double(v, o); noise_given = true; }},
        {"--noise_seed", [&](const std::string& v, const std::string& o) { c.noise_seed = to_u64(v, o); noise_given = true; }},
        {"--phantom", [&](const std::string& v, const std::string&) { c.phantom_file = v; phantom_given = true; }},
        {"--holdout", [&](const std::string& v, const std::string&) { holdout_text = v; holdout_given = true; }},
        {"--holdout_seed", [&](const std::string& v, const std::string& o) { c.holdout_seed = to_u64(v, o); holdout_seed_given = true; }},
        {"--holdout_betas", [&](const std::string& v, const std::string&) { holdout_betas_text = v; holdout_betas_given = true; }},
    };
    std::map<std::string, bool*> flags = {
        {"--logarithmic", &c.logarithmic}, {"--no_guess", &c.no_guess},   {"--use_cpu", &c.use_cpu},
        {"--parallel_read", &c.parallel_read}, {"--resume", &c.resume}, {"--two_pass", &c.two_pass},
        {"--partition_voxels", &c.partition_voxels}, {"--rtm_bf16", &c.rtm_bf16},
        {"--rtm_f16", &c.rtm_f16}, {"--rtm_f16_fused", &c.rtm_f16_fused}, {"--fp64", &c.fp64},
        {"--fit", &c.fit}, {"--fit_only", &c.fit_only}, {"--replicas_keep", &c.replicas_keep},
    };
    const std::map<std::string, std::string> alias = {
        {"-o", "--output_file"},           {"-t", "--time_range"},          {"-w", "--wavelength_threshold"},
        {"-d", "--ray_density_threshold"}, {"-r", "--ray_length_threshold"}, {"-m", "--max_iterations"},
        {"-c", "--conv_tolerance"},        {"-l", "--laplacian_file"},      {"-b", "--beta_laplace"},
        {"-R", "--relaxation"},            {"-n", "--raytransfer_name"},    {"-L", "--logarithmic"},
    };

    size_t i = 0;
    for (; i < argv.size(); ++i) {
        std::string tok = argv[i];
        if (tok == "-h" || tok == "--help") {
            c.help = true;
            return c;
        }
        if (tok.size() < 2 || tok[0] != '-') break;  // first positional: the rest are input files
        std::string value;
        bool has_value = false;
        const size_t eq = tok.find('=');
        if (tok.rfind("--", 0) == 0 && eq != std::string::npos) {
            value = tok.substr(eq + 1);
            tok = tok.substr(0, eq);
            has_value = true;
        }
        auto a = alias.find(tok);
        const std::string name = a != alias.end() ? a->second : tok;
        if (auto f = flags.find(name); f != flags.end()) {
            if (has_value) throw Error("Option " + name + " does not take a value.\n" + usage());
            *f->second = true;
        } else if (auto v = valued.find(name); v != valued.end()) {
            if (!has_value) {
                if (i + 1 >= argv.size()) throw Error("Too few arguments for " + name + ".\n" + usage());
                value = argv[++i];
            }
            v->second(value, name);
        } else {
            throw Error("Unknown argument: " + argv[i] + "\n" + usage());
        }
    }
    for (; i < argv.size(); ++i) c.input_files.push_back(argv[i]);
    const bool batch_one = batch_given && c.batch_frames == 1;  // asked for by name (the default of 1 may be raised)

    // validation (reference arguments.cpp:184-248)
    if (c.ray_density_threshold < 0)
        throw Error("Argument ray_density_threshold must be >= 0, " + fmt(c.ray_density_threshold) + " given.");
    if (c.ray_length_threshold < 0)
        throw Error("Argument ray_length_threshold must be >= 0, " + fmt(c.ray_length_threshold) + " given.");
    if (c.max_iterations < 1)
        throw Error("Argument max_iterations must be >= 1, " + std::to_string(c.max_iterations) + " given.");
    if (c.conv_tolerance <= 0)
        throw Error("Argument conv_tolerance must be > 0, " + fmt(c.conv_tolerance) + " given.");
    if (c.relaxation <= 0 || c.relaxation > 1.0)
        throw Error("Argument relaxation must be within (0, 1] interval," + fmt(c.relaxation) + " given.");
    if (c.beta_laplace < 0) throw Error("Argument beta_laplace must be positive.");
    if (c.max_cached_frames <= 0) throw Error("Argument max_cached_frames must be positive.");
    if (c.max_cached_solutions <= 0) throw Error("Argument max_cached_solutions must be positive.");
    if (c.batch_frames < 1) throw Error("Argument batch_frames must be >= 1.");
    if (c.partition_voxels && (c.batch_frames > 1 || c.use_cpu))
        throw Error("Argument partition_voxels applies to the single-frame GPU solver only.");
    if (c.rtm_bf16 && (c.use_cpu || c.partition_voxels))
        throw Error("Argument rtm_bf16 applies to the GPU solvers with pixel-row shards only.");
    if (c.rtm_f16 && c.rtm_bf16)
        throw Error("Arguments rtm_f16 and rtm_bf16 are exclusive: one storage format per RTM.");
    if (c.rtm_f16 && (c.use_cpu || c.partition_voxels))
        throw Error("Argument rtm_f16 applies to the GPU solvers with pixel-row shards only.");
    if (c.rtm_f16_fused && !c.rtm_f16) throw Error("Argument rtm_f16_fused needs rtm_f16.");
    if (c.rtm_format != "auto" && c.rtm_format != "dense" && c.rtm_format != "sparse")
        throw Error("Argument rtm_format must be auto, dense or sparse, " + c.rtm_format + " given.");
    if (c.rtm_format == "sparse" && (c.partition_voxels || c.rtm_bf16 || c.rtm_f16 || (c.use_cpu && c.batch_frames > 1)))
        throw Error("Argument rtm_format sparse applies to fp32 pixel-row shards (and not to CPU batches).");
    if (semantics_given && !c.fp64) throw Error("Argument fp64_semantics needs fp64.");
    if (c.fp64_semantics != "gpu" && c.fp64_semantics != "cpu")
        throw Error("Argument fp64_semantics must be gpu or cpu, " + c.fp64_semantics + " given.");
    if (c.fp64 && c.use_cpu)
        throw Error("Argument fp64 applies to the GPU solver: use_cpu already computes in double precision.");
    if (c.fp64 && c.batch_frames > 1) throw Error("Argument fp64 applies to the single-frame GPU solver only.");
    if (c.fp64 && c.partition_voxels) throw Error("Argument fp64 applies to pixel-row shards only (no partition_voxels).");
    if (c.fp64 && (c.rtm_bf16 || c.rtm_f16))
        throw Error("Argument fp64 applies to fp32 RTM storage only (no rtm_bf16 / rtm_f16).");
    if (c.fp64 && c.rtm_format == "sparse") throw Error("Argument fp64 applies to dense shards only (no rtm_format sparse).");
    if (c.fit_only && c.resume) throw Error("Argument fit_only solves no frame: it cannot be combined with resume.");
    if (c.fit_only && c.batch_frames > 1)
        throw Error("Argument fit_only solves no frame: it cannot be combined with batch_frames > 1.");
    if (c.fit_only && c.fp64) throw Error("Argument fit_only solves no frame: it cannot be combined with fp64.");
    if (scan_given) {
        c.beta_scan = to_beta_scan(scan_text);
        if (c.laplacian_file.empty()) throw Error("Argument beta_scan needs a laplacian_file.");
        if (c.use_cpu || c.fp64 || c.partition_voxels)
            throw Error("Argument beta_scan applies to the batched GPU solver with pixel-row shards only.");
        if (c.resume || c.fit || c.fit_only)
            throw Error("Argument beta_scan writes its own output: it cannot be combined with resume, fit or fit_only.");
        // every weight is a cold column of the batch engine: at least its narrowest batch, no lead engine, no chain
        if (c.batch_frames == 1) c.batch_frames = 16;
        c.no_guess = true;
    }
    if ((noise_given || c.replicas_keep) && !replicas_given)
        throw Error("Arguments noise_abs, noise_shot, noise_rel, noise_seed and replicas_keep need replicas.");
    if (replicas_given) {
        if (c.replicas < 2 || c.replicas > 1024)
            throw Error("Argument replicas must be within 2 .. 1024, " + std::to_string(c.replicas) + " given.");
        const double noise[3] = {c.noise_abs, c.noise_shot, c.noise_rel};
        const char* names[3] = {"noise_abs", "noise_shot", "noise_rel"};
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(noise[k]) || noise[k] < 0)
                throw Error(std::string("Argument ") + names[k] + " must be finite and >= 0, " + fmt(noise[k]) + " given.");
        if (!(c.noise_abs > 0 || c.noise_shot > 0 || c.noise_rel > 0))
            throw Error("Argument replicas needs a noise term: one of noise_abs, noise_shot, noise_rel must be > 0.");
        if (c.use_cpu || c.fp64 || c.partition_voxels)
            throw Error("Argument replicas applies to the batched GPU solver with pixel-row shards only.");
        if (c.resume || c.fit || c.fit_only || scan_given)
            throw Error("Argument replicas writes its own output: it cannot be combined with resume, fit, fit_only or "
                        "beta_scan.");
        // every replica is a cold column of the batch engine, as a weight of the scan is
        if (c.batch_frames == 1) c.batch_frames = 16;
        c.no_guess = true;
    }
    if (phantom_given) {
        if (c.phantom_file.empty()) throw Error("Argument phantom needs a file name.");
        if (c.use_cpu || c.fp64 || c.partition_voxels || batch_one)
            throw Error("Argument phantom applies to the batched GPU solver with pixel-row shards only.");
        if (c.resume || c.fit || c.fit_only || scan_given)
            throw Error("Argument phantom writes its own output: it cannot be combined with resume, fit, fit_only or "
                        "beta_scan.");
        // every phantom (and every replica of it) is a cold column of the batch engine, as a weight of the scan is
        if (c.batch_frames == 1) c.batch_frames = 16;
        c.no_guess = true;
    }
    if ((holdout_seed_given || holdout_betas_given) && !holdout_given)
        throw Error("Arguments holdout_seed and holdout_betas need holdout.");
    if (holdout_given) {
        if (trim(holdout_text) == "cameras") {
            c.holdout_cameras = true;
        } else {
            c.holdout = to_int(holdout_text, "--holdout");
            if (c.holdout < 2 || c.holdout > 32)
                throw Error("Argument holdout must be cameras or a number of folds within 2 .. 32, " +
                            std::to_string(c.holdout) + " given.");
        }
        if (holdout_seed_given && c.holdout_cameras)
            throw Error("Argument holdout_seed applies to pixel folds: it cannot be combined with holdout cameras.");
        if (holdout_betas_given) {
            c.holdout_betas = to_beta_scan(holdout_betas_text, "holdout_betas");
            if (c.laplacian_file.empty()) throw Error("Argument holdout_betas needs a laplacian_file.");
        }
        if (c.use_cpu || c.fp64 || c.partition_voxels)
            throw Error("Argument holdout applies to the batched GPU solver with pixel-row shards only.");
        if (c.resume || c.fit || c.fit_only || scan_given || replicas_given || phantom_given)
            throw Error("Argument holdout writes its own output: it cannot be combined with resume, fit, fit_only, "
                        "beta_scan, replicas or phantom.");
        // every masked frame is a cold column of the batch engine, as a weight of the scan is
        if (c.batch_frames == 1) c.batch_frames = 16;
        c.no_guess = true;
    }
    if (c.input_files.size() < 2)
        throw Error("At least two input file, one with RTM and one with image, are required, " +
                    std::to_string(c.input_files.size()) + " given.");
    return c;
}

std::vector<std::array<double, 4>> parse_time_intervals(const std::string& spec) {
    std::vector<std::array<double, 4>> out;
    if (spec.empty()) {
        out.push_back({0.0, std::numeric_limits<double>::infinity(), 0.0, 0.0});
        return out;
    }
    std::vector<std::string> pieces;
    {
        size_t pos = 0;
        while (true) {
            const size_t comma = spec.find(',', pos);
            pieces.push_back(spec.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos));
            if (comma == std::string::npos) break;
            pos = comma + 1;
        }
        if (pieces.size() > 1 && pieces.back().empty()) pieces.pop_back();  // trailing ',' is allowed
    }
    for (const auto& piece : pieces) {
        std::vector<std::string> f;
        size_t pos = 0;
        while (pos < piece.size()) {
            const size_t colon = piece.find(':', pos);
            f.push_back(piece.substr(pos, colon == std::string::npos ? std::string::npos : colon - pos));
            pos = colon == std::string::npos ? piece.size() : colon + 1;
        }
        if (f.size() < 2) throw Error("Unable to recognize a time interval in " + piece + ".");
        if (f.size() > 4) throw Error("Too many values in a time interval: " + piece + ".");
        double v[4] = {0, 0, 0, 0};
        for (size_t k = 0; k < f.size(); ++k) {
            // leading blanks are skipped, trailing characters ignored (std::stod semantics)
            const std::string t = f[k];
            char* end = nullptr;
            const char* beg = t.c_str();
            v[k] = std::strtod(beg, &end);
            if (end == beg) throw Error("Unable to convert " + piece + " to the time interval.");
        }
        if (v[0] < 0) throw Error("Time limits must be positive.");
        if (v[1] <= v[0]) throw Error("The upper limit of the time interval must be higher than the lower one.");
        if (v[2] > v[1] - v[0]) throw Error("Time step must be less or equal to the time interval.");
        if (v[3] > v[2]) throw Error("Synchronization threshold must be less or equal to the time step.");
        out.push_back({v[0], v[1], v[2], v[3]});
    }
    return out;
}

}  // namespace sart
