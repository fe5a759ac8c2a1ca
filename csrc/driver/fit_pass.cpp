// The native driver's passes after the frames (main thread, collective): groups of rows of the output file projected in
// fp64 on every rank's shard (FitProjector) for --fit / --fit_only (run_fit_pass), --beta_scan (run_scan_pass) and
// --holdout (run_holdout_pass).
#include <cmath>
#include <sstream>

#include "../kernels/launchers.hpp"
#include "../native/fit.hpp"
#include "driver.hpp"

namespace sart {
namespace {

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

// The fit projection of this rank's shard: device operands X [group][ldx], F [group][ldf] and the sparse kernel's
// voxel-major copy of X
struct FitProjector {
    const Driver& d;
    const Shard& sh;
    const int group;
    DeviceArray<double> dX, dF, dXt;
    int64_t ldx = 0, ldf = 0;
    SparseRtm view;
    FitProjector(const Driver& d_, const Shard& sh_) : d(d_), sh(sh_), group(fit_group(sh_)) {
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
    // Collective. The ray lengths of all pixels: the projection of the all-ones vector (one extra pass; any storage,
    // no engine needed), summed over the ranks
    std::vector<double> ray_lengths() {
        std::vector<double> ell(d.in.npixel, 0.0);
        const std::vector<double> ones(d.in.nvoxel, 1.0);
        project(ones.data(), 1, ell.data());
        d.host->all_reduce_host(ell.data(), ell.size(), ReduceOp::kSum);
        return ell;
    }
    // Collective. `total` rows in groups of up to `group`: rank 0's read(j0, n, X) fills X [n][nvoxel] and is broadcast,
    // every rank projects on its shard (row shards: its rows; column shards: partial sums over its voxels for all
    // pixels), the images are summed over the ranks through a zero-filled host all-reduce, rank 0's
    // consume(j0, n, F) gets F [n][npixel]. The number of groups.
    template <class Read, class Consume>
    uint64_t for_groups(uint64_t total, Read&& read, Consume&& consume) {
        const uint64_t npixel = d.in.npixel, nvoxel = d.in.nvoxel;
        std::vector<double> X((size_t)group * nvoxel), F((size_t)group * npixel);
        uint64_t groups = 0;
        for (uint64_t j0 = 0; j0 < total; j0 += group, ++groups) {
            const int n = (int)std::min<uint64_t>(group, total - j0);
            if (d.rank == 0) read(j0, n, X.data());
            d.host->broadcast_host(X.data(), (size_t)n * nvoxel * sizeof(double), 0);
            std::fill(F.begin(), F.begin() + (size_t)n * npixel, 0.0);
            project(X.data(), n, F.data());
            d.host->all_reduce_host(F.data(), (size_t)n * npixel, ReduceOp::kSum);
            if (d.rank == 0) consume(j0, n, F.data());
        }
        return groups;
    }
};

// rank 0: the measured frames over all pixels
std::unique_ptr<CompositeImage> all_pixel_image(const Driver& d) {
    auto full = std::make_unique<CompositeImage>(d.in.image_files, d.in.frame_masks, d.intervals, d.in.npixel, 0);
    full->set_max_cache_size((uint64_t)d.cfg.max_cached_frames);
    return full;
}

}  // namespace

// --fit / --fit_only: the fitted images f = A x (fp64) of every solution stored in the output file, in groups of up to
// 8 per pass over the shard (4 on bf16 / f16 shards; SART_FIT_GROUP overrides), and their residuals against the
// measured composite frames, into the file's /fit group (docs/FORMATS.md). With the solution writer closed. Rank 0
// reads the stored solutions, computes the statistics and writes. A value depends on its pixel row and solution only
// (csrc/kernels/fit64.hip), so the file is the same for any grouping and any number of row-shard ranks.
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
    FitProjector fp(d, sh);
    const std::vector<double> ell = fp.ray_lengths();
    std::unique_ptr<FitWriter> fw;
    std::unique_ptr<CompositeImage> full;
    std::vector<int64_t> camera_pixels;
    if (d.rank == 0) {
        for (const auto& cam : in.camera_names) {
            const auto& mask = in.frame_masks.at(cam);
            camera_pixels.push_back((int64_t)std::count_if(mask.begin(), mask.end(), [](int32_t v) { return v != 0; }));
        }
        full = all_pixel_image(d);
        fw = std::make_unique<FitWriter>(cfg.output_file, T, npixel, in.camera_names.size());
    }
    const uint64_t groups = fp.for_groups(
        T,
        [&](uint64_t k0, int n, double* X) {
            const std::vector<double> rows = read_solution_rows(cfg.output_file, k0, n, nvoxel);
            std::copy(rows.begin(), rows.end(), X);
        },
        [&](uint64_t k0, int n, const double* F) {
            for (int j = 0; j < n; ++j) {
                const std::vector<double> g = full->frame(frame_of[k0 + j]);
                const double* f = F + (size_t)j * npixel;
                fw->write(k0 + j, f, fit_statistics(f, g.data(), ell.data(), (int64_t)npixel,
                                                    cfg.ray_length_threshold, camera_pixels));
            }
        });
    host->barrier();
    if (d.rank == 0) {
        const double ms = ms_since(t_fit);
        std::cout << "Fit of " << T << " frame(s) in: " << ms << " ms" << std::endl;
        if (d.profile.is_open()) write_fit_line(d.profile, T, groups, ms, sh.storage, sh.format, d.size);
    }
}

// --beta_scan, after the loop: the rows of /beta_scan/value through FitProjector::for_groups -- rank 0 takes the
// residual norm of a row's image against the frame's measured pixels (the /fit/residual_norm definition) and the
// roughness norm of the same device copy of the group (csrc/kernels/rough64.hip). A frame whose nb points are complete
// gets its corner (lcurve_corner); the selected column goes to /solution through the ordinary writer, in frame order.
void run_scan_pass(Driver& d, const Shard& sh, const Csr& lap, const std::vector<uint64_t>& frames, ScanColumns& sc) {
    const Config& cfg = d.cfg;
    const CompositeImage& image = *d.image;
    const auto t_scan = Clock::now();
    const uint64_t npixel = d.in.npixel, nvoxel = d.in.nvoxel;
    const uint64_t nb = cfg.beta_scan.size(), T = frames.size(), nvirt = T * nb;
    // -b names the fallback: the ladder entry nearest to it (ties to the smaller)
    int fallback = 0;
    for (uint64_t i = 1; i < nb; ++i)
        if (std::abs(cfg.beta_scan[i] - cfg.beta_laplace) < std::abs(cfg.beta_scan[fallback] - cfg.beta_laplace))
            fallback = (int)i;
    FitProjector fp(d, sh);
    const std::vector<double> ell = fp.ray_lengths();
    std::unique_ptr<CompositeImage> full;
    DeviceArray<int64_t> lrp;
    DeviceArray<int32_t> lcol;
    DeviceArray<float> lval;
    DeviceArray<double> deta2, dscratch;
    if (d.rank == 0) {
        full = all_pixel_image(d);
        lrp.resize(nvoxel + 1), lcol.resize((size_t)lap.nnz()), lval.resize((size_t)lap.nnz());
        hip_ok(hipMemcpy(lrp.get(), lap.row_ptr.data(), (nvoxel + 1) * sizeof(int64_t), hipMemcpyHostToDevice), "H2D");
        hip_ok(hipMemcpy(lcol.get(), lap.col.data(), (size_t)lap.nnz() * sizeof(int32_t), hipMemcpyHostToDevice), "H2D");
        hip_ok(hipMemcpy(lval.get(), lap.val.data(), (size_t)lap.nnz() * sizeof(float), hipMemcpyHostToDevice), "H2D");
        deta2.resize(8);
        dscratch.resize((size_t)rough64_scratch_elems((int64_t)nvoxel));
    }
    const std::vector<int64_t> one_camera{(int64_t)npixel};  // the norm over all pixels does not depend on the split
    std::vector<double> rho(nvirt), eta(nvirt), x(nvoxel), g;
    uint64_t g_frame = T, decided = 0;  // g: the measured frame g_frame; frames [0, decided) have their corner
    fp.for_groups(
        nvirt, [&](uint64_t j0, int n, double* X) { sc.file->read_columns(j0, n, X); },
        [&](uint64_t j0, int n, const double* F) {
            for (int j = 0; j < n; ++j) {
                const uint64_t k = (j0 + j) / nb;
                if (k != g_frame) g = full->frame(frames[k]), g_frame = k;
                rho[j0 + j] = fit_statistics(F + (size_t)j * npixel, g.data(), ell.data(), (int64_t)npixel,
                                             cfg.ray_length_threshold, one_camera).residual_norm;
            }
            double eta2[8];  // (fp.dX: this group's rows, as its projection left them on the device)
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
        });
    d.host->barrier();
    if (d.rank == 0)
        std::cout << "Beta scan of " << T << " frame(s) x " << nb << " weights in: " << ms_since(t_scan) << " ms"
                  << std::endl;
}

// --holdout, after the loop: the rows of /holdout/value through FitProjector::for_groups -- rank 0 uploads the group's
// images next to the frame's measured pixels, the ray lengths and the fold table and takes the six sums per column and
// camera (csrc/kernels/holdout64.hip; a group that straddles two composite frames is scored in two launches). The
// images are the zero-filled host all-reduce's and a value of the kernel depends on its column and camera alone, so
// /holdout depends neither on the rank count (given the same columns) nor on the grouping. A frame whose nb (K + 1)
// columns are complete gets its scores (holdout_scores); column 0 of the selected weight goes to /solution through the
// ordinary writer, in frame order.
void run_holdout_pass(Driver& d, const Shard& sh, const std::vector<uint64_t>& frames, HoldoutColumns& hc) {
    const Config& cfg = d.cfg;
    const CompositeImage& image = *d.image;
    const auto t_pass = Clock::now();
    const uint64_t npixel = d.in.npixel, nvoxel = d.in.nvoxel;
    const uint64_t nb = (uint64_t)hc.nb(), nc = (uint64_t)hc.K + 1, ncam = (uint64_t)hc.ncam(), T = frames.size();
    const uint64_t per_frame = nb * nc, nvirt = T * per_frame, per_col = ncam * kHoldoutSums;
    const int fallback = holdout_fallback(hc.betas.data(), (int)nb, cfg.beta_laplace);
    FitProjector fp(d, sh);
    const std::vector<double> ell = fp.ray_lengths();
    std::unique_ptr<CompositeImage> full;
    DeviceArray<double> dF, dg, dell, dsums;
    DeviceArray<int32_t> dfold, dheld;
    DeviceArray<int64_t> dcam;
    struct Events {  // the scoring kernel's time (--profile)
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } ev;
    if (d.rank == 0) {
        full = all_pixel_image(d);
        dF.resize((size_t)fp.group * npixel), dg.resize(npixel), dell.resize(npixel), dfold.resize(npixel);
        dheld.resize((size_t)fp.group), dcam.resize(ncam + 1), dsums.resize((size_t)fp.group * per_col);
        hip_ok(hipMemcpy(dell.get(), ell.data(), npixel * sizeof(double), hipMemcpyHostToDevice), "H2D ray lengths");
        hip_ok(hipMemcpy(dfold.get(), hc.folds.data(), npixel * sizeof(int32_t), hipMemcpyHostToDevice), "H2D folds");
        hip_ok(hipMemcpy(dcam.get(), hc.cam_start.data(), (ncam + 1) * sizeof(int64_t), hipMemcpyHostToDevice),
               "H2D cameras");
        hip_ok(hipEventCreate(&ev.e0), "hipEventCreate");
        hip_ok(hipEventCreate(&ev.e1), "hipEventCreate");
    }
    std::vector<double> sums(d.rank == 0 ? nvirt * per_col : 0), x(nvoxel), g;
    std::vector<int32_t> held((size_t)fp.group);
    uint64_t g_frame = T, decided = 0;  // g: the measured frame g_frame (on the device too); frames [0, decided) are scored
    double scoring_ms = 0.0;
    const uint64_t groups = fp.for_groups(
        nvirt, [&](uint64_t j0, int n, double* X) { hc.file->read_columns(j0, n, X); },
        [&](uint64_t j0, int n, const double* F) {
            hip_ok(hipMemcpy(dF.get(), F, (size_t)n * npixel * sizeof(double), hipMemcpyHostToDevice), "H2D images");
            for (int a = 0; a < n;) {  // the columns [a, b) of the group belong to one composite frame
                const uint64_t k = (j0 + a) / per_frame;
                int b = a;
                while (b < n && (j0 + b) / per_frame == k) ++b;
                if (k != g_frame) {
                    g = full->frame(frames[k]), g_frame = k;
                    hip_ok(hipMemcpy(dg.get(), g.data(), npixel * sizeof(double), hipMemcpyHostToDevice), "H2D frame");
                }
                for (int j = a; j < b; ++j) held[j - a] = (int32_t)((j0 + j) % nc) - 1;
                hip_ok(hipMemcpy(dheld.get(), held.data(), (size_t)(b - a) * sizeof(int32_t), hipMemcpyHostToDevice),
                       "H2D held folds");
                hip_ok(hipEventRecord(ev.e0, nullptr), "hipEventRecord");
                launch_holdout64(dF.get() + (size_t)a * npixel, (int64_t)npixel, b - a, dg.get(), dell.get(),
                                 cfg.ray_length_threshold, dfold.get(), dheld.get(), dcam.get(), (int)ncam, dsums.get(),
                                 nullptr);
                hip_ok(hipEventRecord(ev.e1, nullptr), "hipEventRecord");
                hip_ok(hipMemcpy(sums.data() + (j0 + a) * per_col, dsums.get(), (size_t)(b - a) * per_col * sizeof(double),
                                 hipMemcpyDeviceToHost), "D2H hold-out sums");
                float ms = 0.f;
                hip_ok(hipEventElapsedTime(&ms, ev.e0, ev.e1), "hipEventElapsedTime");
                scoring_ms += ms;
                a = b;
            }
            for (; (decided + 1) * per_frame <= j0 + n; ++decided) {
                const uint64_t k = decided, cur = frames[k];
                const HoldoutScores sc = holdout_scores(sums.data() + k * per_frame * per_col,
                                                        hc.ok.data() + k * per_frame, (int)nb, hc.K, (int)ncam, fallback);
                hc.file->write_frame(k, sums.data() + k * per_frame * per_col, sc);
                const uint64_t js = (k * nb + (uint64_t)sc.selected) * nc;
                hc.file->read_columns(js, 1, x.data());  // the stored row itself: /solution/value[k] is its bits
                hc.file->close();                        // the solution writer opens the file itself
                d.writer->add(x, hc.status[js], image.frame_time(cur), image.camera_frame_time(cur), hc.iterations[js]);
            }
        });
    d.host->barrier();
    if (d.rank == 0) {
        const double ms = ms_since(t_pass);
        std::cout << "Hold-out of " << T << " frame(s) x " << nb << " weights x " << hc.K << " folds in: " << ms << " ms"
                  << std::endl;
        if (d.profile.is_open())
            write_holdout_line(d.profile, {cfg.holdout_cameras ? "cameras" : "pixels", hc.K, cfg.holdout_seed, nb, T,
                                           nvirt, groups, scoring_ms, ms});
    }
}

}  // namespace sart
