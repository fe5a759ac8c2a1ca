// The native driver's series of virtual frames (SeriesRun over T nc columns, virtual frame j = k nc + c being column c
// of composite frame k, all cold columns of the multi-frame engine): --beta_scan (run_scan_series), --replicas
// (run_replica_series with its noise source) and --phantom (run_phantom_series with its projection source), the last
// two on one loop (run_replica_columns), and --holdout (run_holdout_series: T nb (K + 1) columns, masked on the reader
// thread).
#include <cstring>
#include <functional>

#include "../kernels/launchers.hpp"
#include "../native/phantom.hpp"
#include "../native/uncertainty.hpp"
#include "driver.hpp"

namespace sart {
namespace {

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
    // launch(stream) between the two events (the caller's copies around it stay outside them)
    template <class Launch>
    void timed(Launch&& launch) {
        hip_ok(hipEventRecord(e0, stream), "hipEventRecord");
        launch(stream);
        hip_ok(hipEventRecord(e1, stream), "hipEventRecord");
    }
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
            ts_.timed([&](hipStream_t st) {
                launch_noise_replicas(dg_.get(), npix_, (uint64_t)d_.blk.offset, bits, (uint32_t)r0, n, cfg_.noise_abs,
                                      cfg_.noise_shot, cfg_.noise_rel, cfg_.noise_seed, dout_.get(), ldo_, st);
            });
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

// --phantom, the frame source's device side: this rank's pixels of the fp64 projections f = A t of the phantom file's
// rows through the shard as stored (csrc/kernels/fit64.hip), fit64_group rows per pass on a stream of its own while the
// engine sweeps the same read-only shard. Every rank reads the rows itself (a row shard holds all voxels): no host
// collective. The series asks for the phantoms in order; a projected row is kept for the replicas of its phantom and
// for /phantom/image. A pixel's bits depend on its row of the matrix and the phantom alone.
class PhantomSource {
   public:
    PhantomSource(const Driver& d, const Shard& sh, const PhantomFile& file)
        : d_(d), sh_(sh), file_(file), npix_((int64_t)d.blk.size), nvoxel_((int64_t)d.in.nvoxel) {
        const DeviceShard* dn = sh.dense.get();
        if (!sh.gpu || (!dn && !sh.sparse)) throw std::runtime_error("phantom projections need a device shard");
        group_ = fit64_group(dn && dn->bf16, dn && dn->f16, !dn);
        if (dn) {
            ldx_ = dn->ld;
            ldf_ = dn->nrows_pad;
        } else {
            ldx_ = (sh.sparse->nvoxel + 63) / 64 * 64;
            ldf_ = (sh.sparse->nrows + 63) / 64 * 64;
            dXt_.resize((size_t)ldx_ * 8);
            view_ = sh.sparse->view();
        }
        if (ldx_ < nvoxel_ || ldf_ < npix_) throw std::runtime_error("phantom projections: the shard's padding");
        dX_.resize((size_t)group_ * ldx_);
        dF_.resize((size_t)group_ * ldf_);
        rows_.resize((size_t)group_ * nvoxel_);
        image_.resize((size_t)file.count() * npix_);
    }
    PhantomSource(const PhantomSource&) = delete;
    PhantomSource& operator=(const PhantomSource&) = delete;
    // this rank's pixels of phantom k's projection (reader thread)
    std::vector<double> frame(int64_t k) {
        while (k >= done_) project_next();
        return std::vector<double>(image_.begin() + (size_t)k * npix_, image_.begin() + (size_t)(k + 1) * npix_);
    }
    const std::vector<double>& image() const { return image_; }  // [n][this rank's pixels], after the series
    double kernel_ms() const { return kernel_ms_; }
    uint64_t groups() const { return groups_; }

   private:
    void project_next() {
        const int64_t k0 = done_;
        const int n = (int)std::min<int64_t>(group_, (int64_t)file_.count() - k0);
        if (n < 1) throw std::runtime_error("phantom beyond the file's rows");
        file_.read_rows((uint64_t)k0, (uint64_t)n, rows_.data());
        const DeviceShard* dn = sh_.dense.get();
        hip_ok(hipSetDevice(d_.device), "hipSetDevice");  // (the reader thread's first call)
        for (int j = 0; j < n; ++j)
            hip_ok(hipMemcpyAsync(dX_.get() + (size_t)j * ldx_, rows_.data() + (size_t)j * nvoxel_,
                                  (size_t)nvoxel_ * sizeof(double), hipMemcpyHostToDevice, ts_.stream), "H2D phantoms");
        ts_.timed([&](hipStream_t st) {
            if (dn)
                launch_fit64(dn->A, dn->bf16, dn->f16, dn->rsc.get(), dn->ld, dn->nrows, dn->nrows_pad, dn->nvoxel,
                             dX_.get(), ldx_, n, dF_.get(), ldf_, st);
            else
                launch_fit64_csr(view_, sh_.sparse->nrows, sh_.sparse->nvoxel, ldx_, dX_.get(), ldx_, n, dXt_.get(),
                                 dF_.get(), ldf_, st);
        });
        for (int j = 0; j < n; ++j)
            hip_ok(hipMemcpyAsync(image_.data() + (size_t)(k0 + j) * npix_, dF_.get() + (size_t)j * ldf_,
                                  (size_t)npix_ * sizeof(double), hipMemcpyDeviceToHost, ts_.stream), "D2H projections");
        hip_ok(hipStreamSynchronize(ts_.stream), "phantom projections");
        kernel_ms_ += ts_.elapsed_ms();
        ++groups_;
        done_ = k0 + n;
    }
    const Driver& d_;
    const Shard& sh_;
    const PhantomFile& file_;
    const int64_t npix_, nvoxel_;
    int group_ = 1;
    int64_t ldx_ = 0, ldf_ = 0;
    DeviceArray<double> dX_, dF_, dXt_;
    SparseRtm view_;
    std::vector<double> rows_, image_;
    TimedStream ts_;
    int64_t done_ = 0;  // the phantoms [0, done_) are projected
    uint64_t groups_ = 0;
    double kernel_ms_ = 0.0;
};

// Where the composite frames of a replica run come from (run_replica_columns): the measured frames or the phantoms
struct FrameOrigin {
    std::function<std::vector<double>(int64_t)> pixels;  // composite frame k: this rank's pixels (reader thread)
    std::function<double(int64_t)> time;
    std::function<std::vector<double>(int64_t)> camera_times;
    std::function<std::string(int64_t)> name;  // in warnings: "frame 12"
};

// rank 0: the columns of a composite frame, all arrived
struct ColumnSet {
    std::vector<double> x;  // [nc][nvoxel]
    std::vector<int32_t> status, iterations;
    std::vector<uint8_t> use;  // [N]: replica r + 1 did not stop on a non-finite iterate
};

// Column r of composite frame k (of T) is its replica r (r = 0: the frame itself), N = cfg.replicas replicas each
// (--phantom alone: 0). Rank 0 keeps a composite frame's columns on the host until the last one has arrived, hands
// them to `arrived` (optional; ms: the moments stream), takes the per-voxel moments of replicas 1 .. N
// (csrc/kernels/moments64.hip, on a stream of its own, synchronised before the buffer is released), writes the frame's
// rows of /uncertainty (file; N > 0) and hands column 0 to the ordinary solution writer in frame order.
void run_replica_columns(Driver& d, Solvers& s, int64_t T, const FrameOrigin& from, UncertaintyWriter* file,
                         const std::function<void(int64_t, const ColumnSet&, TimedStream&)>& arrived) {
    const Config& cfg = d.cfg;
    const int64_t N = cfg.replicas, nc = N + 1;
    const int64_t nvoxel = (int64_t)d.in.nvoxel;
    ColumnCount cols(T, nc);
    std::unique_ptr<ReplicaSource> noise;
    if (N > 0) noise = std::make_unique<ReplicaSource>(d, s.mf->nrows());
    SeriesRun run(d, *s.mf, T * nc, [&](int64_t j) {
        const int64_t k = cols.frame(j);
        std::vector<double> g = from.pixels(k);
        if (cols.column(j) == 0) return g;
        return noise->replica(k, g, from.time(k), (int)cols.column(j));
    });
    // rank 0: the columns of the composite frames in flight, the moments' device operands
    std::map<int64_t, ColumnSet> open;
    InOrder<ColumnSet> done;  // the completed frames, cut down to column 0: to /solution in frame order
    DeviceArray<double> dX, dmean, dstd;
    DeviceArray<uint8_t> duse;
    std::unique_ptr<TimedStream> ms;
    std::vector<double> mean, sd;
    if (d.rank == 0) {
        if (N > 0) {
            dX.resize((size_t)N * nvoxel), dmean.resize((size_t)nvoxel), dstd.resize((size_t)nvoxel);
            duse.resize((size_t)N);
            mean.resize((size_t)nvoxel), sd.resize((size_t)nvoxel);
        }
        ms = std::make_unique<TimedStream>();
    }
    double moments_ms = 0.0;
    run.solve(0, nullptr, false, nullptr, [&](int64_t j, const double* xs, const SolveInfo& info) {
        const int64_t k = cols.frame(j), r = cols.column(j);
        auto it = open.find(k);
        if (it == open.end())
            it = open.emplace(k, ColumnSet{std::vector<double>((size_t)nc * nvoxel), std::vector<int32_t>((size_t)nc),
                                           std::vector<int32_t>((size_t)nc), std::vector<uint8_t>((size_t)N)}).first;
        ColumnSet& c = it->second;
        std::copy(xs, xs + nvoxel, c.x.begin() + (size_t)r * nvoxel);
        c.status[r] = info.status, c.iterations[r] = info.iterations;
        if (r > 0) c.use[r - 1] = info.nonfinite ? 0 : 1;
        if (info.nonfinite)
            std::cerr << "warning: " << from.name(k) << ", replica " << r << ": non-finite iterate, stopped"
                      << std::endl;
        if (!cols.arrived(j)) return;
        if (arrived) arrived(k, c, *ms);
        if (N > 0) {
            hipStream_t mstream = ms->stream;
            hip_ok(hipMemcpyAsync(dX.get(), c.x.data() + nvoxel, (size_t)N * nvoxel * sizeof(double),
                                  hipMemcpyHostToDevice, mstream), "H2D replicas");
            hip_ok(hipMemcpyAsync(duse.get(), c.use.data(), (size_t)N, hipMemcpyHostToDevice, mstream), "H2D mask");
            ms->timed([&](hipStream_t st) {
                launch_moments64(dX.get(), nvoxel, nvoxel, (int)N, duse.get(), dmean.get(), dstd.get(), st);
            });
            hip_ok(hipMemcpyAsync(mean.data(), dmean.get(), (size_t)nvoxel * sizeof(double), hipMemcpyDeviceToHost,
                                  mstream), "D2H mean");
            hip_ok(hipMemcpyAsync(sd.data(), dstd.get(), (size_t)nvoxel * sizeof(double), hipMemcpyDeviceToHost,
                                  mstream), "D2H std");
            hip_ok(hipStreamSynchronize(mstream), "moments");
            moments_ms += ms->elapsed_ms();
            const int32_t count = (int32_t)std::count(c.use.begin(), c.use.end(), (uint8_t)1);
            file->write_frame((uint64_t)k, mean.data(), sd.data(), count, c.status.data(), c.iterations.data(),
                              cfg.replicas_keep ? c.x.data() : nullptr);
        }
        c.x.resize((size_t)nvoxel);  // column 0 alone goes on to the solution writer
        done.put(k, std::move(c));
        open.erase(it);
        run.tick();
        done.drain([&](int64_t w, ColumnSet&& c0) {
            d.writer->add(c0.x, c0.status[0], from.time(w), from.camera_times(w), c0.iterations[0]);
        });
    });
    if (N > 0 && d.rank == 0 && d.profile.is_open())
        write_uncertainty_line(d.profile, {cfg.replicas, cfg.noise_seed, cfg.noise_abs, cfg.noise_shot, cfg.noise_rel,
                                           noise->kernel_ms(), moments_ms, (uint64_t)T});
}

// rank 0: the output file created with its /uncertainty group
std::unique_ptr<UncertaintyWriter> create_uncertainty(const Driver& d, int64_t T) {
    const Config& cfg = d.cfg;
    const double triple[3] = {cfg.noise_abs, cfg.noise_shot, cfg.noise_rel};
    return std::make_unique<UncertaintyWriter>(cfg.output_file, (uint64_t)T, (uint64_t)cfg.replicas, d.in.nvoxel,
                                               triple, cfg.noise_seed, cfg.replicas_keep);
}

}  // namespace

// --beta_scan, the frame loop: column i of composite frame k is the frame at weight i, with a weight per column. Rank
// 0 writes every finished column into /beta_scan as it arrives; nothing goes to /solution yet.
void run_scan_series(Driver& d, Solvers& s, const std::vector<uint64_t>& frames, ScanColumns& sc) {
    const Config& cfg = d.cfg;
    const int64_t nb = (int64_t)cfg.beta_scan.size(), T = (int64_t)frames.size(), nvirt = T * nb;
    ColumnCount cols(T, nb);
    SeriesRun run(d, *s.mf, nvirt,
                  [&](int64_t j) { return d.image->frame(frames[cols.frame(j)]); });  // (the image caches its frames)
    std::vector<float> frame_beta((size_t)nvirt);
    for (int64_t j = 0; j < nvirt; ++j) frame_beta[j] = (float)cfg.beta_scan[cols.column(j)];
    run.solve(0, nullptr, false, frame_beta.data(), [&](int64_t j, const double* xs, const SolveInfo& info) {
        const int64_t k = cols.frame(j), i = cols.column(j);
        sc.file->write_column((uint64_t)k, (uint64_t)i, xs, info.status, info.iterations);
        sc.status[j] = info.status, sc.iterations[j] = info.iterations, sc.ok[j] = info.nonfinite ? 0 : 1;
        if (info.nonfinite)
            std::cerr << "warning: frame " << frames[k] << ", beta " << cfg.beta_scan[i]
                      << ": non-finite iterate, stopped" << std::endl;
        if (cols.arrived(j)) run.tick();
    });
    if (d.rank == 0) sc.file->close();
}

// --holdout, the frame loop: virtual frame j = (k nb + i) (K + 1) + c is composite frame k at weight i, as measured
// (c = 0) or with the pixels of fold c - 1 set to the solver's exclusion marker (reader thread: one pass over this rank's
// pixels, the fold of global pixel blk.offset + p). Rank 0 writes every finished column into /holdout as it arrives;
// nothing goes to /solution yet.
void run_holdout_series(Driver& d, Solvers& s, const std::vector<uint64_t>& frames, HoldoutColumns& hc) {
    const int64_t nb = hc.nb(), nc = hc.K + 1, T = (int64_t)frames.size(), nvirt = T * nb * nc;
    ColumnCount cols(T, nb * nc);
    const int32_t* fold = hc.folds.data() + d.blk.offset;
    SeriesRun run(d, *s.mf, nvirt, [&](int64_t j) {
        std::vector<double> g = d.image->frame(frames[cols.frame(j)]);  // (the image caches its frames)
        const int c = (int)(cols.column(j) % nc);
        if (c > 0) holdout_mask(g.data(), fold, (int64_t)g.size(), c - 1, g.data());
        return g;
    });
    std::vector<float> frame_beta;
    if (!d.cfg.holdout_betas.empty()) {
        frame_beta.resize((size_t)nvirt);
        for (int64_t j = 0; j < nvirt; ++j) frame_beta[j] = (float)hc.betas[cols.column(j) / nc];
    }
    run.solve(0, nullptr, false, frame_beta.empty() ? nullptr : frame_beta.data(),
              [&](int64_t j, const double* xs, const SolveInfo& info) {
        const int64_t k = cols.frame(j), i = cols.column(j) / nc, c = cols.column(j) % nc;
        hc.file->write_column((uint64_t)k, (uint64_t)i, (uint64_t)c, xs, info.status, info.iterations);
        hc.status[j] = info.status, hc.iterations[j] = info.iterations, hc.ok[j] = info.nonfinite ? 0 : 1;
        if (info.nonfinite)
            std::cerr << "warning: frame " << frames[k] << ", beta " << hc.betas[i] << ", hold-out column " << c
                      << ": non-finite iterate, stopped" << std::endl;
        if (cols.arrived(j)) run.tick();
    });
    if (d.rank == 0) hc.file->close();
}

// --replicas: the composite frames are the measured ones (run_replica_columns)
void run_replica_series(Driver& d, Solvers& s, const std::vector<uint64_t>& frames) {
    const CompositeImage& image = *d.image;
    const FrameOrigin measured{
        [&](int64_t k) { return d.image->frame(frames[k]); },  // (the image caches its frames)
        [&](int64_t k) { return image.frame_time(frames[k]); },
        [&](int64_t k) { return image.camera_frame_time(frames[k]); },
        [&](int64_t k) { return "frame " + std::to_string(frames[k]); },
    };
    std::unique_ptr<UncertaintyWriter> file;
    if (d.rank == 0) file = create_uncertainty(d, (int64_t)frames.size());
    run_replica_columns(d, s, (int64_t)frames.size(), measured, file.get(), nullptr);
}

// --phantom: composite frame k is the projection of phantom k (PhantomSource), its time the phantom's. When a phantom's
// columns have all arrived, rank 0 uploads its truth once and scores the columns in groups of 8
// (csrc/kernels/phantom64.hip, on the moments stream) into /phantom; with --replicas the moments go to /uncertainty as
// in any replica run. After the series the ranks' pixels of the noise-free projections are put together (one host
// all-reduce of zero-filled images, main thread) and rank 0 writes /phantom/image.
uint64_t run_phantom_series(Driver& d, Solvers& s, const Shard& sh) {
    const Config& cfg = d.cfg;
    const PhantomFile phantoms(cfg.phantom_file, d.in.nvoxel);
    const int64_t T = (int64_t)phantoms.count(), nc = (int64_t)cfg.replicas + 1;
    const int64_t nvoxel = (int64_t)d.in.nvoxel, npixel = (int64_t)d.in.npixel;
    const std::vector<double>& times = phantoms.times();
    PhantomSource source(d, sh, phantoms);
    const size_t ncam = d.in.camera_names.size();
    const FrameOrigin projected{
        [&](int64_t k) { return source.frame(k); },
        [&](int64_t k) { return times[(size_t)k]; },
        [&](int64_t k) { return std::vector<double>(ncam, times[(size_t)k]); },
        [&](int64_t k) { return "phantom " + std::to_string(k); },
    };
    std::unique_ptr<UncertaintyWriter> ufile;
    std::unique_ptr<PhantomWriter> pfile;
    DeviceArray<double> dt, dX, dsums, dscratch;
    std::vector<double> truth, sums;
    if (d.rank == 0) {
        if (cfg.replicas > 0) ufile = create_uncertainty(d, T);  // creates the file: /phantom is added to it
        pfile = std::make_unique<PhantomWriter>(cfg.output_file, (uint64_t)T, (uint64_t)nc, (uint64_t)npixel,
                                                cfg.phantom_file, times.data(), cfg.replicas > 0);
        dt.resize((size_t)nvoxel), dX.resize((size_t)8 * nvoxel), dsums.resize((size_t)8 * kPhantomSums);
        dscratch.resize((size_t)phantom64_scratch_elems(nvoxel));
        truth.resize((size_t)nvoxel), sums.resize((size_t)nc * kPhantomSums);
    }
    double scoring_ms = 0.0;
    run_replica_columns(d, s, T, projected, ufile.get(), [&](int64_t k, const ColumnSet& c, TimedStream& ms) {
        phantoms.read_rows((uint64_t)k, 1, truth.data());
        hip_ok(hipMemcpyAsync(dt.get(), truth.data(), (size_t)nvoxel * sizeof(double), hipMemcpyHostToDevice,
                              ms.stream), "H2D truth");
        for (int64_t c0 = 0; c0 < nc; c0 += 8) {
            const int nv = (int)std::min<int64_t>(8, nc - c0);
            hip_ok(hipMemcpyAsync(dX.get(), c.x.data() + (size_t)c0 * nvoxel, (size_t)nv * nvoxel * sizeof(double),
                                  hipMemcpyHostToDevice, ms.stream), "H2D columns");
            ms.timed([&](hipStream_t st) {
                launch_phantom64(dX.get(), nvoxel, nvoxel, nv, dt.get(), dsums.get(), dscratch.get(), st);
            });
            hip_ok(hipMemcpyAsync(sums.data() + (size_t)c0 * kPhantomSums, dsums.get(),
                                  (size_t)nv * kPhantomSums * sizeof(double), hipMemcpyDeviceToHost, ms.stream),
                   "D2H sums");
            hip_ok(hipStreamSynchronize(ms.stream), "phantom scores");
            scoring_ms += ms.elapsed_ms();
        }
        pfile->write_phantom((uint64_t)k, sums.data(), c.status.data(), c.iterations.data());
    });
    // the noise-free projections over all pixels: every rank's block into a zero-filled image, summed over the ranks
    std::vector<double> image((size_t)T * npixel, 0.0);
    const std::vector<double>& mine = source.image();
    for (int64_t k = 0; k < T; ++k)
        std::copy(mine.begin() + (size_t)k * d.blk.size, mine.begin() + (size_t)(k + 1) * d.blk.size,
                  image.begin() + (size_t)k * npixel + d.blk.offset);
    d.host->all_reduce_host(image.data(), image.size(), ReduceOp::kSum);
    if (d.rank == 0) {
        pfile->write_images(image.data());
        if (d.profile.is_open())
            write_phantom_line(d.profile, {(uint64_t)T, cfg.replicas, source.groups(), source.kernel_ms(), scoring_ms});
    }
    return (uint64_t)T;
}

}  // namespace sart
