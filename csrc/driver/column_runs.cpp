// The native driver's series of virtual frames (SeriesRun over T nc columns, virtual frame j = k nc + c being column c
// of composite frame k, all cold columns of the multi-frame engine): --beta_scan (run_scan_series) and --replicas
// (run_replica_series with its noise source).
#include <cstring>

#include "../kernels/launchers.hpp"
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

// --replicas: column r of composite frame k is its replica r (r = 0: the measured frame itself). Rank 0 keeps a
// composite frame's columns on the host until the last one has arrived, takes the per-voxel moments of replicas 1 .. N
// (csrc/kernels/moments64.hip, on a stream of its own, synchronised before the buffer is released), writes the frame's
// rows of /uncertainty and hands column 0 to the ordinary solution writer in frame order.
void run_replica_series(Driver& d, Solvers& s, const std::vector<uint64_t>& frames) {
    const Config& cfg = d.cfg;
    const CompositeImage& image = *d.image;
    const int64_t N = cfg.replicas, nc = N + 1, T = (int64_t)frames.size();
    const int64_t nvoxel = (int64_t)d.in.nvoxel;
    ColumnCount cols(T, nc);
    ReplicaSource noise(d, s.mf->nrows());
    SeriesRun run(d, *s.mf, T * nc, [&](int64_t j) {
        const int64_t k = cols.frame(j);
        std::vector<double> g = d.image->frame(frames[k]);  // (the image caches its frames)
        if (cols.column(j) == 0) return g;
        return noise.replica(k, g, d.image->frame_time(frames[k]), (int)cols.column(j));
    });
    // rank 0: the columns of the composite frames in flight, the moments' device operands, the output
    struct Columns {
        std::vector<double> x;  // [nc][nvoxel]
        std::vector<int32_t> status, iterations;
        std::vector<uint8_t> use;  // [N]: replica r + 1 did not stop on a non-finite iterate
    };
    std::map<int64_t, Columns> open;
    InOrder<Columns> done;  // the completed frames, cut down to column 0: to /solution in frame order
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
    double moments_ms = 0.0;
    run.solve(0, nullptr, false, nullptr, [&](int64_t j, const double* xs, const SolveInfo& info) {
        const int64_t k = cols.frame(j), r = cols.column(j);
        auto it = open.find(k);
        if (it == open.end())
            it = open.emplace(k, Columns{std::vector<double>((size_t)nc * nvoxel), std::vector<int32_t>((size_t)nc),
                                         std::vector<int32_t>((size_t)nc), std::vector<uint8_t>((size_t)N)}).first;
        Columns& c = it->second;
        std::copy(xs, xs + nvoxel, c.x.begin() + (size_t)r * nvoxel);
        c.status[r] = info.status, c.iterations[r] = info.iterations;
        if (r > 0) c.use[r - 1] = info.nonfinite ? 0 : 1;
        if (info.nonfinite)
            std::cerr << "warning: frame " << frames[k] << ", replica " << r << ": non-finite iterate, stopped"
                      << std::endl;
        if (!cols.arrived(j)) return;
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
        c.x.resize((size_t)nvoxel);  // column 0 alone goes on to the solution writer
        done.put(k, std::move(c));
        open.erase(it);
        run.tick();
        done.drain([&](int64_t w, Columns&& c0) {
            const uint64_t cur = frames[w];
            d.writer->add(c0.x, c0.status[0], image.frame_time(cur), image.camera_frame_time(cur), c0.iterations[0]);
        });
    });
    if (d.rank == 0 && d.profile.is_open())
        write_uncertainty_line(d.profile, {cfg.replicas, cfg.noise_seed, cfg.noise_abs, cfg.noise_shot, cfg.noise_rel,
                                           noise.kernel_ms(), moments_ms, (uint64_t)T});
}

}  // namespace sart
