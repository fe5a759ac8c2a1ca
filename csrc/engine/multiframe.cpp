#include "multiframe.hpp"

#include <algorithm>
#include <exception>
#include <mutex>
#include <deque>
#include <condition_variable>
#include <chrono>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <thread>

#include "../kernels/launchers.hpp"

namespace sart {

namespace {
void hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}
}  // namespace

MfEnginePlan MultiFrameEngine::checked_plan(const void* A, int64_t nrows, int64_t nrows_pad, int64_t nvoxel, int64_t ld,
                                            Communicator* comm, const EngineConfig& cfg, const SparseRtm* sparse) {
    validate_params(cfg);
    if (cfg.rtm_bf16 && cfg.rtm_f16)
        throw std::invalid_argument("MultiFrameEngine: rtm_f16 and rtm_bf16 are exclusive (one storage format per shard)");
    if (cfg.rtm_f16 && !sparse && !cfg.row_scale)
        throw std::invalid_argument("MultiFrameEngine: an f16 shard needs its row scales (EngineConfig::row_scale)");
    if (sparse) {
        if (cfg.rtm_bf16 || cfg.rtm_f16) throw std::invalid_argument("MultiFrameEngine: a sparse shard holds fp32 values");
        if (!sparse->row_ptr || !sparse->col_ptr)
            throw std::invalid_argument("MultiFrameEngine: sparse shard needs its CSR and CSC arrays");
    } else if (!A) {
        throw std::invalid_argument("MultiFrameEngine: dense shard pointer required");
    }
    if (!comm) throw std::invalid_argument("MultiFrameEngine: communicator required");
    if (ld % 64 || ld < nvoxel || nrows_pad % 64 || nrows_pad < nrows)
        throw std::invalid_argument("MultiFrameEngine: ld and nrows_pad must be multiples of 64 covering the shard");
    const RtmStorage storage = cfg.rtm_f16 ? RtmStorage::f16s : (cfg.rtm_bf16 ? RtmStorage::bf16 : RtmStorage::f32);
    return mf_engine_plan(storage, sparse != nullptr, sparse ? sparse->nnz : 0, cfg.mf_frames, nrows, nrows_pad, ld,
                          comm->size(), cfg.mf_split_a, cfg.check_interval, MfEngineKnobs::from_env());
}

MultiFrameEngine::MultiFrameEngine(int device, const void* A, int64_t nrows, int64_t nrows_pad, int64_t nvoxel,
                                   int64_t ld, Communicator* comm, const EngineConfig& cfg, const SparseRtm* sparse)
    : device_(device), A_(A), P_(nrows), Pp_(nrows_pad), V_(nvoxel), ld_(ld), comm_(comm), cfg_(cfg),
      plan_(checked_plan(A, nrows, nrows_pad, nvoxel, ld, comm, cfg, sparse)) {
    const MfEnginePlan& p = plan_;
    const int NF = p.nf;
    if (sparse) sp_ = *sparse;
    if (cfg_.fault_nan_sweep < 0) cfg_.fault_nan_sweep = p.fault_nan;
    set_device();
    hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    hip_ok(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    hip_ok(hipStreamCreateWithFlags(&copy_stream_, hipStreamNonBlocking), "hipStreamCreate");
    hip_ok(hipHostMalloc(reinterpret_cast<void**>(&hsnap_), 2 * sizeof(Snap)), "hipHostMalloc");
    for (auto& e : ev_) hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    hip_ok(hipEventCreateWithFlags(&ev_copy_, hipEventDisableTiming), "hipEventCreate");
    hip_ok(hipEventCreateWithFlags(&ev_stage_, hipEventDisableTiming), "hipEventCreate");
    // device refill: the queue and the output ring, with their pinned host rows
    hip_ok(hipHostMalloc(reinterpret_cast<void**>(&hg64_), (size_t)p.qcap * Pp_ * sizeof(double)), "hipHostMalloc");
    std::memset(hg64_, 0, (size_t)p.qcap * Pp_ * sizeof(double));  // padding rows stay zero
    g64q_.resize((size_t)p.qcap * Pp_);
    sstats_.resize((size_t)2 * NF);
    hip_ok(hipHostMalloc(reinterpret_cast<void**>(&hx_), (size_t)p.rcap * ld_ * sizeof(float)), "hipHostMalloc");
    q_.resize(1);
    ghq_.resize((size_t)p.qcap * Pp_);
    ring_.resize((size_t)p.rcap * ld_);
    xlast_.resize(ld_);
    xlast2_.resize(ld_);
    if (cfg_.logarithmic) oq_.resize((size_t)p.qcap * ld_);
    X_.resize((size_t)NF * ld_);
    Xprev_.resize((size_t)NF * ld_);
    Fs_.resize((size_t)p.nsf * Pp_ * NF);
    W_.resize((size_t)Pp_ * NF);
    part_.resize((size_t)p.nsb * ld_ * NF);
    buf_.resize((size_t)NF * ld_ + NF);  // [nf][ld] correction + [nf] ||A x||^2: one all-reduce per sweep
    pen_.resize((size_t)NF * ld_);
    if (cfg_.logarithmic) O_.resize((size_t)NF * ld_);
    for (auto* b : {&ghat_, &arow_, &gpos_, &wo_}) b->resize((size_t)Pp_ * NF);
    G64_.resize(NF);
    F2part_.resize((size_t)p.nwb * NF);
    st_.resize(1);
    const float* A32 = static_cast<const float*>(A_);
    if (p.sparse) {
        Xt_.resize((size_t)ld_ * NF);
        if (p.needs_w_planes) Wt_.resize((size_t)Pp_ * NF);  // cold-start / log operands re-laid
    } else {
        // the forward's operands: X as two 16-bit planes, bf16 pieces or f16 pieces with each frame's scale
        auto x_planes = [&](bool f16_pieces) {
            for (auto* b : {&Xh_, &Xl_}) b->resize((size_t)NF * ld_);
            if (!f16_pieces) return;
            xinv_.resize(NF);
            xmax_.resize(NF);
        };
        switch (p.fwd) {
            case MfPath::fp32: break;
            case MfPath::b16:
            case MfPath::x3: x_planes(false); break;
            case MfPath::s16: x_planes(true); break;  // the rows' scales come with the shard (cfg_.row_scale)
            case MfPath::h16:                         // the rows' scales are computed here
                x_planes(true);
                rsc_.resize((size_t)2 * Pp_);
                launch_mf_row_scales(A32, ld_, Pp_, rsc_.get(), stream_);
                break;
        }
        // the back-projection's: W as bf16 planes, or as f16 pairs with each frame's scale
        auto w_f16_pairs = [&] {
            W16_.resize((size_t)2 * NF * Pp_);
            wmax_.resize(NF);
            wscale_.resize(NF);
        };
        switch (p.bwd) {
            case MfPath::fp32: break;
            case MfPath::b16:
            case MfPath::x3:
                Wh_.resize((size_t)(p.bwd == MfPath::x3 ? 2 : 1) * NF * Pp_);  // split-A: hi and mid planes
                Wl_.resize((size_t)NF * Pp_);
                break;
            case MfPath::s16:  // the rows' 1 / s_p goes into W before its split (Ws_); columns need no scales
                w_f16_pairs();
                Ws_.resize((size_t)Pp_ * NF);
                break;
            case MfPath::h16: {  // the columns' scales are computed here
                w_f16_pairs();
                csc_.resize((size_t)2 * ld_);
                DeviceArray<unsigned> cmax;
                cmax.resize(ld_);
                launch_mf_col_scales(A32, ld_, Pp_, cmax.get(), csc_.get(), stream_);
                hip_ok(hipStreamSynchronize(stream_), "column scales");
                break;
            }
        }
        x1_ = reinterpret_cast<uint16_t*>(Xh_.get());
        x2_ = reinterpret_cast<uint16_t*>(Xl_.get());
        w1_ = W16_.get();
        w2_ = W16_.get() + (size_t)NF * Pp_;
    }
    if (p.sparse)
        rs_.compute_sparse(sp_, P_, Pp_, V_, ld_, comm_, cfg_, stream_);
    else
        rs_.compute(A_, P_, Pp_, V_, ld_, comm_, cfg_, stream_, false, p.storage == RtmStorage::bf16,
                    p.storage == RtmStorage::f16s ? cfg_.row_scale + Pp_ : nullptr);
    if (comm_->size() > 1) comm_->prepare(p.collectives);
    if (p.chunks.size() > 2) {
        hip_ok(hipStreamCreateWithFlags(&comm_stream_, hipStreamNonBlocking), "hipStreamCreate");
        cev_.resize(p.chunks.size() - 1);
        for (auto& e : cev_) hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
        hip_ok(hipEventCreateWithFlags(&comm_done_, hipEventDisableTiming), "hipEventCreate");
    }
}

MultiFrameEngine::~MultiFrameEngine() {
    set_device();
    drop_graph();
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (comm_stream_) (void)hipStreamSynchronize(comm_stream_);
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : cev_)
        if (e) (void)hipEventDestroy(e);
    if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);
    if (comm_done_) (void)hipEventDestroy(comm_done_);
    if (comm_stream_) (void)hipStreamDestroy(comm_stream_);
    if (hsnap_) (void)hipHostFree(hsnap_);
    if (hg64_) (void)hipHostFree(hg64_);
    if (hx_) (void)hipHostFree(hx_);
    if (ev_copy_) (void)hipEventDestroy(ev_copy_);
    if (ev_stage_) (void)hipEventDestroy(ev_stage_);
    if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

void MultiFrameEngine::set_device() const { hip_ok(hipSetDevice(device_), "hipSetDevice"); }

void MultiFrameEngine::set_laplacian(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t nnz) {
    set_device();
    has_lap_ = false;
    // a weight per frame will come with the series (mf_frame_beta): kept whatever the scalar weight is
    if (nnz <= 0 || (cfg_.beta_laplace <= 0 && !cfg_.mf_frame_beta)) return;
    if (row_ptr[V_] != nnz) throw std::invalid_argument("Laplacian CSR row pointer does not match nnz");
    lap_rp_.resize(V_ + 1);
    lap_col_.resize(nnz);
    lap_val_.resize(nnz);
    hip_ok(hipMemcpy(lap_rp_.get(), row_ptr, (V_ + 1) * sizeof(int64_t), hipMemcpyHostToDevice), "H2D");
    hip_ok(hipMemcpy(lap_col_.get(), col, nnz * sizeof(int32_t), hipMemcpyHostToDevice), "H2D");
    hip_ok(hipMemcpy(lap_val_.get(), val, nnz * sizeof(float), hipMemcpyHostToDevice), "H2D");
    has_lap_ = true;
}

void MultiFrameEngine::forward() {
    const MfEnginePlan& p = plan_;
    const int NF = p.nf;
    if (p.sparse) {
        launch_mf_sparse_forward(sp_, P_, Pp_, X_.get(), ld_, Xt_.get(), Fs_.get(), NF, p.pw, stream_, g_mf_skip);
        return;
    }
    const float* A32 = static_cast<const float*>(A_);
    switch (p.fwd) {
        case MfPath::fp32: launch_mf_forward(p.fplan, A32, P_, X_.get(), Fs_.get(), stream_); break;
        case MfPath::b16:
            launch_mf_split_x(X_.get(), (int64_t)NF * ld_, Xh_.get(), Xl_.get(), stream_, false, p.xblk ? ld_ : 0);
            launch_mf_forward_b16(p.fplan, static_cast<const bf16_t*>(A_), P_, Xh_.get(), Xl_.get(), Fs_.get(), stream_,
                                  p.xblk);
            break;
        case MfPath::x3:
            launch_mf_split_x(X_.get(), (int64_t)NF * ld_, Xh_.get(), Xl_.get(), stream_, true, p.xblk ? ld_ : 0);
            launch_mf_forward_x3(p.fplan, A32, P_, Xh_.get(), Xl_.get(), Fs_.get(), stream_, p.xblk);
            break;
        case MfPath::h16:
            launch_mf_split_x16(X_.get(), ld_, NF, x1_, x2_, xmax_.get(), xinv_.get(), stream_, true, p.xblk);
            launch_mf_forward_h16(p.fplan, A32, P_, x1_, x2_, Fs_.get(), stream_, p.xblk, rsc_.get(), xinv_.get());
            break;
        case MfPath::s16:  // f16 pieces of X s_f in the bf16 planes' layout (no k permutation)
            launch_mf_split_x16(X_.get(), ld_, NF, x1_, x2_, xmax_.get(), xinv_.get(), stream_, false, p.xblk);
            launch_mf_forward_s16(p.fplan, static_cast<const f16s_t*>(A_), P_, x1_, x2_, Fs_.get(), stream_, p.xblk,
                                  cfg_.row_scale, xinv_.get());
            break;
    }
}

void MultiFrameEngine::backproject(const float* W, bool split_w, int64_t v0, int64_t v1, bool have_max, float* out,
                                   const float* oscale) {
    const MfEnginePlan& p = plan_;
    const int NF = p.nf;
    if (p.sparse) {
        // W_ comes from the weights kernel already in frame-order planes (sweep); the cold-start operands (gpos_,
        // wo_) are re-laid here
        if (p.needs_w_planes && W != W_.get()) {
            if (split_w) launch_mf_w_planes(W, Pp_, NF, p.pw, Wt_.get(), stream_, g_mf_skip);
            W = Wt_.get();
        }
        launch_mf_sparse_backproject(sp_, V_, W, Pp_, out ? out : part_.get(), out ? oscale : nullptr, NF, p.pw, v0,
                                     v1, stream_, g_mf_skip);
        return;
    }
    const float* A32 = static_cast<const float*>(A_);
    switch (p.bwd) {
        case MfPath::fp32: launch_mf_backproject(p.bplan, A32, W, part_.get(), stream_, v0, v1); break;
        case MfPath::b16:
            if (split_w) launch_mf_split_w(W, Pp_, NF, Pp_, Wh_.get(), Wl_.get(), stream_, false);
            launch_mf_backproject_b16(p.bplan, static_cast<const bf16_t*>(A_), Wh_.get(), Wl_.get(), Pp_, part_.get(),
                                      stream_, v0, v1);
            break;
        case MfPath::x3:
            if (split_w) launch_mf_split_w(W, Pp_, NF, Pp_, Wh_.get(), Wl_.get(), stream_, true);
            launch_mf_backproject_x3(p.bplan, A32, Wh_.get(), Wl_.get(), Pp_, part_.get(), stream_, v0, v1);
            break;
        case MfPath::h16:
            if (split_w)
                launch_mf_split_w16(W, Pp_, NF, Pp_, w1_, w2_, wmax_.get(), 1.f, wscale_.get(), stream_, have_max);
            launch_mf_backproject_h16(p.bplan, A32, w1_, w2_, Pp_, part_.get(), stream_, v0, v1, csc_.get(),
                                      wscale_.get());
            break;
        case MfPath::s16:  // the kernel multiplies by A s_p: the rows' 1 / s_p goes into W before its per-frame f16 split
            if (split_w) {
                launch_mf_scale_w_rows(W, cfg_.row_scale + Pp_, Pp_, NF, Ws_.get(), stream_);
                launch_mf_split_w16(Ws_.get(), Pp_, NF, Pp_, w1_, w2_, wmax_.get(), 1.f, wscale_.get(), stream_, false);
            }
            launch_mf_backproject_s16(p.bplan, static_cast<const f16s_t*>(A_), w1_, w2_, Pp_, part_.get(), stream_, v0,
                                      v1, wscale_.get());
            break;
    }
}

void MultiFrameEngine::sweep() {
    const MfEnginePlan& p = plan_;
    const int NF = p.nf;
    MfState* st = st_.get();
    MfQueue* q = q_.get();
    const MfSkipScope skip(&st->all_done);  // every slot done: the sweep's heavy kernels return at once
    // the back-projection (and its operand split) also returns when every running frame is decided at max_iter in
    // this sweep (mf_plan's skip_bwd): its corrections would be discarded; the collect still sums ||A x||^2
    const int* bskip = p.skip_last_bwd ? &q->skip_bwd : &st->all_done;
    float* D = buf_.get();                     // [ld][nf] voxel-major corrections
    float* F2 = buf_.get() + (int64_t)NF * ld_;  // [nf] ||A x||^2, all-reduced with the last chunk
    const float* scale = cfg_.logarithmic ? rs_.dmask.get() : rs_.dscale.get();
    forward();
    // f16-pair back-projection: the weights kernel also leaves each frame's max |w| (its f16 scale) in wmax_
    launch_mf_weights(Fs_.get(), p.nsf, Pp_, ghat_.get(), arow_.get(), cfg_.logarithmic, W_.get(), F2part_.get(),
                      NF, stream_, !p.sparse && p.bwd == MfPath::h16 ? wmax_.get() : nullptr,
                      p.needs_w_planes ? p.pw : 0);
    // D[v0, v1) = scale * A^T W and, with the last chunk, the per-frame ||A x||^2: a sparse shard's SpMM writes the
    // scaled sums itself (the collect then only sums F2part)
    auto bwd_collect = [&](int64_t v0, int64_t v1, bool first, bool lastc) {
        if (p.sparse) {
            {
                const MfSkipScope sb(bskip);
                backproject(W_.get(), first, v0, v1, true, D, scale);
            }
            if (lastc) launch_mf_collect(part_.get(), p.nsb, ld_, 0, 0, scale, D, F2part_.get(), p.nwb, F2, NF, stream_);
            return;
        }
        {
            const MfSkipScope sb(bskip);
            backproject(W_.get(), first, v0, v1, true);
        }
        launch_mf_collect(part_.get(), p.nsb, ld_, v0, v1, scale, D, lastc ? F2part_.get() : nullptr, p.nwb,
                          lastc ? F2 : nullptr, NF, stream_);
    };
    const int nc = (int)p.chunks.size() - 1;
    if (comm_->size() > 1 && nc > 1) {
        // Overlap: the back-projection runs chunk by chunk over the voxel axis on the compute
        // stream; the all-reduce of chunk c (a contiguous [v0, v1) x nf slice of the voxel-major corrections)
        // runs on the comm stream as soon as its collect has finished, next to the back-projection of the later
        // chunks. All compute chunks are queued first so that a host-staged all-reduce, which blocks this thread,
        // still overlaps with them.
        for (int c = 0; c < nc; ++c) {
            const int64_t v0 = p.chunks[c], v1 = p.chunks[c + 1];
            const bool last = c == nc - 1;
            bwd_collect(v0, v1, c == 0, last);
            hip_ok(hipEventRecord(cev_[c], stream_), "event");
        }
        for (int c = 0; c < nc; ++c) {
            const int64_t v0 = p.chunks[c], v1 = p.chunks[c + 1];
            hip_ok(hipStreamWaitEvent(comm_stream_, cev_[c], 0), "wait chunk");
            const size_t n = (size_t)(v1 - v0) * NF + (c == nc - 1 ? (size_t)NF : 0);
            comm_->all_reduce(D + v0 * NF, n, ReduceOp::kSum, comm_stream_);
        }
        hip_ok(hipEventRecord(comm_done_, comm_stream_), "event");
    } else {
        bwd_collect(0, ld_, true, true);
        if (comm_->size() > 1) comm_->all_reduce(buf_.get(), (size_t)NF * ld_ + NF, ReduceOp::kSum, stream_);
    }
    const float* pen = nullptr;
    if (has_lap_) {  // needs X only: runs while the last chunks are being reduced
        launch_mf_penalty(lap_rp_.get(), lap_col_.get(), lap_val_.get(), V_, (float)cfg_.beta_laplace,
                          cfg_.logarithmic, X_.get(), ld_, pen_.get(), st, NF, stream_, beta_dev_, q);
        pen = pen_.get();
    }
    if (comm_->size() > 1 && nc > 1) hip_ok(hipStreamWaitEvent(stream_, comm_done_, 0), "wait all-reduce");
    decide_update_admit(pen);
    if (cfg_.fault_nan_sweep >= 0 && host_sweep_ == cfg_.fault_nan_sweep)  // fault injection (tests): slot 0
        hip_ok(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(X_.get()), 0x7fc00000, 1, stream_), "inject NaN");
    ++host_sweep_;
}

void MultiFrameEngine::drop_graph() {
    if (graph_) (void)hipGraphExecDestroy(graph_);
    graph_ = nullptr;
}

void MultiFrameEngine::run_chunk() {
    RoctxRange r("sart::mf_chunk");
    // capture only after an eager chunk with the current kernels (launchers may set function attributes on first
    // use, which must not happen inside a capture); the captured update kernel holds rf_ by value
    const int chunk = plan_.chunk;
    const bool graphable = plan_.use_graph && !graph_failed_ && warm_chunk_ && comm_->size() == 1 &&
                           comm_->graph_capturable() && cfg_.fault_nan_sweep < 0;
    if (graph_ && (!graphable || std::memcmp(&graph_rf_, &rf_, sizeof(rf_)) != 0 || graph_beta_ != beta_dev_))
        drop_graph();
    if (graphable && !graph_) {
        hipGraph_t g = nullptr;
        bool ok = hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            try {
                for (int i = 0; i < chunk; ++i) sweep();
            } catch (...) {
                ok = false;
            }
            ok = (hipStreamEndCapture(stream_, &g) == hipSuccess) && ok && g;
        }
        if (ok) ok = hipGraphInstantiate(&graph_, g, nullptr, nullptr, 0) == hipSuccess;
        if (g) (void)hipGraphDestroy(g);
        if (!ok) {  // eager launches from now on (the capture queued nothing)
            (void)hipGetLastError();
            graph_ = nullptr;
            graph_failed_ = true;
        } else {
            graph_rf_ = rf_;
            graph_beta_ = beta_dev_;
        }
    }
    if (graphable && graph_) {
        hip_ok(hipGraphLaunch(graph_, stream_), "hipGraphLaunch");
        host_sweep_ += chunk;
    } else {
        for (int i = 0; i < chunk; ++i) sweep();
        warm_chunk_ = true;
    }
}

void MultiFrameEngine::decide_update_admit(const float* pen) {
    const int NF = plan_.nf;
    float* D = buf_.get();              // [ld][nf] voxel-major corrections
    float* F2 = D + (int64_t)NF * ld_;  // [nf] ||A x||^2
    launch_mf_decide(st_.get(), F2, stream_, q_.get());
    launch_mf_update(X_.get(), D, O_.get(), pen, (float)cfg_.relaxation, cfg_.logarithmic, V_, ld_, st_.get(), NF,
                     stream_, Xprev_.get(), q_.get(), &rf_);
    launch_mf_admit_rows(q_.get(), ghq_.get(), P_, Pp_, rs_.ray_len.get(), (float)cfg_.ray_length_threshold,
                         ghat_.get(), arow_.get(), NF, stream_);
}

void MultiFrameEngine::stage(int64_t first, int64_t e0, int k, const FrameSource& src, bool cold) {
    const int NF = plan_.nf, qcap = plan_.qcap, nsb = plan_.nsb;
    if (k <= 0) return;
    if (k > NF) throw std::logic_error("MultiFrameEngine::stage: at most nf frames per call");
    RoctxRange r("sart::mf_stage");
    // the frames' raw pixels straight into the pinned queue rows, then to the device on the copy stream (one or two
    // runs of ring positions), next to the sweeps; normalisation and scalars on the device (k_mf_stage_*)
    const auto ts = std::chrono::steady_clock::now();
    for (int j = 0; j < k; ++j) src(first + e0 + j, hg64_ + (size_t)((e0 + j) % qcap) * Pp_);
    stats_.host_src_ms += ms_since(ts);
    for (int j = 0; j < k;) {
        const int pos = (int)((e0 + j) % qcap);
        const int run = std::min(k - j, qcap - pos);
        if (P_)
            hip_ok(hipMemcpyAsync(g64q_.get() + (size_t)pos * Pp_, hg64_ + (size_t)pos * Pp_,
                                  (size_t)run * Pp_ * sizeof(double), hipMemcpyHostToDevice, copy_stream_),
                   "H2D queue");
        j += run;
    }
    hip_ok(hipEventRecord(ev_stage_, copy_stream_), "event");
    hip_ok(hipStreamWaitEvent(stream_, ev_stage_, 0), "wait staging");
    // per-frame maxima and positive sums of squares over all ranks' pixels (reference sartsolver_cuda.cpp:146-157)
    launch_mf_stage_stats(g64q_.get(), e0, qcap, k, P_, Pp_, sstats_.get(), NF, stream_);
    if (comm_->size() > 1) {
        comm_->all_reduce(sstats_.get(), (size_t)k, ReduceOp::kMax, stream_);
        comm_->all_reduce(sstats_.get() + NF, (size_t)k, ReduceOp::kSum, stream_);
    }
    launch_mf_stage_norm(q_.get(), g64q_.get(), ghq_.get(), sstats_.get(), e0, first + e0, cold, k, P_, Pp_, NF, stream_);
    if (cold || cfg_.logarithmic) {
        // one batched back-projection of the k staged frames (columns 0 .. k - 1): cold starts
        // x0 = max([rho > tau] A^T max(ghat, 0) / rho, 1e-7) (reference sart_kernels.cu:22-60) and / or the
        // frame-constant observed back-projection O = mask A^T (a ghat) of log mode
        const float thr = (float)cfg_.ray_length_threshold;
        launch_mf_stage_ops(ghq_.get(), e0, qcap, k, P_, Pp_, rs_.ray_len.get(), thr, gpos_.get(),
                            cfg_.logarithmic ? wo_.get() : nullptr, NF, stream_);
        if (cold) {
            backproject(gpos_.get(), true, 0, ld_);
            launch_mf_collect(part_.get(), nsb, ld_, 0, ld_, nullptr, buf_.get(), nullptr, 0, nullptr, NF, stream_);
            if (comm_->size() > 1) comm_->all_reduce(buf_.get(), (size_t)NF * ld_, ReduceOp::kSum, stream_);
            launch_mf_stage_cols(buf_.get(), rs_.dinv.get(), e0, qcap, k, V_, ld_, NF, x0q_.get(), stream_);
        }
        if (cfg_.logarithmic) {
            backproject(wo_.get(), true, 0, ld_);
            launch_mf_collect(part_.get(), nsb, ld_, 0, ld_, rs_.dmask.get(), buf_.get(), nullptr, 0, nullptr, NF,
                              stream_);
            if (comm_->size() > 1) comm_->all_reduce(buf_.get(), (size_t)NF * ld_, ReduceOp::kSum, stream_);
            launch_mf_stage_cols(buf_.get(), nullptr, e0, qcap, k, V_, ld_, NF, oq_.get(), stream_);
        }
    }
    launch_mf_publish(q_.get(), e0 + k, stream_);
}

std::vector<SolveInfo> MultiFrameEngine::solve_batch(const double* g, int nframes, double* x_out, const double* x0,
                                                     bool chain, double* starts, const float* frame_beta) {
    std::vector<SolveInfo> out(std::max(nframes, 0));
    if (nframes <= 0) return out;
    const auto t0 = std::chrono::steady_clock::now();
    if (starts) {  // the start value of every frame (normalised on the device; de-normalised below)
        set_device();
        starts_.resize((size_t)nframes * ld_);
        rf_.starts = starts_.get();
    }
    try {
        solve_series(
            nframes, [&](int64_t k, double* dst) { std::memcpy(dst, g + k * P_, (size_t)P_ * sizeof(double)); },
            [&](int64_t k, const double* x, const SolveInfo& info) {
                std::memcpy(x_out + k * V_, x, (size_t)V_ * sizeof(double));
                out[k] = info;
            },
            x0, chain, frame_beta);
    } catch (...) {
        rf_.starts = nullptr;
        throw;
    }
    if (starts) {
        rf_.starts = nullptr;
        std::vector<float> h((size_t)nframes * ld_);
        hip_ok(hipMemcpy(h.data(), starts_.get(), h.size() * sizeof(float), hipMemcpyDeviceToHost), "D2H starts");
        for (int k = 0; k < nframes; ++k)
            for (int64_t v = 0; v < V_; ++v)
                starts[(size_t)k * V_ + v] = (double)h[(size_t)k * ld_ + v] * frame_norm_[k];
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (auto& info : out) info.ms = ms / nframes;
    return out;
}

void MultiFrameEngine::solve_series(int64_t nframes, const FrameSource& src, const FrameSink& sink, const double* x0,
                                    bool chain, const float* frame_beta) {
    set_device();
    RoctxRange range("sart::mf_series");
    stats_ = SeriesStats{};
    if (frame_beta && chain)
        throw std::invalid_argument("MultiFrameEngine: a weight per frame needs cold or x0 starts (chain would start a "
                                    "frame from a neighbour solved at another weight)");
    if (frame_beta && !has_lap_)
        throw std::invalid_argument("MultiFrameEngine: a weight per frame needs the Laplacian "
                                    "(EngineConfig::mf_frame_beta before set_laplacian)");
    beta_dev_ = nullptr;
    if (nframes <= 0) return;
    if (nframes > std::numeric_limits<int32_t>::max()) throw std::invalid_argument("solve_series: too many frames");
    if (frame_beta) {
        // once per series, indexed by the series' frame (MfQueue::slot_frame) through refills, graph replays and a
        // restarted pass alike; the previous series has been synchronised, so the table can be replaced
        for (int64_t k = 0; k < nframes; ++k)
            if (!(frame_beta[k] >= 0.f) || !std::isfinite(frame_beta[k]))
                throw std::invalid_argument("MultiFrameEngine: frame weights must be finite and >= 0");
        if ((int64_t)beta_tab_.size() < nframes) beta_tab_.resize((size_t)nframes);
        hip_ok(hipMemcpy(beta_tab_.get(), frame_beta, (size_t)nframes * sizeof(float), hipMemcpyHostToDevice),
               "H2D frame weights");
        beta_dev_ = beta_tab_.get();
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<char> delivered((size_t)nframes, 0);
    frame_norm_.assign((size_t)nframes, 1.0);
    std::vector<double> newest;  // the newest delivered finite solution (a re-solve's chain start)
    int64_t newest_frame = -1;
    int64_t first = 0;
    for (int attempt = 0;; ++attempt) {
        const bool failed = series_once(first, nframes, src, sink, attempt == 0 ? x0 : (newest_frame >= 0 && chain ? newest.data() : x0),
                                        chain, delivered, attempt, newest, newest_frame);
        if (!failed) break;
        const bool had = comm_->degrade();
        if (comm_->rank() == 0)
            std::fprintf(stderr, "sart: device all-reduce timed out; re-solving the undelivered frames on %s\n",
                         comm_->backend());
        if (!had || attempt >= 1) throw std::runtime_error("MultiFrameEngine: device all-reduce failed");
        ++stats_.restarts;
        while (first < nframes && delivered[first]) ++first;
    }
    comm_->check();
    stats_.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

bool MultiFrameEngine::series_once(int64_t first, int64_t nframes, const FrameSource& src, const FrameSink& sink,
                                   const double* x0, bool chain, std::vector<char>& delivered, int attempt,
                                   std::vector<double>& newest, int64_t& newest_frame) {
    const MfEnginePlan& p = plan_;
    const int NF = p.nf, qcap = p.qcap, rcap = p.rcap;
    const int64_t n = nframes - first;  // frames of this pass: queue entry e = frame first + e
    host_sweep_ = 0;
    // cold starts are staged for every frame without --chain, and for the first nf frames of a chain without x0
    // (later ones start from a frame in flight)
    const bool any_cold = !(chain && x0);
    if (any_cold && x0q_.size() == 0) x0q_.resize((size_t)qcap * ld_);
    if ((int64_t)x064_.size() < V_) x064_.resize(std::max<int64_t>(V_, 1));
    rf_.ring = ring_.get();
    rf_.xlast = xlast_.get();
    rf_.xlast2 = xlast2_.get();
    rf_.x0 = x064_.get();
    rf_.x0q = x0q_.size() ? x0q_.get() : nullptr;
    rf_.oq = oq_.size() ? oq_.get() : nullptr;
    // every slot starts empty (done) with finite zero columns
    for (auto* b : {&X_, &Xprev_, &ghat_, &arow_})
        hip_ok(hipMemsetAsync(b->get(), 0, b->size() * sizeof(float), stream_), "memset");
    if (cfg_.logarithmic) hip_ok(hipMemsetAsync(O_.get(), 0, O_.size() * sizeof(float), stream_), "memset");
    hip_ok(hipMemsetAsync(G64_.get(), 0, G64_.size() * sizeof(double), stream_), "memset");
    launch_mf_state_begin(st_.get(), G64_.get(), 0, cfg_.conv_tolerance, cfg_.max_iterations, NF, stream_);
    const int64_t x0_below = x0 ? (chain ? std::numeric_limits<int64_t>::max() : first + NF) : 0;
    // the plan's chain policy as this series runs it: the queue and the stats hold the same values
    stats_.chunk = p.chunk;
    stats_.admit_cap = chain ? p.admit_cap : 0;
    stats_.src_age = p.src_age;
    stats_.src_finished = p.src_finished;
    stats_.src_extrap = p.src_extrap;
    stats_.drift = chain ? p.drift : 0.0;
    stats_.stage_window = p.stage_window;
    stats_.lead = chain && !x0 && p.lead;
    launch_mf_queue_begin(q_.get(), qcap, rcap, chain, stats_.admit_cap, stats_.src_age, x0_below, stats_.src_finished,
                          stats_.lead, (float)stats_.src_extrap, stream_, (float)stats_.drift);
    if (x0 && V_) hip_ok(hipMemcpyAsync(x064_.get(), x0, V_ * sizeof(double), hipMemcpyHostToDevice, stream_), "H2D x0");

    int64_t staged = 0;
    int64_t window_fin = 0;  // frames finished in the latest snapshot (the staging window's base)
    // stage while the queue has room for a unit (nf with a back-projection), up to `limit` frames
    auto stage_upto = [&](int64_t head, int64_t limit) {
        if (p.stage_window > 0) limit = std::min(limit, window_fin + p.stage_window);
        while (staged < std::min(n, limit)) {
            // the first nf frames start from x0 (or cold without it); later ones cold (!chain) or chained
            const bool cold = chain ? (!x0 && staged < NF) : (!x0 || staged >= NF);
            const int64_t lim = staged < NF ? NF - staged : NF;  // no unit straddles frame nf
            const int64_t room = qcap - (staged - head);
            const int64_t unit = (cold || cfg_.logarithmic) ? std::min<int64_t>(lim, n - staged)
                                                            : std::max<int64_t>(1, std::min<int64_t>(NF / 4, n - staged));
            if (room < unit) return;
            const int k = (int)std::min<int64_t>({room, lim, std::min(n, limit) - staged});
            const auto ts = std::chrono::steady_clock::now();
            stage(first, staged, k, src, cold);
            stats_.host_stage_ms += ms_since(ts);
            staged += k;
        }
    };
    stage_upto(0, NF);  // the first nf frames: the first chunk starts as soon as they are read; the rest next to it
    decide_update_admit(nullptr);  // every slot done: the plan, start values and pixel columns only

    int issued = 0, checked = 0;
    auto issue = [&]() {
        run_chunk();
        const int slot = issued & 1;
        hip_ok(hipMemcpyAsync(&hsnap_[slot].st, st_.get(), sizeof(MfState), hipMemcpyDeviceToHost, stream_), "D2H state");
        hip_ok(hipMemcpyAsync(&hsnap_[slot].q, q_.get(), sizeof(MfQueue), hipMemcpyDeviceToHost, stream_), "D2H queue");
        hip_ok(hipEventRecord(ev_[slot], stream_), "event");
        ++issued;
    };
    struct Pending {
        MfFinish log;
        int pos;
    };
    // Delivery thread: finished frames are de-normalised and handed to the sink (the driver's writer) next to the
    // series thread, which only issues chunks, stages frames and queues the output-ring copies (at ~2000 sparse
    // frames/s the sink alone took a third of the series thread's time, profiles/series_r6_sparse*).
    struct Batch {
        hipEvent_t ev;  // the batch's copies into hx_
        std::vector<Pending> items;
    };
    std::mutex dm;
    std::condition_variable dcv;
    std::deque<Batch> dq;
    bool dstop = false;
    std::exception_ptr derr;
    int64_t dcount = 0, warm_age = 0;  // entries delivered (FIFO: entries [0, dcount) are done with hx_)
    std::thread deliver([&] {
        try {
            hip_ok(hipSetDevice(device_), "hipSetDevice");
            std::vector<double> x(std::max<int64_t>(V_, 1));
            for (;;) {
                Batch b;
                {
                    std::unique_lock<std::mutex> lk(dm);
                    dcv.wait(lk, [&] { return dstop || !dq.empty(); });
                    if (dq.empty()) return;
                    b = std::move(dq.front());
                    dq.pop_front();
                }
                const auto tw = std::chrono::steady_clock::now();
                const hipError_t se = hipEventSynchronize(b.ev);
                (void)hipEventDestroy(b.ev);
                hip_ok(se, "mf copy");
                for (const Pending& pd : b.items) {
                    const MfFinish& L = pd.log;
                    const float* hs = hx_ + (size_t)pd.pos * ld_;
                    for (int64_t v = 0; v < V_; ++v) x[v] = (double)hs[v] * L.norm;
                    stats_.busy_slot_sweeps += L.iters + 1;
                    stats_.mean_iterations += L.iters;
                    if (L.warm_from >= 0) ++stats_.chained, warm_age += (L.frame - L.warm_from);
                    if (L.frame < 0 || L.frame >= nframes || delivered[L.frame]) continue;
                    SolveInfo info;
                    info.status = L.status;
                    info.iterations = L.iters;
                    info.convergence = L.conv;
                    info.nonfinite = (L.flags & 1) != 0;
                    info.used_fused = false;
                    info.warm_from = L.warm_from;
                    info.warm_iter = L.warm_iter;
                    info.warm_live = L.warm_live != 0;
                    info.comm_fallbacks = attempt;
                    info.comm = comm_->backend();
                    info.sweeps = L.iters + 1;
                    frame_norm_[L.frame] = L.norm;
                    delivered[L.frame] = 1;
                    sink(L.frame, x.data(), info);
                    if (L.frame > newest_frame && !info.nonfinite) {
                        newest.assign(x.begin(), x.begin() + V_);
                        newest_frame = L.frame;
                    }
                }
                stats_.host_deliver_ms += ms_since(tw);
                std::lock_guard<std::mutex> lk(dm);
                dcount += (int64_t)b.items.size();
                dcv.notify_all();
            }
        } catch (...) {
            std::lock_guard<std::mutex> lk(dm);
            derr = std::current_exception();
            dcv.notify_all();
        }
    });
    struct JoinDelivery {  // also on an exception of the series thread (a source that throws, a HIP error)
        std::thread& t;
        std::mutex& m;
        std::condition_variable& cv;
        bool& stop;
        std::deque<Batch>& q;
        ~JoinDelivery() {
            {
                std::lock_guard<std::mutex> lk(m);
                stop = true;
            }
            cv.notify_all();
            if (t.joinable()) t.join();
            for (Batch& b : q) (void)hipEventDestroy(b.ev);
        }
    } join_delivery{deliver, dm, dcv, dstop, dq};
    auto check_delivery = [&]() {
        std::lock_guard<std::mutex> lk(dm);
        if (derr) std::rethrow_exception(derr);
    };
    issue();
    stage_upto(0, n);
    issue();
    bool failed = false;
    int64_t seen_fin = 0;
    while (seen_fin < n) {
        check_delivery();
        if (checked >= issued) throw std::runtime_error("MultiFrameEngine: no chunk in flight and frames unfinished");
        const int c = checked++;
        const auto tw = std::chrono::steady_clock::now();
        hip_ok(hipEventSynchronize(ev_[c & 1]), "mf chunk");
        stats_.host_wait_ms += ms_since(tw);
        const MfQueue& Q = hsnap_[c & 1].q;
        const int64_t fin = Q.fin, head = Q.q_head;
        std::vector<Pending> fresh;
        for (int64_t e = seen_fin; e < fin; ++e) {
            const int pos = (int)(e % rcap);
            fresh.push_back({Q.log[pos], pos});
        }
        if (device_comm_failed_anywhere(comm_)) {  // collective: every rank sees the same device state
            failed = true;
            break;
        }
        if (!fresh.empty()) {
            {  // hx_ position of entry e is free once entry e - rcap has been delivered
                const auto tw2 = std::chrono::steady_clock::now();
                std::unique_lock<std::mutex> lk(dm);
                dcv.wait(lk, [&] { return derr || fin - 1 - rcap < dcount; });
                if (derr) std::rethrow_exception(derr);
                stats_.host_wait_ms += ms_since(tw2);
            }
            // solutions from the output ring on the copy stream (the chunk that wrote them has completed: its
            // snapshot was read), next to the sweeps; the ring positions are free again once the copies are done
            for (const Pending& pd : fresh)
                hip_ok(hipMemcpyAsync(hx_ + (size_t)pd.pos * ld_, ring_.get() + (size_t)pd.pos * ld_,
                                      V_ * sizeof(float), hipMemcpyDeviceToHost, copy_stream_),
                       "D2H x");
            seen_fin = fin;
            Batch b;
            hip_ok(hipEventCreateWithFlags(&b.ev, hipEventDisableTiming), "hipEventCreate");
            hip_ok(hipEventRecord(b.ev, copy_stream_), "event");
            hip_ok(hipStreamWaitEvent(stream_, b.ev, 0), "wait ring copies");
            launch_mf_drained(q_.get(), seen_fin, stream_);
            b.items = std::move(fresh);
            std::lock_guard<std::mutex> lk(dm);
            dq.push_back(std::move(b));
            dcv.notify_all();
        }
        window_fin = fin;
        stage_upto(head, n);
        if (fin < n) issue();  // frames left to finish on the device (a chunk still in flight may finish them)
    }
    {  // every handed-over frame delivered (or the delivery failed)
        std::unique_lock<std::mutex> lk(dm);
        dcv.wait(lk, [&] { return derr || dcount >= seen_fin; });
    }
    check_delivery();
    hip_ok(hipStreamSynchronize(stream_), "mf series");
    if (comm_stream_) hip_ok(hipStreamSynchronize(comm_stream_), "mf comm");
    hip_ok(hipStreamSynchronize(copy_stream_), "mf copy stream");
    if (!failed) {
        const MfState& S = hsnap_[(issued - 1) & 1].st;
        const int64_t finished = dcount;
        stats_.sweeps = S.sweep;
        stats_.queued_sweeps = (int64_t)issued * p.chunk;
        stats_.frames = finished;
        if (finished) stats_.mean_iterations /= finished;
        if (stats_.chained) stats_.mean_warm_age = (double)warm_age / stats_.chained;
        if (stats_.sweeps > 0) stats_.slot_util = (double)stats_.busy_slot_sweeps / ((double)stats_.sweeps * NF);
    }
    return failed;
}

}  // namespace sart
