#include "engine64.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>

#include "../kernels/launchers.hpp"

namespace sart {

namespace {
constexpr int kEpiLinear = 1, kEpiLog = 2;
}

Engine64::Engine64(int device, const void* A, int64_t nrows, int64_t nrows_pad, int64_t nvoxel, int64_t ld,
                   Communicator* comm, const EngineConfig& cfg, bool gpu_semantics, const SparseRtm* sparse)
    : device_(device), A_(static_cast<const float*>(A)), P_(nrows), Pp_(nrows_pad), V_(nvoxel), ld_(ld), comm_(comm),
      cfg_(cfg), gpu_(gpu_semantics) {
    validate_params(cfg_);
    if (!comm_) throw std::invalid_argument("Engine64: communicator required");
    if (cfg_.rtm_bf16) throw std::invalid_argument("Engine64: the fp64 solver reads fp32 shards, not bf16 storage (rtm_bf16)");
    if (cfg_.rtm_f16)
        throw std::invalid_argument("Engine64: the fp64 solver reads fp32 shards, not row-scaled f16 storage (rtm_f16)");
    if (sparse) throw std::invalid_argument("Engine64: the fp64 solver reads dense shards, not sparse ones");
    if (cfg_.column_shard)
        throw std::invalid_argument("Engine64: the fp64 solver takes pixel-row shards, not column (voxel) shards");
    if (!A_) throw std::invalid_argument("Engine64: dense shard pointer required");
    if (P_ < 0 || V_ < 1 || ld_ % 64 || ld_ < V_ || Pp_ % 64 || Pp_ < P_)
        throw std::invalid_argument("Engine64: ld and nrows_pad must be multiples of 64 covering the shard");
    cfg_.check_interval = std::max(1, cfg_.check_interval);
    if (gpu_) eps_ = clamp_ = 1e-7;
    else clamp_ = cfg_.logarithmic ? 1e-100 : -1.0;
    set_device();
    hip_call(hipDeviceSynchronize(), "hipDeviceSynchronize");  // the shard may have been filled on another stream
    hip_call(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    for (auto& e : ev_) hip_call(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    hip_call(hipHostMalloc(reinterpret_cast<void**>(&hstate_), 2 * sizeof(SartState)), "hipHostMalloc");
    hip_call(hipHostMalloc(reinterpret_cast<void**>(&hrows_), 4 * Pp_ * sizeof(double)), "hipHostMalloc");
    hip_call(hipHostMalloc(reinterpret_cast<void**>(&hx_), ld_ * sizeof(double)), "hipHostMalloc");
    std::memset(hrows_, 0, 4 * Pp_ * sizeof(double));
    hipDeviceProp_t prop;
    hip_call(hipGetDeviceProperties(&prop, device_), "hipGetDeviceProperties");
    num_cus_ = prop.multiProcessorCount;
    nsplit_ = backproject_num_splits(ld_, P_, 4);
    nF_ = forward_num_blocks(Pp_);
    rows_.resize(4 * Pp_);
    w_.resize(Pp_);
    x_.resize(ld_);
    x0_.resize(ld_);
    red_.resize(ld_ + 1);
    O_.resize(ld_);
    partial_.resize((size_t)nsplit_ * ld_);
    Fpart_.resize(nF_);
    st_.resize(1);
    // ray sums on the device in fp64, the global density all-reduced (reference sartsolver.cpp:38-56)
    rs_.compute(A_, P_, Pp_, V_, ld_, comm_, cfg_, stream_);
    init_scales();
}

Engine64::~Engine64() {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
    if (hstate_) (void)hipHostFree(hstate_);
    if (hrows_) (void)hipHostFree(hrows_);
    if (hx_) (void)hipHostFree(hx_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

void Engine64::set_device() const { hip_call(hipSetDevice(device_), "hipSetDevice"); }

std::vector<double> Engine64::ray_density() const {
    set_device();
    return rs_.density(V_);
}

std::vector<double> Engine64::ray_length() const {
    set_device();
    return rs_.length(P_);
}

void Engine64::init_scales() {
    // CpuSolver::init_scales on the device's fp64 sums
    const std::vector<double> rho = rs_.density(V_), ell = rs_.length(P_);
    std::vector<int32_t> valid(V_);
    std::vector<double> rho_s(V_);
    inv_len_.assign(P_, 0.0);
    for (int64_t v = 0; v < V_; ++v) {
        if (gpu_) {  // fp32 thresholds on fp32-rounded sums, as the fp32 kernels compare
            const float r32 = (float)rho[v];
            valid[v] = r32 > (float)cfg_.ray_density_threshold;
            rho_s[v] = valid[v] ? (double)r32 : 1.0;
        } else {
            valid[v] = rho[v] > cfg_.ray_density_threshold;
            rho_s[v] = valid[v] ? rho[v] : 1.0;
        }
    }
    for (int64_t q = 0; q < P_; ++q) {
        if (gpu_) {
            const float l32 = (float)ell[q];
            inv_len_[q] = l32 > (float)cfg_.ray_length_threshold ? (double)(1.0f / (l32 > 0 ? l32 : 1.0f)) : 0.0;
        } else {
            inv_len_[q] = ell[q] > cfg_.ray_length_threshold ? 1.0 / (ell[q] != 0 ? ell[q] : 1.0) : 0.0;
        }
    }
    dvalid_.resize(ld_);
    rho_s_.resize(ld_);
    hip_call(hipMemcpy(dvalid_.get(), valid.data(), V_ * sizeof(int32_t), hipMemcpyHostToDevice), "H2D valid");
    hip_call(hipMemcpy(rho_s_.get(), rho_s.data(), V_ * sizeof(double), hipMemcpyHostToDevice), "H2D rho");
}

void Engine64::set_laplacian(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t nnz) {
    set_device();
    has_lap_ = false;
    if (nnz <= 0 || cfg_.beta_laplace <= 0) return;
    if (row_ptr[V_] != nnz) throw std::invalid_argument("Laplacian CSR row pointer does not match nnz");
    lap_rp_.resize(V_ + 1);
    lap_col_.resize(nnz);
    lap_val_.resize(nnz);
    pen_.resize(ld_);
    hip_call(hipMemcpy(lap_rp_.get(), row_ptr, (V_ + 1) * sizeof(int64_t), hipMemcpyHostToDevice), "H2D");
    hip_call(hipMemcpy(lap_col_.get(), col, nnz * sizeof(int32_t), hipMemcpyHostToDevice), "H2D");
    hip_call(hipMemcpy(lap_val_.get(), val, nnz * sizeof(float), hipMemcpyHostToDevice), "H2D");
    has_lap_ = true;
}

void Engine64::backproject_reduce(const double* w, double* out) {
    launch_backproject64(A_, ld_, P_, w, nsplit_, partial_.get(), nullptr, stream_);
    launch_reduce_partials_f64(partial_.get(), ld_, nsplit_, out, stream_);
}

double Engine64::setup_frame(const double* g, const double* x0) {
    RoctxRange r("sart::setup_frame64");
    // CpuSolver::solve up to its first sweep; the O(P) row operands are formed on the host in its own statements
    const bool lg = cfg_.logarithmic;
    double* gw = hrows_;
    double* a = hrows_ + Pp_;
    double* w0 = hrows_ + 2 * Pp_;
    double* wobs = hrows_ + 3 * Pp_;
    double norm = 1.0;
    if (gpu_) {
        double mx = -std::numeric_limits<double>::infinity();
        for (int64_t q = 0; q < P_; ++q) mx = std::max(mx, g[q]);
        norm = comm_->host().all_reduce_scalar(mx, ReduceOp::kMax);
        if (!(norm > 0)) norm = 1.0;
        for (int64_t q = 0; q < P_; ++q) gw[q] = (double)(float)(g[q] / norm);
    } else {
        for (int64_t q = 0; q < P_; ++q) gw[q] = g[q];
    }
    double gs = 0.0;
    for (int64_t q = 0; q < P_; ++q)
        if (g[q] > 0) gs += g[q] * g[q];
    const double G = comm_->host().all_reduce_scalar(gs, ReduceOp::kSum) / (norm * norm);
    for (int64_t q = 0; q < P_; ++q) {
        a[q] = gw[q] >= 0 ? inv_len_[q] : 0.0;
        w0[q] = gpu_ ? std::max(gw[q], 0.0) : gw[q];
        wobs[q] = a[q] * gw[q];
    }
    hip_call(hipMemcpyAsync(rows_.get(), hrows_, 4 * Pp_ * sizeof(double), hipMemcpyHostToDevice, stream_), "H2D rows");
    if (!x0) {  // cold start (reference sartsolver.cpp:150-160)
        backproject_reduce(rows_.get() + 2 * Pp_, red_.get());
        comm_->all_reduce(red_.get(), (size_t)V_, ReduceOp::kSum, stream_);
        launch_init_x64(x_.get(), V_, ld_, red_.get(), dvalid_.get(), rho_s_.get(), 1.0, clamp_, stream_);
    } else {
        std::memcpy(hx_, x0, V_ * sizeof(double));
        hip_call(hipMemcpyAsync(x0_.get(), hx_, V_ * sizeof(double), hipMemcpyHostToDevice, stream_), "H2D x0");
        launch_init_x64(x_.get(), V_, ld_, x0_.get(), nullptr, nullptr, norm, clamp_, stream_);
    }
    if (lg) {  // the frame-constant observed back-projection
        backproject_reduce(rows_.get() + 3 * Pp_, O_.get());
        comm_->all_reduce(O_.get(), (size_t)V_, ReduceOp::kSum, stream_);
        launch_mask64(O_.get(), dvalid_.get(), V_, stream_);
    }
    launch_state_begin(st_.get(), G, cfg_.conv_tolerance, cfg_.max_iterations, stream_);
    return norm;
}

void Engine64::sweep() {
    const SartState* st = st_.get();
    const bool lg = cfg_.logarithmic;
    const double* gw = rows_.get();
    const double* a = rows_.get() + Pp_;
    launch_forward64(lg ? kEpiLog : kEpiLinear, A_, ld_, P_, Pp_, V_, x_.get(), gw, a, nullptr, w_.get(), Fpart_.get(),
                     st, stream_);
    launch_backproject64(A_, ld_, P_, w_.get(), nsplit_, partial_.get(), st, stream_);
    launch_reduce_partials_f64(partial_.get(), ld_, nsplit_, red_.get(), stream_);
    launch_sum_f64(Fpart_.get(), nF_, red_.get() + V_, st, stream_);  // slot V, as CpuSolver's redF
    comm_->all_reduce(red_.get(), (size_t)V_ + 1, ReduceOp::kSum, stream_);
    const double* pen = nullptr;
    if (has_lap_) {  // of the iterate before the update
        launch_penalty64(lg, lap_rp_.get(), lap_col_.get(), lap_val_.get(), V_, cfg_.beta_laplace, x_.get(), pen_.get(),
                         st, stream_);
        pen = pen_.get();
    }
    launch_decide64(st_.get(), red_.get() + V_, stream_);
    launch_update64(lg, x_.get(), red_.get(), O_.get(), pen, dvalid_.get(), rho_s_.get(), cfg_.relaxation, eps_, gpu_,
                    V_, st, stream_);
}

SolveInfo Engine64::solve(const double* g, const double* x0, double* x_out) {
    RoctxRange range("sart::solve64");
    set_device();
    const auto t0 = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point a) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    };
    SolveInfo info;
    const double norm = setup_frame(g, x0);
    info.setup_ms = ms_since(t0);
    const auto t_iter = std::chrono::steady_clock::now();
    // sweep s is the forward projection of the iterate after s updates: max_iterations updates need one more
    const int max_sweeps = cfg_.max_iterations + 1;
    int enqueued = 0, issued = 0, checked = 0;
    auto issue = [&]() {
        const int n = std::min(cfg_.check_interval, max_sweeps - enqueued);
        for (int i = 0; i < n; ++i) sweep();
        enqueued += n;
        const int slot = issued & 1;
        hip_call(hipMemcpyAsync(hstate_ + slot, st_.get(), sizeof(SartState), hipMemcpyDeviceToHost, stream_),
                 "D2H state");
        hip_call(hipEventRecord(ev_[slot], stream_), "event");
        ++issued;
    };
    issue();
    while (true) {
        if (enqueued < max_sweeps) issue();  // keep the GPU busy while the previous chunk is checked
        const int slot = checked & 1;
        hip_call(hipEventSynchronize(ev_[slot]), "event sync");
        const SartState s = hstate_[slot];
        ++checked;
        if (s.done || (checked == issued && enqueued >= max_sweeps)) break;
    }
    hip_call(hipStreamSynchronize(stream_), "solve64");
    comm_->check();
    info.queued_sweeps = enqueued;
    info.iterate_ms = ms_since(t_iter);
    const auto t_fin = std::chrono::steady_clock::now();
    SartState s;
    hip_call(hipMemcpyAsync(&hstate_[0], st_.get(), sizeof(SartState), hipMemcpyDeviceToHost, stream_), "D2H state");
    hip_call(hipMemcpyAsync(hx_, x_.get(), V_ * sizeof(double), hipMemcpyDeviceToHost, stream_), "D2H x");
    hip_call(hipStreamSynchronize(stream_), "D2H x");
    s = hstate_[0];
    for (int64_t v = 0; v < V_; ++v) x_out[v] = hx_[v] * norm;
    info.status = s.status == kSuccess ? kSuccess : kMaxIterationsExceeded;
    info.iterations = s.iterations;
    info.convergence = s.conv_last;
    info.nonfinite = (s.flags & 1) != 0;
    info.used_fused = false;
    info.fused_variant = -1;
    info.comm = comm_->backend();
    info.sweeps = s.sweep;
    info.finish_ms = ms_since(t_fin);
    info.ms = ms_since(t0);
    return info;
}

}  // namespace sart
