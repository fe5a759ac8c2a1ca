// Double-precision per-GPU SART engine (--fp64): CpuSolver (csrc/native/cpu_solver.cpp) step for step, with the two
// O(P V) passes of every iteration on the fp64 kernels of csrc/kernels/projection64.hip. The shard is the fp32 dense
// row shard of the fp32 engine; every vector, product and sum is fp64. `gpu_semantics` has CpuSolver's meaning: true
// evaluates the default GPU path (normalisation, eps = 1e-7, fp32-rounded thresholds) in fp64, false the reference
// CPU solver (--use_cpu).
//
// One iteration: forward (f, the next weights and sum f^2 in one pass), split-K back-projection, ONE all-reduce of
// V + 1 doubles (sum f^2 in slot V, as CpuSolver's redF), then the decision and the update. The convergence state
// lives on the device (SartState); the host reads it once per check_interval sweeps with the next chunk already
// queued, and the sweeps queued past the decision are no-ops.
//
// Pixel-row shards of fp32 dense matrices only: bf16 / f16 storage, sparse shards and column shards are refused.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "engine.hpp"

namespace sart {

class Engine64 {
   public:
    // A: device pointer to the fp32 row-major shard [nrows_pad x ld], zero padded (not owned). cfg: the solver
    // parameters and check_interval; its storage / partition flags must describe an fp32 row shard.
    Engine64(int device, const void* A, int64_t nrows, int64_t nrows_pad, int64_t nvoxel, int64_t ld,
             Communicator* comm, const EngineConfig& cfg, bool gpu_semantics, const SparseRtm* sparse = nullptr);
    ~Engine64();
    Engine64(const Engine64&) = delete;
    Engine64& operator=(const Engine64&) = delete;

    // CSR Laplacian over nvoxel rows (host arrays, copied). Ignored when beta_laplace == 0 or nnz == 0.
    void set_laplacian(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t nnz);
    // One frame: g = this rank's pixels (host fp64, nrows), x0 = warm start (host fp64, nvoxel) or null, x_out =
    // solution (host fp64, nvoxel, de-normalised)
    SolveInfo solve(const double* g, const double* x0, double* x_out);

    bool gpu_semantics() const { return gpu_; }
    const EngineConfig& config() const { return cfg_; }
    hipStream_t stream() const { return stream_; }
    int64_t nrows() const { return P_; }
    int64_t nvoxel() const { return V_; }
    int num_cus() const { return num_cus_; }
    std::vector<double> ray_density() const;  // fp64 (nvoxel), global
    std::vector<double> ray_length() const;   // fp64 (nrows), this shard's pixels

   private:
    void set_device() const;
    void init_scales();
    double setup_frame(const double* g, const double* x0);  // returns the normalisation
    void backproject_reduce(const double* w, double* out);  // out[0, ld) = A^T w of this shard
    void sweep();

    int device_;
    const float* A_;
    int64_t P_, Pp_, V_, ld_;
    Communicator* comm_;
    EngineConfig cfg_;
    bool gpu_;
    hipStream_t stream_ = nullptr;
    int num_cus_ = 0;
    int nsplit_ = 1;
    int64_t nF_ = 0;
    double eps_ = 1e-100, clamp_ = -1.0;

    DeviceRaySums rs_;
    DeviceArray<int32_t> dvalid_;
    DeviceArray<double> rho_s_;
    std::vector<double> inv_len_;  // host: [ell > tau] / ell, in the semantics' precision
    // rows_: [gw | a | w0 | wobs], Pp each (one upload per frame); red_: [0, V) the reduced back-projection,
    // [V] sum f^2
    DeviceArray<double> rows_, w_, x_, red_, O_, pen_, partial_, Fpart_, x0_;
    DeviceArray<SartState> st_;
    DeviceArray<int64_t> lap_rp_;
    DeviceArray<int32_t> lap_col_;
    DeviceArray<float> lap_val_;
    bool has_lap_ = false;

    SartState* hstate_ = nullptr;  // pinned [2]
    double* hrows_ = nullptr;      // pinned [4 Pp]
    double* hx_ = nullptr;         // pinned [ld]
    hipEvent_t ev_[2] = {nullptr, nullptr};
};

}  // namespace sart
