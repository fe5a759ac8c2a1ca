// Per-voxel mean and unbiased standard deviation over the replicas of a frame for gfx950 (--replicas,
// models/uncertainty.py): X [n][ldx] fp64, use [n] (0: the replica is left out). One thread per voxel, the replicas in
// index order and in two passes, m = (sum_r x_r) / c, then std = sqrt(sum_r (x_r - m)^2 / (c - 1)), c the number of
// replicas used; std is NaN for c < 2, mean NaN for c = 0. Consecutive threads read consecutive voxels of a replica
// (coalesced); no atomics, no reduction across threads: a voxel's values depend on its own column alone. Entries at and
// beyond nvoxel are neither read nor written. Contraction is off: the sums are the NumPy loop's, operation by
// operation.
#include "sart_common.hpp"

#include <stdexcept>
#include <string>

#include "launchers.hpp"

namespace sart {

__global__ __launch_bounds__(256) void k_moments64(const double* __restrict__ X, int64_t ldx, int64_t nvoxel, int n,
                                                   const uint8_t* __restrict__ use, double* __restrict__ mean,
                                                   double* __restrict__ sd) {
#pragma clang fp contract(off)
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nvoxel) return;
    int c = 0;
    double acc = 0.0;
    for (int r = 0; r < n; ++r) {
        if (!use[r]) continue;  // uniform
        acc += X[(int64_t)r * ldx + v];
        ++c;
    }
    const double nan = __builtin_nan("");
    const double m = c > 0 ? acc / (double)c : nan;
    double dev = 0.0;
    for (int r = 0; r < n; ++r) {
        if (!use[r]) continue;
        const double e = X[(int64_t)r * ldx + v] - m;
        dev += e * e;
    }
    mean[v] = m;
    sd[v] = c > 1 ? sqrt(dev / (double)(c - 1)) : nan;
}

void launch_moments64(const double* X, int64_t ldx, int64_t nvoxel, int n, const uint8_t* use, double* mean,
                      double* std_out, hipStream_t stream) {
    if (n < 0) throw std::runtime_error("moments64: negative replica count");
    if (nvoxel < 0 || ldx < nvoxel) throw std::runtime_error("moments64: X rows must hold nvoxel entries");
    if (nvoxel == 0) return;
    if (nvoxel > (int64_t)0x7fffffff * 256) throw std::runtime_error("moments64: too many voxels for one launch");
    if ((n > 0 && (!X || !use)) || !mean || !std_out) throw std::runtime_error("moments64: null operand");
    const int64_t blocks = (nvoxel + 255) / 256;
    hipLaunchKernelGGL(k_moments64, dim3((unsigned)blocks), dim3(256), 0, stream, X, ldx, nvoxel, n, use, mean, std_out);
    check_launch("k_moments64");
}

}  // namespace sart
