// Scores of reconstructed columns against a known truth for gfx950 (--phantom, models/phantom.py): for nv <= 8 columns
// X [nv][ldx] and one truth t, over the voxels v < nvoxel, ten doubles per column,
//   s_t = sum t, s_x = sum x, s_tt = sum t^2, s_xx = sum x^2, s_xt = sum x t, s_dd = sum (x - t)^2,
//   s_in = sum of x over the voxels with t > 0, m_d = max |x - t|, m_t = max t, m_x = max x.
// All arithmetic is fp64, contraction off: a term is the rounded product (or the rounded square of the rounded
// difference), the sums are plain additions of the terms.
//
// Shape (k_phantom64), after k_rough64: a workgroup of 256 threads owns 256 voxels per tile and walks the tiles
// blockIdx.x, blockIdx.x + grid, ... (grid = min(tiles, 1024): a function of nvoxel alone); thread i takes voxel i of
// each tile, so consecutive threads read consecutive voxels of t and of every column (coalesced). t is read once per
// voxel for all columns. The slots >= nv are not touched at all; a voxel at or beyond nvoxel is not loaded (the padding
// of X and t may hold anything).
//
// Reduction: the 256 running values of a (column, quantity) pair are combined by a fixed xor tree over the 64 lanes of
// each wave, then the four waves in order (through LDS); the workgroup's partials go to scratch [grid][8][10].
// k_phantom64_final (one workgroup per column) combines them: thread i the partials i, i + 256, ... in order, then a
// fixed tree over the 256 threads. No atomics: a column's ten values depend on nvoxel, X[j] and t only -- not on nv, on
// the slot or on the run. The identities of the three maxima are 0 (m_d) and -inf (m_t, m_x).
#include "sart_common.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "launchers.hpp"

namespace sart {

namespace {

constexpr int kPhantomMaxNv = 8;
constexpr int kPhantomMaxBlocks = 1024;
constexpr int kPhantomNsum = 7;  // the quantities 0 .. 6 are sums, 7 .. 9 maxima

int64_t phantom_tiles(int64_t nvoxel) { return (nvoxel + 255) / 256; }
int phantom_grid(int64_t nvoxel) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(phantom_tiles(nvoxel), kPhantomMaxBlocks));
}

__device__ __forceinline__ double phantom_identity(int q) {
    return q <= kPhantomNsum ? 0.0 : -__builtin_inf();  // the sums and m_d (|x - t| >= 0): 0
}
__device__ __forceinline__ double phantom_combine(int q, double a, double b) {
    return q < kPhantomNsum ? a + b : fmax(a, b);
}

}  // namespace

__global__ __launch_bounds__(256) void k_phantom64(const double* __restrict__ X, int64_t ldx, int64_t nvoxel, int nv,
                                                   const double* __restrict__ t, double* __restrict__ scratch) {
#pragma clang fp contract(off)
    constexpr int NVS = kPhantomMaxNv, Q = kPhantomSums;
    __shared__ double ws[NVS][Q][4];
    const int64_t ntile = (nvoxel + 255) / 256;
    double acc[NVS][Q];
#pragma unroll
    for (int j = 0; j < NVS; ++j)
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[j][q] = phantom_identity(q);
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * 256 + threadIdx.x;
        if (v >= nvoxel) continue;  // (no barrier inside the loop)
        const double tv = t[v];
        const double tt = tv * tv;
#pragma unroll
        for (int j = 0; j < NVS; ++j) {
            if (j < nv) {  // uniform
                const double x = X[(int64_t)j * ldx + v];
                const double d = x - tv;
                acc[j][0] += tv;
                acc[j][1] += x;
                acc[j][2] += tt;
                acc[j][3] += x * x;
                acc[j][4] += x * tv;
                acc[j][5] += d * d;
                acc[j][6] += tv > 0.0 ? x : 0.0;
                acc[j][7] = fmax(acc[j][7], fabs(d));
                acc[j][8] = fmax(acc[j][8], tv);
                acc[j][9] = fmax(acc[j][9], x);
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NVS; ++j) {
        if (j < nv) {  // uniform
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                double s = acc[j][q];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s = phantom_combine(q, s, __shfl_xor(s, o, 64));
                if (lane == 0) ws[j][q][wave] = s;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < NVS * Q) {
        const int j = threadIdx.x / Q, q = threadIdx.x % Q;
        double s = phantom_identity(q);
        if (j < nv) {
            s = ws[j][q][0];
            for (int w = 1; w < 4; ++w) s = phantom_combine(q, s, ws[j][q][w]);
        }
        scratch[(int64_t)blockIdx.x * (NVS * Q) + threadIdx.x] = s;
    }
}

// sums[j][q] = the workgroups' partials of column j = blockIdx.x combined in a fixed order
__global__ __launch_bounds__(256) void k_phantom64_final(const double* __restrict__ scratch, int nblocks,
                                                         double* __restrict__ sums) {
    constexpr int Q = kPhantomSums;
    __shared__ double sh[256];
    const int j = blockIdx.x;
    for (int q = 0; q < Q; ++q) {
        double s = phantom_identity(q);
        for (int b = threadIdx.x; b < nblocks; b += 256)
            s = phantom_combine(q, s, scratch[(int64_t)b * (kPhantomMaxNv * Q) + j * Q + q]);
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] = phantom_combine(q, sh[threadIdx.x], sh[threadIdx.x + o]);
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[j * Q + q] = sh[0];
        __syncthreads();  // sh is rewritten by the next quantity
    }
}

int64_t phantom64_scratch_elems(int64_t nvoxel) {
    return (int64_t)phantom_grid(std::max<int64_t>(nvoxel, 0)) * kPhantomMaxNv * kPhantomSums;
}

void launch_phantom64(const double* X, int64_t ldx, int64_t nvoxel, int nv, const double* t, double* sums_out,
                      double* scratch, hipStream_t stream) {
    if (nv < 1 || nv > kPhantomMaxNv)
        throw std::runtime_error("phantom64: no kernel for nv = " + std::to_string(nv) + " columns per pass (1 .. 8)");
    if (nvoxel < 1) throw std::runtime_error("phantom64: needs at least one voxel");
    if (ldx < nvoxel) throw std::runtime_error("phantom64: X rows must hold nvoxel entries");
    if (!X || !t || !sums_out || !scratch) throw std::runtime_error("phantom64: null operand");
    const int grid = phantom_grid(nvoxel);
    hipLaunchKernelGGL(k_phantom64, dim3(grid), dim3(256), 0, stream, X, ldx, nvoxel, nv, t, scratch);
    check_launch("k_phantom64");
    hipLaunchKernelGGL(k_phantom64_final, dim3(nv), dim3(256), 0, stream, scratch, grid, sums_out);
    check_launch("k_phantom64_final");
}

}  // namespace sart
