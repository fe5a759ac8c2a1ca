// Hold-out sums for gfx950 (--holdout, models/holdout.py): for n fp64 fitted images F [n][ldf] of the columns of one
// composite frame g, per column j and camera m (the pixels cam_start[m] .. cam_start[m + 1] - 1) six doubles,
//   sum_H (g - f)^2, sum_H g^2, |H|, sum_Kp (g - f)^2, sum_Kp g^2, |Kp|,
// over the counted pixels of the camera (g >= 0 and ell > threshold; a NaN in g or ell: not counted), H those with
// fold == held[j] (held[j] = -1: none) and Kp the others. All arithmetic is fp64, contraction off: d = g - f, then
// d d, then the addition, each rounded on its own; the counts are exact doubles.
//
// Shape (k_holdout64): grid (ncam, n), 256 threads; block (m, j) owns camera m of column j. Thread t takes the pixels
// cam_start[m] + t, + 256, ... in order with six accumulators, so consecutive threads read consecutive pixels of g, ell,
// fold and F[j] (coalesced). g, ell and fold are read again by every column's block: at 8 columns of 65536 pixels that
// is 4 MB against the 4 MB of F, all of it L2-resident after the first block, and a block per (camera, column) keeps a
// value independent of how many columns a launch carries.
//
// Reduction: the 256 running values of each quantity go to LDS ([6][256] doubles, 12 KB) and are added by a fixed tree,
// s[t] += s[t + stride] for stride 128 .. 1. No atomics, no scratch, no second launch: a value depends on its column,
// its camera range and the inputs alone -- not on n, ncam, the slot or the run. A NaN f at a counted pixel makes its
// (column, camera) sums NaN and nothing else; a pixel that is not counted is never read from F. Nothing at or beyond
// cam_start[ncam] is read.
#include "sart_common.hpp"

#include <stdexcept>
#include <string>

#include "launchers.hpp"

namespace sart {

__global__ __launch_bounds__(256) void k_holdout64(const double* __restrict__ F, int64_t ldf,
                                                   const double* __restrict__ g, const double* __restrict__ ell,
                                                   double threshold, const int32_t* __restrict__ fold,
                                                   const int32_t* __restrict__ held,
                                                   const int64_t* __restrict__ cam_start, double* __restrict__ sums) {
#pragma clang fp contract(off)
    constexpr int Q = kHoldoutSums;
    __shared__ double s[Q][256];
    const int m = blockIdx.x, j = blockIdx.y, t = threadIdx.x;
    const int64_t p0 = cam_start[m], p1 = cam_start[m + 1];
    const int h = held[j];
    const double* __restrict__ f = F + (int64_t)j * ldf;
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0;
    for (int64_t p = p0 + t; p < p1; p += 256) {
        const double gp = g[p];
        if (!(gp >= 0.0 && ell[p] > threshold)) continue;  // (no barrier inside the loop)
        const double d = gp - f[p];
        const double dd = d * d, gg = gp * gp;
        if (h >= 0 && fold[p] == h) {
            acc[0] += dd;
            acc[1] += gg;
            acc[2] += 1.0;
        } else {
            acc[3] += dd;
            acc[4] += gg;
            acc[5] += 1.0;
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q][t] = acc[q];
    __syncthreads();
    for (int stride = 128; stride > 0; stride >>= 1) {
        if (t < stride) {
#pragma unroll
            for (int q = 0; q < Q; ++q) s[q][t] += s[q][t + stride];
        }
        __syncthreads();
    }
    if (t < Q) sums[((int64_t)j * gridDim.x + m) * Q + t] = s[t][0];
}

void launch_holdout64(const double* F, int64_t ldf, int n, const double* g, const double* ell, double threshold,
                      const int32_t* fold, const int32_t* held, const int64_t* cam_start, int ncam, double* sums,
                      hipStream_t stream) {
    if (n < 1 || n > 65535)
        throw std::runtime_error("holdout64: no launch for n = " + std::to_string(n) + " columns (1 .. 65535)");
    if (ncam < 1) throw std::runtime_error("holdout64: needs at least one camera");
    if (ldf < 1) throw std::runtime_error("holdout64: F rows must hold the pixels");
    if (!F || !g || !ell || !fold || !held || !cam_start || !sums) throw std::runtime_error("holdout64: null operand");
    hipLaunchKernelGGL(k_holdout64, dim3(ncam, n), dim3(256), 0, stream, F, ldf, g, ell, threshold, fold, held,
                       cam_start, sums);
    check_launch("k_holdout64");
}

}  // namespace sart
