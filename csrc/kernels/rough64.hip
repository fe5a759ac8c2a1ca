// Roughness norms for gfx950 (--beta_scan, models/lcurve.py): eta2[j] = sum_{r < n} (sum_k L[r, col_k] u_j[col_k])^2
// for nv <= 8 solutions per pass over the Laplacian CSR, u = x (linear solver) or log(max(x, 1e-100)) (logarithmic
// solver: the CPU solver's epsilon keeps a zero voxel finite). X and every product and sum are fp64 FMAs; L's fp32
// values are widened, which is exact.
//
// Shape (k_rough64), after k_fit64_csr: a group of kRoughLanes = 8 lanes per row (a Laplacian row holds ~7 entries),
// each lane one fp64 chain per solution over every 8th entry of the row, the 8 lane sums by a fixed xor tree. The lane
// count is a constant -- never taken from the matrix -- so a row's sum does not depend on the Laplacian's mean row
// length. X is read in place ([nv][ldx]; a column index is < n, so entries at and beyond n are never loaded, and the
// slots >= nv are not touched at all): the operands of one entry are nv scattered 8-byte loads, which is as good as a
// transposed copy for rows this short, whose entries hit the same few lines of each solution.
//
// Reduction: a workgroup of 256 threads owns 32 rows per tile and walks the tiles blockIdx.x, blockIdx.x + grid, ...
// (grid = min(tiles, 2048): a function of n alone). Per tile the 32 row sums of a solution are squared and added
// in row order by one thread per solution (through LDS) onto that thread's running partial; the partials go to
// scratch [grid][8]. k_rough64_final (one workgroup per solution) adds them: thread t the partials t, t + 256, ... in
// order, then a fixed tree over the 256 threads. No atomics: eta2[j] depends on n, L and X[j] only -- not on nv, on
// the slot or on the run.
#include "sart_common.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "launchers.hpp"

namespace sart {

namespace {

constexpr int kRoughLanes = 8;                 // lanes per CSR row: fixed (see the file header)
constexpr int kRoughRpb = 256 / kRoughLanes;   // rows per workgroup and tile
constexpr int kRoughMaxNv = 8;
constexpr int kRoughMaxBlocks = 2048;

__device__ __forceinline__ double rough_sum(double v) {
#pragma unroll
    for (int o = kRoughLanes / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kRoughLanes);
    return v;
}

int64_t rough_tiles(int64_t n) { return (n + kRoughRpb - 1) / kRoughRpb; }
int rough_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(rough_tiles(n), kRoughMaxBlocks)); }

}  // namespace

template <bool LOG>
__global__ __launch_bounds__(256) void k_rough64(const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                 const float* __restrict__ val, int64_t n,
                                                 const double* __restrict__ X, int64_t ldx, int nv,
                                                 double* __restrict__ scratch) {
    constexpr int L = kRoughLanes, NVS = kRoughMaxNv, RPB = kRoughRpb;
    __shared__ double rs[NVS][RPB];
    const int sub = threadIdx.x & (L - 1), rl = threadIdx.x / L;
    const int64_t ntile = (n + RPB - 1) / RPB;
    double part = 0.0;  // thread j < nv: this workgroup's sum of squares of solution j
    for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
        const int64_t row = t * RPB + rl;
        double acc[NVS];
#pragma unroll
        for (int j = 0; j < NVS; ++j) acc[j] = 0.0;
        if (row < n) {
            const int64_t k1 = rp[row + 1];
            for (int64_t k = rp[row] + sub; k < k1; k += L) {
                const double a = (double)val[k];
                const int64_t i = col[k];
#pragma unroll
                for (int j = 0; j < NVS; ++j) {
                    if (j < nv) {  // uniform
                        double u = X[(int64_t)j * ldx + i];
                        if (LOG) u = log(fmax(u, 1e-100));
                        acc[j] = fma(a, u, acc[j]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NVS; ++j) {
            const double s = rough_sum(acc[j]);  // rows >= n and slots >= nv: 0
            if (sub == 0) rs[j][rl] = s;
        }
        __syncthreads();
        if (threadIdx.x < nv) {
#pragma unroll 4
            for (int r = 0; r < RPB; ++r) {
                const double s = rs[threadIdx.x][r];
                part = fma(s, s, part);
            }
        }
        __syncthreads();  // rs is rewritten by the next tile
    }
    if (threadIdx.x < NVS) scratch[(int64_t)blockIdx.x * NVS + threadIdx.x] = threadIdx.x < nv ? part : 0.0;
}

// eta2[j] = sum over the workgroups' partials of solution j = blockIdx.x, in a fixed order
__global__ __launch_bounds__(256) void k_rough64_final(const double* __restrict__ scratch, int nblocks,
                                                       double* __restrict__ eta2) {
    __shared__ double sh[256];
    const int j = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) s += scratch[(int64_t)b * kRoughMaxNv + j];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) eta2[j] = sh[0];
}

int64_t rough64_scratch_elems(int64_t n) { return (int64_t)rough_grid(std::max<int64_t>(n, 0)) * kRoughMaxNv; }

void launch_rough64(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n, const double* X,
                    int64_t ldx, int nv, bool logx, double* eta2_out, double* scratch, hipStream_t stream) {
    if (nv < 1 || nv > kRoughMaxNv)
        throw std::runtime_error("rough64: no kernel for nv = " + std::to_string(nv) + " vectors per pass (1 .. 8)");
    if (n < 0 || ldx < n) throw std::runtime_error("rough64: X rows must hold n entries");
    if (!row_ptr || !X || !eta2_out || !scratch) throw std::runtime_error("rough64: null operand");
    const int grid = rough_grid(n);  // n = 0: one workgroup writes zero partials
    if (logx)
        hipLaunchKernelGGL(k_rough64<true>, dim3(grid), dim3(256), 0, stream, row_ptr, col, val, n, X, ldx, nv, scratch);
    else
        hipLaunchKernelGGL(k_rough64<false>, dim3(grid), dim3(256), 0, stream, row_ptr, col, val, n, X, ldx, nv,
                           scratch);
    check_launch("k_rough64");
    hipLaunchKernelGGL(k_rough64_final, dim3(nv), dim3(256), 0, stream, scratch, grid, eta2_out);
    check_launch("k_rough64_final");
}

}  // namespace sart
