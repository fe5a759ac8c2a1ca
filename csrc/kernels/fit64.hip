// Fit projections for gfx950 (--fit, SARTSolver.fit): F[j][p] = sum_v A[p][v] X[j][v] for nv <= 8 solutions per pass
// over the shard, every product and sum an fp64 FMA, X and F fp64. A is the shard as stored -- fp32, bf16, row-scaled
// f16 (RtmVec<AT>, widened exactly; an f16 row's finished dot times its power-of-two 1 / s_p, exact) or CSR -- so the
// images say how well a solution explains the data under exactly the matrix a solver used, with no rounding added.
//
// Dense shape (k_fit64). Each matrix element feeds nv FMAs and X is nv ld 8 bytes (4 MB at 64k voxels, nv = 8). In
// k_forward64's shape (8 rows per workgroup, every lane reading x itself) a lane would fetch 8 x 8 = 64 bytes of X per
// fp32 column against 32 bytes of A, from L2 rather than HBM but by every workgroup, and 8 rows x 8 vectors x 2 chains
// are 128 fp64 accumulators. So:
//   * a wave owns RW = 4 whole rows (no reduction across waves) and a workgroup of four waves 16 rows; the workgroup
//     walks the row in tiles of 512 columns and shares the X tile through LDS: 512 nv 8 bytes of X are fetched once
//     per tile and workgroup (64 bytes per column at nv = 8) against 16 rows x 512 columns of A (64 bytes per column
//     in fp32, 32 in 16 bits), and X stays in L2 / MALL while A streams from HBM with the non-temporal hint;
//   * a lane holds one chain per row and vector, 4 x nv = 32 fp64 accumulators at nv = 8 (the four rows give the FMA
//     pipe four independent chains per operand; a second chain per pair, as k_forward64 keeps, costs 64 VGPRs and the
//     second wave per SIMD), one 16-byte load of A per row and 64-lane pass, and reads its X operands from LDS as
//     16-byte reads at a 16-byte lane stride (the tile is stored pass-major: no bank conflicts on the read side,
//     which outnumbers the writes 16 to 1);
//   * LDS traffic is nv 8 bytes per lane-column for four rows: 69 GB per pass at 64k x 64k, nv = 8, over 256 CUs x
//     256 B/clk, half a millisecond against 2.5 ms (fp32) / 1.3 ms (16-bit) of HBM time.
//   * A wide pass is NOT HBM-bound as built. Measured (tools/fit_bench.py, profiles/fit_64k.jsonl, 64k x 64k): fp32
//     2.53 / 2.51 / 4.52 ms at nv = 1 / 4 / 8 (k_forward64: 2.46 ms; nv = 1 and 4 run at the HBM rate, 6.8 TB/s),
//     bf16 1.32 / 1.88 / 4.87 ms, f16 1.31 / 1.91 / 5.04 ms. A pass runs at the HBM rate up to nv = 4 on fp32 shards
//     and at nv = 1 on 16-bit ones; beyond that its time grows with the FMA count, about 0.12 ms per G FMA or 16
//     cycles per wave and v_fma_f64 -- several times the part's vector-fp64 issue rate, so the FMA pipe is not
//     saturated either. The cause is not isolated (wall times only, no counters): the nv = 8 build holds 256 VGPRs
//     plus 60-74 AGPR copies of its A tiles at one wave per SIMD, with two barriers per tile. Per frame the best
//     measured widths are 8 (fp32: 0.57 ms a frame against 2.53 alone) and 4 (16-bit: 0.47 against 1.3; the nv = 8
//     kernel loses to two nv = 4 passes): fit64_group().
//   * the tile loop is software-pipelined: the loads of tile t + 1 (X first, then A, so the wait for X leaves the
//     A loads in flight) are issued before the FMAs of tile t; two register sets for A alternate.
// Loads are unconditional with clamped indices (a lane past the row's end re-reads its last vector, rows past nrows
// re-read the last row and are not written, vector slots >= nv re-read vector nv - 1 and are not written); X beyond
// nvoxel is replaced by 0 where the tile is written to LDS, which also masks the clamped lanes (0 * NaN would poison
// a row). No atomics.
//
// Grouping independence: F[j][p] depends on row p and vector j only. A (row, vector) pair has one chain per lane --
// the elements of the lane's 16-byte vectors, columns ascending -- then the fixed xor tree over the 64 lanes; the
// column -> lane map (vector c of the row to lane c % 64) does not depend on nv, the slot or the grid, and the nv
// buckets (1, 4, 8) differ only in how many vectors share a pass.
//
// Sparse shape (k_fit64_csr): a group of L lanes per row as k_csr_forward, each lane one fp64 chain per vector over
// every L-th entry of the row (four entries' loads issued ahead of their products), the L lane sums by a fixed xor
// tree. A row's sum depends on L, so L must not depend on the shard: it is SparseRtm::lanes_rows when the caller sets
// one and kFitCsrLanes = 8 otherwise -- never sparse_lanes() of the shard's mean row length (two ranks' shards have
// other means than the whole matrix) and never the SART_SPARSE_LANES knob -- so the same row gives the same bits on
// any row partition. X is copied once per pass into a voxel-major [ld][8] layout (k_fit64_xt, zero beyond
// nvoxel and in the slots >= nv), so one entry's operands for all vectors are a single 64-byte line (the lesson of
// k_mf_sparse_spmm, profiles/sparse_r5_plane_width.txt); all eight slots are always computed, so a value cannot
// depend on nv.
#include "sart_common.hpp"

#include <stdexcept>
#include <string>
#include <type_traits>

#include "launchers.hpp"

namespace sart {

namespace {

constexpr int kFitRw = 4;        // rows per wave
constexpr int kFitRpb = 4 * 4;   // rows per workgroup (four waves)
constexpr int kFitTile = 512;    // columns per tile
constexpr int kFitMaxNv = 8;
constexpr int kFitCsrLanes = 8;  // lanes per CSR row unless the caller fixes another width (rows of ~48 entries)

template <int L>
__device__ __forceinline__ double group_sum64(double v) {
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, L);
    return v;
}

}  // namespace

template <typename AT, int NV>
__global__ __launch_bounds__(256) void k_fit64(const AT* __restrict__ A, int64_t ld, int64_t nrows, int64_t nvoxel,
                                               const double* __restrict__ X, int64_t ldx, int nv,
                                               const float* __restrict__ rinv, double* __restrict__ F, int64_t ldf) {
    using V = RtmVec<AT>;
    constexpr int RW = kFitRw;
    constexpr int NF4 = V::NF4;
    constexpr int E = 4 * NF4;             // columns per 16-byte vector of A
    constexpr int U = kFitTile / (64 * E);  // 64-lane passes per tile (fp32: 2, 16-bit: 1)
    constexpr int PER = E / 2;             // double2 of X per lane and pass
    constexpr int XQ = kFitTile / 2;       // double2 of X per vector and tile (= 256: one per thread)
    static_assert(U >= 1 && XQ == 256, "tile shape");
    __shared__ double2 xs[NV][XQ];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * kFitRpb + (int64_t)wid * RW;
    const int64_t ldv = ld / E;
    const AT* __restrict__ arow[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int64_t row = row0 + r < nrows ? row0 + r : nrows - 1;
        arow[r] = A + row * ld;
    }
    // this thread's double2 of every vector's tile: tile columns 2 tid, 2 tid + 1; stored pass-major, so that lane l
    // of pass u reads part p at ((u PER + p) 64 + l)
    const int xslot = ((tid / (64 * PER)) * PER + tid % PER) * 64 + (tid / PER) % 64;
    const int jlast = nv - 1;

    double acc[RW][NV];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[r][j] = 0.0;

    const int64_t ntile = (ld + kFitTile - 1) / kFitTile;
    double2 xn[NV];
    float4 a0[U][RW][NF4], a1[U][RW][NF4];

    auto load_x = [&](int64_t t) {
        const int64_t col_raw = t * kFitTile + 2 * tid;
        const int64_t col = col_raw < ld ? col_raw : ld - 2;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int jj = j < jlast ? j : jlast;
            xn[j] = *reinterpret_cast<const double2*>(X + (int64_t)jj * ldx + col);
        }
    };
    auto load_a = [&](int64_t t, float4 (&a)[U][RW][NF4]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t c_raw = t * (64 * U) + u * 64 + lane;
            const int64_t c = c_raw < ldv ? c_raw : ldv - 1;
#pragma unroll
            for (int r = 0; r < RW; ++r) V::load(arow[r], c, a[u][r]);
        }
    };
    auto step = [&](int64_t t, float4 (&ac)[U][RW][NF4], float4 (&an)[U][RW][NF4]) {
        __syncthreads();  // every wave has read tile t - 1
        {
            const int64_t col = t * kFitTile + 2 * tid;
            const bool in0 = col < nvoxel, in1 = col + 1 < nvoxel;
#pragma unroll
            for (int j = 0; j < NV; ++j) xs[j][xslot] = make_double2(in0 ? xn[j].x : 0.0, in1 ? xn[j].y : 0.0);
        }
        __syncthreads();
        if (t + 1 < ntile) {  // uniform
            load_x(t + 1);
            load_a(t + 1, an);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int p = 0; p < PER; ++p) {
                // the LDS reads of one (pass, part) at a time: hoisted together they cost the second wave per SIMD
                asm volatile("" ::: "memory");
                double ae[RW], ao[RW];
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    const float4 q = ac[u][r][p / 2];
                    ae[r] = (double)((p & 1) ? q.z : q.x);
                    ao[r] = (double)((p & 1) ? q.w : q.y);
                }
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const double2 xv = xs[j][(u * PER + p) * 64 + lane];
#pragma unroll
                    for (int r = 0; r < RW; ++r) {
                        acc[r][j] = fma(ae[r], xv.x, acc[r][j]);
                        acc[r][j] = fma(ao[r], xv.y, acc[r][j]);
                    }
                }
            }
        }
    };

    load_x(0);
    load_a(0, a0);
    for (int64_t t = 0; t < ntile; t += 2) {
        step(t, a0, a1);
        if (t + 1 < ntile) step(t + 1, a1, a0);
    }

#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int64_t row = row0 + r;
        double sc = 1.0;
        if (V::kRowScaled && row < nrows) sc = (double)rinv[row];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            double s = wave_sum(acc[r][j]);
            if (V::kRowScaled) s *= sc;
            if (lane == 0 && row < nrows && j < nv) F[(int64_t)j * ldf + row] = s;
        }
    }
}

// X [nv][ldx] -> Xt [ld][8]: zero beyond nvoxel (the caller's padding may hold anything) and in the slots >= nv
__global__ __launch_bounds__(256) void k_fit64_xt(const double* __restrict__ X, int64_t ldx, int nv, int64_t nvoxel,
                                                  int64_t ld, double* __restrict__ Xt) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= ld) return;
    double o[kFitMaxNv];
#pragma unroll
    for (int j = 0; j < kFitMaxNv; ++j) o[j] = (j < nv && v < nvoxel) ? X[(int64_t)j * ldx + v] : 0.0;
    double2* dst = reinterpret_cast<double2*>(Xt + v * kFitMaxNv);
#pragma unroll
    for (int j = 0; j < kFitMaxNv; j += 2) dst[j / 2] = make_double2(o[j], o[j + 1]);
}

template <int L>
__global__ __launch_bounds__(256) void k_fit64_csr(const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                   const float* __restrict__ val, int64_t nrows,
                                                   const double* __restrict__ Xt, int nv, double* __restrict__ F,
                                                   int64_t ldf) {
    constexpr int NVS = kFitMaxNv;
    constexpr int RPB = 256 / L;
    const int sub = threadIdx.x & (L - 1), rl = threadIdx.x / L;
    const int64_t row = (int64_t)blockIdx.x * RPB + rl;
    const double2* __restrict__ xt2 = reinterpret_cast<const double2*>(Xt);
    double acc[NVS];
#pragma unroll
    for (int j = 0; j < NVS; ++j) acc[j] = 0.0;
    if (row < nrows) {
        const int64_t k1 = rp[row + 1];
        int64_t k = rp[row] + sub;
        for (; k + 3 * L < k1; k += 4 * L) {  // four entries' loads ahead of their products
            int32_t i[4];
            double a[4];
            double2 x[4][NVS / 2];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                i[e] = col[k + e * L];
                a[e] = (double)val[k + e * L];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int h = 0; h < NVS / 2; ++h) x[e][h] = xt2[(int64_t)i[e] * (NVS / 2) + h];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int h = 0; h < NVS / 2; ++h) {
                    acc[2 * h] = fma(a[e], x[e][h].x, acc[2 * h]);
                    acc[2 * h + 1] = fma(a[e], x[e][h].y, acc[2 * h + 1]);
                }
        }
        for (; k < k1; k += L) {
            const double a = (double)val[k];
            const int64_t i = col[k];
#pragma unroll
            for (int h = 0; h < NVS / 2; ++h) {
                const double2 x = xt2[i * (NVS / 2) + h];
                acc[2 * h] = fma(a, x.x, acc[2 * h]);
                acc[2 * h + 1] = fma(a, x.y, acc[2 * h + 1]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NVS; ++j) {
        const double s = group_sum64<L>(acc[j]);
        if (sub == 0 && row < nrows && j < nv) F[(int64_t)j * ldf + row] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------------------------
namespace {

void check_fit_nv(int nv, const char* what) {
    if (nv < 1 || nv > kFitMaxNv)
        throw std::runtime_error(std::string(what) + ": no kernel for nv = " + std::to_string(nv) +
                                 " vectors per pass (built: 1 .. 8, in buckets of 1, 4 and 8)");
}

template <typename AT>
void fit64_storage(const AT* A, const char* name, int64_t ld, int64_t nrows, int64_t nvoxel, const double* X,
                   int64_t ldx, int nv, const float* rinv, double* F, int64_t ldf, hipStream_t stream) {
    const dim3 grid((unsigned)((nrows + kFitRpb - 1) / kFitRpb));
    auto go = [&](auto k) {
        hipLaunchKernelGGL(k, grid, dim3(256), 0, stream, A, ld, nrows, nvoxel, X, ldx, nv, rinv, F, ldf);
    };
    if (nv == 1)
        go(k_fit64<AT, 1>);
    else if (nv <= 4)
        go(k_fit64<AT, 4>);
    else
        go(k_fit64<AT, 8>);
    check_launch(name);
}

}  // namespace

// vectors per pass at which a frame costs least (the measurements in the file header)
int fit64_group(bool bf16, bool f16, bool sparse) { return !sparse && (bf16 || f16) ? 4 : kFitMaxNv; }

void launch_fit64(const void* A, bool bf16, bool f16, const float* row_scale, int64_t ld, int64_t nrows,
                  int64_t nrows_pad, int64_t nvoxel, const double* X, int64_t ldx, int nv, double* F, int64_t ldf,
                  hipStream_t stream) {
    check_fit_nv(nv, "fit64");
    if (bf16 && f16) throw std::runtime_error("fit64: bf16 and f16 are exclusive");
    if (f16 && !row_scale) throw std::runtime_error("fit64: f16 storage needs the rows' scales");
    if (ld % 64 != 0 || ld <= 0 || nvoxel > ld || nvoxel < 0)
        throw std::runtime_error("fit64: ld must be a multiple of 64 >= nvoxel");
    if (nrows_pad < nrows) throw std::runtime_error("fit64: padded row count below the row count");
    if (ldx < ld || ldx % 2 != 0) throw std::runtime_error("fit64: X rows must be even and hold ld entries");
    if (ldf < nrows) throw std::runtime_error("fit64: F rows must hold nrows entries");
    if (nrows <= 0) return;
    if (f16)
        fit64_storage(static_cast<const f16s_t*>(A), "k_fit64 (f16)", ld, nrows, nvoxel, X, ldx, nv,
                      row_scale + nrows_pad, F, ldf, stream);
    else if (bf16)
        fit64_storage(static_cast<const bf16_t*>(A), "k_fit64 (bf16)", ld, nrows, nvoxel, X, ldx, nv, nullptr, F, ldf,
                      stream);
    else
        fit64_storage(static_cast<const float*>(A), "k_fit64 (fp32)", ld, nrows, nvoxel, X, ldx, nv, nullptr, F, ldf,
                      stream);
}

void launch_fit64_csr(const SparseRtm& s, int64_t nrows, int64_t nvoxel, int64_t ld, const double* X, int64_t ldx,
                      int nv, double* Xt, double* F, int64_t ldf, hipStream_t stream) {
    check_fit_nv(nv, "fit64_csr");
    if (!s.row_ptr || (s.nnz > 0 && (!s.col || !s.val))) throw std::runtime_error("fit64_csr: incomplete CSR arrays");
    if (ld < nvoxel || nvoxel < 0 || ldx < nvoxel)
        throw std::runtime_error("fit64_csr: ld and X rows must hold nvoxel entries");
    if (ldf < nrows) throw std::runtime_error("fit64_csr: F rows must hold nrows entries");
    if (!Xt) throw std::runtime_error("fit64_csr: the [ld][8] scratch is required");
    if (nrows <= 0 || ld <= 0) return;
    hipLaunchKernelGGL(k_fit64_xt, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, stream, X, ldx, nv, nvoxel, ld,
                       Xt);
    check_launch("k_fit64_xt");
    const int L = s.lanes_rows ? s.lanes_rows : kFitCsrLanes;  // never from the shard: see the file header
    auto go = [&](auto lc) {
        constexpr int LL = decltype(lc)::value;
        hipLaunchKernelGGL(k_fit64_csr<LL>, dim3((unsigned)((nrows + 256 / LL - 1) / (256 / LL))), dim3(256), 0,
                           stream, s.row_ptr, s.col, s.val, nrows, Xt, nv, F, ldf);
    };
    switch (L) {
        case 4: go(std::integral_constant<int, 4>{}); break;
        case 8: go(std::integral_constant<int, 8>{}); break;
        case 16: go(std::integral_constant<int, 16>{}); break;
        case 32: go(std::integral_constant<int, 32>{}); break;
        default:
            throw std::runtime_error("fit64_csr: no kernel for " + std::to_string(L) + " lanes per row (4, 8, 16, 32)");
    }
    check_launch("k_fit64_csr");
}

}  // namespace sart
