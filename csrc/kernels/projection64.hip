// Double-precision two-pass SART kernels for gfx950 (Engine64, --fp64): the shard stays the fp32 row-major
// [nrows_pad x ld] array of the fp32 engine (widening fp32 to fp64 is exact), every vector is fp64 and every product
// and sum an fp64 FMA. They evaluate what CpuSolver (csrc/native/cpu_solver.cpp) evaluates, in either of its
// semantics, at the HBM rate of the fp32 two-pass kernels: a dense fp64 GEMV over an fp32 matrix is bound by the
// matrix bytes on MI355X.
//
//   * k_forward64: row dot products (8 rows per workgroup, two accumulator chains per row and lane), a fixed-order
//     reduction over lanes and waves, and in the same pass f, the next back-projection's weight and one fp64
//     sum f^2 partial per workgroup (k_sum_f64 adds the partials in a fixed order).
//   * k_backproject64: deterministic split-K over rows with the structure of k_colsum_f64 (projection.hip): the
//     per-row weight is wave-uniform, partial[s][c] is written, launch_reduce_partials_f64 sums the splits.
//   * element-wise: cold-start scaling, CSR Laplacian penalty, linear / log update, and the single-lane decision.
//
// No atomics. A is streamed with non-temporal 16-byte loads; the loads of a tile are unconditional (indices clamped
// into the row, the clamped lanes' contributions masked to zero in arithmetic), so the compiler's vmcnt waits stay
// counted. Padding is masked where it is read: x beyond nvoxel is replaced by 0 (0 * NaN would poison a row), rows
// beyond nrows are neither read from w / g nor written.
#include "sart_common.hpp"

#include <math.h>

#include <algorithm>
#include <stdexcept>

#include "launchers.hpp"

namespace sart {

namespace {

constexpr int kRpb64 = 8;  // rows per workgroup of k_forward64 (forward_num_blocks)

__device__ __forceinline__ double sel(bool c, double a, double b) { return c ? a : b; }  // v_cndmask, no branch

}  // namespace

template <int EPI>
__global__ __launch_bounds__(256) void k_forward64(const float* __restrict__ A, int64_t ld, int64_t nrows,
                                                   int64_t nvoxel, const double* __restrict__ x,
                                                   const double* __restrict__ g, const double* __restrict__ arow,
                                                   double* __restrict__ out_f, double* __restrict__ out_w,
                                                   double* __restrict__ Fpart, const SartState* __restrict__ st) {
    if (st != nullptr && st->done) return;
    constexpr int RPB = kRpb64;
    __shared__ double red[4][RPB];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * RPB;
    const int64_t ldv = ld / 4;  // 16-byte vectors per row
    const float* __restrict__ a0 = A + row0 * ld;
    const double2* __restrict__ x2 = reinterpret_cast<const double2*>(x);

    double acc0[RPB], acc1[RPB];
#pragma unroll
    for (int r = 0; r < RPB; ++r) acc0[r] = acc1[r] = 0.0;

    // every lane runs the same number of tiles; a lane past the row's end re-reads the last vector with x = 0
    const int64_t ntile = (ldv + 255) / 256;
#pragma unroll 2
    for (int64_t t = 0; t < ntile; ++t) {
        const int64_t c_raw = t * 256 + tid;
        const int64_t c = c_raw < ldv ? c_raw : ldv - 1;
        const int64_t col = 4 * c;
        float4 av[RPB];
#pragma unroll
        for (int r = 0; r < RPB; ++r) av[r] = load_stream(reinterpret_cast<const float4*>(a0 + r * ld) + c);
        const double2 xa = x2[2 * c], xb = x2[2 * c + 1];
        const bool in = c_raw < ldv;
        const double x0 = sel(in && col + 0 < nvoxel, xa.x, 0.0);
        const double x1 = sel(in && col + 1 < nvoxel, xa.y, 0.0);
        const double x2v = sel(in && col + 2 < nvoxel, xb.x, 0.0);
        const double x3 = sel(in && col + 3 < nvoxel, xb.y, 0.0);
#pragma unroll
        for (int r = 0; r < RPB; ++r) {
            acc0[r] = fma((double)av[r].x, x0, acc0[r]);
            acc1[r] = fma((double)av[r].y, x1, acc1[r]);
            acc0[r] = fma((double)av[r].z, x2v, acc0[r]);
            acc1[r] = fma((double)av[r].w, x3, acc1[r]);
        }
    }

    const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
    for (int r = 0; r < RPB; ++r) {
        const double s = wave_sum(acc0[r] + acc1[r]);
        if (lane == 0) red[wid][r] = s;
    }
    __syncthreads();

    if (tid < 64) {
        double f2 = 0.0;
        if (tid < RPB) {
            const int64_t row = row0 + tid;
            const double f = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
            if (row < nrows) {
                if (out_f) out_f[row] = f;
                if (EPI == 1) out_w[row] = arow[row] * (g[row] - f);  // linear (CpuSolver::solve's sweep)
                if (EPI == 2) out_w[row] = arow[row] * f;             // log
                f2 = f * f;
            }
        }
        if (Fpart != nullptr) {
            f2 = wave_sum(f2);
            if (tid == 0) Fpart[blockIdx.x] = f2;
        }
    }
}

// out[0] = sum of v[0, n) in a fixed order (one workgroup): the second stage of the forward's sum f^2 partials
__global__ __launch_bounds__(256) void k_sum_f64(const double* __restrict__ v, int64_t n, double* __restrict__ out,
                                                 const SartState* __restrict__ st) {
    if (st != nullptr && st->done) return;
    __shared__ double red[4];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) acc += v[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Block (cb, s) owns 1024 columns (256 lanes x one 16-byte vector of A) and the rows of split s; partial[s][c] is
// written for every column of the padded row, also by a split that holds no row (zeros).
template <int UNR>
__global__ __launch_bounds__(256) void k_backproject64(const float* __restrict__ A, int64_t ld, int64_t nrows,
                                                       const double* __restrict__ w, int64_t rows_per_split,
                                                       double* __restrict__ partial,
                                                       const SartState* __restrict__ st) {
    if (st != nullptr && st->done) return;
    const int64_t cv = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t ldv = ld / 4;
    if (cv >= ldv) return;
    const int64_t r_begin = (int64_t)blockIdx.y * rows_per_split;
    int64_t r_end = r_begin + rows_per_split;
    if (r_end > nrows) r_end = nrows;

    double s0[4], s1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s0[j] = s1[j] = 0.0;

    const float4* __restrict__ a4 = reinterpret_cast<const float4*>(A) + cv;
    int64_t r = r_begin;
    for (; r + UNR <= r_end; r += UNR) {  // uniform over the workgroup
        float4 av[UNR];
        double wv[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) av[u] = load_stream(a4 + (r + u) * ldv);
#pragma unroll
        for (int u = 0; u < UNR; ++u) wv[u] = w[r + u];
#pragma unroll
        for (int u = 0; u < UNR; u += 2) {
            s0[0] = fma((double)av[u].x, wv[u], s0[0]);
            s0[1] = fma((double)av[u].y, wv[u], s0[1]);
            s0[2] = fma((double)av[u].z, wv[u], s0[2]);
            s0[3] = fma((double)av[u].w, wv[u], s0[3]);
            s1[0] = fma((double)av[u + 1].x, wv[u + 1], s1[0]);
            s1[1] = fma((double)av[u + 1].y, wv[u + 1], s1[1]);
            s1[2] = fma((double)av[u + 1].z, wv[u + 1], s1[2]);
            s1[3] = fma((double)av[u + 1].w, wv[u + 1], s1[3]);
        }
    }
    for (; r < r_end; ++r) {
        const float4 av = load_stream(a4 + r * ldv);
        const double wr = w[r];
        s0[0] = fma((double)av.x, wr, s0[0]);
        s0[1] = fma((double)av.y, wr, s0[1]);
        s0[2] = fma((double)av.z, wr, s0[2]);
        s0[3] = fma((double)av.w, wr, s0[3]);
    }
    double2* out = reinterpret_cast<double2*>(partial + (int64_t)blockIdx.y * ld + cv * 4);
    out[0] = make_double2(s0[0] + s1[0], s0[1] + s1[1]);
    out[1] = make_double2(s0[2] + s1[2], s0[3] + s1[3]);
}

// ---- element-wise kernels: the statements of CpuSolver::solve, which is compiled with contraction off ----

// x = valid ? src / rho_s : 0 (cold start) or src / div (warm start), then max(x, clamp) when clamp > 0;
// x[n, n_pad) = 0
__global__ __launch_bounds__(256) void k_init_x64(double* __restrict__ x, int64_t n, int64_t n_pad,
                                                  const double* __restrict__ src, const int32_t* __restrict__ valid,
                                                  const double* __restrict__ rho_s, double div, double clamp) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    double v = 0.0;
    if (i < n) {
        if (valid != nullptr)
            v = valid[i] ? src[i] / rho_s[i] : 0.0;
        else
            v = src[i] / div;
        if (clamp > 0) v = v < clamp ? clamp : v;  // std::max(v, clamp)
    }
    x[i] = v;
}

// v[i] = 0 where !valid[i] (the log solver's observed back-projection)
__global__ __launch_bounds__(256) void k_mask64(double* __restrict__ v, const int32_t* __restrict__ valid, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && !valid[i]) v[i] = 0.0;
}

template <bool LOGX>
__global__ __launch_bounds__(256) void k_penalty64(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                   const float* __restrict__ val, int64_t n, double beta,
                                                   const double* __restrict__ x, double* __restrict__ pen,
                                                   const SartState* __restrict__ st) {
#pragma clang fp contract(off)
    if (st != nullptr && st->done) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {  // CSR order
        const double xv = x[col[k]];
        s += (double)val[k] * (LOGX ? log(xv) : xv);
    }
    pen[i] = beta * s;
}

// Single lane: consumes sum f^2 of sweep s (the forward projection of the iterate after s updates) and decides as
// CpuSolver's loop does at its iteration s - 1. Sweep 0 is the start value's: no decision.
__global__ void k_decide64(SartState* __restrict__ st, const double* __restrict__ Fslot) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st->done) return;
    const int s = st->sweep;
    const double F = Fslot[0], G = st->G;
    st->F_last = F;
    int done = 0, status = kRunning;
    if (s >= 1) {
        const double conv = G != 0 ? (G - F) / G : 0.0;
        st->conv_last = conv;
        if (!isfinite(conv)) {
            st->flags |= 1;
            done = 1;
            status = kMaxIterationsExceeded;
        } else if (s >= 2 && fabs(conv - st->conv_prev) < st->tol) {
            done = 1;
            status = kSuccess;
        } else {
            st->conv_prev = conv;
        }
    }
    if (!done && s >= st->max_iter) {
        done = 1;
        status = kMaxIterationsExceeded;
    }
    st->iterations = done ? s : s + 1;
    st->sweep = s + 1;
    st->status = status;
    st->done = done;
}

// gpu_sem: max(x, 0) (the GPU path's clamp) instead of the reference CPU solver's signbit test
template <bool LOGV>
__global__ __launch_bounds__(256) void k_update64(double* __restrict__ x, const double* __restrict__ red,
                                                  const double* __restrict__ O, const double* __restrict__ pen,
                                                  const int32_t* __restrict__ valid, const double* __restrict__ rho_s,
                                                  double alpha, double eps, bool gpu_sem, int64_t n,
                                                  const SartState* __restrict__ st) {
#pragma clang fp contract(off)
    if (st->done) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double pn = pen != nullptr ? pen[i] : 0.0;
    if constexpr (LOGV) {
        const double Fv = valid[i] ? red[i] : 0.0;
        x[i] = x[i] * pow((O[i] + eps) / (Fv + eps), alpha) * exp(-pn);
    } else {
        const double d = (valid[i] ? alpha / rho_s[i] * red[i] : 0.0) - pn;
        const double xn = x[i] + d;
        x[i] = gpu_sem ? (xn < 0.0 ? 0.0 : xn) : (signbit(xn) ? 0.0 : xn);
    }
}

// ---------------------------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------------------------
static unsigned nb256(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + 255) / 256); }

void launch_forward64(int epi, const float* A, int64_t ld, int64_t nrows, int64_t nrows_pad, int64_t nvoxel,
                      const double* x, const double* g, const double* arow, double* out_f, double* out_w,
                      double* Fpart, const SartState* st, hipStream_t stream) {
    if (nrows_pad % kRpb64 != 0 || nrows_pad < nrows)
        throw std::runtime_error("forward64: padded row count must be a multiple of 8 covering the rows");
    if (ld % 64 != 0 || ld <= 0 || nvoxel > ld) throw std::runtime_error("forward64: ld must be a multiple of 64 >= nvoxel");
    if (epi != 0 && (!out_w || !arow || (epi == 1 && !g))) throw std::runtime_error("forward64: epilogue operands missing");
    const dim3 grid((unsigned)(nrows_pad / kRpb64));
    if (grid.x == 0) return;
    switch (epi) {
        case 0:
            hipLaunchKernelGGL(k_forward64<0>, grid, dim3(256), 0, stream, A, ld, nrows, nvoxel, x, g, arow, out_f,
                               out_w, Fpart, st);
            break;
        case 1:
            hipLaunchKernelGGL(k_forward64<1>, grid, dim3(256), 0, stream, A, ld, nrows, nvoxel, x, g, arow, out_f,
                               out_w, Fpart, st);
            break;
        case 2:
            hipLaunchKernelGGL(k_forward64<2>, grid, dim3(256), 0, stream, A, ld, nrows, nvoxel, x, g, arow, out_f,
                               out_w, Fpart, st);
            break;
        default:
            throw std::runtime_error("forward64: unknown epilogue");
    }
    check_launch("k_forward64");
}

void launch_sum_f64(const double* v, int64_t n, double* out, const SartState* st, hipStream_t stream) {
    hipLaunchKernelGGL(k_sum_f64, dim3(1), dim3(256), 0, stream, v, n, out, st);
    check_launch("k_sum_f64");
}

void launch_backproject64(const float* A, int64_t ld, int64_t nrows, const double* w, int nsplit, double* partial,
                          const SartState* st, hipStream_t stream) {
    if (ld % 64 != 0 || ld <= 0) throw std::runtime_error("backproject64: ld must be a multiple of 64");
    if (nsplit < 1 || nsplit > 65535) throw std::runtime_error("backproject64: nsplit must be within [1, 65535]");
    const int64_t ncb = (ld / 4 + 255) / 256;
    const int64_t rps = (std::max<int64_t>(nrows, 0) + nsplit - 1) / nsplit;
    hipLaunchKernelGGL((k_backproject64<8>), dim3((unsigned)ncb, (unsigned)nsplit), dim3(256), 0, stream, A, ld, nrows,
                       w, rps, partial, st);
    check_launch("k_backproject64");
}

void launch_init_x64(double* x, int64_t n, int64_t n_pad, const double* src, const int32_t* valid, const double* rho_s,
                     double div, double clamp, hipStream_t stream) {
    hipLaunchKernelGGL(k_init_x64, dim3(nb256(n_pad)), dim3(256), 0, stream, x, n, n_pad, src, valid, rho_s, div,
                       clamp);
    check_launch("k_init_x64");
}

void launch_mask64(double* v, const int32_t* valid, int64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(k_mask64, dim3(nb256(n)), dim3(256), 0, stream, v, valid, n);
    check_launch("k_mask64");
}

void launch_penalty64(bool logx, const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n, double beta,
                      const double* x, double* pen, const SartState* st, hipStream_t stream) {
    if (logx)
        hipLaunchKernelGGL(k_penalty64<true>, dim3(nb256(n)), dim3(256), 0, stream, row_ptr, col, val, n, beta, x, pen,
                           st);
    else
        hipLaunchKernelGGL(k_penalty64<false>, dim3(nb256(n)), dim3(256), 0, stream, row_ptr, col, val, n, beta, x, pen,
                           st);
    check_launch("k_penalty64");
}

void launch_decide64(SartState* st, const double* Fslot, hipStream_t stream) {
    hipLaunchKernelGGL(k_decide64, dim3(1), dim3(64), 0, stream, st, Fslot);
    check_launch("k_decide64");
}

void launch_update64(bool logmode, double* x, const double* red, const double* O, const double* pen,
                     const int32_t* valid, const double* rho_s, double alpha, double eps, bool gpu_semantics, int64_t n,
                     const SartState* st, hipStream_t stream) {
    if (!st) throw std::runtime_error("update64: state required");
    if (logmode)
        hipLaunchKernelGGL(k_update64<true>, dim3(nb256(n)), dim3(256), 0, stream, x, red, O, pen, valid, rho_s, alpha,
                           eps, gpu_semantics, n, st);
    else
        hipLaunchKernelGGL(k_update64<false>, dim3(nb256(n)), dim3(256), 0, stream, x, red, O, pen, valid, rho_s, alpha,
                           eps, gpu_semantics, n, st);
    check_launch("k_update64");
}

}  // namespace sart
