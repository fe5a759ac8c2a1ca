// Fused single-pass SART sweep for gfx950: one HBM read of the local RTM shard per SART iteration.
//
// The reference streams A twice per iteration: PropagateKernel (A^T.w) and cublasSgemv (A.x)
// (reference sartsolver_cuda.cpp:239-249), i.e. 8*P*V bytes. Here every element of A is loaded into
// registers once and used for both products:
//
//   f_r  = sum_c A[r,c] x[c]              (forward projection, needs the whole row)
//   w_r  = a_r (ghat_r - f_r)   linear    (reference PropagateKernel weight, sart_kernels.cu:79-81)
//        = a_r f_r              log       (fitted half of LogPropagateKernel, sart_kernels.cu:134-146)
//   d_c += sum_r A[r,c] w_r               (back-projection)
//
// Decomposition: a persistent grid of I x J workgroups (<= one per CU, all co-resident).
// Workgroup (i, j) owns column slab j (Wc = 1024*K columns) of row group i and walks the row tiles
// (T = TK/K rows, TK float4 per lane) of its group. Per tile it computes the J-th part of each row dot
// and publishes it as an 8-byte {epoch, value} granule with one write-through (sc1) store -- the data
// IS the flag, no fences (cdna_hip_programming.md Guideline 16, recipe R2). A dedicated exchange wave
// gathers the J granules of a tile, sums them in a fixed lane-parallel tree (every workgroup of the
// group obtains a bitwise identical f_r), forms w_r and hands it to the four compute waves through
// LDS; they back-project that tile L steps after reducing it, from a ring of R tiles held in
// registers (tiles t-L .. t in use, t+1 .. t+R-L-1 in flight).
//
// Latency budget per step (one tile): the exchange wave issues the granule loads of tile t-L+2 in
// step t and consumes them in step t+1, so the memory round trip of the gather (2-3 us under full
// streaming load, MI355X_MICROARCH.md price list 'handoff-1to1') overlaps a whole step instead of
// sitting between two barriers.
//
// Correctness does not depend on workgroup placement or dispatch order: every wait is on data
// tagged with this sweep's epoch, every spin is bounded, and a timeout sets SartState::error so
// the host falls back to the two-pass kernels (no hang, no silent wrong answer).
#include "sart_common.hpp"
#include "launchers.hpp"
#include "fused_rows.hpp"

#include <cstdlib>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <vector>

namespace sart {

// ---------------------------------------------------------------------------------------------
// Variant 3 (fallback for widths variant 6 cannot split): in-flight tiles in registers, held tiles in LDS.
//
// Little's law sizing: at ~24.6 GB/s per CU (6.3 TB/s over 256 CUs) and a loaded HBM latency of
// 2-4 us a CU needs ~100 KB of loads in flight. Holding the L tiles that wait for their SART weights
// in registers (variants 0-2) leaves room for only ~2 tiles (64 KB) in flight and caps the sweep at
// ~4 TB/s (the removed variants 0-2). Here each compute wave keeps AH = 4 tiles (4 x 8 KB) of loads in flight in VGPRs; once a
// tile's row partials are reduced it is parked in an LDS ring (NL = L + 1 slots x 32 KB, each wave
// only touches its own 8 KB per slot, so no barrier guards the ring) and read back L steps later for
// the back-projection. 128 KB of loads in flight per CU, 128 KB of LDS.
// ---------------------------------------------------------------------------------------------
template <int K, bool LOG>
__global__ __launch_bounds__(kFusedThreads) void k_fused_sweep_lds(
    const float* __restrict__ A, int64_t ld, int64_t nrows, int64_t nrows_pad, const float* __restrict__ x,
    const float* __restrict__ ghat, const float* __restrict__ arow, float* __restrict__ partial,
    double* __restrict__ Fpart, uint64_t* __restrict__ gran, int I, int J, SartState* __restrict__ st, int dbg) {
    constexpr int TK = 8;       // float4 per lane per tile (8 KB per wave, 32 KB per workgroup)
    constexpr int T = TK / K;   // rows per tile
    constexpr int L = 3;        // back-projection lag (steps)
    constexpr int NL = L + 1;   // LDS ring slots
    constexpr int AH = 4;       // tiles in flight
    static_assert(T * K == TK, "tile must be whole rows");

    // all LDS in the one dynamic region (16-B aligned base, cdna_hip_programming.md Guideline 17):
    // [NL][4 waves][TK][64 lanes] float4 ring, then s_part[4][4][8] and s_w[4][8] floats
    extern __shared__ __attribute__((aligned(16))) float4 s_ring[];
    float(*s_part)[4][8] = reinterpret_cast<float(*)[4][8]>(s_ring + NL * 4 * TK * 64);
    float(*s_w)[8] = reinterpret_cast<float(*)[8]>(reinterpret_cast<float*>(s_ring + NL * 4 * TK * 64) + 128);

    if (st->done) return;
    const int epoch = st->epoch;

    const int b = blockIdx.x;
    const int gi = b % I;
    const int gj = b / I;
    const int64_t ntiles = nrows_pad / T;
    const int64_t t_begin = ntiles * gi / I;
    const int64_t nt = ntiles * (gi + 1) / I - t_begin;
    constexpr int UNR = 4;  // == AH (register slots are indexed statically)
    const int64_t nsteps = (nt + L + UNR - 1) / UNR * UNR;

    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int64_t ld4 = ld >> 2;

    if (wave < 4) {
        const int64_t col4 = (int64_t)gj * (256 * K) + wave * (64 * K) + lane;
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
        const float4* __restrict__ a4 = reinterpret_cast<const float4*>(A) + col4;
        float4* ring = s_ring + (wave * TK) * 64 + lane;  // + slot * (4 * TK * 64) + q * 64

        // Two-level back-projection sums like variant 6 at T = 1: a lane's chain would otherwise sum all nt * T rows of
        // its group (the chip-wide fallback at 512 x 524288: 1.29x the two-pass error); folded into acc2 every fpass
        // passes of UNR steps, ~sqrt(nt T) rows per chain
        float4 xs[K], acc[K], acc2[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            xs[k] = x4[col4 + k * 64];
            acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            acc2[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        int64_t fpass = (int64_t)__builtin_ceilf(__builtin_sqrtf((float)(nt * T)) / (float)(UNR * T));
        if (fpass < 1) fpass = 1;
        int64_t fcount = 0;
        float4 fl[AH][TK];
        const int64_t tlast = ntiles - 1 - t_begin;  // unconditional clamped loads: see k_fused_sweep_rows
        auto load_tile = [&](float4(&dst)[TK], int64_t t) {
            const float4* src = a4 + (t_begin + (t < tlast ? t : tlast)) * T * ld4;
#pragma unroll
            for (int r = 0; r < T; ++r)
#pragma unroll
                for (int k = 0; k < K; ++k) dst[r * K + k] = load_stream(src + r * ld4 + k * 64);
        };
#pragma unroll
        for (int i = 0; i < AH; ++i) load_tile(fl[i], i);

        auto step = [&](auto bbc, int64_t t) {
            constexpr int bb = decltype(bbc)::value;  // register slot of tile t (t % AH)
            if (t < nt) {
#pragma unroll
                for (int r = 0; r < T; ++r) {
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < K; ++k) s += dot4(fl[bb][r * K + k], xs[k]);
                    s = wave_sum(s);
                    if (lane == 0) s_part[t & 3][wave][r] = s;
                }
                float4* slot = ring + (int)(t % NL) * (4 * TK * 64);
#pragma unroll
                for (int q = 0; q < TK; ++q) slot[q * 64] = fl[bb][q];
            }
            load_tile(fl[bb], t + AH);
            __syncthreads();
            if (t >= L && t - L < nt) {
                const int64_t u = t - L;
                const float4* slot = ring + (int)(u % NL) * (4 * TK * 64);
                const int ws = (int)(u & 3);
#pragma unroll
                for (int r = 0; r < T; ++r) {
                    const float wr = s_w[ws][r];
#pragma unroll
                    for (int k = 0; k < K; ++k) fma4(acc[k], slot[(r * K + k) * 64], wr);
                }
            }
        };

        for (int64_t t0 = 0; t0 < nsteps; t0 += UNR) {
            step(std::integral_constant<int, 0>{}, t0 + 0);
            step(std::integral_constant<int, 1>{}, t0 + 1);
            step(std::integral_constant<int, 2>{}, t0 + 2);
            step(std::integral_constant<int, 3>{}, t0 + 3);
            if (++fcount == fpass) {  // registers only
                fcount = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    add4(acc2[k], acc[k]);
                    acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        }
        float4* out = reinterpret_cast<float4*>(partial + (int64_t)gi * ld) + col4;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            add4(acc[k], acc2[k]);
            out[k * 64] = acc[k];
        }
    } else {
        const int n = J * T;
        bool failed = false;
        double F = 0.0;
        uint64_t pv[2][kGatherRegs];

        // Polls are issued unconditionally at clamped addresses (tile in [0, ntiles), granule < n; lanes past
        // n re-read granule n - 1 and are masked when summing), so the compiler counts the polls in flight
        // instead of draining them (see load_tile in k_fused_sweep_rows).
        const int64_t ulast = ntiles - 1 - t_begin;
        auto issue_poll = [&](uint64_t(&dst)[kGatherRegs], int64_t u) {
            const int64_t uc = u < 0 ? 0 : (u < ulast ? u : ulast);
            const uint64_t* g = gran + (t_begin + uc) * (int64_t)n;
#pragma unroll
            for (int m = 0; m < kGatherRegs; ++m) {
                const int idx = lane + 64 * m;
                dst[m] = __hip_atomic_load(g + (idx < n ? idx : n - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        };
        auto finish_tile = [&](uint64_t(&v)[kGatherRegs], int64_t u) {
            if (!failed) {
                unsigned spins = 0;
                while (true) {
                    bool ok = true;
#pragma unroll
                    for (int m = 0; m < kGatherRegs; ++m) ok &= ((int)(v[m] >> 32) == epoch);
                    if (__all(ok)) break;
                    if (++spins > kSpinLimit) {
                        failed = true;
                        if (lane == 0) atomicOr(&st->error, 1);
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                    issue_poll(v, u);
                }
            }
            float s = 0.f;
            if (!failed) {
#pragma unroll
                for (int m = 0; m < kGatherRegs; ++m)
                    s += (lane + 64 * m < n) ? __uint_as_float((uint32_t)v[m]) : 0.f;
            }
#pragma unroll
            for (int off = T; off < 64; off <<= 1) s += __shfl_xor(s, off, kWave);
            if (lane < T) {
                const int64_t row = (t_begin + u) * T + lane;
                float w = 0.f;
                if (row < nrows) {
                    const float a = arow[row];
                    w = LOG ? a * s : a * (ghat[row] - s);
                    if (gj == 0) F += (double)s * (double)s;
                }
                s_w[u & 3][lane] = w;
            }
        };
        auto xstep = [&](auto pc, int64_t t) {
            constexpr int p = decltype(pc)::value;
            __syncthreads();
            if (dbg & 1) {  // ablation: no inter-workgroup exchange (timing diagnostics only)
                if (lane < T) s_w[(t + 1) & 3][lane] = 0.f;
                return;
            }
            if (t < nt && lane < T) {
                const int ps = (int)(t & 3);
                const float s = ((s_part[ps][0][lane] + s_part[ps][1][lane]) + s_part[ps][2][lane]) +
                                s_part[ps][3][lane];
                uint64_t* g = gran + ((t_begin + t) * J + gj) * T + lane;
                __hip_atomic_store(g, make_granule(epoch, s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const int64_t un = t - L + 2;
            issue_poll(pv[p], un);
            const int64_t uc = t - L + 1;
            if (uc >= 0 && uc < nt) finish_tile(pv[p ^ 1], uc);
        };
        for (int64_t t0 = 0; t0 < nsteps; t0 += 2) {
            xstep(std::integral_constant<int, 0>{}, t0);
            xstep(std::integral_constant<int, 1>{}, t0 + 1);
        }
        F = wave_sum(F);
        if (lane == 0) Fpart[b] = F;
    }
}

static int g_fused_dbg = 0;    // diagnostics only (set through fused_set_debug)
static int g_fused_sched = 4;  // variant 6 pipeline schedule (k_fused_sweep_rows SCHED)
void fused_set_debug(int flags) { g_fused_dbg = flags; }
int fused_debug_flags() { return g_fused_dbg; }
void fused_set_schedule(int sched) {
    if (sched < 0 || sched > 5) throw std::runtime_error("fused_set_schedule: 0 .. 5");
    g_fused_sched = sched;
}
int fused_get_schedule() { return g_fused_sched; }
static int g_fused_last_sched = -1;  // SCHED of the last k_fused_sweep_rows launch (variant 3: -1)
int fused_last_schedule() { return g_fused_last_sched; }
void fused_note_schedule(int sched) { g_fused_last_sched = sched; }

int64_t fused_granules(int64_t nrows_pad, int J, bool xl) {
    (void)xl;  // (XCD-local rows are padded too under SART_FUSED_GPAD=2)
    return nrows_pad * ((J + 15) & ~15);
}
bool fused_split_schedule(int T, bool bf16) {  // mirrors the schedule choice of launch_rows / launch_fused_sweep_bf16
    if (bf16) return T >= 2 || g_fused_sched == 5;
    return g_fused_sched >= 4;  // T = 1: 4 and 5 both run schedule 5; T >= 2: 5 runs 4
}
std::vector<int> fused_debug_map(int nblocks) {
    std::vector<int> out((size_t)nblocks);
    hip_call(hipMemcpyFromSymbol(out.data(), HIP_SYMBOL(g_fused_map), out.size() * sizeof(int), 0, hipMemcpyDeviceToHost), "hipMemcpyFromSymbol");
    return out;
}
void fused_set_trace(unsigned long long* buf, long long tiles) {
    hip_call(hipMemcpyToSymbol(HIP_SYMBOL(g_fused_trace), &buf, sizeof(buf), 0, hipMemcpyHostToDevice), "hipMemcpyToSymbol");
    hip_call(hipMemcpyToSymbol(HIP_SYMBOL(g_fused_trace_tiles), &tiles, sizeof(tiles), 0, hipMemcpyHostToDevice), "hipMemcpyToSymbol");
}
std::vector<unsigned long long> fused_debug_stats(int nblocks) {
    std::vector<unsigned long long> out((size_t)nblocks * 8);
    hip_call(hipMemcpyFromSymbol(out.data(), HIP_SYMBOL(g_fused_stats), out.size() * sizeof(unsigned long long), 0,
                        hipMemcpyDeviceToHost), "hipMemcpyFromSymbol");
    return out;
}


constexpr size_t kLdsRingBytes = 4 /*NL*/ * 4 /*waves*/ * 8 /*TK*/ * 64 * sizeof(float4) + 160 * sizeof(float);

template <int K>
static void launch_lds(bool logmode, dim3 grid, hipStream_t stream, const float* A, int64_t ld, int64_t nrows,
                       int64_t nrows_pad, const float* x, const float* ghat, const float* arow, float* partial,
                       double* Fpart, uint64_t* gran, int I, int J, SartState* st) {
    static bool configured = false;
    if (!configured) {  // opt in to > 64 KiB of dynamic LDS once per instantiation
        hip_call(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fused_sweep_lds<K, true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsRingBytes), "hipFuncSetAttribute");
        hip_call(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fused_sweep_lds<K, false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsRingBytes), "hipFuncSetAttribute");
        configured = true;
    }
    if (logmode)
        hipLaunchKernelGGL((k_fused_sweep_lds<K, true>), grid, dim3(kFusedThreads), kLdsRingBytes, stream, A, ld,
                           nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st, g_fused_dbg);
    else
        hipLaunchKernelGGL((k_fused_sweep_lds<K, false>), grid, dim3(kFusedThreads), kLdsRingBytes, stream, A, ld,
                           nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st, g_fused_dbg);
}

template <int T>
static void launch_rows(bool logmode, dim3 grid, hipStream_t stream, const float* A, int64_t ld, int64_t nrows,
                        int64_t nrows_pad, const float* x_, const float* ghat, const float* arow, float* partial,
                        double* Fpart, uint64_t* gran, int I, int J, SartState* st, unsigned* xcnt,
                        int64_t chain_tiles, int kw, bool xl) {
    if (!xl) {
        // chip-wide row groups (T = 1, schedule 5): workgroup b is (b % I, b / I), granules written through to
        // memory (agent scope), so a group may span XCDs: J up to the CU count, I = CUs / J of any value
        if constexpr (T == 1) {
            auto go_cw = [&](auto lg, auto k, auto sc) {
                launch_rows_t<decltype(lg)::value, false, false, 1, decltype(sc)::value, float, 4, decltype(k)::value>(
                    grid, stream, A, ld, nrows, nrows_pad, x_, ghat, arow, partial, Fpart, gran, I, J, st, xcnt,
                    chain_tiles);
            };
            // kw 6 / 7: schedule 8, the deeper exchange pipeline (+5.3 % at 300000 voxels, +2.8 % at 530432,
            // profiles/ab_r3_cw_sched8.jsonl); SART_FUSED_CW_SCHED=5 keeps schedule 5 (read per launch: A/B runs)
            const char* cws = std::getenv("SART_FUSED_CW_SCHED");
            const bool deep = !(cws && std::atoi(cws) == 5);
            using S5 = std::integral_constant<int, 5>;
            using S8 = std::integral_constant<int, 8>;
            auto by_kw = [&](auto lg) {
                if (kw == 8) go_cw(lg, std::integral_constant<int, 8>{}, S5{});
                else if (kw == 9) go_cw(lg, std::integral_constant<int, 9>{}, S5{});
                else if (kw == 7 && deep) go_cw(lg, std::integral_constant<int, 7>{}, S8{});
                else if (kw == 7) go_cw(lg, std::integral_constant<int, 7>{}, S5{});
                else if (kw == 6 && deep) go_cw(lg, std::integral_constant<int, 6>{}, S8{});
                else if (kw == 6) go_cw(lg, std::integral_constant<int, 6>{}, S5{});
                else go_cw(lg, std::integral_constant<int, 5>{}, S5{});
            };
            if (logmode) by_kw(std::true_type{}); else by_kw(std::false_type{});
            return;
        } else {
            // T = 2 / 4 (schedule 4, x slab in LDS): rows of more than an XCD's 32 slabs of 2048 / 4096 columns
            auto go_cw = [&](auto lg, auto k) {
                launch_rows_t<decltype(lg)::value, false, false, T, 4, float, 4, decltype(k)::value>(
                    grid, stream, A, ld, nrows, nrows_pad, x_, ghat, arow, partial, Fpart, gran, I, J, st, xcnt,
                    chain_tiles);
            };
            auto by_kw = [&](auto lg) {
                if (kw == 8) go_cw(lg, std::integral_constant<int, 8>{});
                else if (kw == 7) go_cw(lg, std::integral_constant<int, 7>{});
                else if (kw == 6) go_cw(lg, std::integral_constant<int, 6>{});
                else throw std::runtime_error("fused_sweep v6: chip-wide T >= 2 needs kw 6 ... 8");
            };
            if (logmode) by_kw(std::true_type{}); else by_kw(std::false_type{});
            return;
        }
    }
    const bool diag = (g_fused_dbg & 2) != 0;  // instrumented build only when asked (timing diagnostics)
    // g_fused_sched: pipeline schedule (k_fused_sweep_rows SCHED); schedules 1-4 hold the x slab in LDS,
    // which has room for it only when T >= 2. T = 1 runs schedule 5 (the split exchange with the x slab in
    // VGPRs) under the default schedule 4 (or 5): +10-14 % over schedule 0 at 73k-262k columns, with and
    // without idle CUs (profiles/probe_r2_t1_sched5.jsonl); schedules 0-3 select schedule 0 for T = 1.
    // Instrumented builds: schedules 0, 2 and 4.
    int sched = T >= 2 ? (g_fused_sched == 5 ? 4 : g_fused_sched) : (g_fused_sched >= 4 ? 5 : 0);
    if (diag && sched != 2 && sched != 4) sched = 0;
    auto go = [&](auto lg, auto d, auto sc) {
        launch_rows_t<decltype(lg)::value, true, decltype(d)::value, T, decltype(sc)::value>(
            grid, stream, A, ld, nrows, nrows_pad, x_, ghat, arow, partial, Fpart, gran, I, J, st, xcnt, chain_tiles);
    };
    using TT = std::true_type;
    using FF = std::false_type;
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, (T >= 2 ? 1 : 0)>;
    using S2 = std::integral_constant<int, (T >= 2 ? 2 : 0)>;
    using S3 = std::integral_constant<int, (T >= 2 ? 3 : 0)>;
    using S4 = std::integral_constant<int, (T >= 2 ? 4 : 0)>;
    using S5 = std::integral_constant<int, (T == 1 ? 5 : 4)>;
    auto by_log = [&](auto d, auto sc) {
        if (logmode) go(TT{}, d, sc); else go(FF{}, d, sc);
    };
    if (kw != 8) {  // narrower slabs: the default schedules only (4 at T >= 2, 5 at T = 1), no diagnostics
        auto go_kw = [&](auto lg, auto k) {
            using SD = std::integral_constant<int, (T >= 2 ? 4 : 5)>;
            launch_rows_t<decltype(lg)::value, true, false, T, SD::value, float, 4, decltype(k)::value>(
                grid, stream, A, ld, nrows, nrows_pad, x_, ghat, arow, partial, Fpart, gran, I, J, st, xcnt,
                chain_tiles);
        };
        auto by_kw = [&](auto lg) {
            if (kw == 7) go_kw(lg, std::integral_constant<int, 7>{});
            else if (kw == 6) go_kw(lg, std::integral_constant<int, 6>{});
            else if constexpr (T == 1) {
                if (kw == 9) go_kw(lg, std::integral_constant<int, 9>{});
                else go_kw(lg, std::integral_constant<int, 5>{});
            }
        };
        if (logmode) by_kw(TT{}); else by_kw(FF{});
        return;
    }
    if (diag) {
        if (sched == 2) by_log(TT{}, S2{});
        else if (sched == 4) by_log(TT{}, S4{});
        else by_log(TT{}, S0{});
        return;
    }
    switch (sched) {
        case 1: by_log(FF{}, S1{}); break;
        case 2: by_log(FF{}, S2{}); break;
        case 3: by_log(FF{}, S3{}); break;
        case 4: by_log(FF{}, S4{}); break;
        case 5: by_log(FF{}, S5{}); break;
        default: by_log(FF{}, S0{}); break;
    }
}

// Variant 3 slab width: 1024 * K columns, K the smallest power of two <= 8 giving at most 32 slabs.
int fused_pick_k(int64_t ld) {
    for (int K = 1; K <= 8; K *= 2) {
        const int64_t wc = 1024 * (int64_t)K;
        if (ld % wc != 0) return K > 1 ? K / 2 : 0;
        if (ld / wc <= 32) return K;
    }
    return 8;
}

int fused_fpart_per_block(int variant) {
    (void)variant;
    return 1;
}

int fused_tile_rows(int K, int variant) {
    return variant == 6 ? K : 8 / K;  // variant 6: K carries the rows per tile; variant 3: 8 float4 per lane
}

void launch_fused_sweep(bool logmode, int K, int variant, const float* A, int64_t ld, int64_t nrows,
                        int64_t nrows_pad, const float* x, const float* ghat, const float* arow, float* partial,
                        double* Fpart, uint64_t* gran, int I, int J, SartState* st, unsigned* xcnt,
                        hipStream_t stream, int64_t chain_tiles, int kw, bool xl) {
    if (variant != 3 && variant != 6) throw std::runtime_error("fused_sweep: variant must be 6 or 3");
    const dim3 grid((unsigned)(I * J));
    if (variant == 6) {
        const int T = K;
        if (T >= 2 && chain_tiles % kChainAlign != 0)
            throw std::runtime_error("fused_sweep v6: segment length must be a multiple of 140 tiles");
        if (T != 1 && T != 2 && T != 4) throw std::runtime_error("fused_sweep v6: rows per tile (K) must be 1, 2 or 4");
        if (kw < 5 || kw > 9) throw std::runtime_error("fused_sweep v6: lane-vectors per lane (kw) must be 5 ... 9");
        if ((kw == 5 || kw == 9) && T != 1) throw std::runtime_error("fused_sweep v6: 5- and 9-KiB slabs need T = 1");
        const int64_t slab = 1024 * kw / T;  // columns per workgroup
        if (ld % slab != 0 || ld / slab != J) throw std::runtime_error("fused_sweep v6: ld must equal J * slab");
        if (nrows_pad % 4 != 0) throw std::runtime_error("fused_sweep v6: padded rows must be a multiple of 4");
        if (J * T > kRowsGather) throw std::runtime_error("fused_sweep v6: J * T > 256");
        if (xl && (xcnt == nullptr || I % 8 != 0))
            throw std::runtime_error("fused_sweep v6: XCD-local groups need the per-XCD ticket counters and I % 8 == 0");
        if (!xl && T != 1 && (kw < 6 || kw > 8))
            throw std::runtime_error("fused_sweep v6: chip-wide row groups at T >= 2 need kw 6 ... 8");
        if (I < 1) throw std::runtime_error("fused_sweep v6: no row groups");
        if (T == 1) launch_rows<1>(logmode, grid, stream, A, ld, nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st, xcnt,
                        chain_tiles, kw, xl);
        else if (T == 2) launch_rows<2>(logmode, grid, stream, A, ld, nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st, xcnt,
                        chain_tiles, kw, xl);
        else launch_rows<4>(logmode, grid, stream, A, ld, nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st, xcnt,
                        chain_tiles, kw, xl);
        check_launch("k_fused_sweep_rows");
        return;
    }
    if (K != 1 && K != 2 && K != 4 && K != 8) throw std::runtime_error("fused_sweep v3: K must be 1, 2, 4 or 8");
    if (ld % (1024 * K) != 0 || ld / (1024 * K) != J) throw std::runtime_error("fused_sweep v3: ld must equal J * 1024 * K");
    const int T = 8 / K;
    if (nrows_pad % T != 0) throw std::runtime_error("fused_sweep v3: padded rows must be a multiple of the tile");
    if (J * T > kMaxGather) throw std::runtime_error("fused_sweep v3: too many slabs for the gather registers");
    g_fused_last_sched = -1;
    switch (K) {
        case 1: launch_lds<1>(logmode, grid, stream, A, ld, nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st); break;
        case 2: launch_lds<2>(logmode, grid, stream, A, ld, nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st); break;
        case 4: launch_lds<4>(logmode, grid, stream, A, ld, nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st); break;
        default: launch_lds<8>(logmode, grid, stream, A, ld, nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st); break;
    }
    check_launch("k_fused_sweep_lds");
}

// bf16-stored RTM: variant 6 only (XCD-local row groups, same exchange as fp32). cpl 8 ("wide": 16-byte loads of
// 8 bf16 per lane, slab 16384 / T columns) needs T = 4 (schedule 4, x slab in LDS) or T = 2 (schedule 6: a
// 3-slot ring next to the two sub-slabs' x slab); cpl 4 ("narrow": 8-byte
// loads, slab 8192 / T) runs schedule 4 for T >= 2 and for T = 1 schedule 0 with the deep bf16 lag (or 5 when
// selected). A protocol timeout falls back to the bf16 two-pass kernels.
void launch_fused_sweep_bf16(bool logmode, int T, const bf16_t* A, int64_t ld, int64_t nrows, int64_t nrows_pad,
                             const float* x, const float* ghat, const float* arow, float* partial, double* Fpart,
                             uint64_t* gran, int I, int J, SartState* st, unsigned* xcnt, hipStream_t stream, int cpl,
                             int64_t chain_tiles, int kw, bool xl) {
    if (T != 1 && T != 2 && T != 4) throw std::runtime_error("fused_sweep bf16: rows per tile must be 1, 2 or 4");
    if (cpl != 4 && !(cpl == 8 && (T == 4 || T == 2)))
        throw std::runtime_error("fused_sweep bf16: wide tiles need T = 4 or 2");
    if (kw != 8 && !(cpl == 8 && kw >= 5 && kw <= 7))
        throw std::runtime_error("fused_sweep bf16: kw 5 ... 7 only with wide tiles (narrow tiles: kw 8)");
    if (nrows_pad % 4 != 0) throw std::runtime_error("fused_sweep bf16: padded rows must be a multiple of 4");
    if (T >= 2 && chain_tiles % kChainAlign != 0)
        throw std::runtime_error("fused_sweep bf16: segment length must be a multiple of 140 tiles");
    const int64_t slab = 256 * (int64_t)cpl * kw / T;  // 4 / T sub-slabs of 64 lanes x kw lane-vectors x cpl columns
    if (ld % slab != 0 || ld / slab != J) throw std::runtime_error("fused_sweep bf16: ld must equal J * slab");
    if (J * 4 > kMaxGather || J * T > kRowsGather) throw std::runtime_error("fused_sweep bf16: too many slabs");
    if (xl && (xcnt == nullptr || I % 8 != 0))
        throw std::runtime_error("fused_sweep bf16: XCD-local groups need ticket counters and I % 8 == 0");
    if (!xl && cpl != 8) throw std::runtime_error("fused_sweep bf16: chip-wide row groups take the wide tiles only");
    if (I < 1) throw std::runtime_error("fused_sweep bf16: no row groups");
    const dim3 grid((unsigned)(I * J));
    // chip-wide row groups (xl false, wide tiles only): the fp32 chip-wide protocol (granules through memory in
    // padded rows, the XCD-balanced map) at T = 4 / 2, where a row of 32 wide slabs does not fit one XCD
    auto go = [&](auto lg, auto tt, auto sc, auto cp) {
        constexpr int TT = decltype(tt)::value, SC = decltype(sc)::value, CP = decltype(cp)::value;
        auto run = [&](auto k) {
            if constexpr (CP == 8) {
                if (!xl) {
                    launch_rows_t<decltype(lg)::value, false, false, TT, SC, bf16_t, CP, decltype(k)::value>(
                        grid, stream, A, ld, nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st, xcnt,
                        chain_tiles);
                    return;
                }
            }
            launch_rows_t<decltype(lg)::value, true, false, TT, SC, bf16_t, CP, decltype(k)::value>(
                grid, stream, A, ld, nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st, xcnt, chain_tiles);
        };
        if constexpr (CP == 8) {  // wide tiles: narrower slabs so that J fills an XCD's 32 CUs at more widths
            if (kw == 7) return run(std::integral_constant<int, 7>{});
            if (kw == 6) return run(std::integral_constant<int, 6>{});
            if (kw == 5) return run(std::integral_constant<int, 5>{});
        }
        run(std::integral_constant<int, 8>{});
    };
    using S0 = std::integral_constant<int, 0>;
    using S4 = std::integral_constant<int, 4>;
    using S5 = std::integral_constant<int, 5>;
    using S6 = std::integral_constant<int, 6>;
    using S7 = std::integral_constant<int, 7>;
    // wide tiles at T = 2: schedule 7 (L = 4) unless SART_BF16_T2_SCHED=6 (read per launch: tests switch it)
    const char* t2e = std::getenv("SART_BF16_T2_SCHED");
    const bool t2_sched6 = t2e && std::atoi(t2e) == 6;
    using C4 = std::integral_constant<int, 4>;
    using C8 = std::integral_constant<int, 8>;
    auto by_t = [&](auto lg) {
        if (cpl == 8 && T == 2 && t2_sched6) go(lg, std::integral_constant<int, 2>{}, S6{}, C8{});
        else if (cpl == 8 && T == 2) go(lg, std::integral_constant<int, 2>{}, S7{}, C8{});
        else if (cpl == 8) go(lg, std::integral_constant<int, 4>{}, S4{}, C8{});
        else if (T == 1 && g_fused_sched == 5) go(lg, std::integral_constant<int, 1>{}, S5{}, C4{});
        else if (T == 1) go(lg, std::integral_constant<int, 1>{}, S0{}, C4{});
        else if (T == 2) go(lg, std::integral_constant<int, 2>{}, S4{}, C4{});
        else go(lg, std::integral_constant<int, 4>{}, S4{}, C4{});
    };
    if (logmode) by_t(std::true_type{}); else by_t(std::false_type{});
    check_launch("k_fused_sweep_rows<bf16>");
}

}  // namespace sart
