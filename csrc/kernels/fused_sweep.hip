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

static int g_fused_last_sched = -1;  // SCHED of the last k_fused_sweep_rows launch (variant 3: -1)
int fused_last_schedule() { return g_fused_last_sched; }

int64_t fused_granules(int64_t nrows_pad, int J, bool xl) {
    (void)xl;  // (XCD-local rows are padded too under SART_FUSED_GPAD=2)
    return nrows_pad * ((J + 15) & ~15);
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


template <int K>
static void launch_lds(bool logmode, dim3 grid, hipStream_t stream, const float* A, int64_t ld, int64_t nrows,
                       int64_t nrows_pad, const float* x, const float* ghat, const float* arow, float* partial,
                       double* Fpart, uint64_t* gran, int I, int J, SartState* st, int dbg) {
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
                           nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st, dbg);
    else
        hipLaunchKernelGGL((k_fused_sweep_lds<K, false>), grid, dim3(kFusedThreads), kLdsRingBytes, stream, A, ld,
                           nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st, dbg);
}

// The kernel tables, generated from engine/fused_variants.hpp (the f16 one: fused_sweep_f16.hip)
namespace {
const FusedVariant<float> kRowsF32[] = {
#define X(...) FUSED_ROWS_ENTRY(RtmStorage::f32, float, __VA_ARGS__)
    FUSED_F32_VARIANTS(X)
#undef X
};
const FusedVariant<bf16_t> kRowsBf16[] = {
#define X(...) FUSED_ROWS_ENTRY(RtmStorage::bf16, bf16_t, __VA_ARGS__)
    FUSED_BF16_VARIANTS(X)
#undef X
};
struct LdsVariant {
    FusedKey key;
    decltype(&launch_lds<8>) fn;
};
const LdsVariant kLds[] = {
#define X(K) {fused_key_v3(K), launch_lds<K>},
    FUSED_V3_VARIANTS(X)
#undef X
};
}  // namespace

// Variant 3 slab width: 1024 * K columns, K the smallest power of two <= 8 giving at most 32 slabs.
int fused_pick_k(int64_t ld) {
    for (int K = 1; K <= 8; K *= 2) {
        const int64_t wc = 1024 * (int64_t)K;
        if (ld % wc != 0) return K > 1 ? K / 2 : 0;
        if (ld / wc <= 32) return K;
    }
    return 8;
}

int fused_tile_rows(int K, int variant) {
    return variant == 6 ? K : 8 / K;  // variant 6: K carries the rows per tile; variant 3: 8 float4 per lane
}

// Variant 6 on the tiles of one storage type: the key's table entry, launched on the plan's debug bits
template <typename AT>
static void launch_rows(typename FusedVariant<AT>::Fn fn, const FusedPlan& p, const FusedArgs& a, hipStream_t stream) {
    fn(dim3((unsigned)(a.I * a.J)), stream, static_cast<const AT*>(a.A), a.ld, a.nrows, a.nrows_pad, a.x, a.ghat, a.arow,
       a.partial, a.Fpart, a.gran, a.I, a.J, a.st, a.xcnt, a.chain_tiles, a.rinv, p.dbg | (a.observed ? 64 : 0));
}

void launch_fused_sweep(const FusedPlan& p, const FusedArgs& a, bool logmode, hipStream_t stream) {
    const FusedKey& k = p.key;
    if (k.storage == RtmStorage::f16s) {
        if (a.observed && !logmode) throw std::runtime_error("fused_sweep f16: the observed sweep is a log-mode sweep");
        if (a.rinv == nullptr) throw std::runtime_error("fused_sweep f16: the rows' inverse scales are required");
    } else if (a.observed) {
        throw std::runtime_error("fused_sweep: the observed sweep exists for f16 tiles only");
    }
    fused_check_launch(p, a.ld, a.nrows_pad, a.I, a.J, a.chain_tiles, a.xcnt != nullptr);
    g_fused_last_sched = k.sched;
    if (k.variant == 3) {
        for (const LdsVariant& v : kLds)
            if (v.key == k)
                v.fn(logmode, dim3((unsigned)(a.I * a.J)), stream, static_cast<const float*>(a.A), a.ld, a.nrows,
                     a.nrows_pad, a.x, a.ghat, a.arow, a.partial, a.Fpart, a.gran, a.I, a.J, a.st, p.dbg);
        check_launch("k_fused_sweep_lds");
    } else if (k.storage == RtmStorage::f32) {
        launch_rows<float>(fused_variant(kRowsF32, k, logmode), p, a, stream);
        check_launch("k_fused_sweep_rows");
    } else if (k.storage == RtmStorage::bf16) {
        launch_rows<bf16_t>(fused_variant(kRowsBf16, k, logmode), p, a, stream);
        check_launch("k_fused_sweep_rows<bf16>");
    } else {
        launch_rows<f16s_t>(fused_variant_f16(k, logmode), p, a, stream);
        check_launch("k_fused_sweep_rows<f16>");
    }
}

}  // namespace sart

