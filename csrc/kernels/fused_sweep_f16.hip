// Fused single-pass SART sweep on row-scaled f16 shards (f16s_t): the variant 6 kernel of fused_rows.hpp on f16
// tiles, in a translation unit of its own so that its instantiations compile next to the fp32 / bf16 ones of
// fused_sweep.hip instead of after them.
//
// Stored values are A[p][v] s_p with a power-of-two s_p per row (sart_common.hpp). The sweep works in that scaled
// domain wherever a value is only passed on (local partials, granules, hand-off words) and leaves it at the one place
// per row where a number is interpreted: the gatherer multiplies the finished row dot by 1 / s_p before it forms
// ||A x||^2 and the SART weight, and the weight by 1 / s_p once more because the back-projection meets A s_p again
// (k_forward's f16 epilogue, projection.hip). Both factors are powers of two, so the fused and the two-pass f16
// kernels differ in summation order only.
//
// Only the planner's defaults are built: wide tiles at T = 4 (schedule 4) and T = 2 (schedule 7) with slabs of
// kw 8 ... 5, XCD-local and chip-wide row groups; narrow tiles at kw 8, XCD-local, T = 1 (schedule 0) and
// T = 2 / 4 (schedule 4). The bf16 sweep's A/B variants (wide T = 2 on schedule 6, narrow T = 1 on schedule 5) are
// refused.
#include "fused_rows.hpp"

namespace sart {

void launch_fused_sweep_f16(bool logmode, int T, const f16s_t* A, int64_t ld, int64_t nrows, int64_t nrows_pad,
                            const float* x, const float* ghat, const float* arow, const float* rinv, float* partial,
                            double* Fpart, uint64_t* gran, int I, int J, SartState* st, unsigned* xcnt,
                            hipStream_t stream, int cpl, int64_t chain_tiles, int kw, bool xl, bool observed) {
    if (observed && !logmode) throw std::runtime_error("fused_sweep f16: the observed sweep is a log-mode sweep");
    if (rinv == nullptr) throw std::runtime_error("fused_sweep f16: the rows' inverse scales are required");
    if (T != 1 && T != 2 && T != 4) throw std::runtime_error("fused_sweep f16: rows per tile must be 1, 2 or 4");
    if (cpl != 4 && !(cpl == 8 && (T == 4 || T == 2)))
        throw std::runtime_error("fused_sweep f16: wide tiles need T = 4 or 2");
    if (kw != 8 && !(cpl == 8 && kw >= 5 && kw <= 7))
        throw std::runtime_error("fused_sweep f16: kw 5 ... 7 only with wide tiles (narrow tiles: kw 8)");
    if (nrows_pad % 4 != 0) throw std::runtime_error("fused_sweep f16: padded rows must be a multiple of 4");
    if (T >= 2 && chain_tiles % kChainAlign != 0)
        throw std::runtime_error("fused_sweep f16: segment length must be a multiple of 140 tiles");
    const int64_t slab = 256 * (int64_t)cpl * kw / T;  // 4 / T sub-slabs of 64 lanes x kw lane-vectors x cpl columns
    if (ld % slab != 0 || ld / slab != J) throw std::runtime_error("fused_sweep f16: ld must equal J * slab");
    if (J * 4 > kMaxGather || J * T > kRowsGather) throw std::runtime_error("fused_sweep f16: too many slabs");
    if (xl && (xcnt == nullptr || I % 8 != 0))
        throw std::runtime_error("fused_sweep f16: XCD-local groups need ticket counters and I % 8 == 0");
    if (!xl && cpl != 8) throw std::runtime_error("fused_sweep f16: chip-wide row groups take the wide tiles only");
    if (I < 1) throw std::runtime_error("fused_sweep f16: no row groups");
    // the bf16 sweep's A/B schedules are not instantiated for f16 tiles
    if (const char* t2e = std::getenv("SART_BF16_T2_SCHED"); cpl == 8 && T == 2 && t2e && std::atoi(t2e) == 6)
        throw std::runtime_error("fused_sweep f16: schedule 6 (SART_BF16_T2_SCHED=6) is not built for f16 tiles; "
                                 "wide tiles at T = 2 run schedule 7");
    if (cpl == 4 && T == 1 && fused_get_schedule() == 5)
        throw std::runtime_error("fused_sweep f16: schedule 5 is not built for f16 tiles; narrow tiles at T = 1 run "
                                 "schedule 0");
    const dim3 grid((unsigned)(I * J));
    auto go = [&](auto lg, auto tt, auto sc, auto cp) {
        constexpr int TT = decltype(tt)::value, SC = decltype(sc)::value, CP = decltype(cp)::value;
        auto run = [&](auto k) {
            if constexpr (CP == 8) {
                if (!xl) {  // chip-wide row groups: granules through memory in padded rows (wide tiles only)
                    launch_rows_t<decltype(lg)::value, false, false, TT, SC, f16s_t, CP, decltype(k)::value>(
                        grid, stream, A, ld, nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st, xcnt,
                        chain_tiles, rinv, observed ? 64 : 0);
                    return;
                }
            }
            launch_rows_t<decltype(lg)::value, true, false, TT, SC, f16s_t, CP, decltype(k)::value>(
                grid, stream, A, ld, nrows, nrows_pad, x, ghat, arow, partial, Fpart, gran, I, J, st, xcnt,
                chain_tiles, rinv, observed ? 64 : 0);
        };
        if constexpr (CP == 8) {
            if (kw == 7) return run(std::integral_constant<int, 7>{});
            if (kw == 6) return run(std::integral_constant<int, 6>{});
            if (kw == 5) return run(std::integral_constant<int, 5>{});
        }
        run(std::integral_constant<int, 8>{});
    };
    using S0 = std::integral_constant<int, 0>;
    using S4 = std::integral_constant<int, 4>;
    using S7 = std::integral_constant<int, 7>;
    using C4 = std::integral_constant<int, 4>;
    using C8 = std::integral_constant<int, 8>;
    auto by_t = [&](auto lg) {
        if (cpl == 8 && T == 2) go(lg, std::integral_constant<int, 2>{}, S7{}, C8{});
        else if (cpl == 8) go(lg, std::integral_constant<int, 4>{}, S4{}, C8{});
        else if (T == 1) go(lg, std::integral_constant<int, 1>{}, S0{}, C4{});
        else if (T == 2) go(lg, std::integral_constant<int, 2>{}, S4{}, C4{});
        else go(lg, std::integral_constant<int, 4>{}, S4{}, C4{});
    };
    if (logmode) by_t(std::true_type{}); else by_t(std::false_type{});
    check_launch("k_fused_sweep_rows<f16>");
}

}  // namespace sart
