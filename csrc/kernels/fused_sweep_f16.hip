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
// Only the planner's defaults are built (FUSED_F16_VARIANTS, engine/fused_variants.hpp): wide tiles at T = 4
// (schedule 4) and T = 2 (schedule 7) with slabs of kw 8 ... 5, XCD-local and chip-wide row groups; narrow tiles at
// kw 8, XCD-local, T = 1 (schedule 0) and T = 2 / 4 (schedule 4). The bf16 sweep's A/B variants (wide T = 2 on
// schedule 6, narrow T = 1 on schedule 5) are refused (fused_check_launch).
#include "fused_rows.hpp"

namespace sart {

namespace {
const FusedVariant<f16s_t> kRowsF16[] = {
#define X(...) FUSED_ROWS_ENTRY(RtmStorage::f16s, f16s_t, __VA_ARGS__)
    FUSED_F16_VARIANTS(X)
#undef X
};
}  // namespace

FusedVariant<f16s_t>::Fn fused_variant_f16(const FusedKey& key, bool logmode) {
    return fused_variant(kRowsF16, key, logmode);
}

}  // namespace sart
