// The kernel variants of the single-frame fused sweep: one list per RTM storage, one entry per instantiation of
// k_fused_sweep_rows (variant 6), X(XL, DIAG, T, SCHED, CPL, KW), plus the K of every k_fused_sweep_lds (variant 3).
// Every entry exists for both LOG values. The planner's table of built keys (fused_plan.cpp) and the kernel tables of
// fused_sweep.hip / fused_sweep_f16.hip are generated from these lists (keys: fused_key / fused_key_v3 in
// fused_plan.hpp, argument for argument).
//
// What is listed: every key fused_plan() returns for a geometry of fused_geometry() / fused_geometry_bf16_wide() under
// any setting of its knobs (fused_set_schedule, fused_set_debug, SART_FUSED_CW_SCHED, SART_BF16_T2_SCHED), except the
// bf16 A/B schedules on f16 tiles, which are refused at launch. To try another combination, add its line here (and
// the rule that selects it to fused_plan()): the static_asserts of k_fused_sweep_rows say what a kernel can be.
#pragma once

// fp32 tiles (CPL 4): 40 keys
#define FUSED_F32_VARIANTS(X) \
    /* chip-wide row groups, T = 1: schedule 5; 7- and 6-KiB slabs also the deeper schedule 8 (their default) */ \
    X(0, 0, 1, 5, 4, 8) X(0, 0, 1, 5, 4, 9) X(0, 0, 1, 5, 4, 5) \
    X(0, 0, 1, 8, 4, 7) X(0, 0, 1, 5, 4, 7) X(0, 0, 1, 8, 4, 6) X(0, 0, 1, 5, 4, 6) \
    /* chip-wide row groups, T = 2 / 4: schedule 4 */ \
    X(0, 0, 2, 4, 4, 8) X(0, 0, 2, 4, 4, 7) X(0, 0, 2, 4, 4, 6) X(0, 0, 4, 4, 4, 8) X(0, 0, 4, 4, 4, 7) X(0, 0, 4, 4, 4, 6) \
    /* XCD-local row groups, slabs other than 8 KiB: the default schedules only (5 at T = 1, 4 at T >= 2) */ \
    X(1, 0, 1, 5, 4, 9) X(1, 0, 1, 5, 4, 7) X(1, 0, 1, 5, 4, 6) X(1, 0, 1, 5, 4, 5) \
    X(1, 0, 2, 4, 4, 7) X(1, 0, 2, 4, 4, 6) X(1, 0, 4, 4, 4, 7) X(1, 0, 4, 4, 4, 6) \
    /* XCD-local row groups, 8-KiB slabs: every schedule of fused_set_schedule */ \
    X(1, 0, 2, 0, 4, 8) X(1, 0, 2, 1, 4, 8) X(1, 0, 2, 2, 4, 8) X(1, 0, 2, 3, 4, 8) X(1, 0, 2, 4, 4, 8) \
    X(1, 0, 4, 0, 4, 8) X(1, 0, 4, 1, 4, 8) X(1, 0, 4, 2, 4, 8) X(1, 0, 4, 3, 4, 8) X(1, 0, 4, 4, 4, 8) \
    X(1, 0, 1, 0, 4, 8) X(1, 0, 1, 5, 4, 8) \
    /* ... and the instrumented builds (fused_set_debug & 2): schedules 0, 2 and 4 */ \
    X(1, 1, 2, 0, 4, 8) X(1, 1, 2, 2, 4, 8) X(1, 1, 2, 4, 4, 8) X(1, 1, 4, 0, 4, 8) X(1, 1, 4, 2, 4, 8) X(1, 1, 4, 4, 4, 8) \
    X(1, 1, 1, 0, 4, 8)

// wide 16-bit tiles (CPL 8) of the default schedules: T = 4 on schedule 4, T = 2 on schedule 7, slabs of kw 8 ... 5,
// XCD-local and chip-wide row groups
#define FUSED_S16_WIDE_DEFAULTS(X) \
    X(1, 0, 4, 4, 8, 8) X(1, 0, 4, 4, 8, 7) X(1, 0, 4, 4, 8, 6) X(1, 0, 4, 4, 8, 5) \
    X(1, 0, 2, 7, 8, 8) X(1, 0, 2, 7, 8, 7) X(1, 0, 2, 7, 8, 6) X(1, 0, 2, 7, 8, 5) \
    X(0, 0, 4, 4, 8, 8) X(0, 0, 4, 4, 8, 7) X(0, 0, 4, 4, 8, 6) X(0, 0, 4, 4, 8, 5) \
    X(0, 0, 2, 7, 8, 8) X(0, 0, 2, 7, 8, 7) X(0, 0, 2, 7, 8, 6) X(0, 0, 2, 7, 8, 5)
// narrow 16-bit tiles (CPL 4) of the default schedules: 8-KiB-equivalent slabs, XCD-local row groups
#define FUSED_S16_NARROW_DEFAULTS(X) X(1, 0, 1, 0, 4, 8) X(1, 0, 2, 4, 4, 8) X(1, 0, 4, 4, 4, 8)

// bf16 tiles: 28 keys, the defaults and the A/B schedules (wide T = 2 on schedule 6: SART_BF16_T2_SCHED=6; narrow
// T = 1 on schedule 5: fused_set_schedule(5))
#define FUSED_BF16_VARIANTS(X) \
    FUSED_S16_WIDE_DEFAULTS(X) \
    X(1, 0, 2, 6, 8, 8) X(1, 0, 2, 6, 8, 7) X(1, 0, 2, 6, 8, 6) X(1, 0, 2, 6, 8, 5) \
    X(0, 0, 2, 6, 8, 8) X(0, 0, 2, 6, 8, 7) X(0, 0, 2, 6, 8, 6) X(0, 0, 2, 6, 8, 5) \
    FUSED_S16_NARROW_DEFAULTS(X) X(1, 0, 1, 5, 4, 8)

// row-scaled f16 tiles: 19 keys, the defaults only
#define FUSED_F16_VARIANTS(X) FUSED_S16_WIDE_DEFAULTS(X) FUSED_S16_NARROW_DEFAULTS(X)

// variant 3 (fp32): k_fused_sweep_lds<K>, slab 1024 K columns
#define FUSED_V3_VARIANTS(X) X(1) X(2) X(4) X(8)
