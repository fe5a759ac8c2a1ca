// Launch plan of the single-frame fused sweep (kernels/fused_sweep.hip, fused_sweep_f16.hip): which kernel runs for a
// geometry, an RTM storage and the knobs as they are now. Plain host C++ (no HIP), like mf_plan: the engine sizes its
// partial rows from the plan it hands to launch_fused_sweep, and tests/test_fused_plan.py reads the rules on the CPU.
// fused_plan() computes a key even where no kernel is built for it (the bf16 A/B schedules on f16 tiles); looking it up
// at launch (fused_check_launch) is what throws, so an engine can be built under a knob it then refuses.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "geometry.hpp"

namespace sart {

enum class RtmStorage { f32, bf16, f16s };  // fp32, bf16, row-scaled f16 (f16s_t)
const char* rtm_storage_name(RtmStorage s);  // "f32", "bf16", "f16"
RtmStorage rtm_storage_from_name(const char* name);

constexpr int kFusedThreads = 320;  // 4 compute waves + 1 exchange wave
constexpr int kMaxGather = 512;     // J*T granules per tile
constexpr int kRowsGather = 256;    // J*T granules per tile, rows kernel (variant 6)
constexpr int64_t kChainAlign = 140;  // lcm of the register-slot counts RS (4, 5, 7) of the T >= 2 pipelines

// Schedules with a separate publisher wave (the split exchange): they may run their row groups in segments
constexpr bool sched_split(int sched) { return sched >= 4 && sched <= 8; }
// Dynamic LDS of k_fused_sweep_rows
constexpr size_t rows_lds_bytes(int T, int sched, int H = 1, int KW = 8) {
    return (sched == 6 || sched == 7 ? 3 : (sched == 8 ? 5 : 4)) /*NL x 4 waves x KW x 64 lanes x 16 B*/ * 4 * KW * 64 * 16 +
           (((sched >= 1 && sched <= 4) || sched == 6 || sched == 7) ? (4 / T) * KW * 64 * H * 16 : 0) +  // x slab
           (8 * 4 * 3 + 8 + 4) * sizeof(float);
}
// ... and of k_fused_sweep_lds (variant 3)
constexpr size_t kLdsRingBytes = 4 /*NL*/ * 4 /*waves*/ * 8 /*TK*/ * 64 * 16 + 160 * sizeof(float);

// Everything but the geometry that selects a kernel: the only reader of SART_FUSED_CW_SCHED, SART_BF16_T2_SCHED,
// SART_FUSED_GPAD and SART_FUSED_CW_MAP, and the home of the process-wide schedule and debug flags.
struct FusedKnobs {
    int sched = 4;                // fused_set_schedule: 0 .. 5 (fp32 XCD-local 8-KiB slabs; 5: also 16-bit narrow T = 1)
    int debug = 0;                // fused_set_debug: 1 no exchange, 2 instrumented build, 4 blockIdx map (diagnostics)
    bool cw_sched5 = false;       // SART_FUSED_CW_SCHED=5: chip-wide 7- / 6-KiB slabs at T = 1 keep schedule 5 (default 8)
    bool bf16_t2_sched6 = false;  // SART_BF16_T2_SCHED=6: wide 16-bit tiles at T = 2 on schedule 6 (default 7)
    int gpad = -1;                // SART_FUSED_GPAD: 0 unpadded granule rows (chip-wide), 2 padded (XCD-local); -1 unset
    int cw_map = 2;               // SART_FUSED_CW_MAP: 0 = b % I, 1 = XCD-balanced, 2 = balanced for even I only
    static FusedKnobs current();  // per launch: tools set the flags and tests the environment after a solver exists
};
void fused_set_schedule(int sched);
int fused_get_schedule();
void fused_set_debug(int flags);

// One kernel instantiation up to LOG (both LOG values exist for every key)
struct FusedKey {
    RtmStorage storage = RtmStorage::f32;
    int variant = 6;    // 6: k_fused_sweep_rows, 3: k_fused_sweep_lds
    bool xl = true;     // XCD-local row groups
    bool diag = false;  // instrumented build
    int T = 0;          // rows per tile (variant 3: K, the slab's 1024-column units)
    int sched = -1;     // pipeline schedule (variant 3: -1)
    int cpl = 4;        // columns per lane per k-slot
    int kw = 8;         // lane-vectors per lane per row
};
constexpr bool operator==(const FusedKey& a, const FusedKey& b) {
    return a.storage == b.storage && a.variant == b.variant && a.xl == b.xl && a.diag == b.diag && a.T == b.T &&
           a.sched == b.sched && a.cpl == b.cpl && a.kw == b.kw;
}
// Keys of the variant lists' entries (fused_variants.hpp), argument for argument
constexpr FusedKey fused_key(RtmStorage s, bool xl, bool diag, int T, int sched, int cpl, int kw) {
    return {s, 6, xl, diag, T, sched, cpl, kw};
}
constexpr FusedKey fused_key_v3(int K) { return {RtmStorage::f32, 3, false, false, K, -1, 4, 8}; }

struct FusedPlan {
    FusedKey key;
    bool split = false;    // the key's schedule is a split one: row groups may run in segments (fused_chain_plan)
    int threads = 0;       // per workgroup
    size_t lds_bytes = 0;  // dynamic LDS
    int dbg = 0;           // the kernel's dbg argument: FusedKnobs::debug and the map / granule padding bits
};
// Throws std::runtime_error for a geometry no kernel can take; never for a key that is merely not built.
FusedPlan fused_plan(const FusedGeometry& g, RtmStorage storage, const FusedKnobs& knobs);
bool fused_variant_built(const FusedKey& key);
std::vector<FusedKey> fused_variants(RtmStorage storage);  // the built keys of one storage
// What launch_fused_sweep checks before it starts a kernel: the shard, row groups and chain plan against the plan's
// key, then that the key's kernel is built. Throws std::runtime_error naming the storage.
void fused_check_launch(const FusedPlan& p, int64_t ld, int64_t nrows_pad, int I, int J, int64_t chain_tiles,
                        bool has_xcnt);

}  // namespace sart
