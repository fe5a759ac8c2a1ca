#include "fused_plan.hpp"

#include <cstdlib>
#include <stdexcept>
#include <string>

#include "fused_variants.hpp"

namespace sart {

namespace {
int g_fused_dbg = 0;    // diagnostics only (set through fused_set_debug)
int g_fused_sched = 4;  // variant 6 pipeline schedule (k_fused_sweep_rows SCHED)

const char* env(const char* name) {
    const char* e = std::getenv(name);
    return (e && *e) ? e : nullptr;
}
// Every message names the sweep: "fused_sweep v3: ", "fused_sweep v6: " (fp32), "fused_sweep bf16: ", "fused_sweep f16: "
[[noreturn]] void fail(const FusedKey& k, const char* what) {
    const std::string who = k.variant == 3 ? "v3" : (k.storage == RtmStorage::f32 ? "v6" : rtm_storage_name(k.storage));
    throw std::runtime_error("fused_sweep " + who + ": " + what);
}

const FusedKey kBuilt[] = {
#define X(...) fused_key(RtmStorage::f32, __VA_ARGS__),
    FUSED_F32_VARIANTS(X)
#undef X
#define X(K) fused_key_v3(K),
    FUSED_V3_VARIANTS(X)
#undef X
#define X(...) fused_key(RtmStorage::bf16, __VA_ARGS__),
    FUSED_BF16_VARIANTS(X)
#undef X
#define X(...) fused_key(RtmStorage::f16s, __VA_ARGS__),
    FUSED_F16_VARIANTS(X)
#undef X
};
}  // namespace

const char* rtm_storage_name(RtmStorage s) {
    return s == RtmStorage::f32 ? "f32" : (s == RtmStorage::bf16 ? "bf16" : "f16");
}
RtmStorage rtm_storage_from_name(const char* name) {
    for (RtmStorage s : {RtmStorage::f32, RtmStorage::bf16, RtmStorage::f16s})
        if (std::string(name) == rtm_storage_name(s)) return s;
    throw std::runtime_error(std::string("RTM storage must be f32, bf16 or f16, not '") + name + "'");
}

void fused_set_debug(int flags) { g_fused_dbg = flags; }
void fused_set_schedule(int sched) {
    if (sched < 0 || sched > 5) throw std::runtime_error("fused_set_schedule: 0 .. 5");
    g_fused_sched = sched;
}
int fused_get_schedule() { return g_fused_sched; }

FusedKnobs FusedKnobs::current() {
    FusedKnobs k;
    k.sched = g_fused_sched;
    k.debug = g_fused_dbg;
    if (const char* e = env("SART_FUSED_CW_SCHED")) k.cw_sched5 = std::atoi(e) == 5;
    if (const char* e = env("SART_BF16_T2_SCHED")) k.bf16_t2_sched6 = std::atoi(e) == 6;
    if (const char* e = env("SART_FUSED_GPAD")) k.gpad = std::atoi(e);
    if (const char* e = env("SART_FUSED_CW_MAP")) k.cw_map = std::atoi(e);
    return k;
}

bool fused_variant_built(const FusedKey& key) {
    for (const FusedKey& k : kBuilt)
        if (k == key) return true;
    return false;
}
std::vector<FusedKey> fused_variants(RtmStorage storage) {
    std::vector<FusedKey> out;
    for (const FusedKey& k : kBuilt)
        if (k.storage == storage) out.push_back(k);
    return out;
}

FusedPlan fused_plan(const FusedGeometry& g, RtmStorage storage, const FusedKnobs& knobs) {
    if (g.variant != 3 && g.variant != 6) throw std::runtime_error("fused_sweep: variant must be 6 or 3");
    const bool s16 = storage != RtmStorage::f32;
    FusedPlan p;
    FusedKey& k = p.key;
    p.dbg = knobs.debug;
    if (g.variant == 3) {
        k = fused_key_v3(g.K);
        if (s16) fail(k, "16-bit tiles run variant 6 only");
        if (g.K != 1 && g.K != 2 && g.K != 4 && g.K != 8) fail(k, "K must be 1, 2, 4 or 8");
        p.threads = kFusedThreads;
        p.lds_bytes = kLdsRingBytes;
        return p;
    }
    const int T = g.K, kw = g.kw, cpl = s16 ? g.cpl : 4;  // variant 6: K carries the rows per tile
    k = fused_key(storage, g.xl, false, T, 0, cpl, kw);
    if (T != 1 && T != 2 && T != 4) fail(k, s16 ? "rows per tile must be 1, 2 or 4" : "rows per tile (K) must be 1, 2 or 4");
    if (!s16) {
        if (kw < 5 || kw > 9) fail(k, "lane-vectors per lane (kw) must be 5 ... 9");
        if ((kw == 5 || kw == 9) && T != 1) fail(k, "5- and 9-KiB slabs need T = 1");  // (so chip-wide T >= 2: kw 6 ... 8)
        if (!g.xl) {
            // chip-wide row groups: T = 1 on schedule 5 (the split exchange, x slab in VGPRs), the 7- and 6-KiB slabs on
            // schedule 8, the deeper exchange pipeline (+5.3 % at 300000 voxels, +2.8 % at 530432,
            // profiles/ab_r3_cw_sched8.jsonl) unless SART_FUSED_CW_SCHED=5; T = 2 / 4 on schedule 4 (x slab in LDS)
            k.sched = T >= 2 ? 4 : (((kw == 7 || kw == 6) && !knobs.cw_sched5) ? 8 : 5);
        } else if (kw != 8) {
            k.sched = T >= 2 ? 4 : 5;  // other slab widths: the default schedules only, no diagnostics
        } else {
            // fused_set_schedule: schedules 1-4 hold the x slab in LDS, which has room for it only when T >= 2 (5 runs 4
            // there). T = 1 runs schedule 5 (the split exchange with the x slab in VGPRs) under the default schedule 4
            // (or 5): +10-14 % over schedule 0 at 73k-262k columns, with and without idle CUs
            // (profiles/probe_r2_t1_sched5.jsonl); schedules 0-3 select schedule 0 for T = 1.
            k.sched = T >= 2 ? (knobs.sched == 5 ? 4 : knobs.sched) : (knobs.sched >= 4 ? 5 : 0);
            k.diag = (knobs.debug & 2) != 0;  // the instrumented build only when asked: schedules 0, 2 and 4
            if (k.diag && k.sched != 2 && k.sched != 4) k.sched = 0;
        }
    } else {
        // 16-bit tiles. cpl 8 ("wide": 16-byte loads of 8 elements per lane, slab 2048 kw / T columns) needs T = 4
        // (schedule 4, x slab in LDS) or T = 2 (schedule 7: a 3-slot ring next to the two sub-slabs' x slab; schedule 6,
        // its 3-step-lag predecessor, with SART_BF16_T2_SCHED=6); cpl 4 ("narrow": 8-byte loads, slab 8192 / T) runs
        // schedule 4 for T >= 2 and for T = 1 schedule 0 with the deep 16-bit lag (or 5 when selected)
        if (cpl != 4 && !(cpl == 8 && (T == 4 || T == 2))) fail(k, "wide tiles need T = 4 or 2");
        if (kw != 8 && !(cpl == 8 && kw >= 5 && kw <= 7)) fail(k, "kw 5 ... 7 only with wide tiles (narrow tiles: kw 8)");
        if (!g.xl && cpl != 8) fail(k, "chip-wide row groups take the wide tiles only");
        if (cpl == 8)
            k.sched = T == 2 ? (knobs.bf16_t2_sched6 ? 6 : 7) : 4;
        else
            k.sched = T == 1 ? (knobs.sched == 5 ? 5 : 0) : 4;
    }
    p.split = sched_split(k.sched);
    p.threads = p.split ? kFusedThreads + 64 : kFusedThreads;
    p.lds_bytes = rows_lds_bytes(T, k.sched, cpl / 4, kw);
    // A/B runs: padded granule rows for XCD-local groups too; chip-wide groups: the group map (0 = b % I, 1 =
    // XCD-balanced, default: balanced for even I only) and unpadded granule rows
    if (g.xl && knobs.gpad == 2) p.dbg |= 32;
    if (!g.xl && (knobs.cw_map == 0 || (knobs.cw_map == 2 && g.I % 2 == 1))) p.dbg |= 8;
    if (!g.xl && knobs.gpad == 0) p.dbg |= 16;
    return p;
}

void fused_check_launch(const FusedPlan& p, int64_t ld, int64_t nrows_pad, int I, int J, int64_t chain_tiles,
                        bool has_xcnt) {
    const FusedKey& k = p.key;
    if (k.variant == 3) {
        const int K = k.T, T = 8 / K;
        if (ld % (1024 * K) != 0 || ld / (1024 * K) != J) fail(k, "ld must equal J * 1024 * K");
        if (nrows_pad % T != 0) fail(k, "padded rows must be a multiple of the tile");
        if (J * T > kMaxGather) fail(k, "too many slabs for the gather registers");
        return;
    }
    const bool s16 = k.storage != RtmStorage::f32;
    if (k.T >= 2 && chain_tiles % kChainAlign != 0) fail(k, "segment length must be a multiple of 140 tiles");
    const int64_t slab = 256 * (int64_t)k.cpl * k.kw / k.T;  // 4 / T sub-slabs of 64 lanes x kw lane-vectors x cpl columns
    if (ld % slab != 0 || ld / slab != J) fail(k, "ld must equal J * slab");
    if (nrows_pad % 4 != 0) fail(k, "padded rows must be a multiple of 4");
    if (s16 && (J * 4 > kMaxGather || J * k.T > kRowsGather)) fail(k, "too many slabs");
    if (!s16 && J * k.T > kRowsGather) fail(k, "J * T > 256");
    if (k.xl && (!has_xcnt || I % 8 != 0))
        fail(k, s16 ? "XCD-local groups need ticket counters and I % 8 == 0"
                    : "XCD-local groups need the per-XCD ticket counters and I % 8 == 0");
    if (I < 1) fail(k, "no row groups");
    if (fused_variant_built(k)) return;
    // the bf16 sweep's A/B schedules are not instantiated for f16 tiles
    if (k.storage == RtmStorage::f16s && k.sched == 6)
        fail(k, "schedule 6 (SART_BF16_T2_SCHED=6) is not built for f16 tiles; wide tiles at T = 2 run schedule 7");
    if (k.storage == RtmStorage::f16s && k.sched == 5)
        fail(k, "schedule 5 is not built for f16 tiles; narrow tiles at T = 1 run schedule 0");
    fail(k, "no kernel is built for this geometry and schedule (csrc/engine/fused_variants.hpp)");
}

}  // namespace sart
