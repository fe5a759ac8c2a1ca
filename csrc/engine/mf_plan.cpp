#include "mf_plan.hpp"

#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "mf_variants.hpp"

namespace sart {

namespace {
int g_set_depth = 0, g_set_rows = 0, g_set_vox = 0;

const char* env(const char* name) {
    const char* e = std::getenv(name);
    return (e && *e) ? e : nullptr;
}
int env_int(const char* name, int dflt) {
    const char* e = env(name);
    return e ? std::atoi(e) : dflt;
}
// "RT,KB[,lds][,as]"; KB defaults to 1; a tile outside rts x {1, 2} is ignored
MfTile env_tile(const char* name, std::initializer_list<int> rts, bool always_lds) {
    const char* e = env(name);
    if (!e) return {};
    const char* c = std::strchr(e, ',');
    MfTile t{std::atoi(e), c ? std::atoi(c + 1) : 1, always_lds || std::strstr(e, "lds") != nullptr,
             std::strstr(e, "as") != nullptr};
    bool ok = false;
    for (int r : rts) ok = ok || t.rt == r;
    return (ok && (t.kb == 1 || t.kb == 2)) ? t : MfTile{};
}
int one_of(int v, int lo, int hi) { return (v >= lo && v <= hi) ? v : 0; }
}  // namespace

void mf_set_depth(int d) { g_set_depth = d; }
void mf_set_rows(int rt) { g_set_rows = rt; }
void mf_set_vox(int vt) { g_set_vox = vt; }

MfKnobs MfKnobs::from_env() {
    MfKnobs k;
    k.depth = one_of(g_set_depth ? g_set_depth : env_int("SART_MF_DEPTH", 0), 1, 3);
    const int rows = g_set_rows ? g_set_rows : env_int("SART_MF_ROWS", 0);
    k.rows = (rows == 2 || rows == 4) ? rows : 0;
    k.vox = one_of(g_set_vox ? g_set_vox : env_int("SART_MF_VOX", 0), 1, 2);
    k.nt = env_int("SART_MF_NT", 0) == 1;
    k.b16_fwd = env_tile("SART_MF_B16_FWD", {2, 4, 8}, false);
    if (const char* e = env("SART_MF_B16_VT")) {
        k.b16_vt = one_of(std::atoi(e), 1, 2);
        k.b16_w_lds = std::strstr(e, "lds") ? 1 : (std::strstr(e, "reg") ? 0 : -1);
    }
    k.x3_fwd = env_tile("SART_MF_X3_FWD", {2, 4}, true);
    k.x3_depth = one_of(env_int("SART_MF_X3_DEPTH", 0), 2, 3);
    k.x3_vt = one_of(env_int("SART_MF_X3_VT", 0), 1, 2);
    if (const char* e = env("SART_MF_XEARLY")) k.xearly = std::atoi(e) != 0;
    if (const char* e = env("SART_MF_WEARLY")) k.wearly = std::atoi(e) != 0;
    if (const char* e = env("SART_MF_H16")) {
        k.h16_ew = std::strstr(e, "ew") != nullptr;
        k.h16_w1 = std::strstr(e, "w1") != nullptr;
    }
    k.h16_fdepth3 = env_int("SART_MF_H16_FDEPTH", 2) == 3;
    if (const char* e = env("SART_MF_FWD_BLOCKS")) k.fwd_blocks = std::atoll(e);
    if (const char* e = env("SART_MF_BP_BLOCKS")) k.bp_blocks = std::atoll(e);
    return k;
}

static std::string tile_str(const MfTile& t, bool with_lds) {
    return std::to_string(t.rt) + "," + std::to_string(t.kb) + (with_lds && t.lds ? ",lds" : "") + (t.as ? ",as" : "");
}

std::string MfKnobs::describe() const {
    std::string s;
    auto add = [&](const char* name, const std::string& v) { s += (s.empty() ? "" : " ") + std::string(name) + "=" + v; };
    if (depth) add("SART_MF_DEPTH", std::to_string(depth));
    if (rows) add("SART_MF_ROWS", std::to_string(rows));
    if (vox) add("SART_MF_VOX", std::to_string(vox));
    if (nt) add("SART_MF_NT", "1");
    if (b16_fwd.rt) add("SART_MF_B16_FWD", tile_str(b16_fwd, true));
    if (b16_vt || b16_w_lds >= 0)
        add("SART_MF_B16_VT", (b16_vt ? std::to_string(b16_vt) : std::string()) +
                                  (b16_w_lds < 0 ? "" : (b16_w_lds ? ",lds" : ",reg")));
    if (x3_fwd.rt) add("SART_MF_X3_FWD", tile_str(x3_fwd, false));
    if (x3_depth) add("SART_MF_X3_DEPTH", std::to_string(x3_depth));
    if (x3_vt) add("SART_MF_X3_VT", std::to_string(x3_vt));
    if (xearly >= 0) add("SART_MF_XEARLY", std::to_string(xearly));
    if (wearly >= 0) add("SART_MF_WEARLY", std::to_string(wearly));
    if (h16_ew || h16_w1) add("SART_MF_H16", std::string(h16_ew ? "ew" : "") + (h16_ew && h16_w1 ? "," : "") + (h16_w1 ? "w1" : ""));
    if (h16_fdepth3) add("SART_MF_H16_FDEPTH", "3");
    if (fwd_blocks) add("SART_MF_FWD_BLOCKS", std::to_string(*fwd_blocks));
    if (bp_blocks) add("SART_MF_BP_BLOCKS", std::to_string(*bp_blocks));
    return s.empty() ? "defaults" : s;
}

const char* mf_path_name(MfPath p) {
    switch (p) {
        case MfPath::fp32: return "fp32";
        case MfPath::b16: return "b16";
        case MfPath::x3: return "x3";
        case MfPath::s16: return "s16";
        default: return "h16";
    }
}

MfPath mf_path_from_name(const std::string& name) {
    for (MfPath p : {MfPath::fp32, MfPath::b16, MfPath::x3, MfPath::h16, MfPath::s16})
        if (name == mf_path_name(p)) return p;
    throw std::runtime_error("multi-frame path must be fp32, b16, x3, h16 or s16, not '" + name + "'");
}

// ------------------------------------------------------------------ the table of supported keys
namespace {
const MfKey kVariants[] = {
#define X(...) mf_key_fwd_f32(__VA_ARGS__),
    MF_FWD_F32_VARIANTS(X)
#undef X
#define X(...) mf_key_fwd_b16(__VA_ARGS__),
    MF_FWD_B16_VARIANTS(X)
#undef X
#define X(...) mf_key_fwd_a32(__VA_ARGS__),
    MF_FWD_A32_VARIANTS(X)
#undef X
#define X(...) mf_key_fwd_s16(__VA_ARGS__),
    MF_FWD_S16_VARIANTS(X)
#undef X
#define X(...) mf_key_bwd_s16(__VA_ARGS__),
    MF_BWD_S16_VARIANTS(X)
#undef X
#define X(...) mf_key_bwd_f32(__VA_ARGS__),
    MF_BWD_F32_VARIANTS(X)
#undef X
#define X(...) mf_key_bwd_b16(__VA_ARGS__),
    MF_BWD_B16_VARIANTS(X)
#undef X
#define X(...) mf_key_bwd_x3(__VA_ARGS__),
    MF_BWD_X3_VARIANTS(X)
#undef X
#define X(...) mf_key_bwd_h16(__VA_ARGS__),
    MF_BWD_H16_VARIANTS(X)
#undef X
};

std::string key_str(const MfKey& k) {
    return std::string(mf_path_name(k.path)) + (k.forward ? " forward" : " back-projection") + " NG=" +
           std::to_string(k.ng) + " depth=" + std::to_string(k.depth) + (k.forward ? " RT=" : " VT=") +
           std::to_string(k.tile) + (k.forward && k.path != MfPath::fp32 ? " KB=" + std::to_string(k.kb) : "") +
           (k.lds ? " lds" : "") + (k.as ? " as" : "") + (k.early ? " early" : "") + (k.nt ? " nt" : "") +
           (k.mw ? " MW=" + std::to_string(k.mw) : "");
}

void require_variant(const MfKey& key, const MfKnobs& k) {
    if (!mf_variant_supported(key))
        throw std::runtime_error("multi-frame " + std::string(mf_path_name(key.path)) + " path: no kernel for " +
                                 k.describe() + " (" + key_str(key) + " is not in the variant table)");
}

// 128 frames (8 column groups): the split-A forward, the bf16-storage kernels and the f16-pair back-projection
void check_nf(int nf, const std::string& what, bool with128) {
    if (nf == 128 && with128) return;
    if (nf != 16 && nf != 32 && nf != 64)
        throw std::runtime_error(what + (with128 ? ": nf must be 16, 32, 64 or 128" : ": nf must be 16, 32 or 64"));
}

int clamp_splits(int64_t target, int64_t nblk, int64_t smax) {
    int64_t s = (target + nblk - 1) / nblk;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    return (int)s;
}

// ---- fp32 MFMA kernels (multiframe.hip)
// Register-ring depth (steps of loads in flight per wave). Defaults per kernel and batch width from
// tools/probe_mf.py on 64k x 64k (profiles/probe_r1_mf_tiles.jsonl, with the default tilings below: forward
// 64 rows per wave, back-projection 64 voxels per wave at nf = 16 and 128 at nf = 32 / 64)
int f32_depth(const MfKnobs& k, bool forward, int nf) {
    if (k.depth) return k.depth;
    if (forward) return nf == 64 ? 2 : 3;  // with 64-row waves (profiles/probe_r1_mf_tiles.jsonl)
    return nf == 32 ? 1 : 2;               // nf 16: 64-voxel waves; nf 32 / 64: 128-voxel waves
}
// 64-voxel tiles per wave of the back-projection: 1 or 2 (ld % 128 == 0)
int f32_vox(const MfKnobs& k, int64_t ld, int nf) {
    const int vt = k.vox ? k.vox : (nf >= 32 ? 2 : 1);
    return (vt == 2 && ld % 128 == 0) ? 2 : 1;
}
// Row tiles per wave of the forward kernel: 2 (32 rows) or 4 (64 rows)
int f32_rows(const MfKnobs& k) { return k.rows ? k.rows : 4; }

// Split-K of the forward projection: >= ~1024 workgroups, >= 1024 columns per split. (Splitting further
// so that a split's X chunk stays L2-resident measured 0-9 % slower at nf = 16..64, 64k x 64k.)
int fwd_splits(const MfKnobs& k, int64_t ld, int64_t nrows_pad, int target_blocks) {
    const int64_t rows_per_block = (nrows_pad % 64 == 0 ? f32_rows(k) : 2) * 64;  // 4 waves x 16 * rt rows
    const int64_t nblk = (nrows_pad + rows_per_block - 1) / rows_per_block;
    const int64_t target = k.fwd_blocks ? *k.fwd_blocks : (target_blocks > 0 ? target_blocks : 1024);
    return clamp_splits(target, nblk, ld / 1024);
}

// Split-K of the back-projection: ~512 workgroups. The kernel time is flat from 4 to 32 splits at
// 64k x 64k (profiles/probe_r1_mf_splits.jsonl) while k_mf_collect reads nsplit partial slices.
int bwd_f32_splits(const MfKnobs& k, int64_t ld, int64_t nrows) {
    const int64_t nblk = (ld / (64 * f32_vox(k, ld, 64)) + 3) / 4;  // the fp32 kernels' widest batch
    // 2048 (4 x the 512 of round 1): a split's rows are one fp32 MFMA accumulation chain; 16k-row splits at 64k x 64k
    // were the larger share of the multi-frame engine's error against the fp32 two-pass kernels
    // (profiles/parity_r6_64k_mf_chains.jsonl); the extra partial slices cost k_mf_collect ~1.5 % of a sweep
    return clamp_splits(k.bp_blocks ? *k.bp_blocks : 2048, nblk, (nrows + 63) / 64);
}

// ---- bf16-storage kernels (multiframe_bf16.hip; tools/probe_mf_b16.py). Defaults from the probe at 64k x 64k
// (profiles/probe_r2_mf_b16.jsonl).
int b16_depth(const MfKnobs& k) { return k.depth ? k.depth : 3; }  // profiles/probe_r2_mf_b16_bwd.jsonl
MfTile b16_fwd_tile(const MfKnobs& k, int nf) {
    if (k.b16_fwd.rt) return k.b16_fwd;
    // profiles/probe_r2_mf_b16_lds.jsonl, profiles/probe_r2_mf_as.jsonl (A staged: +9 % at 32 frames, a tie at 16 / 64)
    if (nf == 32) return MfTile{2, 2, true, true};
    return nf == 16 ? MfTile{2, 2, true} : MfTile{4, 2, true};
}
int b16_vt(const MfKnobs& k, int64_t ld, int nf) {
    if (nf == 128) return 1;  // 8 column groups: one 64-voxel tile per wave
    const int vt = k.b16_vt ? k.b16_vt : 2;
    return (vt == 2 && ld % 128 == 0) ? 2 : 1;
}

// ---- split-A kernels (fp32 A on the 16-bit matrix cores; tools/probe_mf_x3.py). Twice the bytes of A per fragment
// as bf16 storage, so smaller register tiles.
MfTile x3_fwd_tile(const MfKnobs& k, int nf, int64_t ld) {
    if (k.x3_fwd.rt) return k.x3_fwd;
    // profiles/probe_r2_mf_x3.jsonl, profiles/probe_r2_mf_as.jsonl; with blocked X planes (round 4,
    // profiles/probe_r4_mf_x3_fwd_tiles_xblk.jsonl) 64 frames on rows of >= 128k columns take two 32-voxel blocks per
    // step (16384 x 262144: 3.08 against 3.21 ms; 64k x 64k: 2.96 against 2.90, so narrower rows keep one)
    // 32 frames take the A-staged tile too since its loads are non-temporal (+3.2 % at 64k x 64k,
    // profiles/ab_r5_mf32_as.txt)
    if (nf == 64 || nf == 32) return ld >= 131072 ? MfTile{2, 2, true, true} : MfTile{2, 1, true, true};
    if (nf == 128) return MfTile{2, 1, true, true};  // 128 frames: one 32-voxel block per step (registers)
    return MfTile{2, 2, true};
}
// the forward's ring: 2 steps ahead on blocked X planes (64k x 64k: 2.90 against 2.98 ms at 3, 16384 x 262144
// equal; profiles/probe_r4_mf_x3_fwd_tiles_xblk.jsonl)
int x3_depth(const MfKnobs& k) { return k.x3_depth ? k.x3_depth : 2; }
int x3_vt(const MfKnobs& k, int64_t ld) {
    const int vt = k.x3_vt ? k.x3_vt : 1;
    return (vt == 2 && ld % 128 == 0) ? 2 : 1;
}

// Split-K of the bf16 / split-A back-projection: ~1024 workgroups (4 waves x 64 VT voxels each), >= 64 rows per
// split. The voxel tile is the path's widest (bf16 storage: not the 128-frame kernel's single tile), as is the
// alignment of the engine's voxel chunks below: a multiple of every kernel's tile on the path.
int split_vt(const MfKnobs& k, int64_t ld, bool a32) { return a32 ? x3_vt(k, ld) : b16_vt(k, ld, 0); }
int bwd_b16_splits(const MfKnobs& k, int64_t ld, int64_t nrows, bool a32) {
    const int64_t nblk = (ld / (64 * split_vt(k, ld, a32)) + 3) / 4;
    // bf16 storage: ~512 (fewer partial slices for k_mf_collect: +1.3 % with 512-block forwards at 64 frames,
    // profiles/ab_r4_mf_split_blocks_low.jsonl); split-A ~1024 (256: -5 %)
    // x 4 in round 6 (split-A 4096, bf16 storage 2048): each split's rows are one fp32 MFMA accumulation chain, the
    // larger share of the engine's error against the fp32 two-pass kernels at 64k x 64k (16k-row chains;
    // profiles/parity_r6_64k_mf_chains.jsonl)
    // (split-A with the LDS two-level sums of k_mf_backproject_h16: back to ~1024, chains of 12 steps)
    const int64_t target = k.bp_blocks ? *k.bp_blocks : (a32 ? (SART_MF_BWD_FLUSH > 0 ? 1024 : 4096) : 2048);
    return clamp_splits(target, nblk, (nrows + 63) / 64);
}

// Row-scaled f16 storage runs the bf16-storage kernels (same bytes, same tiles): its key is the bf16-storage key of
// the same shape and knobs under its own path. Its variant lists hold the default keys only, so a knob that moves
// the bf16-storage key elsewhere throws in require_variant.
MfKey as_s16(MfKey k) {
    k.path = MfPath::s16;
    return k;
}

MfKey fwd_key(MfPath path, int nf, int64_t ld, int64_t nrows_pad, const MfKnobs& k) {
    const int ng = nf / 16;
    if (path == MfPath::s16) return as_s16(fwd_key(MfPath::b16, nf, ld, nrows_pad, k));
    if (path == MfPath::fp32) {
        const int rt = (nrows_pad % 64 == 0) ? f32_rows(k) : 2;  // a wave's 16 * rt rows lie inside the padding
        return mf_key_fwd_f32(ng, f32_depth(k, true, nf), rt, k.nt);
    }
    if (path == MfPath::h16) {
        // The f16-pair split-A forward (default for fp32 shards at 32 / 64 / 128 frames): the x3 tilings with RT = 2
        // and a ring two steps deep, X loaded early. SART_MF_H16_FDEPTH=3: a register ring three steps deep for the
        // A-staged tilings (A/B runs)
        MfTile tl = x3_fwd_tile(k, nf, ld);
        if (nf == 128) tl.as = true;
        return mf_key_fwd_a32(true, ng, tl.as && k.h16_fdepth3 ? 3 : 2, 2, tl.kb, tl.as, true);
    }
    const bool a32 = path == MfPath::x3;
    MfTile tl = a32 ? x3_fwd_tile(k, nf, ld) : b16_fwd_tile(k, nf);
    if (nrows_pad % (16 * tl.rt) != 0) tl = MfTile{2, 1, tl.lds, a32 && tl.as};  // a wave's rows inside the padding
    // the 128-frame tilings; bf16 storage stages A through LDS (+3.8 %, profiles/ab_r4_mfb128_variants.jsonl)
    if (nf == 128) tl = MfTile{2, a32 ? tl.kb : 2, true, true};
    const int d = a32 ? x3_depth(k) : b16_depth(k);
    if (nf == 128)  // 8 column groups (64 accumulator registers at RT = 2): A staged; split-A loads X early; rings of 2 / 3
        return a32 ? mf_key_fwd_a32(false, 8, d, 2, tl.kb, true, true) : mf_key_fwd_b16(true, 8, d >= 3 ? 3 : 2, 2, 2, true, false);
    if (tl.rt == 8) tl.kb = 1;  // 128 rows per wave: one 32-voxel block per step
    // SART_MF_XEARLY=0 / 1: X loaded with A / a step earlier (A/B runs). Default: split-A only (+0.3 %; bf16 storage
    // -2.7 %, profiles/ab_r4_mf_early_operands.jsonl)
    const bool ex = (k.xearly >= 0 ? k.xearly : (a32 ? 1 : 0)) != 0;
    const bool as = tl.as && (a32 || tl.kb == 2);  // A staged: full 128-B row segments per step (bf16: KB = 2)
    if (a32) return mf_key_fwd_a32(false, ng, d, tl.rt, tl.kb, as, ex);
    const bool lds = as || tl.lds;
    return mf_key_fwd_b16(lds, ng, d, tl.rt, tl.kb, as, lds && ex);  // the register-operand kernel has no early X
}

MfKey bwd_key(MfPath path, int nf, int64_t ld, const MfKnobs& k) {
    const int ng = nf / 16;
    if (path == MfPath::s16) return as_s16(bwd_key(MfPath::b16, nf, ld, k));
    if (path == MfPath::fp32) return mf_key_bwd_f32(ng, f32_depth(k, false, nf), f32_vox(k, ld, nf));
    if (path == MfPath::h16) {
        // SART_MF_H16 (A/B runs): "ew" early W loads, "w1" one wave per SIMD (512 registers), "ew,w1".
        // 128 frames: 8 column groups, one wave per SIMD (128 accumulator registers)
        const int mw = (nf == 128 || k.h16_w1) ? 1 : 2;
        const int d = (k.h16_ew && mw == 2) ? 2 : x3_depth(k);  // early W at two waves per SIMD: the ring of 2 only
        return mf_key_bwd_h16(ng, d, k.h16_ew, mw);
    }
    if (path == MfPath::b16) {
        const int d = b16_depth(k);
        // 128 frames: 8 column groups, one 64-voxel tile per wave (VT = 1), W in LDS, W loaded early
        if (nf == 128) return mf_key_bwd_b16(true, 8, d >= 3 ? 3 : 2, 1, true);
        // W shared through LDS (k_mf_backproject_b16_lds): SART_MF_B16_VT = "VT,lds" / "VT,reg"
        const bool lds = k.b16_w_lds != 0;
        // SART_MF_WEARLY=0 / 1: W loaded in one batch with A / one step earlier (A/B runs). Default on for bf16
        // storage (+0.9 %); off for split-A, whose two-waves-per-SIMD budget spills 40 VGPRs with the extra W slot
        // (-12 %, profiles/ab_r4_mf_early_operands.jsonl)
        const bool ew = lds && (k.wearly >= 0 ? k.wearly : 1) != 0;
        return mf_key_bwd_b16(lds, ng, d, b16_vt(k, ld, nf), ew);
    }
    return mf_key_bwd_x3(ng, x3_depth(k), x3_vt(k, ld), (k.wearly >= 0 ? k.wearly : 0) != 0);
}
}  // namespace

bool mf_variant_supported(const MfKey& key) {
    for (const MfKey& v : kVariants)
        if (v == key) return true;
    return false;
}

std::vector<MfKey> mf_variants(MfPath path, bool forward, int nf) {
    std::vector<MfKey> out;
    for (const MfKey& v : kVariants)
        if (v.path == path && v.forward == forward && v.ng == nf / 16) out.push_back(v);
    return out;
}

MfFwdPlan mf_plan_forward(MfPath path, int nf, int64_t ld, int64_t nrows_pad, const MfKnobs& k, int nsplit) {
    const std::string what = std::string("mf_forward_") + mf_path_name(path);
    if (ld % 64 != 0) throw std::runtime_error(what + ": ld must be a multiple of 64");
    if (nsplit < 0) throw std::runtime_error(what + ": nsplit must be >= 1");
    check_nf(nf, what, path != MfPath::fp32);
    const int pad = (path == MfPath::h16 || path == MfPath::s16) ? 64 : 32;
    if (nrows_pad % pad != 0)
        throw std::runtime_error(what + ": padded rows must be a multiple of " + std::to_string(pad));
    MfFwdPlan p;
    p.key = fwd_key(path, nf, ld, nrows_pad, k);
    require_variant(p.key, k);
    p.nf = nf;
    p.ld = ld;
    p.nrows_pad = nrows_pad;
    // bf16 storage: ~512 workgroups (see the back-projection)
    const bool stored16 = path == MfPath::b16 || path == MfPath::s16;  // two bytes per element in HBM
    p.nsplit = nsplit > 0 ? nsplit : fwd_splits(k, ld, nrows_pad, stored16 ? 512 : 0);
    const int64_t unit = path == MfPath::fp32 ? 16 : 64;
    p.cps = ((ld + p.nsplit - 1) / p.nsplit + unit - 1) / unit * unit;
    const int64_t rows_per_block = 64 * p.key.tile;  // 4 waves x 16 RT rows per workgroup
    p.grid_x = (unsigned)((nrows_pad + rows_per_block - 1) / rows_per_block);
    return p;
}

MfBwdPlan mf_plan_backproject(MfPath path, int nf, int64_t ld, int64_t nrows, const MfKnobs& k, int nsplit) {
    const std::string what = std::string("mf_backproject_") + mf_path_name(path);
    if (ld % 64 != 0) throw std::runtime_error(what + ": ld must be a multiple of 64");
    if (nsplit < 0) throw std::runtime_error(what + ": nsplit must be >= 1");
    // 128 frames: bf16 storage and the f16 pairs (the bf16-piece split-A engine takes the h16 back-projection)
    const bool stored16 = path == MfPath::b16 || path == MfPath::s16;  // two bytes per element in HBM
    check_nf(nf, what, stored16 || path == MfPath::h16);
    MfBwdPlan p;
    p.key = bwd_key(path, nf, ld, k);
    require_variant(p.key, k);
    p.nf = nf;
    p.ld = ld;
    p.nrows = nrows;
    if (path == MfPath::fp32) {
        p.nsplit = nsplit > 0 ? nsplit : bwd_f32_splits(k, ld, nrows);
        p.rps = ((nrows + p.nsplit - 1) / p.nsplit + 15) / 16 * 16;
        p.vox_align = 64 * p.key.tile;
    } else {
        p.nsplit = nsplit > 0 ? nsplit : bwd_b16_splits(k, ld, nrows, !stored16);
        const int64_t nrows32 = (nrows + 31) / 32 * 32;
        p.rps = ((nrows32 + p.nsplit - 1) / p.nsplit + 31) / 32 * 32;
        p.vox_align = 64 * split_vt(k, ld, !stored16);
    }
    return p;
}

int mf_forward_num_splits(int64_t ld, int64_t nrows_pad, int target) {
    return fwd_splits(MfKnobs::from_env(), ld, nrows_pad, target);
}
int mf_backproject_num_splits(int64_t ld, int64_t nrows) { return bwd_f32_splits(MfKnobs::from_env(), ld, nrows); }
int mf_backproject_b16_num_splits(int64_t ld, int64_t nrows, bool a32) {
    return bwd_b16_splits(MfKnobs::from_env(), ld, nrows, a32);
}
int mf_backproject_b16_vox_align(int64_t ld, bool a32) { return 64 * split_vt(MfKnobs::from_env(), ld, a32); }

std::vector<std::pair<std::string, std::string>> mf_key_env(const MfKey& key) {
    std::vector<std::pair<std::string, std::string>> e;
    const std::string d = std::to_string(key.depth), t = std::to_string(key.tile);
    if (key.path == MfPath::fp32) {
        e = {{"SART_MF_DEPTH", d}, {key.forward ? "SART_MF_ROWS" : "SART_MF_VOX", t}};
        if (key.forward) e.push_back({"SART_MF_NT", key.nt ? "1" : "0"});
    } else if ((key.path == MfPath::b16 || key.path == MfPath::s16) && key.forward) {
        e = {{"SART_MF_DEPTH", d}, {"SART_MF_B16_FWD", tile_str({key.tile, key.kb, key.lds, key.as}, true)},
             {"SART_MF_XEARLY", key.early ? "1" : "0"}};
    } else if (key.path == MfPath::b16 || key.path == MfPath::s16) {
        e = {{"SART_MF_DEPTH", d}, {"SART_MF_B16_VT", t + (key.lds ? ",lds" : ",reg")},
             {"SART_MF_WEARLY", key.early ? "1" : "0"}};
    } else if (key.forward) {
        e = {{"SART_MF_X3_FWD", tile_str({key.tile, key.kb, true, key.as}, false)}};
        if (key.path == MfPath::x3) {
            e.push_back({"SART_MF_X3_DEPTH", d});
            e.push_back({"SART_MF_XEARLY", key.early ? "1" : "0"});
        } else {
            e.push_back({"SART_MF_H16_FDEPTH", d});
        }
    } else if (key.path == MfPath::x3) {
        e = {{"SART_MF_X3_DEPTH", d}, {"SART_MF_X3_VT", t}, {"SART_MF_WEARLY", key.early ? "1" : "0"}};
    } else {
        e = {{"SART_MF_X3_DEPTH", d},
             {"SART_MF_H16", std::string(key.early ? "ew" : "") + (key.mw == 1 && key.ng != 8 ? ",w1" : "")}};
    }
    return e;
}

}  // namespace sart
