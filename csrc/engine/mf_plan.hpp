// Launch plans of the multi-frame MFMA projections (kernels/multiframe.hip, kernels/multiframe_bf16.hip): which
// kernel variant runs, on what grid, with what split-K. Plain host C++ (no HIP): the engine builds its plans once, in
// its constructor, and sizes its buffers from the same objects it hands to the launchers; the Python bindings build a
// plan per call from MfKnobs::from_env().
//
// A plan's kernel key always names an entry of the variant lists in mf_variants.hpp. A well-formed knob setting
// that asks for a kernel outside them throws std::runtime_error naming the knobs and the path; nothing falls back.
#pragma once

#include <cstddef>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

// Two-level accumulation of the f16-pair back-projection's split-K sums through LDS (k_mf_backproject_h16): every
// SART_MF_BWD_FLUSH outer iterations the accumulators are added into a lane-private LDS sum; 0 disables (A/B builds,
// for every file that includes this header); the split count then has to shorten the chains instead
// (SART_MF_BP_BLOCKS).
#ifndef SART_MF_BWD_FLUSH
#define SART_MF_BWD_FLUSH 4
#endif

namespace sart {

// fp32: fp32 MFMA. b16: bf16 storage. x3: split-A on bf16 pieces (fp32 A split in registers). h16: split-A on f16 pairs.
// s16: row-scaled f16 storage (the bf16-storage kernels on the f16 MFMA; the bf16-storage defaults, no knobs of its own).
enum class MfPath { fp32, b16, x3, h16, s16 };

// Forward tile "RT,KB[,lds][,as]": 16-row tiles per wave, 32-voxel blocks per step, X shared through LDS, A staged
// through LDS in full row segments. rt == 0: not set (or malformed: ignored).
struct MfTile {
    int rt = 0, kb = 0;
    bool lds = false, as = false;
};

// Every launch-shape knob of the multi-frame projections. 0 / -1 / nullopt: not set, the planner's default applies.
struct MfKnobs {
    int depth = 0;        // SART_MF_DEPTH 1..3 (fp32 and bf16-storage kernels), mf_set_depth
    int rows = 0;         // SART_MF_ROWS 2 / 4 (fp32 forward), mf_set_rows
    int vox = 0;          // SART_MF_VOX 1 / 2 (fp32 back-projection), mf_set_vox
    bool nt = false;      // SART_MF_NT=1: non-temporal A loads in the fp32 forward
    MfTile b16_fwd;       // SART_MF_B16_FWD = "RT,KB[,lds][,as]", RT 2 / 4 / 8, KB 1 / 2
    int b16_vt = 0;       // SART_MF_B16_VT = "VT[,lds|,reg]", VT 1 / 2
    int b16_w_lds = -1;   //   "lds" 1 / "reg" 0: W shared through LDS
    MfTile x3_fwd;        // SART_MF_X3_FWD = "RT,KB[,as]", RT 2 / 4, KB 1 / 2 (X always in LDS)
    int x3_depth = 0;     // SART_MF_X3_DEPTH 2 / 3
    int x3_vt = 0;        // SART_MF_X3_VT 1 / 2
    int xearly = -1;      // SART_MF_XEARLY 0 / 1
    int wearly = -1;      // SART_MF_WEARLY 0 / 1
    bool h16_ew = false;  // SART_MF_H16 contains "ew": early W loads
    bool h16_w1 = false;  //   contains "w1": one wave per SIMD
    bool h16_fdepth3 = false;             // SART_MF_H16_FDEPTH=3
    std::optional<int64_t> fwd_blocks;    // SART_MF_FWD_BLOCKS: target workgroups of the forward's split-K
    std::optional<int64_t> bp_blocks;     // SART_MF_BP_BLOCKS: of the back-projection's

    // The only reader of the SART_MF_* launch-shape variables; mf_set_depth / rows / vox win over the environment.
    static MfKnobs from_env();
    std::string describe() const;  // the set knobs as "NAME=value ..." ("defaults" if none)
};

// Process-wide overrides of SART_MF_DEPTH / ROWS / VOX (0 clears), picked up by MfKnobs::from_env().
void mf_set_depth(int d);  // 1..3: register-ring depth of the MFMA projections
void mf_set_rows(int rt);  // 2 or 4: 16-row tiles per wave of the fp32 MFMA forward projection
void mf_set_vox(int vt);   // 1 or 2: 64-voxel tiles per wave of the fp32 MFMA back-projection

// One kernel instantiation. Fields a family does not have stay 0 / false.
struct MfKey {
    MfPath path = MfPath::fp32;
    bool forward = true;
    int ng = 0;          // MFMA column groups: nf / 16
    int depth = 0;       // register-ring depth
    int tile = 0;        // forward: RT (16-row tiles per wave); back-projection: VT (64-voxel tiles per wave)
    int kb = 0;          // forward, 16-bit paths: 32-voxel blocks per step
    bool lds = false;    // X / W shared through LDS
    bool as = false;     // forward: A staged through LDS
    bool early = false;  // X / W loaded a step ahead of A (EX / EW)
    bool nt = false;     // fp32 forward: non-temporal A loads
    int mw = 0;          // h16 back-projection: waves per SIMD of the register budget
};
constexpr bool operator==(const MfKey& a, const MfKey& b) {
    return a.path == b.path && a.forward == b.forward && a.ng == b.ng && a.depth == b.depth && a.tile == b.tile &&
           a.kb == b.kb && a.lds == b.lds && a.as == b.as && a.early == b.early && a.nt == b.nt && a.mw == b.mw;
}

// Keys of the variant lists' entries (mf_variants.hpp), argument for argument: shared by the planner's table of
// supported keys and the kernel tables of the .hip files, which therefore cannot disagree.
constexpr MfKey mf_key_fwd_f32(int ng, int depth, int rt, bool nt) {
    return {MfPath::fp32, true, ng, depth, rt, 0, false, false, false, nt, 0};
}
constexpr MfKey mf_key_fwd_b16(bool lds, int ng, int depth, int rt, int kb, bool as, bool ex) {
    return {MfPath::b16, true, ng, depth, rt, kb, lds, as, ex, false, 0};
}
constexpr MfKey mf_key_fwd_a32(bool h16, int ng, int depth, int rt, int kb, bool as, bool ex) {
    return {h16 ? MfPath::h16 : MfPath::x3, true, ng, depth, rt, kb, true, as, ex, false, 0};
}
constexpr MfKey mf_key_fwd_s16(int ng, int depth, int rt, int kb, bool as, bool ex) {
    return {MfPath::s16, true, ng, depth, rt, kb, true, as, ex, false, 0};
}
constexpr MfKey mf_key_bwd_s16(int ng, int depth, int vt, bool ew) {
    return {MfPath::s16, false, ng, depth, vt, 0, true, false, ew, false, 0};
}
constexpr MfKey mf_key_bwd_f32(int ng, int depth, int vt) {
    return {MfPath::fp32, false, ng, depth, vt, 0, false, false, false, false, 0};
}
constexpr MfKey mf_key_bwd_b16(bool lds, int ng, int depth, int vt, bool ew) {
    return {MfPath::b16, false, ng, depth, vt, 0, lds, false, ew, false, 0};
}
constexpr MfKey mf_key_bwd_x3(int ng, int depth, int vt, bool ew) {
    return {MfPath::x3, false, ng, depth, vt, 0, true, false, ew, false, 0};
}
constexpr MfKey mf_key_bwd_h16(int ng, int depth, bool ew, int mw) {
    return {MfPath::h16, false, ng, depth, 1, 0, true, false, ew, false, mw};
}

// An entry of a kernel table (the .hip files: one table per kernel signature, generated from mf_variants.hpp) and
// the lookup of a plan's key in it.
template <typename Fn>
struct MfVariant {
    MfKey key;
    Fn fn;
};
template <typename Fn, size_t N>
Fn mf_variant(const MfVariant<Fn> (&table)[N], const MfKey& key, const char* what) {
    for (const MfVariant<Fn>& v : table)
        if (v.key == key) return v.fn;
    throw std::runtime_error(std::string(what) + ": the plan's kernel is not in this table");
}

struct MfFwdPlan {
    MfKey key;
    int nf = 0;
    int64_t ld = 0, nrows_pad = 0;
    int nsplit = 1;       // split-K over columns: grid.y, and the slices of the forward's output
    int64_t cps = 0;      // columns per split
    unsigned grid_x = 0;  // workgroups over rows (4 waves x 16 RT rows each)
};

struct MfBwdPlan {
    MfKey key;
    int nf = 0;
    int64_t ld = 0, nrows = 0;
    int nsplit = 1;     // split-K over rows: grid.y, and the partial slices
    int64_t rps = 0;    // rows per split
    int vox_align = 0;  // voxel ranges [v0, v1) start and end on multiples of this (a multiple of the wave's 64 VT)
    unsigned grid_x(int64_t v0, int64_t v1) const {  // workgroups over [v0, v1): 4 waves x 64 VT voxels each
        const int64_t w = 64 * key.tile;
        return (unsigned)(((v1 - v0 + w - 1) / w + 3) / 4);
    }
};

// nsplit > 0: the caller's split count (direct kernel calls); 0: the planner's (what the engine allocates for).
MfFwdPlan mf_plan_forward(MfPath path, int nf, int64_t ld, int64_t nrows_pad, const MfKnobs& k, int nsplit = 0);
MfBwdPlan mf_plan_backproject(MfPath path, int nf, int64_t ld, int64_t nrows, const MfKnobs& k, int nsplit = 0);

bool mf_variant_supported(const MfKey& key);
// The table's keys of one path and direction for an nf-frame batch (tools/probe_mf_*.py iterate these).
std::vector<MfKey> mf_variants(MfPath path, bool forward, int nf);
// The knob setting that selects `key` (variable name, value), for the probes.
std::vector<std::pair<std::string, std::string>> mf_key_env(const MfKey& key);

MfPath mf_path_from_name(const std::string& name);  // "fp32", "b16", "x3", "h16", "s16"
const char* mf_path_name(MfPath p);

// Split counts for given knobs (Python bindings mf_*_num_splits; the plans hold the same numbers).
int mf_forward_num_splits(int64_t ld, int64_t nrows_pad, int target = 0);
int mf_backproject_num_splits(int64_t ld, int64_t nrows);
int mf_backproject_b16_num_splits(int64_t ld, int64_t nrows, bool a32 = false);
int mf_backproject_b16_vox_align(int64_t ld, bool a32 = false);

}  // namespace sart
