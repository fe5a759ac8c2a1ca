// The plan of a MultiFrameEngine: everything its constructor decides before it allocates. Which projection path a
// shard runs on, the batch width the path allows, the launch plans of the two projections (mf_plan), the operand
// layout, the refill queue's capacities, the sweeps per chunk, the chain policy and the voxel chunks of the overlapped
// all-reduce. Plain host C++ (this header has no HIP): the engine keeps one const plan and only executes it, the
// Python binding mf_engine_plan() returns the same plan as a dict, tests/test_mf_engine_plan.py reads the rules on
// the CPU.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "fused_plan.hpp"  // RtmStorage
#include "mf_plan.hpp"

namespace sart {

// The engine-level knobs. from_env() is the only reader of these seventeen variables; an unset or empty variable
// leaves the default (the launch shapes have their own reader, MfKnobs).
struct MfEngineKnobs {
    int x3 = -1;                   // SART_MF_X3 0 / 1: split-A for fp32 shards (-1: on from 32 frames)
    bool bwd16 = true;             // SART_MF_BWD16=0: split-A back-projection on bf16 hi + mid + lo (six products)
    bool fwd16 = true;             // SART_MF_FWD16=0: split-A forward on bf16 hi + lo
    bool xblk = true;              // SART_MF_XBLK=0: frame-major X planes (A/B runs)
    bool last_bwd = false;         // SART_MF_LAST_BWD=1: run the final sweep's back-projection anyway (A/B)
    int chunk = 0;                 // SART_MF_CHUNK: sweeps per host check (>= 1; 0: the plan's estimate)
    bool graph = true;             // SART_MF_GRAPH=0: eager launches
    int admit_cap = -1;            // SART_MF_ADMIT_CAP: admissions per sweep of a chain (0: any; -1: nf / 4)
    int src_age = 3;               // SART_MF_SRC_AGE: updates a chain source needs
    bool src_finished = false;     // SART_MF_SRC_FINISHED=1: sources are finished frames only
    bool lead = true;              // SART_MF_LEAD=0: no lead frame
    double src_extrap = 4.0;       // SART_MF_SRC_EXTRAP: extrapolation of a source along its last update
    double drift = 0.0;            // SART_MF_DRIFT: drift-extrapolated chain starts (MfQueue::drift)
    int stage_window = 0;          // SART_MF_STAGE_WINDOW=w: entry e staged only once e < finished + w (0: off)
    int chunks = 4;                // SART_MF_CHUNKS: voxel chunks of the overlapped all-reduce (several ranks)
    int sparse_pw = 64;            // SART_MF_SPARSE_PW 16 / 32 / 64: frames per SpMM plane (checked by the plan)
    int fault_nan = -1;            // SART_FAULT_NAN: applies when EngineConfig::fault_nan_sweep < 0 (tests)

    static MfEngineKnobs from_env();
};

struct MfEnginePlan {
    RtmStorage storage = RtmStorage::f32;
    bool sparse = false;  // fp32 SpMM projections: fwd / bwd and the launch plans are unused, no operand splits
    int nf = 16;          // batch width: 16, 32, 64 or 128
    bool split_a = false;  // fp32 shard on the 16-bit matrix cores
    MfPath fwd = MfPath::fp32, bwd = MfPath::fp32;
    bool xblk = false;  // X planes blocked [ld / 32][nf][32] (every 16-bit operand path unless SART_MF_XBLK=0)
    MfFwdPlan fplan;    // dense shards
    MfBwdPlan bplan;
    int nsf = 1, nsb = 1, nwb = 1;  // split-K slices of the two projections; blocks of the weights kernel
    int pw = 0;                     // sparse: frames per SpMM plane
    bool needs_w_planes = false;    // sparse: W re-laid as frame-order planes for the back-projection
    int qcap = 32, rcap = 32;       // refill queue entries / output ring entries
    int chunk = 4;                  // sweeps per host check
    // chain policy of a time series
    int admit_cap = 0, src_age = 0;
    bool src_finished = false, lead = true;
    double src_extrap = 0.0, drift = 0.0;
    int stage_window = 0;
    bool skip_last_bwd = true, use_graph = true;
    int fault_nan = -1;  // fault injection (tests): EngineConfig::fault_nan_sweep where that is < 0
    // overlapped back-projection / all-reduce: voxel chunk bounds [0, ..., ld] on multiples of vox_align, and the
    // fp32 collectives of a sweep (several ranks; what Communicator::prepare times)
    int64_t vox_align = 64;
    std::vector<int64_t> chunks;
    std::vector<int64_t> collectives;

    // "f16x2" range-safe f16 pairs, "bf16x2" / "bf16x3" bf16 pieces, "fp32" (fp32 MFMA), "bf16-storage",
    // "f16-storage" or "sparse-fp32"
    std::string forward_split() const;
    std::string backproject_split() const;
    std::string describe() const;
};

// 16, 32, 64 or 128: the smallest batch width that holds `frames` (128 for anything larger; the plan takes 64 where
// the path has no 128-column kernels)
int mf_batch_width(int frames);

// sparse: nnz entries in the shard (dense: ignored). mf_split_a: EngineConfig's (-1: default). Throws
// std::runtime_error for a plane width or launch knobs no kernel takes.
MfEnginePlan mf_engine_plan(RtmStorage storage, bool sparse, int64_t nnz, int requested_frames, int64_t nrows,
                            int64_t nrows_pad, int64_t ld, int ranks, int mf_split_a, int check_interval,
                            const MfEngineKnobs& knobs);

// Frames per SpMM plane of an nf-frame batch: pw (16, 32 or 64), or nf below it.
int mf_sparse_plane_width(int nf, int pw);
// The sparse back-projection reads W in its slot layout only for one plane of <= 32 frames: there the 16 lanes of
// each quarter wave (one pass of the address path) still touch a single 128-B line. At 64 frames the slot order
// spreads them over the whole 256-B row, twice the lines per gather (113.5k against 183.5k frame-it/s per 64-frame
// plane, profiles/sparse_r5_plane_width.txt), so W is re-laid in frame order first (launch_mf_w_planes).
inline bool mf_sparse_needs_w_planes(int nf, int pw) { return pw < nf || pw > 32; }

}  // namespace sart
