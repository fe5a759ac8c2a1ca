#include "mf_engine_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stdexcept>

#include "../kernels/launchers.hpp"  // kMfQueueMax, mf_weights_num_blocks (no HIP call is made here)

namespace sart {

namespace {
const char* env(const char* name) {
    const char* e = std::getenv(name);
    return (e && *e) ? e : nullptr;
}
bool is16(MfPath p) { return p != MfPath::fp32; }
}  // namespace

MfEngineKnobs MfEngineKnobs::from_env() {
    MfEngineKnobs k;
    if (const char* e = env("SART_MF_X3")) k.x3 = std::atoi(e) != 0;
    if (const char* e = env("SART_MF_BWD16")) k.bwd16 = std::atoi(e) != 0;
    if (const char* e = env("SART_MF_FWD16")) k.fwd16 = std::atoi(e) != 0;
    if (const char* e = env("SART_MF_XBLK")) k.xblk = std::atoi(e) != 0;
    if (const char* e = env("SART_MF_LAST_BWD")) k.last_bwd = std::atoi(e) != 0;
    if (const char* e = env("SART_MF_CHUNK")) k.chunk = std::max(1, std::atoi(e));
    if (const char* e = env("SART_MF_GRAPH")) k.graph = std::atoi(e) != 0;
    if (const char* e = env("SART_MF_ADMIT_CAP")) k.admit_cap = std::max(0, std::atoi(e));
    if (const char* e = env("SART_MF_SRC_AGE")) k.src_age = std::max(0, std::atoi(e));
    if (const char* e = env("SART_MF_SRC_FINISHED")) k.src_finished = std::atoi(e) != 0;
    if (const char* e = env("SART_MF_LEAD")) k.lead = std::atoi(e) != 0;
    if (const char* e = env("SART_MF_SRC_EXTRAP")) k.src_extrap = std::atof(e);
    if (const char* e = env("SART_MF_DRIFT")) k.drift = std::atof(e);
    if (const char* e = env("SART_MF_STAGE_WINDOW")) k.stage_window = std::max(0, std::atoi(e));
    if (const char* e = env("SART_MF_CHUNKS")) k.chunks = std::max(1, std::atoi(e));
    if (const char* e = env("SART_MF_SPARSE_PW")) k.sparse_pw = std::atoi(e);
    if (const char* e = env("SART_FAULT_NAN")) k.fault_nan = std::atoi(e);
    return k;
}

int mf_batch_width(int frames) { return frames <= 16 ? 16 : (frames <= 32 ? 32 : (frames <= 64 ? 64 : 128)); }

int mf_sparse_plane_width(int nf, int pw) {
    if (pw != 16 && pw != 32 && pw != 64) throw std::runtime_error("SART_MF_SPARSE_PW must be 16, 32 or 64");
    return nf < pw ? nf : pw;
}

MfEnginePlan mf_engine_plan(RtmStorage storage, bool sparse, int64_t nnz, int requested_frames, int64_t nrows,
                            int64_t nrows_pad, int64_t ld, int ranks, int mf_split_a, int check_interval,
                            const MfEngineKnobs& knobs) {
    MfEnginePlan p;
    p.storage = storage;
    p.sparse = sparse;
    p.nf = mf_batch_width(requested_frames);
    // split-A back-projection: f16 pairs (three products) unless SART_MF_BWD16=0 (bf16 hi + mid + lo, six); split-A
    // forward: f16 pairs unless SART_MF_FWD16=0 (bf16 hi + lo, whose 2^-17 per product is not fp32-grade on rows
    // dominated by a few entries: tests/test_gpu_realistic.py)
    if (sparse) {
        // fp32 SpMM on the frames' fp32 state: no operand splits
    } else if (storage == RtmStorage::f16s) {
        p.fwd = p.bwd = MfPath::s16;
    } else if (storage == RtmStorage::bf16) {
        p.fwd = p.bwd = MfPath::b16;
    } else {
        p.split_a = mf_split_a >= 0 ? mf_split_a != 0 : (knobs.x3 >= 0 ? knobs.x3 != 0 : p.nf >= 32);
        if (p.split_a) {
            p.fwd = knobs.fwd16 ? MfPath::h16 : MfPath::x3;
            p.bwd = knobs.bwd16 ? MfPath::h16 : MfPath::x3;
        }
    }
    // 128 columns (8 MFMA column groups) exist for the SpMM, for 16-bit storage and for split-A with the f16-pair
    // back-projection; the fp32 MFMA and three-piece bf16 back-projection paths take 64-frame batches
    if (p.nf == 128 && !(sparse || p.bwd == MfPath::b16 || p.bwd == MfPath::s16 || p.bwd == MfPath::h16)) p.nf = 64;
    const int NF = p.nf;
    // X planes blocked [ld / 32][nf][32] for the forward (SART_MF_XBLK=0: frame-major, A/B runs)
    p.xblk = !sparse && is16(p.fwd) && knobs.xblk;
    if (!sparse) {
        // the launch plans of the two projections: buffer sizes, the chunk alignment and every launch come from
        // these two objects
        const MfKnobs launch = MfKnobs::from_env();
        p.fplan = mf_plan_forward(p.fwd, NF, ld, nrows_pad, launch);
        p.bplan = mf_plan_backproject(p.bwd, NF, ld, nrows, launch);
        p.nsf = p.fplan.nsplit;
        p.nsb = p.bplan.nsplit;
    } else {  // the SpMM kernels write complete sums
        p.pw = mf_sparse_plane_width(NF, knobs.sparse_pw);
        p.needs_w_planes = mf_sparse_needs_w_planes(NF, p.pw);
    }
    p.nwb = mf_weights_num_blocks(nrows_pad);
    // queue and output ring: 4 nf entries (at most kMfQueueMax; staging and draining run a chunk behind the sweeps,
    // ~nf frames finish per chunk at ~8 sweeps per frame), down to 2 nf where their pinned host rows (fp64 pixels /
    // fp32 voxels) would pass 1 GiB
    p.qcap = p.rcap = std::min(kMfQueueMax, 4 * NF);
    while (p.qcap > 2 * NF && (double)p.qcap * nrows_pad * 8 > 1073741824.0) p.qcap /= 2;
    while (p.rcap > 2 * NF && (double)p.rcap * ld * 4 > 1073741824.0) p.rcap /= 2;
    if (knobs.chunk > 0) {
        p.chunk = knobs.chunk;
    } else {
        // sweeps per chunk: ~1.5 ms of estimated sweep time (dense: two reads of A at ~5 TB/s; sparse: two gathers
        // over the entries; plus ~13 launches), at least min(check_interval, 4): the host's per-chunk work (snapshot,
        // drain, staging) must hide behind the chunk in flight when sweeps are short (sparse shards); the host check
        // does not gate a refill, only the staging and the drain
        const double bytes = sparse ? 2.0 * (double)nnz * 8.0
                                    : 2.0 * (double)nrows_pad * ld * (storage == RtmStorage::f32 ? 4 : 2);
        const double t_sweep = bytes / 5e12 + 13 * 4e-6;
        p.chunk = (int)std::min<double>(
            32, std::max<double>(std::min(std::max(1, check_interval), 4), std::ceil(1.5e-3 / t_sweep)));
    }
    // admissions per sweep of a time series (0: any): a frame admitted together with others starts from the same
    // source iterate, so a burst of admissions starts frames far from their predecessors
    p.admit_cap = knobs.admit_cap >= 0 ? knobs.admit_cap : std::max(1, NF / 4);
    // chain sources: the newest frame with at least 3 updates, extrapolated along its last update by 4 x (linear mode):
    // a young iterate's slowest modes decay by ~rho = 0.86 per sweep on the 64k ray-traced series, so x + c (x - x_prev)
    // with c ~ rho / (1 - rho) removes most of the error it would pass on, once its fast modes are gone (>= 3 updates).
    // Measured there at 64 frames: 27.8 -> 22.9 iterations per frame, 253 -> 290 frames/s
    // (profiles/series_r6_raytraced_64k_refill_policies*.jsonl)
    p.src_age = knobs.src_age;
    p.src_extrap = knobs.src_extrap;
    p.src_finished = knobs.src_finished;
    p.lead = knobs.lead;
    // drift across the frame gap (linear mode): a source is >= src_age sweeps old, so frames newer than it are already
    // in flight and an admitted frame sits several frames of drift away from its source; the start adds that many
    // times the per-frame change between the two newest finished solutions (MfQueue::drift)
    p.drift = knobs.drift;
    // staging window w > 0 (tests): entry e is staged only once e < fin + w, fin the frames finished in the latest
    // snapshot, so the queue starves on purpose: w = 1 admits frame f when every earlier frame has finished (the
    // sequential warm-start chain, through idle plans and xlast), whatever the host's timing
    p.stage_window = knobs.stage_window;
    p.skip_last_bwd = !knobs.last_bwd;
    p.use_graph = knobs.graph;
    p.fault_nan = knobs.fault_nan;
    // chunks of the overlapped back-projection / all-reduce pipeline (several ranks only): voxel ranges aligned to
    // the back-projection's voxel tile, each >= 1 MiB of corrections
    int nchunks = 1;
    if (ranks > 1) {
        const int64_t min_vox = std::max<int64_t>(1, (1 << 20) / (4 * NF));
        nchunks = (int)std::max<int64_t>(1, std::min<int64_t>(knobs.chunks, ld / min_vox));
    }
    // (a sparse shard's SpMM has no voxel tile: 128 voxels from 32 frames on where the row allows, as the fp32 kernels)
    p.vox_align = sparse ? (NF >= 32 && ld % 128 == 0 ? 128 : 64) : p.bplan.vox_align;
    p.chunks.assign(1, 0);
    for (int c = 1; c < nchunks; ++c) {
        const int64_t v = (ld * c / nchunks) / p.vox_align * p.vox_align;
        if (v > p.chunks.back() && v < ld) p.chunks.push_back(v);
    }
    p.chunks.push_back(ld);
    if (ranks > 1) {  // the fp32 collectives of a sweep (p2p auto mode times exactly these sizes)
        p.collectives = {(int64_t)NF * ld + NF, (int64_t)NF * ld, (int64_t)NF};
        for (size_t c = 0; c + 1 < p.chunks.size(); ++c)
            p.collectives.push_back((p.chunks[c + 1] - p.chunks[c]) * NF + (c + 2 == p.chunks.size() ? NF : 0));
    }
    return p;
}

namespace {
const char* split_name(const MfEnginePlan& p, MfPath path, bool forward) {
    if (p.sparse) return "sparse-fp32";
    switch (path) {
        case MfPath::s16: return "f16-storage";
        case MfPath::b16: return "bf16-storage";
        case MfPath::h16: return "f16x2";
        case MfPath::x3: return forward ? "bf16x2" : "bf16x3";
        default: return "fp32";
    }
}
}  // namespace

std::string MfEnginePlan::forward_split() const { return split_name(*this, fwd, true); }
std::string MfEnginePlan::backproject_split() const { return split_name(*this, bwd, false); }

std::string MfEnginePlan::describe() const {
    std::string s = std::string(sparse ? "sparse" : rtm_storage_name(storage)) + " nf=" + std::to_string(nf) + " " +
                    forward_split() + " / " + backproject_split() + (xblk ? " xblk" : "");
    if (sparse) s += " pw=" + std::to_string(pw) + (needs_w_planes ? " wplanes" : "");
    s += " splits=" + std::to_string(nsf) + "/" + std::to_string(nsb) + " qcap=" + std::to_string(qcap) +
         " rcap=" + std::to_string(rcap) + " chunk=" + std::to_string(chunk) +
         " admit_cap=" + std::to_string(admit_cap) + " src_age=" + std::to_string(src_age) +
         " voxel_chunks=" + std::to_string(chunks.size() - 1) + (use_graph ? "" : " eager");
    return s;
}

}  // namespace sart
