// The --profile line kinds of the native driver: key names and key order are the format (docs/FORMATS.md,
// tests/test_driver_profile_schema.py).
#include "profile_lines.hpp"

#include "../engine/multiframe.hpp"
#include "shard_load.hpp"

namespace sart {

namespace {
// the keys every frame record starts with
JsonLine& frame_prefix(JsonLine& j, const FrameId& f, const SolveInfo& info) {
    return j("frame", f.frame)("time", f.time)("status", info.status)("iterations", info.iterations)(
        "convergence", info.convergence);
}
}  // namespace

void write_load_line(std::ostream& os, const LoadLine& l, const LoadStats& r) {
    JsonLine j(os);
    const LoadLine::Max& mx = l.max;
    const LoadLine::Sum& sm = l.sum;
    j("load", true)("load_s", mx.load_s)("rtm_GB", sm.bytes / 1e9)(
        "load_GBps", mx.load_s > 0 ? sm.bytes / 1e9 / mx.load_s : 0.0)("setup_s", mx.setup_s)("read_s", sm.read_s)(
        "h2d_s", sm.h2d_s)("wait_read_s", sm.wait_read_s)("wait_copy_s", sm.wait_copy_s)("ranks", l.ranks)(
        "parallel_read", l.parallel_read);
    j.open("rank0")("load_s", r.wall_s)("setup_s", r.setup_s)("read_s", r.read_s)("h2d_s", r.h2d_s)(
        "blocks", r.blocks)("rows_per_block", r.rows_per_block)("rows_per_read", r.rows_per_read)(
        "staging_MB", r.staging_bytes / 1048576.0)("rss_hwm_before_MB", r.rss_hwm_before_mb)(
        "rss_hwm_after_malloc_MB", r.rss_after_malloc_mb)("rss_hwm_after_memset_MB", r.rss_after_memset_mb)(
        "rss_hwm_after_pinned_MB", r.rss_after_pinned_mb)("rss_hwm_after_setup_MB", r.rss_after_setup_mb)(
        "rss_hwm_after_first_read_MB", r.rss_after_first_read_mb)("rss_hwm_after_MB", r.rss_hwm_after_mb);
    j.close()("rss_growth_MB_max", mx.rss_growth_mb)("shard_MB_max", mx.shard_bytes / 1048576.0)(
        "sparse", l.has_sparse)("rtm_format", l.format)("rtm_storage", l.storage)(
        "f16_flushed", (uint64_t)l.f16.flushed)(
        "f16_flushed_fraction", l.f16.nonzeros > 0 ? l.f16.flushed / l.f16.nonzeros : 0.0)(
        "solver_path", l.solver_path);
    if (!l.fp64_semantics.empty()) j("fp64_semantics", l.fp64_semantics);
    j("nnz", l.nnz)("driver", "native").end();
}

void write_frame_line(std::ostream& os, const FrameId& f, const SolveInfo& info, const FrameCosts& c) {
    // throughput of the solve (4 P V flop and one or two reads of every rank's shard per sweep)
    const double sweeps = c.gpu ? (double)info.sweeps : (double)info.iterations;
    const double secs = info.ms > 0 ? 1e-3 * info.ms : 1e-3 * f.ms;
    const double reads = c.gpu && info.used_fused ? 1.0 : 2.0;
    JsonLine j(os);
    frame_prefix(j, f, info)("sweeps", sweeps)("iters_per_s", sweeps / secs)(
        "gflops", 4.0 * c.pv * sweeps / secs / 1e9)("rtm_GBps", reads * c.elem_bytes * c.pv * sweeps / secs / 1e9)(
        "comm_ms", info.comm_ms)("comm_fallbacks", info.comm_fallbacks)("ms", f.ms)("solve_ms", info.ms)(
        "setup_ms", info.setup_ms)("iterate_ms", info.iterate_ms)("finish_ms", info.finish_ms)(
        "writer_ms", c.writer_ms)("queued_sweeps", info.queued_sweeps)("wait_frame_ms", c.wait_frame_ms)(
        "fused", info.used_fused)("ranks", c.ranks)("comm", c.comm)("device_comm", c.device_comm)(
        "driver", "native").end();
}

void write_lead_line(std::ostream& os, const FrameId& f, const SolveInfo& info, int batch) {
    JsonLine j(os);
    frame_prefix(j, f, info)("ms", f.ms)("batch", batch)("warm_from", -1)("warm_iter", -1)("lead", true)(
        "fused", info.used_fused)("driver", "native").end();
}

void write_batched_line(std::ostream& os, const FrameId& f, const SolveInfo& info, int batch, int64_t warm_from) {
    JsonLine j(os);
    frame_prefix(j, f, info)("ms", f.ms)("batch", batch)("warm_from", warm_from)("warm_iter", info.warm_iter)(
        "warm_live", info.warm_live ? 1 : 0)("comm_fallbacks", info.comm_fallbacks)("driver", "native").end();
}

void write_series_line(std::ostream& os, const MultiFrameEngine& mf, double reader_ms, double sink_ms) {
    const auto& ss = mf.series_stats();
    JsonLine j(os);
    j("series", true)("frames", ss.frames)("sweeps", ss.sweeps)("queued_sweeps", ss.queued_sweeps)(
        "slot_util", ss.slot_util)("mean_iterations", ss.mean_iterations)("chained", ss.chained)(
        "mean_warm_age", ss.mean_warm_age)("series_ms", ss.ms)("chunk", ss.chunk)("admit_cap", ss.admit_cap)(
        "src_age", ss.src_age)("src_finished", ss.src_finished ? 1 : 0)("lead", ss.lead ? 1 : 0)(
        "src_extrap", ss.src_extrap)("drift", ss.drift)("stage_window", ss.stage_window)("restarts", ss.restarts)(
        "host_wait_ms", ss.host_wait_ms)("host_stage_ms", ss.host_stage_ms)("host_src_ms", ss.host_src_ms)(
        "host_deliver_ms", ss.host_deliver_ms)("reader_ms", reader_ms)("sink_ms", sink_ms)(
        "batch", mf.batch_frames())("driver", "native").end();
}

void write_uncertainty_line(std::ostream& os, const UncertaintyLine& u) {
    JsonLine j(os);
    j("uncertainty", true)("replicas", u.replicas)("seed", u.seed)("noise_abs", u.noise_abs)(
        "noise_shot", u.noise_shot)("noise_rel", u.noise_rel)("noise_kernel_ms", u.noise_kernel_ms)(
        "moments_kernel_ms", u.moments_kernel_ms)("frames", u.frames).end();
}

void write_phantom_line(std::ostream& os, const PhantomLine& p) {
    JsonLine j(os);
    j("phantom", true)("phantoms", p.phantoms)("replicas", p.replicas)("groups", p.groups)(
        "projection_kernel_ms", p.projection_kernel_ms)("scoring_kernel_ms", p.scoring_kernel_ms).end();
}

void write_holdout_line(std::ostream& os, const HoldoutLine& h) {
    JsonLine j(os);
    j("holdout", true)("mode", h.mode)("folds", h.folds)("seed", h.seed)("betas", h.betas)("frames", h.frames)(
        "columns", h.columns)("groups", h.groups)("scoring_kernel_ms", h.scoring_kernel_ms)("ms", h.ms).end();
}

void write_fit_line(std::ostream& os, uint64_t frames, uint64_t groups, double ms, const char* storage,
                    const char* format, int ranks) {
    JsonLine j(os);
    j("fit", true)("frames", frames)("groups", groups)("fit_ms", ms)("rtm_storage", storage)("rtm_format", format)(
        "ranks", ranks).end();
}

}  // namespace sart
