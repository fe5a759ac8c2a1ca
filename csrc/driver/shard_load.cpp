// The shard loaders of the native driver: HDF5 -> HBM (dense row / column shards, sparse CSR + CSC shards) and the
// two --use_cpu loads, behind load_shard (shard_load.hpp).
#include "shard_load.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <future>

#include "../engine/geometry.hpp"
#include "../kernels/launchers.hpp"

namespace sart {

double rss_hwm_mb() {
    std::ifstream f("/proc/self/status");
    std::string line;
    while (std::getline(f, line))
        if (line.rfind("VmHWM:", 0) == 0) return std::atof(line.c_str() + 6) / 1024.0;
    return 0.0;
}

namespace {

// The HIP runtime's one-time host footprint is not the loader's: its first kernel launch (code objects, device
// queues: ~0.4 GB of resident memory on the MI355X box), its first pitched host -> device copy and the copy
// stream itself (~0.19 GB: the stream's device queue) are paid here, before the baseline is taken
// (profiles/load_r5_rss_checkpoints*.jsonl); what the load adds after it is the loader's own memory.
hipStream_t dense_warm_up() {
    hip_ok(hipFree(nullptr), "hipFree");
    hipStream_t s;
    hip_ok(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
    void* d = nullptr;
    float* h = nullptr;
    hip_ok(hipMalloc(&d, 1 << 20), "hipMalloc(warm-up)");
    hip_ok(hipHostMalloc(reinterpret_cast<void**>(&h), 4096), "hipHostMalloc(warm-up)");
    hip_ok(hipMemsetAsync(d, 0, 1 << 20, s), "hipMemset(warm-up)");
    hip_ok(hipMemcpy2DAsync(d, 4096, h, 1024, 1024, 4, hipMemcpyHostToDevice, s), "hipMemcpy2D(warm-up)");
    hip_ok(hipStreamSynchronize(s), "warm-up sync");
    (void)hipHostFree(h);
    (void)hipFree(d);
    return s;
}

// 16-bit shards: rows [r0, r0 + nr) of the fp32 staging block into the shard, stream-ordered (the next block's copy
// into the staging rows waits for this conversion)
void round_block(DeviceShard& sh, const float* stage, uint64_t r0, uint64_t nr, hipStream_t s) {
    if (sh.f16)
        launch_f32_to_f16_rows(stage, (int64_t)nr, sh.ld, sh.nvoxel, static_cast<f16s_t*>(sh.A) + r0 * sh.ld,
                               sh.rsc.get() + r0, sh.rsc.get() + sh.nrows_pad + r0,
                               reinterpret_cast<unsigned long long*>(sh.counts.get()), s);
    else if (sh.bf16)
        launch_f32_to_bf16(stage, (int64_t)nr * sh.ld, static_cast<bf16_t*>(sh.A) + r0 * sh.ld, s);
}

// col0 / ncols: only that voxel block of every row (--partition_voxels), read as a column hyperslab.
std::unique_ptr<DeviceShard> load_device_shard(const InputSet& in, uint64_t row0, uint64_t nrows, size_t block_bytes,
                                               uint64_t col0, uint64_t ncols, bool bf16, bool f16, LoadStats* stats) {
    LoadStats ls;
    hipStream_t s = dense_warm_up();
    ls.rss_hwm_before_mb = rss_hwm_mb();
    const auto t_load = std::chrono::steady_clock::now();
    auto sh = std::make_unique<DeviceShard>();
    sh->bf16 = bf16;
    sh->f16 = f16;
    const bool stored16 = bf16 || f16;
    if (ncols == 0) ncols = in.nvoxel - col0;
    sh->nrows = (int64_t)nrows;
    sh->nvoxel = (int64_t)ncols;
    sh->ld = choose_ld(sh->nvoxel, 0.10, !stored16);  // 16-bit shards keep the 8-KiB slabs of their tiles
    sh->nrows_pad = (sh->nrows + 63) / 64 * 64;
    const size_t bytes = (size_t)sh->nrows_pad * sh->ld * (stored16 ? sizeof(bf16_t) : sizeof(float));
    if (f16) {  // scale 1 for the padding rows (the conversion writes the rows it sees)
        sh->rsc.resize(2 * (size_t)sh->nrows_pad);
        sh->counts.resize(2);
        const std::vector<float> ones(2 * (size_t)sh->nrows_pad, 1.f);
        hip_ok(hipMemcpy(sh->rsc.get(), ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice), "H2D scales");
    }
    hip_ok(hipMalloc(&sh->A, bytes), "hipMalloc(RTM shard)");
    ls.rss_after_malloc_mb = rss_hwm_mb();
    // on the copy stream: a fill on the null stream would bring up that stream's device queue (~0.19 GB resident)
    hip_ok(hipMemsetAsync(sh->A, 0, bytes, s), "hipMemset(RTM shard)");
    hip_ok(hipStreamSynchronize(s), "hipMemset sync");
    ls.rss_after_memset_mb = rss_hwm_mb();
    const uint64_t V = ncols;  // staging row length: the column window only
    RtmReader reader(in.rtm_files, in.rtm_name, in.nvoxel, col0, col0 + ncols);
    if (const char* e = std::getenv("SART_RTM_ROWS_PER_READ"); e && *e) {
        ls.rows_per_read = (uint64_t)std::max(0ll, std::atoll(e));
        reader.set_rows_per_read(ls.rows_per_read);
    }
    const uint64_t rows_per_block = std::max<uint64_t>(1, std::min<uint64_t>(nrows, block_bytes / (4 * V)));
    ls.rows_per_block = rows_per_block;
    ls.staging_bytes = 2 * rows_per_block * V * sizeof(float);
    float* buf[2] = {nullptr, nullptr};
    for (auto& b : buf) hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b), rows_per_block * V * sizeof(float)), "hipHostMalloc");
    ls.rss_after_pinned_mb = rss_hwm_mb();
    // bf16 / f16: fp32 staging rows [rows_per_block x ld], padding columns zero (the 2-D copies write ncols only)
    DeviceArray<float> stage;
    if (stored16) stage.resize(rows_per_block * (size_t)sh->ld);
    hipEvent_t ev[2];
    for (auto& e : ev) hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    bool ev_used[2] = {false, false};
    std::vector<std::pair<uint64_t, uint64_t>> blocks;
    for (uint64_t r = 0; r < nrows; r += rows_per_block) blocks.emplace_back(r, std::min(nrows, r + rows_per_block));
    // timing events around every block copy (GPU time of the H2D traffic)
    std::vector<hipEvent_t> tev(2 * blocks.size(), nullptr);
    for (auto& e : tev) hip_ok(hipEventCreate(&e), "hipEventCreate");
    std::vector<double> read_s(blocks.size(), 0.0);  // one slot per block: written by whichever thread reads it
    auto read_into = [&](size_t k, float* b) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint64_t r0 = blocks[k].first, r1 = blocks[k].second;
        std::memset(b, 0, (r1 - r0) * V * sizeof(float));  // sparse COO rows are scattered into zeros
        reader.read(row0 + r0, row0 + r1, b, V);  // one reader: sparse arrays are read once per shard
        read_s[k] = seconds_since(t0);
    };
    auto release = [&]() {
        for (auto& e : tev)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : ev) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(s);
        for (auto& b : buf) (void)hipHostFree(b);
    };
    ls.setup_s = seconds_since(t_load);
    ls.rss_after_setup_mb = rss_hwm_mb();
    try {
        if (!blocks.empty()) read_into(0, buf[0]);
        ls.rss_after_first_read_mb = rss_hwm_mb();
        for (size_t k = 0; k < blocks.size(); ++k) {
            float* cur = buf[k % 2];
            std::future<void> next;
            if (k + 1 < blocks.size()) {
                const int nb = (k + 1) % 2;
                if (ev_used[nb]) {  // the staging buffer of block k + 1 still feeds the copy of block k - 1
                    const auto tw = std::chrono::steady_clock::now();
                    hip_ok(hipEventSynchronize(ev[nb]), "event sync");
                    ls.wait_copy_s += seconds_since(tw);
                }
                next = std::async(std::launch::async, read_into, k + 1, buf[nb]);
            }
            const uint64_t r0 = blocks[k].first, nr = blocks[k].second - blocks[k].first;
            float* dst = stored16 ? stage.get() : static_cast<float*>(sh->A) + r0 * sh->ld;
            hip_ok(hipEventRecord(tev[2 * k], s), "event");
            hip_ok(hipMemcpy2DAsync(dst, sh->ld * sizeof(float), cur, V * sizeof(float), ncols * sizeof(float), nr,
                                    hipMemcpyHostToDevice, s),
                   "H2D RTM block");
            hip_ok(hipEventRecord(tev[2 * k + 1], s), "event");
            round_block(*sh, stage.get(), r0, nr, s);
            hip_ok(hipEventRecord(ev[k % 2], s), "event");
            ev_used[k % 2] = true;
            if (next.valid()) {
                const auto tw = std::chrono::steady_clock::now();
                next.get();
                ls.wait_read_s += seconds_since(tw);
            }
        }
        hip_ok(hipStreamSynchronize(s), "RTM upload");
        if (f16) {
            uint64_t c[2] = {0, 0};
            hip_ok(hipMemcpy(c, sh->counts.get(), sizeof(c), hipMemcpyDeviceToHost), "D2H f16 counts");
            ls.f16_flushed = c[0];
            ls.f16_nonzeros = c[1];
        }
    } catch (...) {
        (void)hipStreamSynchronize(s);
        release();
        throw;
    }
    for (size_t k = 0; k < blocks.size(); ++k) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, tev[2 * k], tev[2 * k + 1]) == hipSuccess) ls.h2d_s += 1e-3 * ms;
        ls.read_s += read_s[k];
    }
    release();
    ls.blocks = blocks.size();
    ls.bytes = nrows * V * sizeof(float);
    ls.wall_s = seconds_since(t_load);
    ls.rss_hwm_after_mb = rss_hwm_mb();
    if (stats) *stats = ls;
    return sh;
}

std::unique_ptr<DeviceSparseShard> load_sparse_shard(const InputSet& in, uint64_t row0, uint64_t nrows,
                                                     LoadStats* stats) {
    LoadStats ls;
    // The HIP runtime's one-time host footprint first, as in load_device_shard: each device queue comes up with its
    // first command, ~0.19 GB resident apiece on the MI355X box whatever the shard size -- the null stream's (the
    // fills of DeviceArray::resize, which the engine runs anyway), the copy stream's and the copy engine's, which a
    // small copy does not use (profiles/sparse_load_rss_r6.jsonl: +0.19 / +0.41 GB after the CSR + CSC without
    // these). The baseline is taken after them.
    hip_ok(hipFree(nullptr), "hipFree");
    hipStream_t s;
    hip_ok(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
    constexpr size_t kStage = (size_t)16 << 20;  // two pinned 16-MiB staging buffers (the upload's only host memory)
    char* stg[2] = {nullptr, nullptr};
    hipEvent_t ev[2];
    {
        DeviceArray<float> d;
        d.resize(kStage / sizeof(float));  // (null-stream fill)
        void* h = nullptr;
        hip_ok(hipHostMalloc(&h, kStage), "hipHostMalloc(warm-up)");
        for (auto& e : ev) hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
        hip_ok(hipMemsetAsync(d.get(), 0, kStage, s), "hipMemset(warm-up)");
        hip_ok(hipMemcpyAsync(d.get(), h, kStage, hipMemcpyHostToDevice, s), "hipMemcpy(warm-up)");
        for (auto& e : ev) hip_ok(hipEventRecord(e, s), "hipEventRecord");
        hip_ok(hipStreamSynchronize(s), "warm-up sync");
        (void)hipHostFree(h);
    }
    ls.rss_hwm_before_mb = rss_hwm_mb();
    const auto t0 = std::chrono::steady_clock::now();
    RtmReader reader(in.rtm_files, in.rtm_name, in.nvoxel);
    const HostCsr a = reader.read_csr(row0, row0 + nrows);
    ls.rss_after_first_read_mb = rss_hwm_mb();  // (streamed COO chunks: the CSR and the reader's 20 MB of chunks)
    const HostCsr t = csr_transpose(a);
    ls.rss_after_setup_mb = rss_hwm_mb();  // CSR + CSC
    ls.read_s = seconds_since(t0);
    auto sh = std::make_unique<DeviceSparseShard>();
    sh->nrows = (int64_t)nrows;
    sh->nvoxel = (int64_t)in.nvoxel;
    sh->nnz = a.nnz();
    const size_t n = (size_t)std::max<int64_t>(1, sh->nnz);
    sh->rp.resize(a.ptr.size());
    sh->cp.resize(t.ptr.size());
    sh->col.resize(n);
    sh->row.resize(n);
    sh->val.resize(n);
    sh->cval.resize(n);
    const auto t1 = std::chrono::steady_clock::now();
    for (auto& b : stg) hip_ok(hipHostMalloc(reinterpret_cast<void**>(&b), kStage), "hipHostMalloc");
    // through the pinned buffers, double-buffered: a pageable hipMemcpy of a large array stages through the
    // runtime's own pinned memory, which stays resident after the load
    int k = 0;
    auto up = [&](void* d, const void* h, size_t bytes) {
        for (size_t o = 0; o < bytes; o += kStage, k ^= 1) {
            const size_t m = std::min(kStage, bytes - o);
            hip_ok(hipEventSynchronize(ev[k]), "hipEventSynchronize");  // the copy that last used this buffer
            std::memcpy(stg[k], static_cast<const char*>(h) + o, m);
            hip_ok(hipMemcpyAsync(static_cast<char*>(d) + o, stg[k], m, hipMemcpyHostToDevice, s), "H2D sparse RTM");
            hip_ok(hipEventRecord(ev[k], s), "hipEventRecord");
        }
    };
    up(sh->rp.get(), a.ptr.data(), a.ptr.size() * sizeof(int64_t));
    up(sh->cp.get(), t.ptr.data(), t.ptr.size() * sizeof(int64_t));
    up(sh->col.get(), a.idx.data(), a.idx.size() * sizeof(int32_t));
    up(sh->val.get(), a.val.data(), a.val.size() * sizeof(float));
    up(sh->row.get(), t.idx.data(), t.idx.size() * sizeof(int32_t));
    up(sh->cval.get(), t.val.data(), t.val.size() * sizeof(float));
    hip_ok(hipStreamSynchronize(s), "H2D sparse RTM sync");
    for (auto& e : ev) (void)hipEventDestroy(e);
    for (auto& b : stg) (void)hipHostFree(b);
    (void)hipStreamDestroy(s);
    ls.staging_bytes = 2 * kStage;
    ls.h2d_s = seconds_since(t1);
    ls.blocks = 1;
    ls.rows_per_block = nrows;
    ls.bytes = (uint64_t)sh->nnz * 16 + (a.ptr.size() + t.ptr.size()) * sizeof(int64_t);
    ls.wall_s = seconds_since(t0);
    ls.rss_hwm_after_mb = rss_hwm_mb();
    if (stats) *stats = ls;
    return sh;
}

}  // namespace

void reload_host_csr(Shard& sh, const InputSet& in, const Block& blk) {
    sh.csr = RtmReader(in.rtm_files, in.rtm_name, in.nvoxel).read_csr(blk.offset, blk.offset + blk.size);
}

Shard load_shard(const Config& cfg, const InputSet& in, const Block& blk, const Block& vblk, bool sparse, bool gpu,
                 LoadStats* stats) {
    Shard sh;
    sh.gpu = gpu;
    if (sparse) sh.csr_format = true, sh.format = "sparse";
    if (gpu && !sparse) sh.storage = cfg.rtm_f16 ? "f16" : (cfg.rtm_bf16 ? "bf16" : "fp32");
    if (sparse && !gpu) {  // (the CPU solver's CSR alone; the load line as on the GPU path)
        stats->rss_hwm_before_mb = rss_hwm_mb();
        const auto t0 = std::chrono::steady_clock::now();
        reload_host_csr(sh, in, blk);
        stats->wall_s = stats->read_s = seconds_since(t0);
        sh.nnz = sh.csr.nnz();
        stats->bytes = (uint64_t)sh.nnz * 8 + sh.csr.ptr.size() * sizeof(int64_t);
        stats->rss_hwm_after_mb = rss_hwm_mb();
    } else if (sparse) {
        sh.sparse = load_sparse_shard(in, blk.offset, blk.size, stats);
        sh.nnz = sh.sparse->nnz;
    } else if (gpu) {
        size_t block_bytes = (size_t)256 << 20;  // per staging buffer (two of them)
        if (const char* e = std::getenv("SART_RTM_BLOCK_MB"); e && *e)
            block_bytes = (size_t)std::max(1.0, std::atof(e) * 1048576.0);
        sh.dense = load_device_shard(in, blk.offset, blk.size, block_bytes, vblk.offset, vblk.size, cfg.rtm_bf16,
                                     cfg.rtm_f16, stats);
    } else {
        sh.host.assign(blk.size * in.nvoxel, 0.f);
        RtmReader(in.rtm_files, in.rtm_name, in.nvoxel).read(blk.offset, blk.offset + blk.size, sh.host.data(), in.nvoxel);
    }
    return sh;
}

}  // namespace sart
