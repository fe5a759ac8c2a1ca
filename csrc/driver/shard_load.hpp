// This rank's shard of the ray-transfer matrix, in one of four homes (dense or CSR, in HBM or --use_cpu host
// memory), its loaders (shard_load.cpp) and the one place that turns a shard into engine constructor arguments.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../engine/engine.hpp"
#include "../native/config.hpp"
#include "../native/host_comm.hpp"
#include "../native/inputs.hpp"
#include "../native/solver_params.hpp"

namespace sart {

inline void hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
inline double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
double rss_hwm_mb();  // VmHWM of this process, MiB (0 where /proc is unavailable)

// Device-resident row shard [nrows_pad x ld] filled by streaming HDF5 row blocks through two pinned
// buffers: block k+1 is read on a helper thread while block k is copied host -> HBM. bf16 (--rtm_bf16):
// each block lands in an fp32 staging buffer in HBM and is rounded into the bf16 shard on the device; f16
// (--rtm_f16): likewise, by the row-scaling conversion kernel, which also writes the rows' scales (rsc) and counts
// the non-zeros it stores as zero or subnormal.
struct DeviceShard {
    void* A = nullptr;  // fp32, or bf16 bit patterns when bf16, or row-scaled f16 bits when f16
    bool bf16 = false, f16 = false;
    DeviceArray<float> rsc;        // f16: [nrows_pad] row scales, then [nrows_pad] inverses
    DeviceArray<uint64_t> counts;  // f16: [0] non-zeros stored as zero / subnormal, [1] non-zeros
    int64_t nrows = 0, nrows_pad = 0, nvoxel = 0, ld = 0;
    ~DeviceShard() {
        if (A) (void)hipFree(A);
    }
};

// Sparse device shard (--rtm_format): the rows' non-zeros as CSR + CSC (csrc/kernels/sparse.hip). Read through
// RtmReader::read_csr (COO arrays of sparse datasets, non-zeros of dense row blocks), transposed on the host, copied
// once; host memory is the two CSR copies of the shard, freed after the upload.
struct DeviceSparseShard {
    DeviceArray<int64_t> rp, cp;
    DeviceArray<int32_t> col, row;
    DeviceArray<float> val, cval;
    int64_t nrows = 0, nvoxel = 0, nnz = 0;
    SparseRtm view() const {
        SparseRtm s;
        s.row_ptr = rp.get(), s.col = col.get(), s.val = val.get();
        s.col_ptr = cp.get(), s.row = row.get(), s.cval = cval.get();
        s.nnz = nnz;
        return s;
    }
};

// Load-path observability (--profile's first line): wall time of the whole load, the summed HDF5 read time of the
// reader, the summed GPU time of the host -> HBM copies, the time the copy loop waited for a read (read-bound) and for
// a staging buffer to drain (copy-bound), and the resident-set high-water mark before / after, the baseline taken after
// the HIP runtime's one-time set-up (the loader's own host memory is the two pinned staging blocks). With the double
// buffer working, wall ~ max(read, h2d) + one block.
struct LoadStats {
    // setup_s: device allocation, pinned staging and opening the files (before the first block read)
    double wall_s = 0, setup_s = 0, read_s = 0, h2d_s = 0, wait_read_s = 0, wait_copy_s = 0;
    uint64_t bytes = 0, blocks = 0, rows_per_block = 0, staging_bytes = 0, rows_per_read = 0;
    double rss_hwm_before_mb = 0, rss_hwm_after_mb = 0, rss_after_setup_mb = 0, rss_after_first_read_mb = 0;
    // setup checkpoints (VmHWM, MiB): after the device allocation, after its zero fill, after the pinned staging
    double rss_after_malloc_mb = 0, rss_after_memset_mb = 0, rss_after_pinned_mb = 0;
    uint64_t f16_flushed = 0, f16_nonzeros = 0;  // --rtm_f16: non-zeros stored as zero / subnormal, all non-zeros
};

// The shard's owner: exactly one of the four homes is filled (what the solvers and the fit pass project with)
struct Shard {
    std::unique_ptr<DeviceShard> dense;         // GPU, dense storage (row or column shard)
    std::unique_ptr<DeviceSparseShard> sparse;  // GPU, CSR + CSC
    std::vector<float> host;                    // --use_cpu, dense fp32 [rows][nvoxel]
    HostCsr csr;                                // --use_cpu, CSR (the CPU solver takes it: reload_host_csr)
    bool gpu = false, csr_format = false;  // csr_format: one of the two CSR homes
    const char* storage = "fp32";          // "fp32" / "bf16" / "f16": the stored element of a dense device shard
    const char* format = "dense";          // "dense" / "sparse" (csr_format)
    int64_t nnz = 0;                       // csr_format: stored non-zeros
};

// sparse: --rtm_format decided by the caller; gpu: device shards (else the two --use_cpu loads). col window vblk:
// only that voxel block of every row (--partition_voxels), read as a column hyperslab (dense device shards).
Shard load_shard(const Config& cfg, const InputSet& in, const Block& blk, const Block& vblk, bool sparse, bool gpu,
                 LoadStats* stats);
void reload_host_csr(Shard& sh, const InputSet& in, const Block& blk);  // after a CpuSolver took Shard::csr

// Shard -> engine: pointer, rows, padded rows, voxels, ld, storage flags, row scales or the sparse view, then the
// Laplacian. E: Engine, MultiFrameEngine, or Engine64 (extra: its gpu_semantics flag).
template <class E, class... Extra>
std::unique_ptr<E> make_engine(const Shard& sh, int device, Communicator* comm, EngineConfig ec, const Csr& lap,
                               Extra... extra) {
    std::unique_ptr<E> e;
    if (sh.sparse) {
        const DeviceSparseShard& s = *sh.sparse;
        const SparseRtm view = s.view();
        e = std::make_unique<E>(device, nullptr, s.nrows, (s.nrows + 63) / 64 * 64, s.nvoxel,
                                (s.nvoxel + 63) / 64 * 64, comm, ec, extra..., &view);
    } else {
        const DeviceShard& d = *sh.dense;
        ec.rtm_bf16 = d.bf16, ec.rtm_f16 = d.f16, ec.row_scale = d.rsc.get();
        e = std::make_unique<E>(device, d.A, d.nrows, d.nrows_pad, d.nvoxel, d.ld, comm, ec, extra..., nullptr);
    }
    if (lap.nnz()) e->set_laplacian(lap.row_ptr.data(), lap.col.data(), lap.val.data(), lap.nnz());
    return e;
}

}  // namespace sart
