// Host launchers of the gfx950 SART kernels (csrc/kernels/*.hip). Launchers never allocate, copy or
// synchronise, so they may be captured into HIP graphs; every one checks hipGetLastError.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "sart_common.hpp"
#include "../engine/fused_plan.hpp"
#include "../engine/mf_plan.hpp"

namespace sart {
// projection.hip (RTM in fp32, or bf16 storage with fp32 products and sums)
int64_t forward_num_blocks(int64_t nrows_pad);
void launch_forward(int epi, const float* A, int64_t ld, int64_t nrows, int64_t nrows_pad, const float* x,
                    const float* ghat, const float* arow, float* out_f, float* out_w, double* Fpart,
                    const SartState* st, hipStream_t stream);
void launch_forward(int epi, const bf16_t* A, int64_t ld, int64_t nrows, int64_t nrows_pad, const float* x,
                    const float* ghat, const float* arow, float* out_f, float* out_w, double* Fpart,
                    const SartState* st, hipStream_t stream);
void launch_rowsum_f64(const float* A, int64_t ld, int64_t nrows, double* out, hipStream_t stream);
void launch_rowsum_f64(const bf16_t* A, int64_t ld, int64_t nrows, double* out, hipStream_t stream);
int backproject_num_splits(int64_t ld, int64_t nrows, int elem_bytes = 4);
void launch_backproject(const float* A, int64_t ld, int64_t nrows, const float* w, int nsplit, float* partial,
                        const SartState* st, hipStream_t stream);
void launch_backproject(const bf16_t* A, int64_t ld, int64_t nrows, const float* w, int nsplit, float* partial,
                        const SartState* st, hipStream_t stream);
void launch_colsum_f64(const float* A, int64_t ld, int64_t nrows, int nsplit, double* partial, hipStream_t stream);
void launch_colsum_f64(const bf16_t* A, int64_t ld, int64_t nrows, int nsplit, double* partial, hipStream_t stream);
// Row-scaled f16 storage (f16s_t, sart_common.hpp): A holds f16 bits of A s_p, rinv[p] = 1 / s_p (the second half of
// the shard's scale array rsc: [nrows_pad] scales, then [nrows_pad] inverses). The forward writes f = rinv dot(H, x)
// and, for the back-projection (which meets H again), the weight rinv a (ghat - f) / rinv a f; ||f||^2 is taken
// from f. The back-projection's w must carry rinv (launch_scale_rows for operands made elsewhere). Row sums are
// rinv sum H, column sums sum_p H[p][v] rinv[p], both exact products in fp64.
void launch_forward(int epi, const f16s_t* A, int64_t ld, int64_t nrows, int64_t nrows_pad, const float* x,
                    const float* ghat, const float* arow, float* out_f, float* out_w, double* Fpart,
                    const SartState* st, hipStream_t stream, const float* rinv);
void launch_rowsum_f64(const f16s_t* A, int64_t ld, int64_t nrows, double* out, hipStream_t stream,
                       const float* rinv);
void launch_backproject(const f16s_t* A, int64_t ld, int64_t nrows, const float* w, int nsplit, float* partial,
                        const SartState* st, hipStream_t stream);
void launch_colsum_f64(const f16s_t* A, int64_t ld, int64_t nrows, int nsplit, double* partial, hipStream_t stream,
                       const float* rinv);
// One launch: a device fp32 block of whole rows [n][ld] -> its f16 bits (dst [n][ld]; columns >= nvoxel zero) and
// its scales (scale[i] = s_p, inv_scale[i] = 1 / s_p for i < n). counts (optional, two device words per shard):
// counts[0] += the non-zero finite inputs stored as zero or as an f16 subnormal, counts[1] += the non-zero finite
// inputs. utils/f16rows.py is the NumPy definition.
void launch_f32_to_f16_rows(const float* src, int64_t n, int64_t ld, int64_t nvoxel, f16s_t* dst, float* scale,
                            float* inv_scale, unsigned long long* counts, hipStream_t stream);
// v[i] *= rinv[i] for i < n
void launch_scale_rows(float* v, const float* rinv, int64_t n, hipStream_t stream);
// sparse.hip: a sparse RTM shard held twice on the device, as CSR (rows: the forward projection and the row sums) and
// CSC (columns: the back-projection and the column sums), so both projections are gathers with one writer per output
// (no atomics: bitwise reproducible). Indices are 32-bit column / row numbers, offsets 64-bit.
struct SparseRtm {
    const int64_t* row_ptr = nullptr;  // [nrows + 1]
    const int32_t* col = nullptr;      // [nnz]
    const float* val = nullptr;        // [nnz]
    const int64_t* col_ptr = nullptr;  // [nvoxel + 1]
    const int32_t* row = nullptr;      // [nnz]
    const float* cval = nullptr;       // [nnz]
    int64_t nnz = 0;
    // lanes per row / column (4, 8, 16 or 32; 0: sparse_lanes()): one power-of-two group of a wave per row, so short
    // rows do not leave most of a wave idle (set once per engine: the forward's Fpart layout depends on it)
    int lanes_rows = 0, lanes_cols = 0;
};
// lanes per row for rows of `avg` entries on average (env SART_SPARSE_LANES overrides)
int sparse_lanes(double avg);
// fp64 ||f||^2 partials of launch_csr_forward: one per 256 / lanes_rows rows
int64_t csr_forward_num_blocks(const SparseRtm& s, int64_t nrows_pad);
// f = A x with the epilogues of launch_forward (kEpiPlain / kEpiLinear / kEpiLog); Fpart: csr_forward_num_blocks
// fp64 partial sums of f^2
void launch_csr_forward(int epi, const SparseRtm& s, int64_t nrows, int64_t nrows_pad, const float* x,
                        const float* ghat, const float* arow, float* out_f, float* out_w, double* Fpart,
                        const SartState* st, hipStream_t stream);
// out[v] = sum_p A[p, v] w[p] for v < nvoxel (one split: out is a partial row of k_reduce_partials)
void launch_csc_backproject(const SparseRtm& s, int64_t nvoxel, const float* w, float* out, const SartState* st,
                            hipStream_t stream);
// multi-frame engine, sparse shard: F [nrows_pad][nf] = A X^T (X frame-major [nf][ld], copied voxel-major into Xt
// [nf / PW][ld][PW] first, PW = pw (mf_sparse_plane_width); padded rows written 0) and part [v][nf] = sum_p A[p][v]
// W[p][f] for v in [v0, v1) (columns >= nvoxel written 0; times scale[v] when given). W: the back-projection
// layout of launch_mf_weights ([wrows][nf], mf_bp_slot), or with mf_sparse_needs_w_planes(nf, pw) the frame-order
// planes [nf / PW][wrows][PW] (launch_mf_w_planes, or launch_mf_weights with wplane = PW).
// pw and the W layout are the engine plan's (engine/mf_engine_plan.hpp), which lays X and W out for them
void launch_mf_sparse_forward(const SparseRtm& s, int64_t nrows, int64_t nrows_pad, const float* X, int64_t ld,
                              float* Xt, float* Fout, int nf, int pw, hipStream_t stream, const int* skip);
void launch_mf_sparse_backproject(const SparseRtm& s, int64_t nvoxel, const float* W, int64_t wrows, float* part,
                                  const float* scale, int nf, int pw, int64_t v0, int64_t v1, hipStream_t stream,
                                  const int* skip);
void launch_mf_w_planes(const float* W, int64_t rows, int nf, int pw, float* Wt, hipStream_t stream,
                        const int* skip);
void launch_csr_rowsum_f64(const SparseRtm& s, int64_t nrows, double* out, hipStream_t stream);
void launch_csc_colsum_f64(const SparseRtm& s, int64_t nvoxel, double* out, hipStream_t stream);
// fp32 -> bf16, round to nearest even (n a multiple of 4)
void launch_f32_to_bf16(const float* src, int64_t n, bf16_t* dst, hipStream_t stream);
// Fout (optional): Fout[0] = sum of Fpart (fp32), Fout[1] = st->error (the sweep's error word, reduced with it)
void launch_reduce_partials(const float* partial, int64_t ld, int nsplit, const float* scale, float* out,
                            const double* Fpart, int64_t nF, float* Fout, const SartState* st, hipStream_t stream);
void launch_reduce_partials_f64(const double* partial, int64_t ld, int nsplit, double* out, hipStream_t stream);
// projection64.hip: the double-precision two-pass kernels of Engine64 (fp32 shard [nrows_pad][ld], fp64 vectors, fp64
// FMAs; no atomics). st (optional unless noted): the launch returns at once when st->done.
// f = A x (x: ld doubles, entries at and beyond nvoxel are not used) with the epilogues of launch_forward: epi 0 f only,
// 1 out_w = arow (g - f), 2 out_w = arow f; rows >= nrows are neither read from g / arow nor written. Fpart (optional):
// forward_num_blocks(nrows_pad) fp64 partial sums of f^2 (launch_sum_f64 adds them)
void launch_forward64(int epi, const float* A, int64_t ld, int64_t nrows, int64_t nrows_pad, int64_t nvoxel,
                      const double* x, const double* g, const double* arow, double* out_f, double* out_w,
                      double* Fpart, const SartState* st, hipStream_t stream);
// out[0] = sum v[0, n), fixed order
void launch_sum_f64(const double* v, int64_t n, double* out, const SartState* st, hipStream_t stream);
// partial[s][c] = sum over the rows of split s of A[p][c] w[p] for c < ld (written, also by empty splits);
// launch_reduce_partials_f64 sums the nsplit rows. w beyond nrows is not read
void launch_backproject64(const float* A, int64_t ld, int64_t nrows, const double* w, int nsplit, double* partial,
                          const SartState* st, hipStream_t stream);
// x[i] = valid[i] ? src[i] / rho_s[i] : 0 (valid given: cold start) or src[i] / div, then max(x, clamp) when
// clamp > 0; x[n, n_pad) = 0
void launch_init_x64(double* x, int64_t n, int64_t n_pad, const double* src, const int32_t* valid, const double* rho_s,
                     double div, double clamp, hipStream_t stream);
void launch_mask64(double* v, const int32_t* valid, int64_t n, hipStream_t stream);  // v[i] = 0 where !valid[i]
// pen = beta L x (or beta L log x), each row summed in CSR order
void launch_penalty64(bool logx, const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n, double beta,
                      const double* x, double* pen, const SartState* st, hipStream_t stream);
// The stopping rule of CpuSolver::solve on the device state: Fslot[0] = sum f^2 of the sweep, over all ranks
void launch_decide64(SartState* st, const double* Fslot, hipStream_t stream);
// CpuSolver::solve's update (linear: red the reduced back-projection; log: red = A^T (a f), O the observed one);
// gpu_semantics selects max(x, 0) over the signbit test. pen optional. st required
void launch_update64(bool logmode, double* x, const double* red, const double* O, const double* pen,
                     const int32_t* valid, const double* rho_s, double alpha, double eps, bool gpu_semantics, int64_t n,
                     const SartState* st, hipStream_t stream);
// fit64.hip: fit projections F[j][p] = sum_v A[p][v] X[j][v] for nv <= 8 fp64 vectors per pass over
// the shard (fp64 FMAs; no atomics; F[j][p] depends on row p and vector j only, not on nv, the slot or the grid).
// X: [nv][ldx] (ldx >= ld, even; entries at and beyond nvoxel are not used), F: [nv][ldf] (ldf >= nrows; rows beyond
// nrows are neither read nor written). A shape without a kernel throws by name before any launch.
// vectors per pass at which a frame costs least for the storage (measured: 8, and 4 on bf16 / f16 shards)
int fit64_group(bool bf16, bool f16, bool sparse);
// dense shard [nrows_pad][ld] in the storage the engines select: fp32, bf16 bits (bf16) or row-scaled f16 bits (f16,
// row_scale: the shard's [nrows_pad] scales, then their inverses)
void launch_fit64(const void* A, bool bf16, bool f16, const float* row_scale, int64_t ld, int64_t nrows,
                  int64_t nrows_pad, int64_t nvoxel, const double* X, int64_t ldx, int nv, double* F, int64_t ldf,
                  hipStream_t stream);
// sparse shard (the CSR arrays of s; lanes per row: s.lanes_rows, or a fixed 8 when it is 0 -- never derived from the
// shard, so a row's bits do not depend on the row partition); Xt: scratch of ld x 8 doubles (X voxel-major, written here)
void launch_fit64_csr(const SparseRtm& s, int64_t nrows, int64_t nvoxel, int64_t ld, const double* X, int64_t ldx,
                      int nv, double* Xt, double* F, int64_t ldf, hipStream_t stream);
// rough64.hip: squared roughness norms eta2[j] = sum_{r < n} (sum_k L[r, col_k] u_j[col_k])^2 of nv <= 8 fp64
// solutions X [nv][ldx] per pass over the Laplacian CSR (u = x, or log(max(x, 1e-100)) with logx); every product and
// sum an fp64 FMA, a fixed 8 lanes per row, per-block partial sums into scratch (rough64_scratch_elems(n) doubles),
// then a fixed-order second stage: no atomics, eta2[j] depends on X[j] alone. Entries of X at and beyond n are not
// read. eta2_out: nv device doubles.
int64_t rough64_scratch_elems(int64_t n);
void launch_rough64(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n, const double* X,
                    int64_t ldx, int nv, bool logx, double* eta2_out, double* scratch, hipStream_t stream);
// noise.hip: replicas r0 .. r0 + nrep - 1 (nrep <= kNoiseMaxChunk per launch) of this rank's n pixels g (device fp64)
// under the noise definition of philox.hpp, out[r - r0][p] with row stride ldo; replica 0 is g itself. pixel0: the
// global index of g[0] (pixel0 + n <= 2^32); time_bits: the frame time's IEEE-754 bits. One thread per (pixel,
// replica); padding beyond n is never written.
constexpr int kNoiseMaxChunk = 64;
void launch_noise_replicas(const double* g, int64_t n, uint64_t pixel0, uint64_t time_bits, uint32_t r0, int nrep,
                           double abs_, double shot, double rel, uint64_t seed, double* out, int64_t ldo,
                           hipStream_t stream);
// moments64.hip: per-voxel mean and unbiased std over the rows r of X [n][ldx] (device fp64) with use[r] != 0, in index
// order and two passes (mean, then deviations), one thread per voxel, no atomics; c rows used: std NaN for c < 2, mean
// NaN for c = 0. Entries at and beyond nvoxel are neither read nor written.
void launch_moments64(const double* X, int64_t ldx, int64_t nvoxel, int n, const uint8_t* use, double* mean,
                      double* std_out, hipStream_t stream);
// phantom64.hip: nv <= 8 fp64 columns X [nv][ldx] scored against one truth t over the voxels v < nvoxel, ten doubles
// per column into sums_out [nv][kPhantomSums] (device): sum t, sum x, sum t^2, sum x^2, sum x t, sum (x - t)^2, sum of x
// over the voxels with t > 0, max |x - t|, max t, max x. Plain fp64 products and additions (no contraction), per-block
// partials into scratch (phantom64_scratch_elems(nvoxel) doubles), then a fixed-order second stage: no atomics, a
// column's ten values depend on X[j] and t alone. Entries at and beyond nvoxel are not read. nvoxel >= 1.
constexpr int kPhantomSums = 10;
int64_t phantom64_scratch_elems(int64_t nvoxel);
void launch_phantom64(const double* X, int64_t ldx, int64_t nvoxel, int nv, const double* t, double* sums_out,
                      double* scratch, hipStream_t stream);
// holdout64.hip: the hold-out sums of n fp64 fitted images F [n][ldf] against one frame g over the pixels of ncam
// cameras (camera m: the pixels cam_start[m] .. cam_start[m + 1] - 1; all device arrays). A pixel counts when g >= 0
// and ell > threshold (a NaN in either: it does not); column j holds out the counted pixels with fold == held[j]
// (held[j] = -1: none). sums [n][ncam][kHoldoutSums]: sum (g - f)^2, sum g^2 and the count over the held-out pixels,
// then the same three over the others. Plain fp64 (no contraction): thread t of a block of 256 takes the pixels
// cam_start[m] + t, + 256, ... in order, then a fixed tree over the 256 threads in LDS; no atomics, no scratch: a value
// depends on its column, its camera range and the inputs alone. Nothing at or beyond cam_start[ncam] is read.
// 1 <= n <= 65535, ncam >= 1, ldf >= cam_start[ncam] (the caller's to keep).
constexpr int kHoldoutSums = 6;
void launch_holdout64(const double* F, int64_t ldf, int n, const double* g, const double* ell, double threshold,
                      const int32_t* fold, const int32_t* held, const int64_t* cam_start, int ncam, double* sums,
                      hipStream_t stream);
// sart_update.hip
void launch_prep_rows(const double* g, int64_t nrows, int64_t nrows_pad, double inv_s, const float* ray_length,
                      float len_thres, float* ghat, float* arow, float* gpos, float* wo, hipStream_t stream);
void launch_init_solution(float* x, int64_t n, int64_t n_pad, const float* src_f32, const double* src_f64,
                          double scale, hipStream_t stream);
// x = fp32((x a) b), clamped (a warm start from the solution left on the device by the previous solve)
void launch_rescale_solution(float* x, int64_t n, int64_t n_pad, double a, double b, hipStream_t stream);
void launch_penalty(bool logx, const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n, float beta,
                    const float* x, float* pen, const SartState* st, hipStream_t stream);
void launch_decide(SartState* st, const float* Fslot, hipStream_t stream);
// launch_decide + launch_update_{linear,log} in one kernel (d = the reduced corrections, or Fv for log with O the
// observed back-projection); ticket: one device word, 0 between launches (re-armed by the kernel itself).
void launch_decide_update(bool logmode, SartState* st, const float* Fslot, float* x, const float* d, const float* O,
                          const float* pen, float alpha, int64_t n, unsigned* xcnt, float* xprev, unsigned* ticket,
                          hipStream_t stream);
// One rank: launch_reduce_partials (into registers, not d) + launch_decide_update in one kernel; x is bitwise the
// two-launch x. nF: the Fpart partials every workgroup sums (keep it small, e.g. the fused sweep's grid).
void launch_reduce_decide_update(bool logmode, SartState* st, const float* partial, int64_t ld, int nsplit,
                                 const float* scale, const double* Fpart, int64_t nF, float* x, const float* O,
                                 const float* pen, float alpha, int64_t n, unsigned* xcnt, float* xprev,
                                 unsigned* ticket, hipStream_t stream);
// xcnt (optional): fused-sweep ticket counters to zero for the next sweep; xprev (optional): receives x
// before the update (rollback point of the NaN/Inf guard)
void launch_update_linear(float* x, const float* d, const float* pen, int64_t n, const SartState* st,
                          hipStream_t stream, unsigned* xcnt = nullptr, float* xprev = nullptr);
void launch_update_log(float* x, const float* O, const float* Fv, const float* pen, float alpha, int64_t n,
                       const SartState* st, hipStream_t stream, unsigned* xcnt = nullptr, float* xprev = nullptr);
void launch_state_begin(SartState* st, double G, double tol, int max_iter, hipStream_t stream);
// the next exchange epoch without a decision (after a fused sweep run outside the iteration, whose granules must not
// be taken for the next sweep's); leaves SartState::error for the next sweep's decision
void launch_state_next_epoch(SartState* st, hipStream_t stream);
// w = a (ghat - f) (linear) or a f (log) from a complete forward projection f; Fpart[block] = sum f^2 (fp64)
int weights_num_blocks(int64_t nrows_pad);
void launch_weights(bool logmode, const float* f, const float* ghat, const float* arow, int64_t nrows,
                    int64_t nrows_pad, float* w, double* Fpart, const SartState* st, hipStream_t stream);
// dst[offset + i] = src[i] for i < n (gather of a column shard's slice into a full-length vector)
void launch_copy_slice(const float* src, int64_t n, float* dst, int64_t offset, hipStream_t stream);
void launch_density_scales(const double* rho, int64_t n, int64_t n_pad, float thres, float alpha, float* dinv,
                           float* dscale, float* dmask, hipStream_t stream);
void launch_f64_to_f32(const double* src, float* dst, int64_t n, hipStream_t stream);
// synth.hip
void launch_synth_matrix(float* A, int64_t ld, int64_t nrows_pad, int64_t nrows, int64_t ncols, int64_t row_offset,
                         uint64_t seed, float lo, float hi, hipStream_t stream);
// block [row_offset, +nrows) x [col_offset, +ncols) of a global nrows_total x ncols_total synthetic matrix
void launch_synth_matrix_block(float* A, int64_t ld, int64_t nrows_pad, int64_t nrows, int64_t ncols,
                               int64_t row_offset, int64_t col_offset, int64_t ncols_total, uint64_t seed, float lo,
                               float hi, hipStream_t stream);
void launch_synth_vector(double* out, int64_t n, int64_t offset, uint64_t seed, double lo, double hi,
                         hipStream_t stream);
// fused_sweep.hip
int fused_pick_k(int64_t ld);
int fused_tile_rows(int K, int variant);
// pipeline schedule the last variant-6 launch ran (T / kw / chip-wide pick it), -1: v3
int fused_last_schedule();
// granule buffer entries (uint64) of a variant-6 sweep: chip-wide groups pad each tile's row to 16 granules
int64_t fused_granules(int64_t nrows_pad, int J, bool xl);
void fused_set_trace(unsigned long long* buf, long long tiles);
std::vector<int> fused_debug_map(int nblocks);
std::vector<unsigned long long> fused_debug_stats(int nblocks);
// The operands of one fused sweep; the kernel, its threads, LDS and debug bits are the plan's (engine/fused_plan.hpp:
// fused_plan of the geometry, the storage and FusedKnobs::current(), which also holds fused_set_schedule / _debug).
struct FusedArgs {
    const void* A = nullptr;      // the shard in the plan's storage: float, bf16_t or f16s_t, [nrows_pad][ld]
    const float* rinv = nullptr;  // f16 tiles: the rows' 1 / s_p, applied where a tile's row dots are finished
    int64_t ld = 0, nrows = 0, nrows_pad = 0;
    const float *x = nullptr, *ghat = nullptr, *arow = nullptr;
    float* partial = nullptr;     // I rows of ld floats, or I * T * segments (fused_chain_plan)
    double* Fpart = nullptr;      // one ||A x||^2 partial per workgroup
    uint64_t* gran = nullptr;     // fused_granules
    int I = 0, J = 0;             // row groups x column slabs = the persistent grid
    SartState* st = nullptr;
    unsigned* xcnt = nullptr;     // per-XCD ticket counters (XCD-local row groups), zero before every sweep
    // variant 6; 0 = off. T = 1: every ~chain_tiles tiles a compute wave folds its fp32 back-projection chain into a
    // second register set (two-level sums). T >= 2 with a split schedule (FusedPlan::split): the row groups run in
    // segments of chain_tiles tiles (a multiple of kChainAlign); segment s writes the partial blocks
    // (s * T + row) * I + gi, so partial must hold I * T * segments rows of ld floats
    int64_t chain_tiles = 0;
    // f16 tiles, log mode: the sweep back-projects the caller's row operand, passed as ghat (a max(ghat, 0) / s_p), in
    // place of the weights it forms from the row dots: partial then holds A^T of that operand in the sweep's own
    // summation order (the log solver's frame-constant O; Fpart is written and meaningless)
    bool observed = false;
};
// Checks the shape against the plan (fused_check_launch: a key whose kernel is not built throws here) and launches.
void launch_fused_sweep(const FusedPlan& p, const FusedArgs& a, bool logmode, hipStream_t stream);
// p2p_allreduce.hip: one-shot push all-reduce through IPC-mapped peer buffers (at most 8 ranks, fp32).
// Receive buffer of every rank: [2 parities][kP2pMaxRanks sources][cap] floats; flags: [sources][blocks].
constexpr int kP2pMaxRanks = 8;
constexpr int kP2pMaxBlocks = 1024;
struct P2pArgs {
    float* recv[kP2pMaxRanks];      // rank j's receive buffer as mapped in this process
    unsigned* flags[kP2pMaxRanks];  // rank j's flag array as mapped in this process
    const unsigned* abort_word;     // this rank's abort word: set remotely by a peer that aborts
    // workgroups per call (0: kP2pMaxBlocks). Identical on every rank. Ranks sharing one GPU (one-GPU rehearsals)
    // use few: every workgroup spins until its peers' chunks arrive, and the spinning workgroups of all ranks must
    // leave room for the peers' persistent sweeps and their own all-reduce kernels.
    int max_blocks;
};
int64_t p2p_chunk(int64_t n, int max_blocks = kP2pMaxBlocks);  // elements per workgroup
// op: 0 sum, 1 max. `epoch` strictly increases by one per call on every rank (starts at 1).
// skip_flags (fault injection, tests): push the data but raise no flag, so the peers time out in this call.
void launch_p2p_allreduce(const float* in, float* out, int64_t n, const P2pArgs& a, int rank, int nranks,
                          unsigned epoch, int64_t cap, int op, unsigned* err, double timeout_s, hipStream_t stream,
                          bool skip_flags = false);
// The per-sweep vector of the single-frame engine before its all-reduce, as launch_reduce_partials writes it:
// v[i] = scale[i] * sum_s partial[s][i] for i < ld (scale nullptr: 1), v[ld] = sum Fpart[0:nF] (fp64 -> fp32),
// v[ld + 1] = st->error (st nullptr: 0). partial: nsplit rows of ld floats, 16-byte aligned, ld % 64 == 0.
struct ReduceSrc {
    const float* partial = nullptr;
    int64_t ld = 0;
    int nsplit = 0;
    const float* scale = nullptr;
    const double* Fpart = nullptr;
    int64_t nF = 0;
    const SartState* st = nullptr;
};
// The SART update after the per-sweep all-reduce (launch_decide_update's operands), for the P2P kernel's fused tail
struct UpdateArgs {
    SartState* st = nullptr;
    float* x = nullptr;
    const float* O = nullptr;    // log mode: the observed back-projection
    const float* pen = nullptr;  // optional
    float alpha = 1.f;
    int64_t n = 0;               // voxels
    unsigned* xcnt = nullptr;    // optional: per-XCD tickets of the next fused sweep, zeroed here
    float* xprev = nullptr;      // optional: the iterate before the update (NaN/Inf rollback point)
    unsigned* ticket = nullptr;  // the last workgroup to arrive writes the new state
    bool logmode = false;
};
// launch_reduce_partials + launch_p2p_allreduce (sum) of its ld + 2 floats in ONE kernel: each workgroup forms its
// chunk of v in registers and pushes it. out (ld + 2 floats) receives the all-reduced v, bitwise the two-launch result.
// upd (optional): also launch_decide_update in the same kernel -- every workgroup takes ||A x||^2 and the error word
// from the tail slots of all ranks (its own rank's tail computed locally), decides, and updates its chunk's voxels
// (x, state and xprev bitwise those of the separate launch). At N > 1 a SART iteration is then the sweep plus this
// one kernel, as at N = 1 (k_reduce_decide_update).
void launch_p2p_reduce_allreduce(const ReduceSrc& src, float* out, const P2pArgs& a, int rank, int nranks,
                                 unsigned epoch, int64_t cap, unsigned* err, double timeout_s, hipStream_t stream,
                                 bool skip_flags = false, const UpdateArgs* upd = nullptr);
// multiframe.hip (nf = frames per batch: 16, 32 or 64; the 16-bit kernels of multiframe_bf16.hip also take 128)
// The launchers of the MFMA projections take the plan of their path (engine/mf_plan.hpp: kernel variant, grid,
// split-K; mf_plan_forward / mf_plan_backproject); shapes, tunables and split counts are the plan's. X: [nf][ld].
void launch_mf_forward(const MfFwdPlan& p, const float* A, int64_t nrows, const float* X, float* Fout,
                       hipStream_t stream);
// voxel range [v0, v1) (default: the whole row), aligned to the wave's voxel tile (the plan's vox_align is)
void launch_mf_backproject(const MfBwdPlan& p, const float* A, const float* W, float* partial, hipStream_t stream,
                           int64_t v0 = 0, int64_t v1 = -1);
// multiframe_glue.hip
// No-op sweeps of the multi-frame engine: while a MfSkipScope is alive on the calling thread, the heavy multi-frame
// kernels (projections, weights, collect, operand splits) launched from it return at once when *skip != 0 (the
// device flag MfState::all_done: every slot's frame is done and the sweep would change nothing).
extern thread_local const int* g_mf_skip;
struct MfSkipScope {
    explicit MfSkipScope(const int* p) : prev(g_mf_skip) { g_mf_skip = p; }
    ~MfSkipScope() { g_mf_skip = prev; }
    MfSkipScope(const MfSkipScope&) = delete;
    MfSkipScope& operator=(const MfSkipScope&) = delete;
    const int* prev;
};
// bf16-stored RTM (multiframe_bf16.hip): the same projections on v_mfma_f32_16x16x32_bf16 with the fp32
// operand (X or W) split into hi + lo bf16 planes (k_mf_split_x: X [nf][ld] -> planes [nf][ld]; k_mf_split_w:
// W [rows][16][nf / 16] -> frame-major planes [nf][ldw], ldw >= rows rounded up to 32).
// xblk: X planes in the blocked layout [ld / 32][nf][32] (launch_mf_split_x with ld > 0), else frame-major [nf][ld]
void launch_mf_forward_b16(const MfFwdPlan& p, const bf16_t* A, int64_t nrows, const bf16_t* Xh, const bf16_t* Xl,
                           float* Fout, hipStream_t stream, bool xblk = false);
void launch_mf_backproject_b16(const MfBwdPlan& p, const bf16_t* A, const bf16_t* Wh, const bf16_t* Wl, int64_t ldw,
                               float* partial, hipStream_t stream, int64_t v0 = 0, int64_t v1 = -1);
// the split-A kernels (fp32 A split into hi + lo bf16 in registers, three products)
void launch_mf_forward_x3(const MfFwdPlan& p, const float* A, int64_t nrows, const bf16_t* Xh, const bf16_t* Xl,
                          float* Fout, hipStream_t stream, bool xblk = false);
// Wh: hi and mid planes ([2][nf][ldw], launch_mf_split_w with three), Wl: lo plane
void launch_mf_backproject_x3(const MfBwdPlan& p, const float* A, const bf16_t* Wh, const bf16_t* Wl, int64_t ldw,
                              float* partial, hipStream_t stream, int64_t v0 = 0, int64_t v1 = -1);
// perm: the split-A forward's k order (launch_mf_forward_x3 reads planes written with perm = true). ld > 0: X is
// [nf = n / ld][ld] and the planes are written blocked, [ld / 32][nf][32] (the forward's xblk layout)
void launch_mf_split_x(const float* X, int64_t n, bf16_t* hi, bf16_t* lo, hipStream_t stream, bool perm = false,
                       int64_t ld = 0);
// fp16-pair back-projection operands: frame-major planes w1, w2 ([nf][ldw] of f16 bits) of w s_f with a per-frame
// power-of-two scale s_f (from the frame's max |w|, wmax: nf words of scratch), inv_scale[f] = 1 / (a_scale s_f)
// have_max: wmax already holds the frames' max |w| (launch_mf_weights with wmax), else it is computed here
void launch_mf_split_w16(const float* W, int64_t nrows_pad, int nf, int64_t ldw, uint16_t* w1, uint16_t* w2,
                         unsigned* wmax, float a_scale, float* inv_scale, hipStream_t stream, bool have_max = false);
// power-of-two scale 2^(14 - e) for max |A| = m 2^e over n floats (1 if A is zero); synchronises the stream
float absmax_pow2_scale(const float* A, int64_t n, unsigned* scratch, hipStream_t stream);
// split-A back-projection on f16 pairs (two pieces of A s_v and of W s_f, three v_mfma_f32_16x16x32_f16 products,
// fp32 accumulation, the output scaled by 1 / s_v and inv_scale[f] = 1 / s_f): W1 / W2 from launch_mf_split_w16
// (a_scale 1), csc from launch_mf_col_scales
void launch_mf_backproject_h16(const MfBwdPlan& p, const float* A, const uint16_t* W1, const uint16_t* W2, int64_t ldw,
                               float* partial, hipStream_t stream, int64_t v0, int64_t v1, const float* csc,
                               const float* inv_scale);
// Range-safe f16 scales (multiframe_glue.hip): powers of two per row (rsc: [nrows_pad] scales then their inverses)
// and per column (csc: [ld] then [ld]; scratch: ld words) of an fp32 shard
void launch_mf_row_scales(const float* A, int64_t ld, int64_t nrows_pad, float* rsc, hipStream_t stream);
void launch_mf_col_scales(const float* A, int64_t ld, int64_t nrows_pad, unsigned* scratch, float* csc,
                          hipStream_t stream);
// X [nf][ld] -> f16 pieces of X s_f (per-frame power-of-two scale from max |X[f]|; xmax: nf words of scratch,
// xinv[f] = 1 / s_f), in the layout of launch_mf_split_x (perm; blocked = the ld > 0 layout)
void launch_mf_split_x16(const float* X, int64_t ld, int nf, uint16_t* x1, uint16_t* x2, unsigned* xmax, float* xinv,
                         hipStream_t stream, bool perm, bool blocked);
// split-A forward on f16 pairs: A s_p (rsc, per row) times X s_f (launch_mf_split_x16), three f16 products, the
// output scaled by 1 / (s_p s_f)
void launch_mf_forward_h16(const MfFwdPlan& p, const float* A, int64_t nrows, const uint16_t* X1, const uint16_t* X2,
                           float* Fout, hipStream_t stream, bool xblk, const float* rsc, const float* xinv);
// Row-scaled f16 storage (MfPath::s16): the bf16-storage kernels on v_mfma_f32_16x16x32_f16. A holds f16 bits of
// A s_p (rsc: the shard's [nrows_pad] scales, then their inverses); X1 / X2 from launch_mf_split_x16 with perm false
// (blocked when xblk), W1 / W2 from launch_mf_split_w16 (a_scale 1) of launch_mf_scale_w_rows' output; two products
// per element; the forward's output is scaled by 1 / (s_p s_f), the back-projection's by inv_scale[f]
void launch_mf_forward_s16(const MfFwdPlan& p, const f16s_t* A, int64_t nrows, const uint16_t* X1, const uint16_t* X2,
                           float* Fout, hipStream_t stream, bool xblk, const float* rsc, const float* xinv);
void launch_mf_backproject_s16(const MfBwdPlan& p, const f16s_t* A, const uint16_t* W1, const uint16_t* W2,
                               int64_t ldw, float* partial, hipStream_t stream, int64_t v0, int64_t v1,
                               const float* inv_scale);
// out[p][s] = W[p][s] rinv[p] for W [nrows_pad][nf] (the rows' 1 / s_p folded into the back-projection operand)
void launch_mf_scale_w_rows(const float* W, const float* rinv, int64_t nrows_pad, int nf, float* out,
                            hipStream_t stream);
// three: hi [nf][ldw] then mid [nf][ldw] in `hi` (2 nf ldw elements), lo: the split-A back-projection's planes
void launch_mf_split_w(const float* W, int64_t nrows_pad, int nf, int64_t ldw, bf16_t* hi, bf16_t* lo,
                       hipStream_t stream, bool three = false);
int mf_weights_num_blocks(int64_t nrows_pad);
// wmax (optional, nf words): also the per-frame max |w| over finite weights (zeroed here first; as k_mf_wmax)
void launch_mf_weights(const float* Fs, int nsplit, int64_t nrows_pad, const float* ghat, const float* arow,
                       bool logmode, float* W, double* F2part, int nf, hipStream_t stream, unsigned* wmax = nullptr,
                       int wplane = 0);
// D[v][f] (voxel-major) for v in [v0, v1); F2out (optional) = per-frame sums of F2part
void launch_mf_collect(const float* part, int nsplit, int64_t ld, int64_t v0, int64_t v1, const float* scale, float* D,
                       const double* F2part, int nF2, float* F2out, int nf, hipStream_t stream);
// beta_tab (optional, with q): a weight per frame of the series; slot f uses beta_tab[q->slot_frame[f]], else beta
void launch_mf_penalty(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n, float beta, bool logx,
                       const float* X, int64_t ld, float* pen, const MfState* st, int nf, hipStream_t stream,
                       const float* beta_tab = nullptr, const MfQueue* q = nullptr);
// q (optional): the device refill plan follows the decisions (mf_plan, MultiFrameEngine::solve_series)
void launch_mf_decide(MfState* st, const float* F2, hipStream_t stream, MfQueue* q = nullptr);
// Xprev (optional): receives X before the update (NaN/Inf guard rollback). q / rf: the refill of this sweep's plan
// (retired iterates into the ring, start values and log O of the admitted frames)
void launch_mf_update(float* X, const float* D, float* O, const float* pen, float alpha, bool logmode,
                      int64_t nvox, int64_t ld, const MfState* st, int nf, hipStream_t stream, float* Xprev = nullptr,
                      const MfQueue* q = nullptr, const MfRefill* rf = nullptr);
// device refill: ghat / arow columns of the admitted frames from the staged pixels ghq [qcap][nrows_pad]
void launch_mf_admit_rows(const MfQueue* q, const float* ghq, int64_t nrows, int64_t nrows_pad, const float* ray_length,
                          float len_thres, float* ghat, float* arow, int nf, hipStream_t stream);
// back-projection operands (gpos, and wo unless null) of k staged entries, columns j < k (layout of k_mf_prep_slots)
void launch_mf_stage_ops(const float* ghq, int64_t e0, int qcap, int k, int64_t nrows, int64_t nrows_pad,
                         const float* ray_length, float len_thres, float* gpos, float* wo, int nf, hipStream_t stream);
// columns j < k of a reduced voxel-major D [ld][nf] into rows (e0 + j) % qcap of out [qcap][ld]: cold starts
// max(D dinv, 1e-7) with dinv, else copies
void launch_mf_stage_cols(const float* D, const float* dinv, int64_t e0, int qcap, int k, int64_t nvox, int64_t ld,
                          int nf, float* out, hipStream_t stream);
// staging on the device: raw fp64 pixels g64q [qcap][nrows_pad] of k entries -> per-frame max / positive sum of squares
// (stats [2][nf], all-reduced by the caller) -> the queue metadata and the normalised pixels ghq [qcap][nrows_pad]
void launch_mf_stage_stats(const double* g64q, int64_t e0, int qcap, int k, int64_t nrows, int64_t nrows_pad,
                           double* stats, int nf, hipStream_t stream);
void launch_mf_stage_norm(MfQueue* q, const double* g64q, float* ghq, const double* stats, int64_t e0, int64_t frame0,
                          bool cold, int k, int64_t nrows, int64_t nrows_pad, int nf, hipStream_t stream);
void launch_mf_publish(MfQueue* q, int64_t q_tail, hipStream_t stream);
void launch_mf_drained(MfQueue* q, int64_t drained, hipStream_t stream);
void launch_mf_queue_begin(MfQueue* q, int qcap, int rcap, bool chain, int admit_cap, int src_age, int64_t x0_below,
                           bool src_finished, bool lead, float src_extrap, hipStream_t stream, float drift = 0.f);
void launch_mf_state_begin(MfState* st, const double* G, int nused, double tol, int max_iter, int nf,
                           hipStream_t stream);
// tests: every CU's LDS filled with `word` (sink: one device word, set only if a store was lost)
void launch_lds_fill(unsigned word, unsigned* sink, hipStream_t stream);
}  // namespace sart
