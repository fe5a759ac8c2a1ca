// Noisy replicas of a measured frame for gfx950 (--replicas, models/uncertainty.py): out[r - r0][p] is replica r of
// pixel p of g, perturbed by the noise definition of philox.hpp -- the text the host build compiles too. One thread per
// (pixel, replica): blockIdx.x walks the pixels in workgroups of 256 threads, so a row's stores are coalesced;
// blockIdx.y is the replica of the chunk. Padding beyond n is never written. The counter takes the global pixel index
// pixel0 + p as uint32 (the driver refuses 2^32 pixels and more), so a rank's slice carries the bits of the whole
// frame's call.
#include "sart_common.hpp"

#include <stdexcept>
#include <string>

#include "launchers.hpp"
#include "philox.hpp"

namespace sart {

__global__ __launch_bounds__(256) void k_noise_replicas(const double* __restrict__ g, int64_t n, uint64_t pixel0,
                                                        uint64_t time_bits, uint32_t r0, double abs_, double shot,
                                                        double rel, uint64_t seed, double* __restrict__ out,
                                                        int64_t ldo) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t r = r0 + blockIdx.y;
    const double v = g[p];
    double o = v;
    if (r != 0) o = noise_perturb(v, noise_normal(seed, time_bits, (uint32_t)(pixel0 + (uint64_t)p), r), abs_, shot, rel);
    out[(int64_t)blockIdx.y * ldo + p] = o;
}

void launch_noise_replicas(const double* g, int64_t n, uint64_t pixel0, uint64_t time_bits, uint32_t r0, int nrep,
                           double abs_, double shot, double rel, uint64_t seed, double* out, int64_t ldo,
                           hipStream_t stream) {
    if (nrep < 1 || nrep > kNoiseMaxChunk)
        throw std::runtime_error("noise_replicas: " + std::to_string(nrep) + " replicas in one launch (1 .. 64)");
    if (n < 0 || ldo < n) throw std::runtime_error("noise_replicas: out rows must hold n pixels");
    if (pixel0 + (uint64_t)n > (uint64_t)1 << 32) throw std::runtime_error("noise_replicas: pixel index beyond 2^32");
    if (!(abs_ >= 0) || !(shot >= 0) || !(rel >= 0)) throw std::runtime_error("noise_replicas: negative noise term");
    if (n == 0) return;
    if (!g || !out) throw std::runtime_error("noise_replicas: null operand");
    const int64_t blocks = (n + 255) / 256;  // n <= 2^32: fits the grid's x
    hipLaunchKernelGGL(k_noise_replicas, dim3((unsigned)blocks, (unsigned)nrep), dim3(256), 0, stream, g, n, pixel0,
                       time_bits, r0, abs_, shot, rel, seed, out, ldo);
    check_launch("k_noise_replicas");
}

}  // namespace sart
