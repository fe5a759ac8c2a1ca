// The noise definition of --replicas (README "Replicas"): Philox4x32-10 and one standard normal per counter, as
// __host__ __device__ inline functions -- the host build (native_module.cpp, g++) and the kernel (noise.hip) compile
// this text. Counter = (global pixel index, replica, low and high word of the frame time's IEEE-754 bits), key = (low,
// high word of the seed): a value depends on (seed, time, pixel, replica) alone.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SART_HD __host__ __device__
#else
#define SART_HD
#endif

namespace sart {

struct Philox4 {
    uint32_t w[4];
};

SART_HD inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// the counter's normal: u1 in (0, 1] and u2 in [0, 1) from 53 bits each, Box-Muller's cosine branch, all fp64
SART_HD inline double noise_normal(uint64_t seed, uint64_t time_bits, uint32_t pixel, uint32_t replica) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const Philox4 o = philox4x32_10(pixel, replica, (uint32_t)time_bits, (uint32_t)(time_bits >> 32), (uint32_t)seed,
                                    (uint32_t)(seed >> 32));
    const uint64_t a = ((uint64_t)o.w[0] << 21) + (o.w[1] >> 11), b = ((uint64_t)o.w[2] << 21) + (o.w[3] >> 11);
    const double u1 = (double)(a + 1) * 0x1p-53, u2 = (double)b * 0x1p-53;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// replica r >= 1 of a pixel: an excluded pixel (g < 0) stays; else max(g + sigma z, 0) with
// sigma^2 = abs^2 + shot g + (rel g)^2
SART_HD inline double noise_perturb(double g, double z, double abs_, double shot, double rel) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (g < 0.0) return g;
    const double rg = rel * g;
    const double sigma = sqrt(abs_ * abs_ + shot * g + rg * rg);
    const double v = g + sigma * z;
    return v < 0.0 ? 0.0 : v;  // (a NaN stays NaN)
}

}  // namespace sart
