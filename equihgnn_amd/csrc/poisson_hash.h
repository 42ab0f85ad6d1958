// Poisson(1) bootstrap weights as a hash of (seed, element position, bootstrap copy): ONE definition for the device kernel
// that accumulates the resampled metrics (metrics.hip) and for the host function the tests build their expectations from.
// No weight matrix is ever stored: each of the `copies` workgroups recomputes its row of it.
//
// (drop_hash.h's functions are device-only and decide in 16 bits; this sampler needs 32 uniform bits and a host twin, and
// its cost per draw -- two 64-bit finalisers over a few hundred elements per batch -- does not matter.)
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

// the splitmix64 finaliser (as drop_key's)
__host__ __device__ static inline uint64_t poisson_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// T_k = floor(2^32 * sum_{j <= k} e^-1 / j!), k = 0..12: the Poisson(1) CDF quantised to 2^-32
#define POISSON1_THRESHOLDS                                                                                              \
    {1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u, 4294609777u, 4294923276u, 4294962463u, \
     4294966817u, 4294967252u, 4294967292u, 4294967295u}

// A Poisson(1) draw that is a pure function of its arguments.  `position`: the element's ordinal since the metrics were
// reset (64 bits); copy < 64.  The seed is finalised once into a key, the key plus the element's stream index (position *
// 64 + copy, times the splitmix increment) is finalised again, and the high 32 bits are inverted through the CDF by a
// compare chain: the result is the number of thresholds T_k <= u, 0..13, with P(k) = Poisson(1) to within 2^-32.
__host__ __device__ static inline uint32_t poisson1(uint64_t seed, uint64_t position, uint32_t copy) {
    const uint64_t key = poisson_mix64(seed + 0x9E3779B97F4A7C15ull);
    const uint64_t index = position * 64ull + (uint64_t)copy;
    const uint32_t u = (uint32_t)(poisson_mix64(key + (index + 1ull) * 0x9E3779B97F4A7C15ull) >> 32);
    const uint32_t t[13] = POISSON1_THRESHOLDS;
    uint32_t k = 0;
#pragma unroll
    for (int j = 0; j < 13; ++j) k += (t[j] <= u) ? 1u : 0u;
    return k;
}
