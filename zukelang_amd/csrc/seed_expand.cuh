// The coefficient generator of the random-combination checks (key_check.hip, srs.hip): a 32-byte seed, drawn after the bytes under test
// are fixed, expanded into canonical scalars below 2^254.  One definition for every check: a seed gives the same coefficients wherever it is used.
#pragma once
#include "ec.cuh"

#include <random>
#include <string.h>

namespace zk {

struct KeychkSeed { uint64_t w[4]; };
// seed: 32 bytes, or null: drawn here
static inline KeychkSeed seed_take(const uint8_t* seed) {
    KeychkSeed sd;
    if (seed) memcpy(sd.w, seed, 32);
    else {
        std::random_device rd;
        for (int q = 0; q < 4; q++) sd.w[q] = ((uint64_t)rd() << 32) | (uint64_t)rd();
    }
    return sd;
}
// Element i of the expansion.  Limb q (64 bits) of every scalar is a splitmix64 stream of its own, keyed by bytes 8q .. 8q+7 of the seed: all 256 bits
// of the seed reach the scalars.
FF_INLINE Fr seed_expand_at(const KeychkSeed& seed, uint64_t i) {
    Fr r;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint64_t x = seed.w[q] + (i + 1) * 0x9E3779B97F4A7C15ull;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        x ^= x >> 31;
        r.v[2 * q] = (uint32_t)x;
        r.v[2 * q + 1] = (uint32_t)(x >> 32);
    }
    r.v[7] &= 0x3fffffffu;
    return r;
}

}  // namespace zk
