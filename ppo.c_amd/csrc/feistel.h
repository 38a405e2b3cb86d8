// feistel.h — libppo's device shuffle: a 4-round Feistel bijection on 2^(2·half) ≥ limit, cycle-walked into
// [0, limit); no storage, no host work.  The one definition for the gather kernels (buffer.hip) and the
// phase kernels (tiny.hip, cluster.hip, cluster_deep.hip); restated bit-exactly in oracle/ref_cpu.c
// (ref_feistel_index).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ppo {

struct Feistel { uint32_t k[4]; uint32_t half, mask, n; };

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t feistel_index(uint32_t i, const Feistel& f) {
    uint32_t x = i;
    do {
        uint32_t L = x >> f.half, R = x & f.mask;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t nl = R;
            R = L ^ (mix32(R ^ f.k[r]) & f.mask);
            L = nl;
        }
        x = (L << f.half) | R;
    } while (x >= f.n);
    return x;
}

// host: the domain of a buffer of `limit` rows (half, mask, n; round keys zero)
inline Feistel feistel_domain(int limit) {
    Feistel f{};
    int bits = 2;
    while ((1ULL << bits) < (unsigned long long)limit) bits++;
    f.half = (uint32_t)((bits + 1) / 2);
    f.mask = (1u << f.half) - 1u;
    f.n = (uint32_t)limit;
    return f;
}

// host: the order of `limit` rows under the four round keys k[0..3]
inline Feistel feistel_make(int limit, const uint32_t* k) {
    Feistel f = feistel_domain(limit);
    for (int r = 0; r < 4; ++r) f.k[r] = k[r];
    return f;
}

}  // namespace ppo
