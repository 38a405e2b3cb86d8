// tile_io.h — moving a tile of rows between global memory and LDS for the heads that own row tiles (gauss_sd.hip,
// beta.hip): n floats of A-float rows, by 16-byte accesses where VEC (the pointer is 16-byte aligned) and scalar ones
// for the < 4 floats at the end, into or out of an LDS image [rows][pitch].  T: the workgroup's threads.
#pragma once
#include <hip/hip_runtime.h>

namespace ppo {

// n floats from src (16-byte aligned when VEC) into an LDS tile [rows][pitch], columns < keep only; A floats a row
template <int T, bool VEC>
__device__ __forceinline__ void tile_load(float* tile, int pitch, const float* __restrict__ src, int n, int A,
                                          int keep, int tid) {
    int done = 0;
    if (VEC) {
        const int n4 = n >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        for (int q = tid; q < n4; q += T) {
            const float4 v = s4[q];
            const float c[4] = {v.x, v.y, v.z, v.w};
            int row = (4 * q) / A, k = 4 * q - row * A;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (k < keep) tile[row * pitch + k] = c[i];
                if (++k == A) { k = 0; ++row; }
            }
        }
        done = n4 << 2;
    }
    for (int e = done + tid; e < n; e += T) {
        const int row = e / A, k = e - row * A;
        if (k < keep) tile[row * pitch + k] = src[e];
    }
}

template <int T, bool VEC>
__device__ __forceinline__ void tile_store(const float* tile, int pitch, float* __restrict__ dst, int n, int A,
                                           int tid) {
    int done = 0;
    if (VEC) {
        const int n4 = n >> 2;
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int q = tid; q < n4; q += T) {
            float c[4];
            int row = (4 * q) / A, k = 4 * q - row * A;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                c[i] = tile[row * pitch + k];
                if (++k == A) { k = 0; ++row; }
            }
            d4[q] = make_float4(c[0], c[1], c[2], c[3]);
        }
        done = n4 << 2;
    }
    for (int e = done + tid; e < n; e += T) {
        const int row = e / A, k = e - row * A;
        dst[e] = tile[row * pitch + k];
    }
}

}  // namespace ppo
