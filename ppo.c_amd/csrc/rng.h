// rng.h — the device random generator, shared by sample.hip and rollout.hip.
//
// Counter-based Philox-4x32-10 (Salmon et al., SC'11): a draw is a pure function of
// (counter, offset, seed), so results do not depend on launch geometry and every consumer owns the
// (counter, offset) pairs it reads.  tests/rng_ref.py restates this file in numpy.
//
// Stream table — which (key, counter, offset) each consumer reads:
//
//   ppo_fill_synthetic(seed), s0 = splitmix64(seed):
//     state          key s0 ^ 1   counter i (element)        offset 0x5EED    .x      U(−1, 1)
//     terminated     key s0 ^ 2   counter i (row)            offset 0x7E4     .x      u01 < p
//     next_state     key s0 ^ 3   counter k (element)        offset 0x4E57    .x      U(−1, 1), unlinked rows
//     reward         key s0 ^ 4   counter i (row)            offset 0xA11CE   .x .y   0.1·N(0, 1)
//     action noise   key s0 ^ 5   counter i·A + j            offset 0         .x .y   N(0, 1)
//   ppo_sample_action_device(seed, offset):
//     action noise   key seed     counter i·A + j            offset `offset`  .x .y   N(0, 1)
//   ppo_rollout_device(seed); g = the step counter that advances with every step of every call:
//     first reset    key splitmix64(seed)               counter e (Pendulum) or e·S + j   offset kReset − 1   .x (.y)
//     policy noise   key splitmix64(seed ^ 0x524F4C4C)  counter e·A + j   offset kNoise + g        .x .y   N(0, 1)
//     env decision   same key                           counter e         offset kEnv + 2g         .x .y reward noise, .z done
//     env ε          same key                           counter e·S + j   offset kEnv + 2g + 1     .x .y   N(0, 1)
//     reset          same key                           counter e (Pendulum: .x θ, .y θ̇) or e·S + j (.x)   offset kReset + g
//   CartPole-v1 (env_kind 2): first reset and reset at counter e, .x .y .z .w → x, ẋ, θ, θ̇ ~ U(−0.05, 0.05)
//   categorical policy (ppo_set_action_dist 1; discrete.hip at D = 1; tests/categorical_ref.py restates these rows):
//     ppo_fill_synthetic      action noise   key s0 ^ 5   counter i (row)   offset 0          .x   u01, inverse CDF
//     ppo_rollout_device / ppo_eval_device
//                             policy noise   key splitmix64(seed ^ 0x524F4C4C)  counter e   offset kNoise + g   .x   u01, inverse CDF
//     ppo_categorical_sample_device(key, offset)          counter i (row)   offset `offset`   .x   u01, inverse CDF
//   multi-discrete policy (ppo_set_action_multidiscrete; discrete.hip; tests/multidiscrete_ref.py restates
//   these rows): one uniform per (row, component d); key and offset are the categorical rows' above at each call
//   site, the counter's high word is d >> 2 and the word is d & 3 — d = 0 is the categorical draw
//     ppo_fill_synthetic      action noise   key s0 ^ 5   counter i | (d >> 2) << 32   offset 0   word d & 3 (.x .y .z .w)
//     ppo_rollout_device / ppo_eval_device / ppo_rollout_act / ppo_act_device
//                             policy noise   key splitmix64(seed ^ 0x524F4C4C)  counter e | (d >> 2) << 32   offset kNoise + g   word d & 3
//     ppo_multidiscrete_sample_device(key, offset)        counter i | (d >> 2) << 32   offset `offset`   word d & 3
//   action masking (ppo_set_action_mask; discrete.hip): the same sampler under a mask reads the multi-discrete rows
//   above, word for word (the categorical policy as D = 1) — ppo_rollout_act_masked / ppo_act_device_masked the policy-noise
//   row, ppo_masked_sample_device(key, offset) the last one; only the CDF it inverts differs
//   state-dependent-σ Gaussian (ppo_set_action_gaussian_sd; gauss_sd.hip; Aa = A / 2; tests/gauss_sd_ref.py): the
//   Gaussian rows' key and offset at each call site, the counter over the Aa action columns
//     ppo_fill_synthetic      action noise   key s0 ^ 5   counter i·Aa + j   offset 0   .x .y   N(0, 1)
//     ppo_rollout_device / ppo_eval_device / ppo_rollout_act / ppo_act_device
//                             policy noise   key splitmix64(seed ^ 0x524F4C4C)  counter e·Aa + j   offset kNoise + g   .x .y   N(0, 1)
//     ppo_gauss_sd_sample_device(key, offset)             counter i·Aa + j   offset `offset`   .x .y   N(0, 1)
#pragma once

#include <cmath>
#include <cstdint>

namespace ppo_rng {

struct u32x4 { uint32_t x, y, z, w; };

__device__ __forceinline__ u32x4 philox(uint64_t counter, uint64_t offset, uint64_t seed) {
    uint32_t c0 = (uint32_t)counter, c1 = (uint32_t)(counter >> 32);
    uint32_t c2 = (uint32_t)offset, c3 = (uint32_t)(offset >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return u32x4{c0, c1, c2, c3};
}

// uniform in (0, 1] from the top 24 bits n = x >> 8: (n + 0.5)·2⁻²⁴ evaluated in fp32.  Exact (and
// strictly inside (0, 1), minimum 2⁻²⁵) for n < 2²³; from 2²³ on n + 0.5 is not representable and
// rounds to even, so neighbouring n share a value and n = 2²⁴ − 1 gives exactly 1.0f.
__device__ __forceinline__ float u01(uint32_t x) { return ((x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// Box–Muller from the .x and .y words of one draw
__device__ __forceinline__ float normal_at(uint64_t idx, uint64_t offset, uint64_t seed) {
    const u32x4 r = philox(idx, offset, seed);
    const float u1 = u01(r.x), u2 = u01(r.y);
    return sqrtf(-2.f * logf(u1)) * cosf(2.f * (float)M_PI * u2);
}

// Streams of the rollout's Philox key space (offset high bits): policy noise, env noise, resets.
constexpr uint64_t kNoise = 1ull << 40, kEnv = 2ull << 40, kReset = 3ull << 40;

}  // namespace ppo_rng
