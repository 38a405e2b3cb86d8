// categorical.hip — the head of the categorical policy over A discrete choices (ppo_set_action_dist(ppo, 1); no
// counterpart in the reference): the clipped surrogate of a policy minibatch step while no action mask is on.  μ's A
// outputs are the logits.  The per-row arithmetic is ppo_math.h's cat_* atoms and ppo::surrogate, called, never
// restated.  The policy is discrete.hip's at D = 1, offsets {0, A}, bit for bit, and its sampler, its greedy action
// and its masked head are discrete.hip's kernels.  This head stays as the dist-1 fast path: it keeps a row in
// registers and moves it between lanes by DPP, where discrete.hip's tile head walks components through LDS, and the
// two have not been timed against each other at D = 1.
//
// HEAD.  One launch per policy step.  It reads the logits [m, A] once and writes their gradient [m, A]: the
// traffic is 2·m·A·4 bytes plus 12 bytes per row (advantage, old log-prob, column 0 of the stored action — of
// the action row only that column is read, but at A < 32 every 128-byte line of the array is still touched), so
// the kernel is memory-bound and shaped for it: no row is read twice and nothing goes through LDS that a
// register or a cross-lane move can carry.
//   A <= 32   one lane owns a row.  A workgroup stages its 256 rows through LDS by coalesced loads (a lane
//             reading its own row from HBM would stride 4·A bytes between lanes), at an odd row pitch so that the
//             256 lanes read their rows without bank conflicts; the lane keeps the row's logits in registers for
//             its three passes (max; s and t; the gradient), puts the gradient back into the tile and the
//             workgroup stores the tile coalesced.
//   A > 32    one wave (64 lanes) owns a row, lane l the logits k = l, l + 64, …, in registers (K = ⌈A/64⌉ of
//             them, K a template parameter: 1, 2, 4, 8, 16, 32 or 64, so A <= 4096).  The max, the two sums and
//             their broadcast are DPP row reductions and lane reads (dev.h), no LDS round trip; loads and stores
//             are coalesced by construction.  Four rows per workgroup.
// s and t are summed k ascending inside a lane and the lanes by dev.h's fixed wave_sum64 tree, so a row's outputs
// are bit-reproducible.  The two cross-row sums — the loss and Σ H — follow the Gaussian head: one fp32 partial
// per workgroup by a fixed tree, then one floating-point atomic per workgroup into the loss word / the entropy
// word.  That last step IS order-dependent (the workgroups arrive in any order), exactly as the Gaussian head's
// loss word is today; neither word feeds back into a parameter.
// log σ is not used and no gradient is written to it.
#include "dev.h"
#include "ppo_math.h"

#include <cmath>

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;

// ------------------------------------------------------------------ head, A <= 32: one lane per row
template <int AMAX>
__global__ __launch_bounds__(TPB) void cat_head_lane_kernel(
    const float* __restrict__ logits, const float* __restrict__ action, const float* __restrict__ adv,
    const float* __restrict__ old_lp, int m, int A, float eps, float ent_coeff, float* __restrict__ grad,
    float* __restrict__ lp_out, float* __restrict__ ent_out, float* d_loss_accum, float* d_ent_accum) {
    extern __shared__ float tile[];                  // [TPB][pitch], then [WAVES]
    const int pitch = A | 1;
    float* red = tile + TPB * pitch;
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * TPB;
    const int nr = (int)min((long)TPB, (long)m - r0);
    const long base = r0 * A;
    for (int e = tid; e < nr * A; e += TPB) {
        const int row = e / A, k = e - row * A;
        tile[row * pitch + k] = logits[base + e];
    }
    __syncthreads();
    float sur = 0.f, H = 0.f;
    if (tid < nr) {
        float* zr = tile + tid * pitch;
        float z[AMAX];
#pragma unroll
        for (int k = 0; k < AMAX; ++k) z[k] = k < A ? zr[k] : 0.f;
        float M = z[0];
#pragma unroll
        for (int k = 1; k < AMAX; ++k)
            if (k < A) M = fmaxf(M, z[k]);
        float s = 0.f, t = 0.f;
#pragma unroll
        for (int k = 0; k < AMAX; ++k)
            if (k < A) {
                const float e = ppo::cat_exp(z[k], M);
                s += e;
                t += e * (z[k] - M);
            }
        const long i = r0 + tid;
        const int a = ppo::cat_index(action[i * A], A);
        const float ls = logf(s);
        float za = z[0];
#pragma unroll
        for (int k = 1; k < AMAX; ++k)
            if (k == a) za = z[k];
        const float lp = ppo::cat_log_prob(za, M, ls);
        H = ppo::cat_entropy(ls, t, s);
        float g;
        sur = ppo::surrogate(adv[i], lp, old_lp[i], eps, m, &g);
        const float cm = ent_coeff / m;
#pragma unroll
        for (int k = 0; k < AMAX; ++k)
            if (k < A) zr[k] = ppo::cat_grad(g, k == a, z[k], M, s, ls, H, cm);
        if (lp_out) lp_out[i] = lp;
        if (ent_out) ent_out[i] = H;
    }
    __syncthreads();
    for (int e = tid; e < nr * A; e += TPB) {
        const int row = e / A, k = e - row * A;
        grad[base + e] = tile[row * pitch + k];
    }
    const float ws = ppo::wave_sum64(sur), wh = ppo::wave_sum64(H);
    const float bs = ppo::block_sum_waves<WAVES>(ws, red);
    const float bh = ppo::block_sum_waves<WAVES>(wh, red);
    if (tid == 0) {
        if (d_loss_accum) atomicAdd(d_loss_accum, -bs / m - ent_coeff * bh / m);
        if (d_ent_accum) atomicAdd(d_ent_accum, bh);
    }
}

// ------------------------------------------------------------------ head, A > 32: one wave per row
template <int K>
__global__ __launch_bounds__(TPB) void cat_head_wave_kernel(
    const float* __restrict__ logits, const float* __restrict__ action, const float* __restrict__ adv,
    const float* __restrict__ old_lp, int m, int A, float eps, float ent_coeff, float* __restrict__ grad,
    float* __restrict__ lp_out, float* __restrict__ ent_out, float* d_loss_accum, float* d_ent_accum) {
    __shared__ float red[WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const long i = (long)blockIdx.x * WAVES + (tid >> 6);          // the wave's row: uniform over the wave
    float sur = 0.f, H = 0.f;
    if (i < m) {
        const float* zr = logits + i * A;
        float z[K];
        float M = -INFINITY;
#pragma unroll
        for (int q = 0; q < K; ++q) {
            const int k = lane + 64 * q;
            z[q] = k < A ? zr[k] : -INFINITY;
            M = fmaxf(M, z[q]);
        }
        M = ppo::wave_max64(M);
        float s = 0.f, t = 0.f;
#pragma unroll
        for (int q = 0; q < K; ++q)
            if (lane + 64 * q < A) {
                const float e = ppo::cat_exp(z[q], M);
                s += e;
                t += e * (z[q] - M);
            }
        s = ppo::wave_sum64(s);
        t = ppo::wave_sum64(t);
        const int a = ppo::cat_index(action[i * A], A);
        const float ls = logf(s);
        const float lp = ppo::cat_log_prob(zr[a], M, ls);         // one broadcast read of a line the wave holds
        H = ppo::cat_entropy(ls, t, s);
        float g;
        sur = ppo::surrogate(adv[i], lp, old_lp[i], eps, m, &g);
        const float cm = ent_coeff / m;
        float* gr = grad + i * A;
#pragma unroll
        for (int q = 0; q < K; ++q) {
            const int k = lane + 64 * q;
            if (k < A) gr[k] = ppo::cat_grad(g, k == a, z[q], M, s, ls, H, cm);
        }
        if (lane == 0) {
            if (lp_out) lp_out[i] = lp;
            if (ent_out) ent_out[i] = H;
        }
    }
    // every lane of a wave holds the same sur / H: the wave's total is its row's value
    const float bs = ppo::block_sum_waves<WAVES>(sur, red);
    const float bh = ppo::block_sum_waves<WAVES>(H, red);
    if (tid == 0) {
        if (d_loss_accum) atomicAdd(d_loss_accum, -bs / m - ent_coeff * bh / m);
        if (d_ent_accum) atomicAdd(d_ent_accum, bh);
    }
}

}  // namespace

extern "C" {

void phip_cat_head(const float* logits, const float* action, const float* adv, const float* old_lp, int m, int A,
                   float epsilon, float ent_coeff, float* grad, float* lp_out, float* ent_out, float* d_loss_accum,
                   float* d_ent_accum) {
    if (m <= 0) return;
    PPO_REQUIRE(A >= 2 && A <= PHIP_CAT_MAX_A, "phip_cat_head: action size out of range");
    PPO_REQUIRE(logits && action && adv && old_lp && grad, "phip_cat_head: operands");
    ppo::ProfScope ps(PPO_K_HEAD, 4.0 * m * (2.0 * A + 3));
#define CAT_LANE(AMAX)                                                                                              \
    hipLaunchKernelGGL(cat_head_lane_kernel<AMAX>, dim3(ppo_divup(m, TPB)), dim3(TPB),                              \
                       sizeof(float) * ((size_t)TPB * (A | 1) + WAVES), ppo::stream(), logits, action, adv, old_lp, \
                       m, A, epsilon, ent_coeff, grad, lp_out, ent_out, d_loss_accum, d_ent_accum)
#define CAT_WAVE(K)                                                                                               \
    hipLaunchKernelGGL(cat_head_wave_kernel<K>, dim3(ppo_divup(m, WAVES)), dim3(TPB), 0, ppo::stream(), logits,   \
                       action, adv, old_lp, m, A, epsilon, ent_coeff, grad, lp_out, ent_out, d_loss_accum,        \
                       d_ent_accum)
    if (A <= 8) CAT_LANE(8);
    else if (A <= 32) CAT_LANE(32);
    else if (A <= 64) CAT_WAVE(1);
    else if (A <= 128) CAT_WAVE(2);
    else if (A <= 256) CAT_WAVE(4);
    else if (A <= 512) CAT_WAVE(8);
    else if (A <= 1024) CAT_WAVE(16);
    else if (A <= 2048) CAT_WAVE(32);
    else CAT_WAVE(64);
#undef CAT_LANE
#undef CAT_WAVE
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
