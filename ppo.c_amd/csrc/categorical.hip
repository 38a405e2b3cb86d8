// categorical.hip — the categorical policy over A discrete choices (ppo_set_action_dist(ppo, 1); no counterpart
// in the reference): the clipped-surrogate head of a policy minibatch step, the inverse-CDF sampler of rollouts,
// evaluation and ppo_fill_synthetic, and the greedy action of deterministic evaluation.  μ's A outputs are the
// logits.  The per-row arithmetic is ppo_math.h's cat_* atoms and ppo::surrogate, called, never restated.
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
//
// SAMPLER.  One lane per row, one uniform per row: u = u01(philox(counter, offset, key).x) ∈ (0, 1],
// c_k = Σ_{j<=k} e_j in fp32 with k ascending, thr = u·c_{A−1}, a = min{k : thr <= c_k}, clamped to A − 1;
// log-prob = cat_log_prob of a with s = c_{A−1}.  The action row is written as A floats: column 0 the index as
// an exact float, columns 1 … A−1 zero.  The streams it reads are listed in rng.h's table.
#include "dev.h"
#include "ppo_math.h"
#include "rng.h"

#include <cmath>

namespace {

using namespace ppo_rng;

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;

// wave max on DPP moves, the tree of dev.h's row_sum16 / wave_sum64: every lane gets the wave's value
__device__ __forceinline__ float wave_max64(float v) {
    v = fmaxf(v, ppo::dpp_mov<0xB1>(v));
    v = fmaxf(v, ppo::dpp_mov<0x4E>(v));
    v = fmaxf(v, ppo::dpp_mov<0x141>(v));
    v = fmaxf(v, ppo::dpp_mov<0x140>(v));
    return fmaxf(fmaxf(ppo::lane_value(v, 0), ppo::lane_value(v, 16)),
                 fmaxf(ppo::lane_value(v, 32), ppo::lane_value(v, 48)));
}

// the workgroup's sum of one value per wave-leader (lanes with (tid & 63) == 0 pass theirs), to thread 0
__device__ __forceinline__ float block_sum_waves(float wave_total, float* red) {
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) red[tid >> 6] = wave_total;
    __syncthreads();
    float r = 0.f;
    if (tid == 0)
        for (int w = 0; w < WAVES; ++w) r += red[w];
    __syncthreads();
    return r;
}

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
    const float bs = block_sum_waves(ws, red);
    const float bh = block_sum_waves(wh, red);
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
        M = wave_max64(M);
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
    const float bs = block_sum_waves(sur, red);
    const float bh = block_sum_waves(H, red);
    if (tid == 0) {
        if (d_loss_accum) atomicAdd(d_loss_accum, -bs / m - ent_coeff * bh / m);
        if (d_ent_accum) atomicAdd(d_ent_accum, bh);
    }
}

// ------------------------------------------------------------------ sampler / greedy action
// row e of `logits`; the action and log-prob go to row rows[e] (NULL: e)
__global__ void cat_sample_kernel(const float* __restrict__ logits, const int* __restrict__ rows,
                                  float* __restrict__ action, float* __restrict__ logprob, int m, int A,
                                  uint64_t key, uint64_t offset) {
    const long e = (long)blockIdx.x * TPB + threadIdx.x;
    if (e >= m) return;
    const float* z = logits + e * A;
    const float M = ppo::cat_row_max(z, A);
    const float s = ppo::cat_row_sum(z, A, M, nullptr);
    const float thr = u01(philox((uint64_t)e, offset, key).x) * s;
    int a = A - 1;                                   // the clamp: u <= 1 gives thr <= c_{A−1} already
    float c = 0.f;
    for (int k = 0; k < A; ++k) {
        c += ppo::cat_exp(z[k], M);
        if (thr <= c) { a = k; break; }
    }
    const long row = rows ? rows[e] : e;
    float* ar = action + row * A;
    ar[0] = (float)a;
    for (int k = 1; k < A; ++k) ar[k] = 0.f;
    if (logprob) logprob[row] = ppo::cat_log_prob(z[a], M, logf(s));
}

// argmax_k z_k, the lowest index on ties; action [m, A] compact
__global__ void cat_argmax_kernel(const float* __restrict__ logits, float* __restrict__ action, int m, int A) {
    const long e = (long)blockIdx.x * TPB + threadIdx.x;
    if (e >= m) return;
    const float* z = logits + e * A;
    int a = 0;
    float best = z[0];
    for (int k = 1; k < A; ++k)
        if (z[k] > best) { best = z[k]; a = k; }
    float* ar = action + e * A;
    ar[0] = (float)a;
    for (int k = 1; k < A; ++k) ar[k] = 0.f;
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

void phip_cat_sample(const float* logits, const int* rows, float* action, float* logprob, int m, int A, uint64_t key,
                     uint64_t offset) {
    if (m <= 0) return;
    PPO_REQUIRE(A >= 2 && logits && action, "phip_cat_sample: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * (2.0 * A + 1));
    hipLaunchKernelGGL(cat_sample_kernel, dim3(ppo_divup(m, TPB)), dim3(TPB), 0, ppo::stream(), logits, rows, action,
                       logprob, m, A, key, offset);
    PPO_LAUNCH_CHECK();
}

void phip_cat_sample_rows(const float* logits, const int* rows, float* action, float* logprob, int E, int A,
                          uint64_t key, uint64_t step) {
    phip_cat_sample(logits, rows, action, logprob, E, A, key, kNoise + step);
}

void phip_cat_argmax(const float* logits, float* action, int m, int A) {
    if (m <= 0) return;
    PPO_REQUIRE(A >= 2 && logits && action, "phip_cat_argmax: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * (2.0 * A));
    hipLaunchKernelGGL(cat_argmax_kernel, dim3(ppo_divup(m, TPB)), dim3(TPB), 0, ppo::stream(), logits, action, m, A);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
