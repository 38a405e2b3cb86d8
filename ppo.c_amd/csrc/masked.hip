// masked.hip — invalid-action masking for the categorical and the multi-discrete policy (ppo_set_action_mask; no
// counterpart in the reference).  The definition is ppo_math.h's ("Action masking": mask_component and the masked
// atoms), called, never restated: a row carries W = (A + 31) / 32 words, bit k & 31 of word k >> 5 = column k
// allowed; a component with no stored bit set reads as fully allowed; the head and the KL monitor also allow the
// chosen column.  Masked columns enter no max and no sum, their gradient is +0 and their logits never reach
// arithmetic.  categorical.hip and multidiscrete.hip are untouched: with masking off nothing here runs, and with a
// full mask every kernel here gives its multidiscrete.hip counterpart's bits (the categorical policy runs here as
// nvec = {A}).
//
// HEAD.  md_head_kernel's tile design (multidiscrete.hip: R rows stay in LDS across both phases, a lane per (row,
// component) when every n_d <= 32 and a wave per item otherwise, coalesced loads and stores, the same loss and
// entropy partials) with one more LDS block: row i of the minibatch reads its W words at mask[rows[i]·W] (rows NULL:
// i) — the buffer row the minibatch gather already hands the policy step, so no gather launch is added — into
// mw[R][W | 1].  The odd pitch keeps the lanes of a wave, which walk neighbouring rows of one component, on distinct
// banks; they test bits from LDS.  A one-lane item folds its component's effective mask into one register word
// (mask_component) before its loops.
// LDS per row: (A | 1) + 5·D + 1 + (D | 1) + (W | 1) words — 908 bytes at nvec = [7]·17 (R = 32, 29 KB a workgroup),
// 8.3 KB at [2]·256 (R = 4, 34 KB), 16.9 KB at [4096] (R = 2, 34 KB); the largest legal row (A = 4096, D = 256) is
// 23 KB, so every legal shape fits the 40 KB no-opt-in budget with R >= 1.
// Traffic per row: multidiscrete.hip's 4·(2A + D + 2) bytes plus the 4·W mask bytes, at worst one more 128-byte
// line per scattered row.
//
// SAMPLER / ARGMAX.  One lane per row, as multidiscrete.hip's, over a dense mask [m, W]: the same Philox word per
// (row, component), the CDF inverted over the allowed columns only (c accumulates e_k over allowed k ascending, the
// first allowed k with u·s_d <= c, the fallback the last allowed k).  The sampler also copies the row's W words to
// mask_out[row·W] when given one, so a rollout stores the mask it sampled under without another launch.
#include "dev.h"
#include "ppo_math.h"
#include "rng.h"

#include <cmath>

namespace {

using namespace ppo_rng;

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MASKED_LDS_BUDGET = 40 * 1024;

// multidiscrete.hip's wave max (the tree of dev.h's wave_sum64): every lane gets the wave's value
__device__ __forceinline__ float wave_max64(float v) {
    v = fmaxf(v, ppo::dpp_mov<0xB1>(v));
    v = fmaxf(v, ppo::dpp_mov<0x4E>(v));
    v = fmaxf(v, ppo::dpp_mov<0x141>(v));
    v = fmaxf(v, ppo::dpp_mov<0x140>(v));
    return fmaxf(fmaxf(ppo::lane_value(v, 0), ppo::lane_value(v, 16)),
                 fmaxf(ppo::lane_value(v, 32), ppo::lane_value(v, 48)));
}

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

// words of LDS one row of the tile needs, and the launch's total in bytes
__host__ __device__ inline int masked_row_words(int A, int D, int W) {
    return (A | 1) + 5 * D + 1 + (D | 1) + (W | 1);
}
inline size_t masked_lds_bytes(int A, int D, int W, int R) {
    return sizeof(float) * ((size_t)R * masked_row_words(A, D, W) + (D + 1) + WAVES);
}

// one component of one row by a whole wave (the wide form; every lane active, every lane gets the record):
// multidiscrete.hip's md_component_wave over the allowed columns
__device__ __forceinline__ ppo::MdComp masked_component_wave(const float* z, int n, int a, const ppo::MaskComp& mc,
                                                             int lane) {
    if (n <= 32) return ppo::md_component_masked(z, n, a, mc);
    ppo::MdComp c;
    float M = -INFINITY;
    for (int k = lane; k < n; k += 64)
        if (mc.allowed(k)) M = fmaxf(M, z[k]);
    c.M = wave_max64(M);
    float s = 0.f, t = 0.f;
    for (int k = lane; k < n; k += 64) {
        if (!mc.allowed(k)) continue;
        const float e = ppo::cat_exp(z[k], c.M);
        s += e;
        t += e * (z[k] - c.M);
    }
    c.s = ppo::wave_sum64(s);
    t = ppo::wave_sum64(t);
    c.ls = logf(c.s);
    c.lp = ppo::cat_log_prob(z[a], c.M, c.ls);
    c.H = ppo::cat_entropy(c.ls, t, c.s);
    return c;
}

// R = 1 << lgR rows per workgroup; WIDE: a wave per (row, component) item, else a lane
template <bool WIDE>
__global__ __launch_bounds__(TPB) void masked_head_kernel(
    const float* __restrict__ logits, const float* __restrict__ action, const float* __restrict__ adv,
    const float* __restrict__ old_lp, const uint32_t* __restrict__ mask, const int* __restrict__ rows,
    const int* __restrict__ off, int m, int A, int D, int W, int lgR, float eps, float ent_coeff,
    float* __restrict__ grad, float* __restrict__ lp_out, float* __restrict__ ent_out, float* d_loss_accum,
    float* d_ent_accum) {
    extern __shared__ float lds[];
    const int R = 1 << lgR, pitch = A | 1, Dp = D | 1, Wp = W | 1, DR = D << lgR;
    float* tile = lds;                               // [R][pitch]
    float* st = tile + R * pitch;                    // [5][D][R]: M, s, ls, lp, H of item d·R + r
    float* gro = st + 5 * DR;                        // [R]: the row's g
    float* aidx = gro + R;                           // [R][Dp]: the stored indices, clamped on read
    uint32_t* mw = (uint32_t*)(aidx + R * Dp);       // [R][Wp]: the rows' mask words
    int* offs = (int*)(mw + R * Wp);                 // [D + 1]
    float* red = (float*)(offs + D + 1);             // [WAVES]
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x << lgR;
    const int nr = (int)min((long)R, (long)m - r0);
    const long base = r0 * A;
    for (int e = tid; e < nr * A; e += TPB) {
        const int row = e / A, k = e - row * A;
        tile[row * pitch + k] = logits[base + e];
    }
    for (int e = tid; e < nr * D; e += TPB) {
        const int row = e / D, d = e - row * D;
        aidx[row * Dp + d] = action[(r0 + row) * A + d];
    }
    for (int e = tid; e < nr * W; e += TPB) {
        const int row = e / W, j = e - row * W;
        const long src = rows ? (long)rows[r0 + row] : r0 + row;
        mw[row * Wp + j] = mask[src * W + j];
    }
    for (int d = tid; d <= D; d += TPB) offs[d] = off[d];
    __syncthreads();

    if (WIDE) {
        const int lane = tid & 63;
        for (int it = tid >> 6; it < DR; it += WAVES) {          // uniform over the wave
            const int d = it >> lgR, r = it & (R - 1);
            if (r >= nr) continue;
            const int o = offs[d], n = offs[d + 1] - o;
            const int a = ppo::cat_index(aidx[r * Dp + d], n);
            const ppo::MaskComp mc = ppo::mask_component(mw + r * Wp, o, n, a);
            const ppo::MdComp c = masked_component_wave(tile + r * pitch + o, n, a, mc, lane);
            if (lane == 0) {
                st[it] = c.M; st[DR + it] = c.s; st[2 * DR + it] = c.ls; st[3 * DR + it] = c.lp; st[4 * DR + it] = c.H;
            }
        }
    } else {
        for (int it = tid; it < DR; it += TPB) {
            const int d = it >> lgR, r = it & (R - 1);
            if (r >= nr) continue;
            const int o = offs[d], n = offs[d + 1] - o;
            const int a = ppo::cat_index(aidx[r * Dp + d], n);
            const ppo::MaskComp mc = ppo::mask_component(mw + r * Wp, o, n, a);
            const ppo::MdComp c = ppo::md_component_masked(tile + r * pitch + o, n, a, mc);
            st[it] = c.M; st[DR + it] = c.s; st[2 * DR + it] = c.ls; st[3 * DR + it] = c.lp; st[4 * DR + it] = c.H;
        }
    }
    __syncthreads();

    float sur = 0.f, H = 0.f;
    if (tid < nr) {                                  // R <= TPB: one lane per row
        float lp = st[3 * DR + tid];
        H = st[4 * DR + tid];
        for (int d = 1; d < D; ++d) {
            lp += st[3 * DR + (d << lgR) + tid];
            H += st[4 * DR + (d << lgR) + tid];
        }
        const long i = r0 + tid;
        float g;
        sur = ppo::surrogate(adv[i], lp, old_lp[i], eps, m, &g);
        gro[tid] = g;
        if (lp_out) lp_out[i] = lp;
        if (ent_out) ent_out[i] = H;
    }
    __syncthreads();

    const float cm = ent_coeff / m;
    if (WIDE) {
        const int lane = tid & 63;
        for (int it = tid >> 6; it < DR; it += WAVES) {
            const int d = it >> lgR, r = it & (R - 1);
            if (r >= nr) continue;
            const int o = offs[d], n = offs[d + 1] - o;
            const int a = ppo::cat_index(aidx[r * Dp + d], n);
            const ppo::MaskComp mc = ppo::mask_component(mw + r * Wp, o, n, a);
            const float M = st[it], s = st[DR + it], ls = st[2 * DR + it], Hd = st[4 * DR + it], g = gro[r];
            float* zr = tile + r * pitch + o;
            for (int k = lane; k < n; k += 64)
                zr[k] = mc.allowed(k) ? ppo::cat_grad(g, k == a, zr[k], M, s, ls, Hd, cm) : 0.f;
        }
    } else {
        for (int it = tid; it < DR; it += TPB) {
            const int d = it >> lgR, r = it & (R - 1);
            if (r >= nr) continue;
            const int o = offs[d], n = offs[d + 1] - o;
            const int a = ppo::cat_index(aidx[r * Dp + d], n);
            const ppo::MaskComp mc = ppo::mask_component(mw + r * Wp, o, n, a);
            const float M = st[it], s = st[DR + it], ls = st[2 * DR + it], Hd = st[4 * DR + it], g = gro[r];
            float* zr = tile + r * pitch + o;
            for (int k = 0; k < n; ++k)
                zr[k] = mc.allowed(k) ? ppo::cat_grad(g, k == a, zr[k], M, s, ls, Hd, cm) : 0.f;
        }
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

// ------------------------------------------------------------------ sampler / greedy action: one lane per row
// row e of `logits` under row e of `mask`; the action, the joint log-prob and (mask_out) the mask go to row rows[e]
// (NULL: e)
__global__ void masked_sample_kernel(const float* __restrict__ logits, const uint32_t* __restrict__ mask,
                                     const int* __restrict__ rows, const int* __restrict__ off,
                                     float* __restrict__ action, float* __restrict__ logprob,
                                     uint32_t* __restrict__ mask_out, int m, int A, int D, int W, uint64_t key,
                                     uint64_t offset) {
    const long e = (long)blockIdx.x * TPB + threadIdx.x;
    if (e >= m) return;
    const long row = rows ? rows[e] : e;
    const uint32_t* mr = mask + e * W;
    float* ar = action + row * A;
    float lp = 0.f;
    u32x4 w = {0u, 0u, 0u, 0u};
    for (int d = 0; d < D; ++d) {
        const int o = off[d], n = off[d + 1] - o;
        const float* z = logits + e * A + o;
        if ((d & 3) == 0) w = philox((uint64_t)e | ((uint64_t)(d >> 2) << 32), offset, key);
        const uint32_t word = (d & 3) == 0 ? w.x : ((d & 3) == 1 ? w.y : ((d & 3) == 2 ? w.z : w.w));
        const ppo::MaskComp mc = ppo::mask_component(mr, o, n, -1);
        const float M = ppo::masked_row_max(z, n, mc);
        const float s = ppo::masked_row_sum(z, n, M, mc, nullptr);
        const float thr = u01(word) * s;
        int a = 0;                                   // ends as the last allowed column unless the CDF is met first
        float c = 0.f;
        for (int k = 0; k < n; ++k) {
            if (!mc.allowed(k)) continue;
            a = k;
            c += ppo::cat_exp(z[k], M);
            if (thr <= c) break;
        }
        ar[d] = (float)a;
        const float l = ppo::cat_log_prob(z[a], M, logf(s));
        lp = d == 0 ? l : lp + l;
    }
    for (int k = D; k < A; ++k) ar[k] = 0.f;
    if (logprob) logprob[row] = lp;
    if (mask_out)
        for (int j = 0; j < W; ++j) mask_out[row * W + j] = mr[j];
}

// per component the lowest allowed index holding the maximum over the allowed columns; action [m, A] compact
__global__ void masked_argmax_kernel(const float* __restrict__ logits, const uint32_t* __restrict__ mask,
                                     const int* __restrict__ off, float* __restrict__ action, int m, int A, int D,
                                     int W) {
    const long e = (long)blockIdx.x * TPB + threadIdx.x;
    if (e >= m) return;
    float* ar = action + e * A;
    for (int d = 0; d < D; ++d) {
        const int o = off[d], n = off[d + 1] - o;
        const float* z = logits + e * A + o;
        const ppo::MaskComp mc = ppo::mask_component(mask + e * W, o, n, -1);
        int a = -1;
        float best = 0.f;
        for (int k = 0; k < n; ++k) {
            if (!mc.allowed(k)) continue;
            if (a < 0 || z[k] > best) { best = z[k]; a = k; }
        }
        ar[d] = (float)a;
    }
    for (int k = D; k < A; ++k) ar[k] = 0.f;
}

// rows[e]'s W words ← all ones (a step laid by the unmasked sampler while masking is on)
__global__ void mask_fill_rows_kernel(uint32_t* __restrict__ mask, const int* __restrict__ rows, int E, int W) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long)E * W) return;
    const long e = i / W, j = i - e * W;
    mask[(long)rows[e] * W + j] = ~0u;
}

bool shape_ok(int A, int D, int W) { return A >= 2 && A <= PHIP_CAT_MAX_A && D >= 1 && 2 * D <= A && W == (A + 31) / 32; }

}  // namespace

extern "C" {

void phip_masked_head(const float* logits, const float* action, const float* adv, const float* old_lp,
                      const uint32_t* mask, const int* rows, int m, int A, const int* d_off, int D, int max_n,
                      float epsilon, float ent_coeff, float* grad, float* lp_out, float* ent_out, float* d_loss_accum,
                      float* d_ent_accum) {
    if (m <= 0) return;
    const int W = (A + 31) / 32;
    PPO_REQUIRE(shape_ok(A, D, W) && D <= PHIP_MD_MAX_D && max_n >= 2 && max_n <= A,
                "phip_masked_head: shape out of range");
    PPO_REQUIRE(logits && action && adv && old_lp && grad && d_off && mask, "phip_masked_head: operands");
    int lgR = 8;                                     // R <= TPB: phase 3 is one lane per row
    while (lgR > 0 && masked_lds_bytes(A, D, W, 1 << lgR) > (size_t)MASKED_LDS_BUDGET) --lgR;
    PPO_REQUIRE(masked_lds_bytes(A, D, W, 1 << lgR) <= (size_t)MASKED_LDS_BUDGET,
                "phip_masked_head: one row exceeds the LDS budget");
    while (lgR > 0 && (1 << (lgR - 1)) >= m) --lgR;  // a minibatch smaller than the tile: no LDS left unused
    const size_t lds = masked_lds_bytes(A, D, W, 1 << lgR);
    const int grid = ppo_divup(m, 1 << lgR);
    ppo::ProfScope ps(PPO_K_HEAD, 4.0 * m * (2.0 * A + D + 2 + W));
    if (max_n > 32)
        hipLaunchKernelGGL(masked_head_kernel<true>, dim3(grid), dim3(TPB), lds, ppo::stream(), logits, action, adv,
                           old_lp, mask, rows, d_off, m, A, D, W, lgR, epsilon, ent_coeff, grad, lp_out, ent_out,
                           d_loss_accum, d_ent_accum);
    else
        hipLaunchKernelGGL(masked_head_kernel<false>, dim3(grid), dim3(TPB), lds, ppo::stream(), logits, action, adv,
                           old_lp, mask, rows, d_off, m, A, D, W, lgR, epsilon, ent_coeff, grad, lp_out, ent_out,
                           d_loss_accum, d_ent_accum);
    PPO_LAUNCH_CHECK();
}

void phip_masked_sample(const float* logits, const uint32_t* mask, const int* rows, const int* d_off, float* action,
                        float* logprob, uint32_t* mask_out, int m, int A, int D, uint64_t key, uint64_t offset) {
    if (m <= 0) return;
    const int W = (A + 31) / 32;
    PPO_REQUIRE(shape_ok(A, D, W) && logits && mask && action && d_off, "phip_masked_sample: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * (2.0 * A + 1 + 2.0 * W));
    hipLaunchKernelGGL(masked_sample_kernel, dim3(ppo_divup(m, TPB)), dim3(TPB), 0, ppo::stream(), logits, mask, rows,
                       d_off, action, logprob, mask_out, m, A, D, W, key, offset);
    PPO_LAUNCH_CHECK();
}

void phip_masked_sample_rows(const float* logits, const uint32_t* mask, const int* rows, const int* d_off,
                             float* action, float* logprob, uint32_t* mask_out, int E, int A, int D, uint64_t key,
                             uint64_t step) {
    phip_masked_sample(logits, mask, rows, d_off, action, logprob, mask_out, E, A, D, key, kNoise + step);
}

void phip_masked_argmax(const float* logits, const uint32_t* mask, const int* d_off, float* action, int m, int A,
                        int D) {
    if (m <= 0) return;
    const int W = (A + 31) / 32;
    PPO_REQUIRE(shape_ok(A, D, W) && logits && mask && action && d_off, "phip_masked_argmax: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * (2.0 * A + W));
    hipLaunchKernelGGL(masked_argmax_kernel, dim3(ppo_divup(m, TPB)), dim3(TPB), 0, ppo::stream(), logits, mask,
                       d_off, action, m, A, D, W);
    PPO_LAUNCH_CHECK();
}

void phip_mask_fill_rows(uint32_t* mask, const int* rows, int E, int A) {
    if (E <= 0) return;
    const int W = (A + 31) / 32;
    PPO_REQUIRE(mask && rows && A >= 1, "phip_mask_fill_rows: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * E * W);
    hipLaunchKernelGGL(mask_fill_rows_kernel, dim3(ppo_divup((long)E * W, TPB)), dim3(TPB), 0, ppo::stream(), mask,
                       rows, E, W);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
