// discrete.hip — the discrete policies' tile head, sampler and greedy action (ppo_set_action_multidiscrete,
// ppo_set_action_dist(ppo, 1) as D = 1, ppo_set_action_mask; no counterpart in the reference), each defined once and
// instantiated with and without an action mask.  μ's A outputs are D softmaxes side by side, component d over the
// logits [o_d, o_d + n_d).  The joint log-prob and the entropy of a row are the d-ascending sums of the components',
// one clipped surrogate runs on the joint ratio, and a logit's gradient takes its own component's entropy.  The
// definition is ppo_math.h's (the cat_* atoms, md_component, md_log_prob_row, "Action masking"), called, never
// restated.  D = 1, offsets {0, A}, is the categorical policy bit for bit: its sampler, greedy action and masked head
// run here, its unmasked head is categorical.hip's.
//
// MASKS.  A row carries W = (A + 31) / 32 words, bit k & 31 of word k >> 5 = column k allowed; a component with no
// stored bit set reads as fully allowed; the head and the KL monitor also allow the chosen column.  Masked columns
// enter no max and no sum, their gradient is +0 and their logits never reach arithmetic.  Every kernel is a template
// over MASKED, and a launcher given a NULL mask launches the unmasked instantiation: it has no mask operand, no
// mask words in LDS and ppo_math.h's NoMask, whose allowed() is `true`, in place of the component mask.  A full
// mask skips nothing, so it gives the unmasked instantiation's bits.
//
// HEAD.  One launch per policy step; logits [m, A] read once, gradient [m, A] written once, both coalesced: the
// traffic is 2·m·A·4 bytes plus (D + 2)·4 per row (the D stored indices, advantage, old log-prob), so the kernel
// is memory-bound.  The gradient of every component needs g = ∂loss/∂lp, which needs all D components' lp_d: two
// phases over a tile that stays in LDS.  A workgroup (256 lanes) owns R rows, R a power of two chosen by the
// launcher so that the tile and the per-(row, component) records fit DISC_LDS_BUDGET (40 KB: four workgroups share
// a CU's 160 KB, and no opt-in attribute is needed):
//   1. the R × A logits go to LDS by coalesced loads at the odd row pitch A | 1; the R × D indices likewise at
//      the odd pitch D | 1; the offsets o_0 … o_D once.  MASKED: row i of the minibatch reads its W words at
//      mask[rows[i]·W] (rows NULL: i) — the buffer row the minibatch gather already hands the policy step, so no
//      gather launch is added — into mw[R][W | 1];
//   2. item (d, r) — numbered d·R + r, so the lanes of a wave walk neighbouring rows of one component: their LDS
//      addresses differ by the odd pitch (no bank conflict; the mask words' too) and their loops have one length —
//      makes its component's passes from LDS and leaves M_d, s_d, ls_d, lp_d, H_d in LDS ([5][D][R]).  MASKED: a
//      one-lane item folds its component's effective mask into one register word (mask_component) before its loops;
//   3. barrier; lane r < R sums lp and H with d ascending (stride-1 LDS reads), takes the surrogate, leaves g;
//   4. barrier; item (d, r) overwrites its segment of the tile with the gradient;
//   5. barrier; the tile is stored coalesced.
// LDS per row: (A | 1) + 5·D + 1 + (D | 1) words, and (W | 1) more when MASKED —
//   unmasked: 888 bytes at nvec = [7]·17 (R = 32, 28 KB a workgroup), 8.2 KB at [2]·256 (R = 4), 16.4 KB at [4096]
//             (R = 2);
//   masked:   908 bytes at [7]·17 (R = 32, 29 KB), 8.3 KB at [2]·256 (R = 4, 34 KB), 16.9 KB at [4096] (R = 2,
//             34 KB); the largest legal row (A = 4096, D = 256) is 23 KB, so every legal shape fits the budget with
//             R >= 1.
// Traffic per row when MASKED: the 4·W mask bytes more, at worst one more 128-byte line per scattered row.
// Items: every n_d <= 32 — one lane per item (md_component: k ascending in the lane, categorical.hip's lane
// kernel's order, hence its bits at D = 1).  Some n_d > 32 — the wide form, one wave per item: a component with
// n_d <= 32 is still walked k ascending (every lane of the wave walks it, the reads broadcast); a wider one has lane
// l sum k = l, l + 64, … ascending and the lanes combine by dev.h's fixed trees (wave_max64, wave_sum64).  Correct
// for every legal nvec; only the one-lane form is shaped for speed.
// The two cross-row sums follow categorical.hip: one fp32 partial per workgroup by a fixed tree, one atomic into
// the loss word and one into the entropy word.  R decides which rows share a partial.
//
// SAMPLER / ARGMAX.  One lane per row walks the D components: component d draws u = u01 of word d & 3 of
// philox(e | (d >> 2) << 32, offset, key), u ∈ (0, 1], and inverts its own CDF over the allowed columns:
// c accumulates e_k in fp32 over allowed k ascending, thr = u·s_d, the action is the first allowed k with thr <= c,
// the fallback the last allowed k.  Columns 0 … D−1 take the indices as exact floats, D … A−1 are zeroed, the
// log-prob is the joint one.  MASKED reads a dense mask [m, W] and also copies the row's W words to mask_out[row·W]
// when given one, so a rollout stores the mask it sampled under without another launch.  The greedy action is, per
// component, the lowest allowed index holding the maximum over the allowed columns.  rng.h lists the streams.
#include "dev.h"
#include "ppo_math.h"
#include "rng.h"

#include <cmath>

namespace {

using namespace ppo_rng;

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int DISC_LDS_BUDGET = 40 * 1024;

// the launch's LDS in bytes: R rows of the tile and their records, the offsets, the workgroup reduction
inline size_t disc_lds_bytes(int A, int D, int W, bool masked, int R) {
    const int row_words = (A | 1) + 5 * D + 1 + (D | 1) + (masked ? (W | 1) : 0);
    return sizeof(float) * ((size_t)R * row_words + (D + 1) + WAVES);
}

// one component of one row by a whole wave (the wide form; every lane active, every lane gets the record)
template <class Mask>
__device__ __forceinline__ ppo::MdComp component_wave(const float* z, int n, int a, const Mask& mc, int lane) {
    if (n <= 32) return ppo::md_component(z, n, a, mc);
    ppo::MdComp c;
    float M = -INFINITY;
    for (int k = lane; k < n; k += 64)
        if (mc.allowed(k)) M = fmaxf(M, z[k]);
    c.M = ppo::wave_max64(M);
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

// R = 1 << lgR rows per workgroup; WIDE: a wave per (row, component) item, else a lane; mask, rows and W are unread
// unless MASKED
template <bool WIDE, bool MASKED>
__global__ __launch_bounds__(TPB) void disc_head_kernel(
    const float* __restrict__ logits, const float* __restrict__ action, const float* __restrict__ adv,
    const float* __restrict__ old_lp, const uint32_t* __restrict__ mask, const int* __restrict__ rows,
    const int* __restrict__ off, int m, int A, int D, int W, int lgR, float eps, float ent_coeff,
    float* __restrict__ grad, float* __restrict__ lp_out, float* __restrict__ ent_out, float* d_loss_accum,
    float* d_ent_accum) {
    extern __shared__ float lds[];
    const int R = 1 << lgR, pitch = A | 1, Dp = D | 1, Wp = MASKED ? W | 1 : 0, DR = D << lgR;
    float* tile = lds;                               // [R][pitch]
    float* st = tile + R * pitch;                    // [5][D][R]: M, s, ls, lp, H of item d·R + r
    float* gro = st + 5 * DR;                        // [R]: the row's g
    float* aidx = gro + R;                           // [R][Dp]: the stored indices, clamped on read
    uint32_t* mw = (uint32_t*)(aidx + R * Dp);       // [R][Wp]: the rows' mask words (MASKED only)
    int* offs = (int*)(mw + R * Wp);                 // [D + 1]
    float* red = (float*)(offs + D + 1);             // [WAVES]
    const int tid = threadIdx.x, lane = tid & 63;
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
    if (MASKED)
        for (int e = tid; e < nr * W; e += TPB) {
            const int row = e / W, j = e - row * W;
            const long src = rows ? (long)rows[r0 + row] : r0 + row;
            mw[row * Wp + j] = mask[src * W + j];
        }
    for (int d = tid; d <= D; d += TPB) offs[d] = off[d];
    __syncthreads();

    // the items of this thread (WIDE: of its wave, uniform over the wave) and its columns inside an item
    const int it0 = WIDE ? tid >> 6 : tid, its = WIDE ? WAVES : TPB, k0 = WIDE ? lane : 0, ks = WIDE ? 64 : 1;
    for (int it = it0; it < DR; it += its) {
        const int d = it >> lgR, r = it & (R - 1);
        if (r >= nr) continue;
        const int o = offs[d], n = offs[d + 1] - o;
        const int a = ppo::cat_index(aidx[r * Dp + d], n);
        const auto mc = ppo::mask_row<MASKED>(mw + r * Wp).component(o, n, a);
        const float* zr = tile + r * pitch + o;
        const ppo::MdComp c = WIDE ? component_wave(zr, n, a, mc, lane) : ppo::md_component(zr, n, a, mc);
        if (!WIDE || lane == 0) {
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
    for (int it = it0; it < DR; it += its) {
        const int d = it >> lgR, r = it & (R - 1);
        if (r >= nr) continue;
        const int o = offs[d], n = offs[d + 1] - o;
        const int a = ppo::cat_index(aidx[r * Dp + d], n);
        const auto mc = ppo::mask_row<MASKED>(mw + r * Wp).component(o, n, a);
        const float M = st[it], s = st[DR + it], ls = st[2 * DR + it], Hd = st[4 * DR + it], g = gro[r];
        float* zr = tile + r * pitch + o;
        for (int k = k0; k < n; k += ks)
            zr[k] = mc.allowed(k) ? ppo::cat_grad(g, k == a, zr[k], M, s, ls, Hd, cm) : 0.f;
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

// ------------------------------------------------------------------ sampler / greedy action: one lane per row
// row e of `logits` (MASKED: under row e of `mask`); the action, the joint log-prob and (MASKED, mask_out) the mask
// go to row rows[e] (NULL: e)
template <bool MASKED>
__global__ void disc_sample_kernel(const float* __restrict__ logits, const uint32_t* __restrict__ mask,
                                   const int* __restrict__ rows, const int* __restrict__ off,
                                   float* __restrict__ action, float* __restrict__ logprob,
                                   uint32_t* __restrict__ mask_out, int m, int A, int D, int W, uint64_t key,
                                   uint64_t offset) {
    const long e = (long)blockIdx.x * TPB + threadIdx.x;
    if (e >= m) return;
    const long row = rows ? rows[e] : e;
    const uint32_t* mr = MASKED ? mask + e * W : nullptr;
    float* ar = action + row * A;
    float lp = 0.f;
    u32x4 w = {0u, 0u, 0u, 0u};
    for (int d = 0; d < D; ++d) {
        const int o = off[d], n = off[d + 1] - o;
        const float* z = logits + e * A + o;
        if ((d & 3) == 0) w = philox((uint64_t)e | ((uint64_t)(d >> 2) << 32), offset, key);
        const uint32_t word = (d & 3) == 0 ? w.x : ((d & 3) == 1 ? w.y : ((d & 3) == 2 ? w.z : w.w));
        const auto mc = ppo::mask_row<MASKED>(mr).component(o, n, -1);
        const float M = ppo::cat_row_max(z, n, mc);
        const float s = ppo::cat_row_sum(z, n, M, nullptr, mc);
        const float thr = u01(word) * s;
        int a = 0;                                   // ends as the last allowed column unless the CDF is met first
        float c = 0.f;                               // (u <= 1 gives thr <= the last c already)
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
    if (MASKED && mask_out)
        for (int j = 0; j < W; ++j) mask_out[row * W + j] = mr[j];
}

// per component the lowest allowed index holding the maximum over the allowed columns; action [m, A] compact
template <bool MASKED>
__global__ void disc_argmax_kernel(const float* __restrict__ logits, const uint32_t* __restrict__ mask,
                                   const int* __restrict__ off, float* __restrict__ action, int m, int A, int D,
                                   int W) {
    const long e = (long)blockIdx.x * TPB + threadIdx.x;
    if (e >= m) return;
    const uint32_t* mr = MASKED ? mask + e * W : nullptr;
    float* ar = action + e * A;
    for (int d = 0; d < D; ++d) {
        const int o = off[d], n = off[d + 1] - o;
        const float* z = logits + e * A + o;
        const auto mc = ppo::mask_row<MASKED>(mr).component(o, n, -1);
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

bool shape_ok(int A, int D) { return A >= 2 && A <= PHIP_CAT_MAX_A && D >= 1 && 2 * D <= A; }

}  // namespace

extern "C" {

void phip_disc_head(const float* logits, const float* action, const float* adv, const float* old_lp,
                    const uint32_t* mask, const int* rows, int m, int A, const int* d_off, int D, int max_n,
                    float epsilon, float ent_coeff, float* grad, float* lp_out, float* ent_out, float* d_loss_accum,
                    float* d_ent_accum) {
    if (m <= 0) return;
    const int W = (A + 31) / 32;
    const bool masked = mask != nullptr;
    PPO_REQUIRE(shape_ok(A, D) && D <= PHIP_MD_MAX_D && max_n >= 2 && max_n <= A, "phip_disc_head: shape out of range");
    PPO_REQUIRE(logits && action && adv && old_lp && grad && d_off, "phip_disc_head: operands");
    int lgR = 8;                                     // R <= TPB: phase 3 is one lane per row
    while (lgR > 0 && disc_lds_bytes(A, D, W, masked, 1 << lgR) > (size_t)DISC_LDS_BUDGET) --lgR;
    PPO_REQUIRE(disc_lds_bytes(A, D, W, masked, 1 << lgR) <= (size_t)DISC_LDS_BUDGET,
                "phip_disc_head: one row exceeds the LDS budget");
    while (lgR > 0 && (1 << (lgR - 1)) >= m) --lgR;  // a minibatch smaller than the tile: no LDS left unused
    const size_t lds = disc_lds_bytes(A, D, W, masked, 1 << lgR);
    const int grid = ppo_divup(m, 1 << lgR);
    ppo::ProfScope ps(PPO_K_HEAD, 4.0 * m * (2.0 * A + D + 2 + (masked ? W : 0)));
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(TPB), lds, ppo::stream(), logits, action, adv, old_lp, mask, rows,
                           d_off, m, A, D, W, lgR, epsilon, ent_coeff, grad, lp_out, ent_out, d_loss_accum,
                           d_ent_accum);
    };
    if (max_n > 32) masked ? launch(disc_head_kernel<true, true>) : launch(disc_head_kernel<true, false>);
    else masked ? launch(disc_head_kernel<false, true>) : launch(disc_head_kernel<false, false>);
    PPO_LAUNCH_CHECK();
}

void phip_disc_sample(const float* logits, const uint32_t* mask, const int* rows, const int* d_off, float* action,
                      float* logprob, uint32_t* mask_out, int m, int A, int D, uint64_t key, uint64_t offset) {
    if (m <= 0) return;
    const int W = (A + 31) / 32;
    PPO_REQUIRE(shape_ok(A, D) && logits && action && d_off && (mask || !mask_out), "phip_disc_sample: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * (2.0 * A + 1 + (mask ? 2.0 * W : 0.0)));
    hipLaunchKernelGGL(mask ? disc_sample_kernel<true> : disc_sample_kernel<false>, dim3(ppo_divup(m, TPB)), dim3(TPB),
                       0, ppo::stream(), logits, mask, rows, d_off, action, logprob, mask_out, m, A, D, W, key, offset);
    PPO_LAUNCH_CHECK();
}

void phip_disc_sample_rows(const float* logits, const uint32_t* mask, const int* rows, const int* d_off, float* action,
                           float* logprob, uint32_t* mask_out, int E, int A, int D, uint64_t key, uint64_t step) {
    phip_disc_sample(logits, mask, rows, d_off, action, logprob, mask_out, E, A, D, key, kNoise + step);
}

void phip_disc_argmax(const float* logits, const uint32_t* mask, const int* d_off, float* action, int m, int A,
                      int D) {
    if (m <= 0) return;
    const int W = (A + 31) / 32;
    PPO_REQUIRE(shape_ok(A, D) && logits && action && d_off, "phip_disc_argmax: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * (2.0 * A + (mask ? W : 0)));
    hipLaunchKernelGGL(mask ? disc_argmax_kernel<true> : disc_argmax_kernel<false>, dim3(ppo_divup(m, TPB)), dim3(TPB),
                       0, ppo::stream(), logits, mask, d_off, action, m, A, D, W);
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
