// multidiscrete.hip — the multi-discrete policy (ppo_set_action_multidiscrete; no counterpart in the reference):
// μ's A outputs are D softmaxes side by side, component d over the logits [o_d, o_d + n_d).  The joint log-prob
// and the entropy of a row are the d-ascending sums of the components', one clipped surrogate runs on the joint
// ratio, and a logit's gradient takes its own component's entropy.  The definition is ppo_math.h's (the cat_*
// atoms, md_component, md_log_prob_row), called, never restated.  D = 1 is categorical.hip's policy bit for bit.
//
// HEAD.  One launch per policy step; logits [m, A] read once, gradient [m, A] written once, both coalesced: the
// traffic is 2·m·A·4 bytes plus (D + 2)·4 per row (the D stored indices, advantage, old log-prob), so the kernel
// is memory-bound.  The gradient of every component needs g = ∂loss/∂lp, which needs all D components' lp_d: two
// phases over a tile that stays in LDS.  A workgroup (256 lanes) owns R rows, R a power of two chosen by the
// launcher so that the tile and the per-(row, component) records fit MD_LDS_BUDGET (40 KB: four workgroups share
// a CU's 160 KB, and no opt-in attribute is needed):
//   1. the R × A logits go to LDS by coalesced loads at the odd row pitch A | 1; the R × D indices likewise at
//      the odd pitch D | 1; the offsets o_0 … o_D once;
//   2. item (d, r) — numbered d·R + r, so the lanes of a wave walk neighbouring rows of one component: their LDS
//      addresses differ by the odd pitch (no bank conflict) and their loops have one length — makes its
//      component's passes from LDS and leaves M_d, s_d, ls_d, lp_d, H_d in LDS ([5][D][R]);
//   3. barrier; lane r < R sums lp and H with d ascending (stride-1 LDS reads), takes the surrogate, leaves g;
//   4. barrier; item (d, r) overwrites its segment of the tile with the gradient;
//   5. barrier; the tile is stored coalesced.
// LDS per row: (A | 1) + 5·D + 1 + (D | 1) floats — 888 bytes at nvec = [7]·17 (R = 32, 28 KB a workgroup), 8.2 KB
// at [2]·256 (R = 4), 16.4 KB at [4096] (R = 2).
// Items: every n_d <= 32 — one lane per item (md_component: k ascending in the lane, dist 1's lane kernel's
// order, hence its bits at D = 1).  Some n_d > 32 — the wide form, one wave per item: a component with n_d <= 32
// is still walked k ascending (every lane of the wave walks it, the reads broadcast); a wider one has lane l sum
// k = l, l + 64, … ascending and the lanes combine by dev.h's fixed trees (wave_max64 below, wave_sum64).  Correct
// for every legal nvec; only the one-lane form is shaped for speed.
// The two cross-row sums follow categorical.hip: one fp32 partial per workgroup by a fixed tree, one atomic into
// the loss word and one into the entropy word.
//
// SAMPLER / ARGMAX.  One lane per row walks the D components: component d draws u01 of word d & 3 of
// philox(e | (d >> 2) << 32, offset, key) and inverts its own CDF exactly as categorical.hip's sampler; columns
// 0 … D−1 take the indices, D … A−1 are zeroed, the log-prob is the joint one.  rng.h lists the streams.
#include "dev.h"
#include "ppo_math.h"
#include "rng.h"

#include <cmath>

namespace {

using namespace ppo_rng;

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MD_LDS_BUDGET = 40 * 1024;

// wave max on DPP moves, the tree of dev.h's wave_sum64 (categorical.hip's): every lane gets the wave's value
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

// floats of LDS one row of the tile needs, and the launch's total in bytes
__host__ __device__ inline int md_row_floats(int A, int D) { return (A | 1) + 5 * D + 1 + (D | 1); }
inline size_t md_lds_bytes(int A, int D, int R) {
    return sizeof(float) * ((size_t)R * md_row_floats(A, D) + (D + 1) + WAVES);
}

// one component of one row by a whole wave (the wide form; every lane active, every lane gets the record)
__device__ __forceinline__ ppo::MdComp md_component_wave(const float* z, int n, int a, int lane) {
    if (n <= 32) return ppo::md_component(z, n, a);
    ppo::MdComp c;
    float M = -INFINITY;
    for (int k = lane; k < n; k += 64) M = fmaxf(M, z[k]);
    c.M = wave_max64(M);
    float s = 0.f, t = 0.f;
    for (int k = lane; k < n; k += 64) {
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
__global__ __launch_bounds__(TPB) void md_head_kernel(
    const float* __restrict__ logits, const float* __restrict__ action, const float* __restrict__ adv,
    const float* __restrict__ old_lp, const int* __restrict__ off, int m, int A, int D, int lgR, float eps,
    float ent_coeff, float* __restrict__ grad, float* __restrict__ lp_out, float* __restrict__ ent_out,
    float* d_loss_accum, float* d_ent_accum) {
    extern __shared__ float lds[];
    const int R = 1 << lgR, pitch = A | 1, Dp = D | 1, DR = D << lgR;
    float* tile = lds;                               // [R][pitch]
    float* st = tile + R * pitch;                    // [5][D][R]: M, s, ls, lp, H of item d·R + r
    float* gro = st + 5 * DR;                        // [R]: the row's g
    float* aidx = gro + R;                           // [R][Dp]: the stored indices, clamped on read
    int* offs = (int*)(aidx + R * Dp);               // [D + 1]
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
    for (int d = tid; d <= D; d += TPB) offs[d] = off[d];
    __syncthreads();

    if (WIDE) {
        const int lane = tid & 63;
        for (int it = tid >> 6; it < DR; it += WAVES) {          // uniform over the wave
            const int d = it >> lgR, r = it & (R - 1);
            if (r >= nr) continue;
            const int o = offs[d], n = offs[d + 1] - o;
            const int a = ppo::cat_index(aidx[r * Dp + d], n);
            const ppo::MdComp c = md_component_wave(tile + r * pitch + o, n, a, lane);
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
            const ppo::MdComp c = ppo::md_component(tile + r * pitch + o, n, a);
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
            const float M = st[it], s = st[DR + it], ls = st[2 * DR + it], Hd = st[4 * DR + it], g = gro[r];
            float* zr = tile + r * pitch + o;
            for (int k = lane; k < n; k += 64) zr[k] = ppo::cat_grad(g, k == a, zr[k], M, s, ls, Hd, cm);
        }
    } else {
        for (int it = tid; it < DR; it += TPB) {
            const int d = it >> lgR, r = it & (R - 1);
            if (r >= nr) continue;
            const int o = offs[d], n = offs[d + 1] - o;
            const int a = ppo::cat_index(aidx[r * Dp + d], n);
            const float M = st[it], s = st[DR + it], ls = st[2 * DR + it], Hd = st[4 * DR + it], g = gro[r];
            float* zr = tile + r * pitch + o;
            for (int k = 0; k < n; ++k) zr[k] = ppo::cat_grad(g, k == a, zr[k], M, s, ls, Hd, cm);
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
// row e of `logits`; the action and the joint log-prob go to row rows[e] (NULL: e)
__global__ void md_sample_kernel(const float* __restrict__ logits, const int* __restrict__ rows,
                                 const int* __restrict__ off, float* __restrict__ action,
                                 float* __restrict__ logprob, int m, int A, int D, uint64_t key, uint64_t offset) {
    const long e = (long)blockIdx.x * TPB + threadIdx.x;
    if (e >= m) return;
    const long row = rows ? rows[e] : e;
    float* ar = action + row * A;
    float lp = 0.f;
    u32x4 w = {0u, 0u, 0u, 0u};
    for (int d = 0; d < D; ++d) {
        const int o = off[d], n = off[d + 1] - o;
        const float* z = logits + e * A + o;
        if ((d & 3) == 0) w = philox((uint64_t)e | ((uint64_t)(d >> 2) << 32), offset, key);
        const uint32_t word = (d & 3) == 0 ? w.x : ((d & 3) == 1 ? w.y : ((d & 3) == 2 ? w.z : w.w));
        const float M = ppo::cat_row_max(z, n);
        const float s = ppo::cat_row_sum(z, n, M, nullptr);
        const float thr = u01(word) * s;
        int a = n - 1;                               // the clamp: u <= 1 gives thr <= c_{n−1} already
        float c = 0.f;
        for (int k = 0; k < n; ++k) {
            c += ppo::cat_exp(z[k], M);
            if (thr <= c) { a = k; break; }
        }
        ar[d] = (float)a;
        const float l = ppo::cat_log_prob(z[a], M, logf(s));
        lp = d == 0 ? l : lp + l;
    }
    for (int k = D; k < A; ++k) ar[k] = 0.f;
    if (logprob) logprob[row] = lp;
}

// per component argmax_k z_k, the lowest index on ties; action [m, A] compact
__global__ void md_argmax_kernel(const float* __restrict__ logits, const int* __restrict__ off,
                                 float* __restrict__ action, int m, int A, int D) {
    const long e = (long)blockIdx.x * TPB + threadIdx.x;
    if (e >= m) return;
    float* ar = action + e * A;
    for (int d = 0; d < D; ++d) {
        const int o = off[d], n = off[d + 1] - o;
        const float* z = logits + e * A + o;
        int a = 0;
        float best = z[0];
        for (int k = 1; k < n; ++k)
            if (z[k] > best) { best = z[k]; a = k; }
        ar[d] = (float)a;
    }
    for (int k = D; k < A; ++k) ar[k] = 0.f;
}

}  // namespace

extern "C" {

void phip_md_head(const float* logits, const float* action, const float* adv, const float* old_lp, int m, int A,
                  const int* d_off, int D, int max_n, float epsilon, float ent_coeff, float* grad, float* lp_out,
                  float* ent_out, float* d_loss_accum, float* d_ent_accum) {
    if (m <= 0) return;
    PPO_REQUIRE(A >= 2 && A <= PHIP_CAT_MAX_A && D >= 1 && D <= PHIP_MD_MAX_D && 2 * D <= A && max_n >= 2 &&
                    max_n <= A,
                "phip_md_head: shape out of range");
    PPO_REQUIRE(logits && action && adv && old_lp && grad && d_off, "phip_md_head: operands");
    int lgR = 8;                                     // R <= TPB: phase 3 is one lane per row
    while (lgR > 0 && md_lds_bytes(A, D, 1 << lgR) > (size_t)MD_LDS_BUDGET) --lgR;
    PPO_REQUIRE(md_lds_bytes(A, D, 1 << lgR) <= (size_t)MD_LDS_BUDGET, "phip_md_head: one row exceeds the LDS budget");
    while (lgR > 0 && (1 << (lgR - 1)) >= m) --lgR;  // a minibatch smaller than the tile: no LDS left unused
    const size_t lds = md_lds_bytes(A, D, 1 << lgR);
    const int grid = ppo_divup(m, 1 << lgR);
    ppo::ProfScope ps(PPO_K_HEAD, 4.0 * m * (2.0 * A + D + 2));
    if (max_n > 32)
        hipLaunchKernelGGL(md_head_kernel<true>, dim3(grid), dim3(TPB), lds, ppo::stream(), logits, action, adv,
                           old_lp, d_off, m, A, D, lgR, epsilon, ent_coeff, grad, lp_out, ent_out, d_loss_accum,
                           d_ent_accum);
    else
        hipLaunchKernelGGL(md_head_kernel<false>, dim3(grid), dim3(TPB), lds, ppo::stream(), logits, action, adv,
                           old_lp, d_off, m, A, D, lgR, epsilon, ent_coeff, grad, lp_out, ent_out, d_loss_accum,
                           d_ent_accum);
    PPO_LAUNCH_CHECK();
}

void phip_md_sample(const float* logits, const int* rows, const int* d_off, float* action, float* logprob, int m,
                    int A, int D, uint64_t key, uint64_t offset) {
    if (m <= 0) return;
    PPO_REQUIRE(A >= 2 && D >= 1 && 2 * D <= A && logits && action && d_off, "phip_md_sample: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * (2.0 * A + 1));
    hipLaunchKernelGGL(md_sample_kernel, dim3(ppo_divup(m, TPB)), dim3(TPB), 0, ppo::stream(), logits, rows, d_off,
                       action, logprob, m, A, D, key, offset);
    PPO_LAUNCH_CHECK();
}

void phip_md_sample_rows(const float* logits, const int* rows, const int* d_off, float* action, float* logprob, int E,
                         int A, int D, uint64_t key, uint64_t step) {
    phip_md_sample(logits, rows, d_off, action, logprob, E, A, D, key, kNoise + step);
}

void phip_md_argmax(const float* logits, const int* d_off, float* action, int m, int A, int D) {
    if (m <= 0) return;
    PPO_REQUIRE(A >= 2 && D >= 1 && 2 * D <= A && logits && action && d_off, "phip_md_argmax: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * (2.0 * A));
    hipLaunchKernelGGL(md_argmax_kernel, dim3(ppo_divup(m, TPB)), dim3(TPB), 0, ppo::stream(), logits, d_off, action,
                       m, A, D);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
