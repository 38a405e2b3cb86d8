// kl.hip — approximate KL and clip fraction of a policy minibatch step, and the target-KL stop decision,
// on the device (no counterpart in the reference).
//
// One launch per policy minibatch step, after the step's forward has left μ in HBM and before its Adam:
//   lp_i  = Gaussian log-prob of action_i under (μ_i, log σ)           (ppo_math.h log_prob_row, as the loss)
//           — or, with a categorical policy (dist 1), cat_log_prob_row of the index in the action's column 0
//           under the logits μ_i; or, with a multi-discrete policy (dist 2), md_log_prob_row: the joint log-prob
//           of the indices in columns 0 … D−1; nothing else differs.  With action masking (mask not NULL; dist 2,
//           the categorical policy as nvec = {A}): md_log_prob_row under the W words at mask[rows[i]·W] (rows
//           NULL: i) — the masked head's lp; mask NULL is the unmasked path and its bits
//   x_i   = (double)lp_i − (double)old_lp_i
//   kl    = Σ (expm1(x_i) − x_i) / rows          (Schulman's k3 estimator; double: (r − 1) − log r cancels in fp32)
//   frac  = Σ 1[|(float)exp(x_i) − 1| > ε] / rows
//   if (!stopped && kl > 1.5f · target_kl) { stopped = 1; stop_step = step; }      (Stable-Baselines3's rule)
// With the KL-adaptive learning-rate schedule on (ppo_set_lr_schedule, PPO_LR_ADAPTIVE) the same decision first moves
// the record's rate: lr /= 1.5 (floor lr_min) when kl > 2·desired_kl, lr *= 1.5 (cap lr_max) when 0 < kl < desired_kl/2;
// lr_hist[step] keeps the rate the step's Adam then reads through a pointer.
// left in a device record; the step's Adam reads `stopped` through a pointer (adam.hip) and takes no step once
// it is set.  The host never reads the record inside an epoch.
//
// Deterministic by construction, as clip.hip: the grid is a function of m only, every thread sums its
// grid-stride rows in index order in double, a workgroup folds its 256 sums by a fixed LDS tree, and the last
// workgroup to arrive folds the ≤ 256 workgroup partials by the same tree — no floating-point atomic.  The tree
// (block_sum_halving) and the hand-off (ticket_publish / ticket_load, two 8-byte partials per workgroup) are
// reduce.h's, which holds the ordering argument.
//
// Without a communicator the last arriver takes the decision itself (one launch per step).  With one, it only
// writes the local sums; the caller all-reduces those four floats and kl_decide_kernel decides from the global
// sums, so every rank takes the same decision from the same bits.
#include "dev.h"
#include "ppo_math.h"
#include "reduce.h"

namespace {

constexpr int TPB = 256;

// reduce.h's halving tree over the workgroup's 256 doubles
__device__ __forceinline__ double block_sum(double v, double* s) { return ppo::block_sum_halving<TPB>(v, s); }

// one thread, from rec->sums (local, or all-reduced over the ranks): the step's statistics and the decision
__device__ __forceinline__ void decide(PhipKlRec* rec, float target_kl, double rows_global) {
    const float kl = (float)((double)rec->sums[0] / rows_global);
    rec->kl = kl;
    rec->clip_frac = (float)((double)rec->sums[1] / rows_global);
    unsigned stopped = rec->stopped;
    const unsigned step = rec->step;
    /* the KL-adaptive learning rate (lr_kl = desired_kl; 0: the schedule is off and nothing here runs): rl_games' /
     * rsl_rl's rule on this step's kl, in fp32 with IEEE division and product, before the stop test; once the update
     * has stopped the rate stays.  The step's Adam launches read rec->lr behind this launch (adam.hip, RateWord). */
    const float want = rec->lr_kl;
    if (want > 0.f) {
        float lr = rec->lr;
        if (!stopped) {
            if (kl > 2.0f * want) {                       // NaN compares false on both branches: nothing changes
                lr = fmaxf(rec->lr_min, lr / 1.5f);
                rec->lr_lowered += 1u;
            } else if (kl < 0.5f * want && kl > 0.0f) {
                lr = fminf(rec->lr_max, lr * 1.5f);
                rec->lr_raised += 1u;
            }
            rec->lr = lr;
        }
        if (step < (unsigned)PHIP_KL_HIST) rec->lr_hist[step] = lr;
    }
    if (!stopped && kl > 1.5f * target_kl) {          // NaN compares false: never stops
        stopped = 1u;
        rec->stopped = 1u;
        rec->stop_step = (int)step;
    }
    if (step < (unsigned)PHIP_KL_HIST) rec->hist[step] = kl;
    rec->step = step + 1u;
    rec->applied += stopped ? 0u : 1u;
}

__global__ void __launch_bounds__(TPB) kl_sum_kernel(const float* __restrict__ mu, const float* __restrict__ log_std,
                                                     const float* __restrict__ action,
                                                     const float* __restrict__ old_lp, int m, int A, int dist,
                                                     float eps, float target_kl, double rows_global, int decide_here,
                                                     PhipKlRec* rec, const int* __restrict__ md_off, int D,
                                                     const uint32_t* __restrict__ mask, const int* __restrict__ rows) {
    __shared__ double s[TPB + 1];             // s[TPB]: "this workgroup drew the last ticket"
    double kl = 0.0, cnt = 0.0;
    for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < m; i += (long)gridDim.x * TPB) {
        const int W = (A + 31) / 32;
        const float lp = mask      ? ppo::md_log_prob_row(mu + i * A, md_off, D, action + i * A,
                                                          ppo::MaskRow{mask + (rows ? (long)rows[i] : i) * W})
                         : dist == 2 ? ppo::md_log_prob_row(mu + i * A, md_off, D, action + i * A, ppo::NoMask{})
                         : dist  ? ppo::cat_log_prob_row(mu + i * A, A, ppo::cat_index(action[i * A], A))
                                 : ppo::log_prob_row(mu + i * A, log_std, action + i * A, A);
        const double x = (double)lp - (double)old_lp[i];
        kl += expm1(x) - x;
        cnt += fabsf((float)exp(x) - 1.0f) > eps ? 1.0 : 0.0;
    }
    const double part_kl = block_sum(kl, s);
    const double part_cnt = block_sum(cnt, s);

    const double part[2] = {part_kl, part_cnt};
    if (!ppo::ticket_publish(&rec->partial[2 * blockIdx.x], part, &rec->ticket, &s[TPB])) return;

    // the last workgroup: every partial of this launch is visible; fold them in index order
    double pk = 0.0, pc = 0.0;
    if (threadIdx.x < gridDim.x) {
        pk = ppo::ticket_load(&rec->partial[2 * threadIdx.x]);
        pc = ppo::ticket_load(&rec->partial[2 * threadIdx.x + 1]);
    }
    const double tk = block_sum(pk, s);
    const double tc = block_sum(pc, s);
    if (threadIdx.x == 0) {
        rec->sums[0] = (float)tk;
        rec->sums[1] = (float)tc;
        rec->sums[2] = 0.f;
        rec->sums[3] = 0.f;
        if (decide_here) decide(rec, target_kl, rows_global);
        __hip_atomic_store(&rec->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch's
    }
}

__global__ void kl_decide_kernel(PhipKlRec* rec, float target_kl, double rows_global) {
    if (blockIdx.x == 0 && threadIdx.x == 0) decide(rec, target_kl, rows_global);
}

// value-rate coupling, one thread, once per update ahead of the loops' fork: the value Adam's word for the whole
// update, lr_v = lr_V · (lr / base), base = clamp(lr_policy, lr_min, lr_max) — one fp32 division, one product
__global__ void lr_couple_kernel(PhipKlRec* rec, float lr_V, float base) {
    if (blockIdx.x == 0 && threadIdx.x == 0) rec->lr_v = lr_V * (rec->lr / base);
}

int grid_for(int m) {
    long g = ((long)m + TPB - 1) / TPB;
    if (g < 1) g = 1;
    if (g > PHIP_KL_PARTS) g = PHIP_KL_PARTS;
    return (int)g;
}

}  // namespace

extern "C" {

void phip_policy_kl(const float* mu, const float* log_std, const float* action, const float* old_lp, int m, int A,
                    int dist, float eps, float target_kl, long rows_global, int decide_here, PhipKlRec* rec,
                    const int* md_off, int D, const uint32_t* mask, const int* rows) {
    static_assert(PHIP_KL_PARTS <= TPB, "the last workgroup folds one pair of partials per thread");
    PPO_REQUIRE(m > 0 && A > 0 && rows_global > 0 && rec, "phip_policy_kl: shape");
    PPO_REQUIRE(dist != 2 || (md_off && D >= 1 && 2 * D <= A), "phip_policy_kl: multi-discrete offsets");
    PPO_REQUIRE(!mask || dist == 2, "phip_policy_kl: a mask needs the multi-discrete form (dist 1 as nvec = {A})");
    ppo::ProfScope ps(PPO_K_ADAM, 8.0 * (double)m * A + 4.0 * m);
    hipLaunchKernelGGL(kl_sum_kernel, dim3(grid_for(m)), dim3(TPB), 0, ppo::stream(), mu, log_std, action, old_lp, m,
                       A, dist, eps, target_kl, (double)rows_global, decide_here, rec, md_off, D, mask, rows);
    PPO_LAUNCH_CHECK();
}

void phip_kl_decide(PhipKlRec* rec, float target_kl, long rows_global) {
    PPO_REQUIRE(rows_global > 0 && rec, "phip_kl_decide: shape");
    ppo::ProfScope ps(PPO_K_ADAM, 64.0);
    hipLaunchKernelGGL(kl_decide_kernel, dim3(1), dim3(64), 0, ppo::stream(), rec, target_kl, (double)rows_global);
    PPO_LAUNCH_CHECK();
}

void phip_lr_couple(PhipKlRec* rec, float lr_V, float base) {
    PPO_REQUIRE(rec && base > 0.f, "phip_lr_couple: arguments");
    ppo::ProfScope ps(PPO_K_OTHER, 16.0);              // not an Adam launch: kept out of that class's counts
    hipLaunchKernelGGL(lr_couple_kernel, dim3(1), dim3(64), 0, ppo::stream(), rec, lr_V, base);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
