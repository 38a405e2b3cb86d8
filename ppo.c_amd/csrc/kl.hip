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
// The closed-form estimator (ppo_set_kl_estimator, PPO_KL_EXACT; `ex` not NULL): the same launch also sums, per row,
// ppo_math.h's KL(old ‖ new) between the behaviour distribution — row rows[i] of the store ppo_update filled at its
// head, read in place through the step's row indices — and the μ the forward just left.  It is a third double per
// thread, a third partial per workgroup (partial_x, three per workgroup) and sums[2]; k3 and the count are summed by
// the same threads in the same order and keep their bits.  decide() then takes sums[2] and keeps k3 beside it.
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

// one thread, from rec->sums (local, or all-reduced over the ranks): the step's statistics and the decision.
// EXACT: the deciding kl is the closed-form one (sums[2]); k3 goes to hist_other / kl_other.  Otherwise nothing
// behind lr_hist is touched.
template <bool EXACT>
__device__ __forceinline__ void decide(PhipKlRec* rec, float target_kl, double rows_global) {
    const float k3 = (float)((double)rec->sums[0] / rows_global);
    float kl = k3;
    if constexpr (EXACT) kl = (float)((double)rec->sums[2] / rows_global);
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
    if constexpr (EXACT) {
        if (step < (unsigned)PHIP_KL_HIST) rec->hist_other[step] = k3;
        rec->kl_other = k3;
    }
    rec->step = step + 1u;
    rec->applied += stopped ? 0u : 1u;
}

// ---- the closed-form estimator's wide rows: one wave per row, for a discrete policy with a component wider than
// 32.  Lane l sums its columns k = l, l + 64, … ascending through ppo_math.h's atoms; the lanes combine by the xor
// butterfly (offsets 32, 16 … 1), which leaves every lane the same bits — a row's value is a fixed-order function of
// its inputs and of nothing else.  A masked column is skipped before it is read.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <class RowMask>
__device__ __forceinline__ double wave_cat_row(const float* zo, const float* zn, const int* off, int D,
                                               const float* action, const RowMask& rm) {
    const int lane = threadIdx.x & 63;
    double kl = 0.0;
    for (int d = 0; d < D; ++d) {
        const int o = off[d], n = off[d + 1] - o;
        const int a = action ? ppo::cat_index(action[d], n) : -1;
        const auto mk = rm.component(o, n, a);
        int has = 0;
        float Mo = 0.f, Mn = 0.f;
        for (int k = lane; k < n; k += 64) {
            if (!mk.allowed(k)) continue;
            Mo = has ? fmaxf(Mo, zo[o + k]) : zo[o + k];
            Mn = has ? fmaxf(Mn, zn[o + k]) : zn[o + k];
            has = 1;
        }
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) {
            const float po = __shfl_xor(Mo, x, 64), pn = __shfl_xor(Mn, x, 64);
            const int ph = __shfl_xor(has, x, 64);
            if (ph) {
                Mo = has ? fmaxf(Mo, po) : po;
                Mn = has ? fmaxf(Mn, pn) : pn;
                has = 1;
            }
        }
        double so = 0.0, sn = 0.0;
        for (int k = lane; k < n; k += 64) {
            if (!mk.allowed(k)) continue;
            so += ppo::kl_cat_exp(zo[o + k], Mo);
            sn += ppo::kl_cat_exp(zn[o + k], Mn);
        }
        const double lso = log(wave_sum(so)), lsn = log(wave_sum(sn));
        double s = 0.0;
        for (int k = lane; k < n; k += 64) {
            if (!mk.allowed(k)) continue;
            s += ppo::kl_cat_term(ppo::kl_cat_logp(zo[o + k], Mo, lso), ppo::kl_cat_logp(zn[o + k], Mn, lsn));
        }
        kl += ppo::kl_cat_clamp(wave_sum(s));
    }
    return kl;
}

// EXACT = false: the k3 launch.  EXACT = true: the same rows by the same threads in the same order — thread t of a
// workgroup owns rows base + t, base = 256·(blockIdx + j·gridDim) — so the k3 sum and the count keep their bits,
// plus the row's closed-form KL into a third sum.  Under ex.wide the workgroup's wave w walks its 64 rows one after
// the other and hands row r's value to lane r, the thread that owns it.
template <bool EXACT>
__global__ void __launch_bounds__(TPB) kl_sum_kernel(const float* __restrict__ mu, const float* __restrict__ log_std,
                                                     const float* __restrict__ action,
                                                     const float* __restrict__ old_lp, int m, int A, int dist,
                                                     float eps, float target_kl, double rows_global, int decide_here,
                                                     PhipKlRec* rec, const int* __restrict__ md_off, int D,
                                                     const uint32_t* __restrict__ mask, const int* __restrict__ rows,
                                                     PhipKlExact ex, float sd_lo, float sd_hi) {
    __shared__ double s[TPB + 1];             // s[TPB]: "this workgroup drew the last ticket"
    double kl = 0.0, cnt = 0.0, klx = 0.0;
    const int W = (A + 31) / 32;
    for (long base = blockIdx.x * (long)TPB; base < m; base += (long)gridDim.x * TPB) {
        const long i = base + threadIdx.x;
        if (i < m && (!EXACT || old_lp)) {
            const float lp = dist == 3 ? ppo::sd_row(mu + i * A, action + i * A, A >> 1, sd_lo, sd_hi).lp
                             : mask    ? ppo::md_log_prob_row(mu + i * A, md_off, D, action + i * A,
                                                              ppo::MaskRow{mask + (rows ? (long)rows[i] : i) * W})
                             : dist == 2 ? ppo::md_log_prob_row(mu + i * A, md_off, D, action + i * A, ppo::NoMask{})
                             : dist  ? ppo::cat_log_prob_row(mu + i * A, A, ppo::cat_index(action[i * A], A))
                                     : ppo::log_prob_row(mu + i * A, log_std, action + i * A, A);
            const double x = (double)lp - (double)old_lp[i];
            kl += expm1(x) - x;
            cnt += fabsf((float)exp(x) - 1.0f) > eps ? 1.0 : 0.0;
        }
        if constexpr (EXACT) {
            if (!ex.wide) {
                if (i < m) {
                    const float* zo = ex.old_dist + (ex.rows ? (long)ex.rows[i] : i) * A;
                    const float* act = mask ? action + i * A : nullptr;
                    const double r = dist == 3 ? ppo::sd_kl_row(zo, mu + i * A, A >> 1, sd_lo, sd_hi)
                                     : !ex.off ? ppo::kl_gauss_row(zo, ex.old_log_std, mu + i * A, log_std, A)
                                     : mask  ? ppo::kl_cat_row(zo, mu + i * A, ex.off, ex.D, act,
                                                               ppo::MaskRow{mask + (rows ? (long)rows[i] : i) * W})
                                             : ppo::kl_cat_row(zo, mu + i * A, ex.off, ex.D, act, ppo::NoMask{});
                    klx += r;
                    if (ex.row_kl) ex.row_kl[i] = r;
                }
            } else {
                const int lane = threadIdx.x & 63;
                const long first = base + (threadIdx.x & ~63);
                for (int r = 0; r < 64 && first + r < m; ++r) {          // uniform over the wave
                    const long row = first + r;
                    const float* zo = ex.old_dist + (ex.rows ? (long)ex.rows[row] : row) * A;
                    const float* act = mask ? action + row * A : nullptr;
                    const double v = mask ? wave_cat_row(zo, mu + row * A, ex.off, ex.D, act,
                                                         ppo::MaskRow{mask + (rows ? (long)rows[row] : row) * W})
                                          : wave_cat_row(zo, mu + row * A, ex.off, ex.D, act, ppo::NoMask{});
                    if (lane == r) {
                        klx += v;
                        if (ex.row_kl) ex.row_kl[row] = v;
                    }
                }
            }
        }
    }
    const double part_kl = block_sum(kl, s);
    const double part_cnt = block_sum(cnt, s);
    constexpr int K = EXACT ? 3 : 2;
    double* const slots = EXACT ? rec->partial_x : rec->partial;
    double part[K] = {part_kl, part_cnt};
    if constexpr (EXACT) part[2] = block_sum(klx, s);
    if (!ppo::ticket_publish(&slots[K * blockIdx.x], part, &rec->ticket, &s[TPB])) return;

    // the last workgroup: every partial of this launch is visible; fold them in index order
    double pk = 0.0, pc = 0.0, px = 0.0;
    if (threadIdx.x < gridDim.x) {
        pk = ppo::ticket_load(&slots[K * threadIdx.x]);
        pc = ppo::ticket_load(&slots[K * threadIdx.x + 1]);
        if constexpr (EXACT) px = ppo::ticket_load(&slots[K * threadIdx.x + 2]);
    }
    const double tk = block_sum(pk, s);
    const double tc = block_sum(pc, s);
    double tx = 0.0;
    if constexpr (EXACT) tx = block_sum(px, s);
    if (threadIdx.x == 0) {
        rec->sums[0] = (float)tk;
        rec->sums[1] = (float)tc;
        rec->sums[2] = (float)tx;
        rec->sums[3] = 0.f;
        if (decide_here) decide<EXACT>(rec, target_kl, rows_global);
        __hip_atomic_store(&rec->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch's
    }
}

__global__ void kl_decide_kernel(PhipKlRec* rec, float target_kl, double rows_global, int exact) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (exact) decide<true>(rec, target_kl, rows_global);
        else decide<false>(rec, target_kl, rows_global);
    }
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
                    const int* md_off, int D, const uint32_t* mask, const int* rows, const PhipKlExact* ex,
                    const float* sd) {
    static_assert(PHIP_KL_PARTS <= TPB, "the last workgroup folds one pair of partials per thread");
    PPO_REQUIRE(m > 0 && A > 0 && rows_global > 0 && rec, "phip_policy_kl: shape");
    PPO_REQUIRE(dist != 2 || (md_off && D >= 1 && 2 * D <= A), "phip_policy_kl: multi-discrete offsets");
    PPO_REQUIRE(!mask || dist == 2, "phip_policy_kl: a mask needs the multi-discrete form (dist 1 as nvec = {A})");
    PPO_REQUIRE(ex || old_lp, "phip_policy_kl: the k3 launch needs the old log-probs");
    PPO_REQUIRE(dist != 3 || (sd && !mask && (A & 1) == 0 && A / 2 <= PHIP_SD_MAX_AA),
                "phip_policy_kl: the state-dependent-σ form needs its bounds and an even A <= 64");
    PPO_REQUIRE(!ex || (ex->old_dist && (ex->off ? ex->D >= 1 && dist != 0 && dist != 3
                                                 : (dist == 3 || (dist == 0 && ex->old_log_std)) && !ex->wide)),
                "phip_policy_kl: the closed-form estimator's inputs");
    const float sd_lo = dist == 3 ? sd[0] : 0.f, sd_hi = dist == 3 ? sd[1] : 0.f;
    ppo::ProfScope ps(PPO_K_ADAM, (ex ? 12.0 : 8.0) * (double)m * A + 4.0 * m);
    if (ex)
        hipLaunchKernelGGL(kl_sum_kernel<true>, dim3(grid_for(m)), dim3(TPB), 0, ppo::stream(), mu, log_std, action,
                           old_lp, m, A, dist, eps, target_kl, (double)rows_global, decide_here, rec, md_off, D, mask,
                           rows, *ex, sd_lo, sd_hi);
    else
        hipLaunchKernelGGL(kl_sum_kernel<false>, dim3(grid_for(m)), dim3(TPB), 0, ppo::stream(), mu, log_std, action,
                           old_lp, m, A, dist, eps, target_kl, (double)rows_global, decide_here, rec, md_off, D, mask,
                           rows, PhipKlExact{}, sd_lo, sd_hi);
    PPO_LAUNCH_CHECK();
}

void phip_kl_decide(PhipKlRec* rec, float target_kl, long rows_global, int exact) {
    PPO_REQUIRE(rows_global > 0 && rec, "phip_kl_decide: shape");
    ppo::ProfScope ps(PPO_K_ADAM, 64.0);
    hipLaunchKernelGGL(kl_decide_kernel, dim3(1), dim3(64), 0, ppo::stream(), rec, target_kl, (double)rows_global,
                       exact);
    PPO_LAUNCH_CHECK();
}

void phip_lr_couple(PhipKlRec* rec, float lr_V, float base) {
    PPO_REQUIRE(rec && base > 0.f, "phip_lr_couple: arguments");
    ppo::ProfScope ps(PPO_K_OTHER, 16.0);              // not an Adam launch: kept out of that class's counts
    hipLaunchKernelGGL(lr_couple_kernel, dim3(1), dim3(64), 0, ppo::stream(), rec, lr_V, base);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
