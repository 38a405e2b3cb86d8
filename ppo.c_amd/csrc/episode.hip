// episode.hip — episode-return statistics of a rollout-laid buffer, and the deterministic action of the device
// evaluation (no counterpart in the reference; what Stable-Baselines3's Monitor / evaluate_policy and CleanRL's
// episodic_return report; ppo_ext.h ppo_episode_scan_device).
//
// The buffer holds E segments of T rows, transition (e, t) at row e·T + t.  Row (e, t) ends an episode iff
//     term ∨ (trunc ∧ (t < T−1 ∨ cont == NULL ∨ ¬cont[e]))
// — the truncation that ppo_rollout_device writes on every segment's last row ends nothing while cont[e] says the
// environment was not reset.  Each environment carries four doubles {ret, disc, w, len} (fresh {0, 0, 1, 0}) and
// walks its rows left to right:  ret += r;  disc += w·r;  w *= g;  len += 1;  at an end row the episode
// (ret, disc, len) is emitted and the state set fresh.  The multiply and the add of disc round separately: the
// pragma below and the Makefile's -ffp-contract=off both forbid a fused multiply-add.
//
// Two launches, whatever E and T are:
//   1. episode_scan_kernel   one workgroup of four waves per 64 environments.  An environment's T rows are
//      contiguous, so 64 lanes walking 64 segments would stride by T: instead the workgroup stages a tile of 64
//      environments × 64 rows through LDS — each wave takes every fourth environment of the tile, its 64 lanes
//      read 64 consecutive rewards (256 B) and flags (64 B + 64 B), decide the end rule and store {reward, end}
//      at [env][row] with a row pitch of 65 words — and wave 0, lane = environment, walks [e][0 … 63] eight rows'
//      reads at a time: bank (e + row) mod 64, no conflict either way.  2 × 64 × 65 × 4 B = 33 280 B of LDS per
//      workgroup.  Emitted episodes are merged, in the order they end, into the environment's own aggregate
//      (⊕ below with a one-episode right-hand side).
//   2. episode_fold_kernel   one workgroup of 256 threads folds the environments' aggregates in reduce.h's
//      fold_runs_tree order (contiguous runs of ⌈E/256⌉ in index order, then the pairwise tree over the threads).
//      The batch aggregate goes to `out`; the running window (may be null) becomes window ⊕ batch.
// ⊕ on aggregates {n, mean, M2, min, max, Σlen, mean disc} is Chan et al.'s combine ((n, mean, M2): reduce.h's chan):
//     n = na + nb;  f = nb / n;  δ = mean_b − mean_a;  mean = mean_a + δ·f;  M2 = (M2a + M2b) + δ·δ·(na·f);
//     mdisc = mdisc_a + (mdisc_b − mdisc_a)·f;  min, max;  Σlen = Σlen_a + Σlen_b
// an empty side leaves the other as it is, so a scan that emits nothing yields the zero aggregate.  No atomics;
// the order is a function of E alone.
#include "dev.h"
#include "reduce.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE_E = 64;                // environments per workgroup
constexpr int SCAN_TPB = 256;             // four waves stage a tile; wave 0 walks it
constexpr int TILE_T = 64;                // rows staged per tile
constexpr int PITCH = TILE_T + 1;
constexpr int FOLD_TPB = 256;
constexpr int NPART = 8;                  // doubles per aggregate slot: PPO_EP_NBATCH + 1
static_assert(NPART == PPO_EP_NBATCH + 1, "slot 7 of an aggregate counts the environments left mid-episode");

struct Agg { double n, mean, m2, mn, mx, len, mdisc; };

__device__ __forceinline__ void merge(Agg& a, const Agg& b) {
    if (!(b.n > 0.0)) return;
    if (!(a.n > 0.0)) { a = b; return; }
    const double f = b.n / (a.n + b.n);               // the nb / n of ppo::chan: the same operands, the same bits
    a.mdisc = a.mdisc + (b.mdisc - a.mdisc) * f;
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
    a.len = a.len + b.len;
    ppo::chan(a.n, a.mean, a.m2, b.n, b.mean, b.m2);
}

__device__ __forceinline__ Agg load_agg(const double* p) { return Agg{p[0], p[1], p[2], p[3], p[4], p[5], p[6]}; }
__device__ __forceinline__ void store_agg(double* p, const Agg& a) {
    p[0] = a.n; p[1] = a.mean; p[2] = a.m2; p[3] = a.mn; p[4] = a.mx; p[5] = a.len; p[6] = a.mdisc;
}

__global__ void __launch_bounds__(SCAN_TPB) episode_scan_kernel(
    const float* __restrict__ reward, const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc,
    const uint8_t* __restrict__ cont, int E, int T, double g, const double* state_in /* may be state_out */,
    double* state_out, double* __restrict__ row_ret, double* __restrict__ row_disc,
    double* __restrict__ part) {
    __shared__ float s_r[TILE_E * PITCH];
    __shared__ uint32_t s_end[TILE_E * PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e0 = blockIdx.x * TILE_E;
    const int e = e0 + lane;
    const int ne = min(TILE_E, E - e0);
    const bool walker = wave == 0 && e < E;                           // wave 0: lane = environment
    double ret = 0.0, disc = 0.0, w = 1.0, len = 0.0;
    if (walker && state_in) {
        ret = state_in[4 * (long)e]; disc = state_in[4 * (long)e + 1];
        w = state_in[4 * (long)e + 2]; len = state_in[4 * (long)e + 3];
    }
    Agg a{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t0 = 0; t0 < T; t0 += TILE_T) {
        const int nt = min(TILE_T, T - t0);
        const bool last_row = lane == nt - 1 && t0 + nt == T;         // this lane stages row T − 1
        __syncthreads();                                              // the previous tile has been walked
        if (lane < nt) {                                              // every wave stages a quarter of the tile
#pragma unroll 16
            for (int r = wave; r < ne; r += SCAN_TPB / 64) {
                const long i = (long)(e0 + r) * T + t0 + lane;
                const bool open = last_row && cont && cont[e0 + r];   // the segment's end continues the episode
                s_r[r * PITCH + lane] = reward[i];
                s_end[r * PITCH + lane] = (term[i] || (trunc[i] && !open)) ? 1u : 0u;
            }
        }
        __syncthreads();
        if (walker) {
            for (int tb = 0; tb < nt; tb += 8) {                      // eight rows' LDS reads in flight at a time
                float rr[8];
                uint32_t ee[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {                         // tb + j < TILE_T: inside the tile's arrays
                    rr[j] = s_r[lane * PITCH + tb + j];
                    ee[j] = s_end[lane * PITCH + tb + j];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int tt = tb + j;
                    if (tt < nt) {
                        const double r = (double)rr[j];
                        ret = ret + r;
                        disc = disc + w * r;
                        w = w * g;
                        len = len + 1.0;
                        if (row_ret) row_ret[(long)e * T + t0 + tt] = ret;
                        if (row_disc) row_disc[(long)e * T + t0 + tt] = disc;
                        if (ee[j]) {
                            merge(a, Agg{1.0, ret, 0.0, ret, ret, len, disc});
                            ret = 0.0; disc = 0.0; w = 1.0; len = 0.0;
                        }
                    }
                }
            }
        }
    }
    if (!walker) return;
    if (state_out) {
        state_out[4 * (long)e] = ret; state_out[4 * (long)e + 1] = disc;
        state_out[4 * (long)e + 2] = w; state_out[4 * (long)e + 3] = len;
    }
    store_agg(part + (long)NPART * e, a);
    part[(long)NPART * e + 7] = len > 0.0 ? 1.0 : 0.0;
}

// an aggregate and, in slot 7, the count of environments left mid-episode (an exact integer, a plain add)
struct Slot { Agg a; double open; };
static_assert(sizeof(Slot) == NPART * sizeof(double), "a slot of `part` and of the fold's LDS");
struct SlotMerge {
    __device__ Slot operator()(Slot x, const Slot& y) const { merge(x.a, y.a); x.open += y.open; return x; }
};

__global__ void __launch_bounds__(FOLD_TPB) episode_fold_kernel(const double* __restrict__ part, int E,
                                                                double* __restrict__ out, double* __restrict__ window) {
    __shared__ Slot s[FOLD_TPB];
    const Slot r = ppo::fold_runs_tree<FOLD_TPB>(
        s, E, Slot{Agg{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, 0.0},
        [&](int i) { return Slot{load_agg(part + (long)NPART * i), part[(long)NPART * i + 7]}; }, SlotMerge{});
    if (threadIdx.x != 0) return;
    store_agg(out, r.a);
    out[7] = r.open;
    if (window) {
        Agg wnd = load_agg(window);
        merge(wnd, r.a);
        store_agg(window, wnd);
        window[7] = r.open;
    }
}

// a = μ, bit for bit: the deterministic action (no noise drawn, no log-prob)
__global__ void mean_action_kernel(const float* __restrict__ mu, float* __restrict__ action, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) action[i] = mu[i];
}

// per-environment aggregates of the scan in flight (grow-only, one per process and never freed, as retnorm.hip's):
// libppo's launchers are called from one host thread and these launches go to libppo's main stream, so
// consecutive scans are stream-ordered and may share it
double* g_part = nullptr;
int     g_part_cap = 0;

}  // namespace

extern "C" {

void phip_episode_scan(const float* reward, const uint8_t* term, const uint8_t* trunc, const uint8_t* cont, int E,
                       int T, float gamma, const double* state_in, double* state_out, double* row_ret,
                       double* row_disc, double* out, double* window) {
    PPO_REQUIRE(reward && term && trunc && out && E > 0 && T > 0, "phip_episode_scan: operands");
    if (E > g_part_cap) {
        if (g_part) phip_free(g_part);
        g_part_cap = E + 64;
        g_part = (double*)phip_malloc(sizeof(double) * NPART * (size_t)g_part_cap);
    }
    hipStream_t s = ppo::stream();
    {
        ppo::ProfScope ps(PPO_K_OTHER, 6.0 * E * T + 128.0 * E);
        hipLaunchKernelGGL(episode_scan_kernel, dim3(ppo_divup(E, TILE_E)), dim3(SCAN_TPB), 0, s, reward, term, trunc,
                           cont, E, T, (double)gamma, state_in, state_out, row_ret, row_disc, g_part);
        PPO_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(episode_fold_kernel, dim3(1), dim3(FOLD_TPB), 0, s, g_part, E, out, window);
    PPO_LAUNCH_CHECK();
}

void phip_mean_action(const float* mu, float* action, long n) {
    PPO_REQUIRE(mu && action && n > 0, "phip_mean_action: operands");
    hipLaunchKernelGGL(mean_action_kernel, dim3(ppo_divup(n, 256)), dim3(256), 0, ppo::stream(), mu, action, n);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
