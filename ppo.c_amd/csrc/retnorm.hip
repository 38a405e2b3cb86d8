// retnorm.hip — running return-based reward normalisation for the device PPO update (no counterpart in the
// reference; the reward half of Stable-Baselines3's VecNormalize, ppo_ext.h ppo_set_reward_norm).
//
// The discounted return is a segmented FORWARD scan over the buffer, the mirror image of gae.hip's reverse one:
//     k_i = !(term_i ∨ trunc_i)  (k_{-1} = 0),      R_i = r_i + g·(k_{i-1}·R_{i-1} + c_i)      (double throughout)
// with c_i a carried return, non-zero only at the first row of a segment (seg_len > 0: rows e·seg_len take
// carry_in[e]).  Row i is the affine map x ↦ d_i + a_i·x with a_i = g·k_{i-1}, d_i = r_i + g·c_i; maps compose
// associatively, (a, d) after (a′, d′) = (a·a′, d + a·d′), in double, and a_i = 0 behind every episode end, so
// segments never mix.  Three passes, every cross-workgroup dependency through a kernel boundary (no spinning,
// no look-back), ≈ 6 B read per row per pass:
//   1. ret_block_kernel   each workgroup composes its 2048 rows → its (a, d) aggregate
//   2. ret_carry_kernel   one wave, left to right over the aggregates → the return entering each workgroup
//   3. ret_apply_kernel   recompute with the true carry; the returns themselves are written only when the
//                         caller wants them; emits carry_out[e] = cont[e] ? R_{e·T+T−1} : 0 and the workgroup's
//                         Welford triple (n, mean, M2), two passes over registers, in double
// (the affine map, its block scan — here double, left to right — and the two-pass triple are reduce.h's)
// then ret_finish_kernel — one workgroup: the partials combined by reduce.h's chan in fold_runs_tree's fixed order
// (each thread a contiguous run in index order, then a pairwise tree), folded into the running triple, the
// fp32 scale s = (float)(1/sqrt(M2/n + 1e-8)) refreshed and the clamp counters cleared, in one launch — and
// ret_scale_kernel: y = clamp(r·s, ±c) into a shadow of the rewards, counting clamped elements with integer
// atomics.  The composition order is a function of (n, seg_len) only and there is no floating-point atomic, so
// the same input gives the same bits.
#include "dev.h"
#include "reduce.h"

namespace {

constexpr int TPB = 256;
constexpr int EPT = 8;                    // rows per thread
constexpr int CHUNK = TPB * EPT;          // rows per workgroup (ppo_ext.h PPO_RET_CHUNK)
static_assert(CHUNK == PPO_RET_CHUNK, "ppo_ext.h PPO_RET_CHUNK is the scan's workgroup chunk");

using ppo::compose;
using ppo::LeftToRight;
using Aff = ppo::Affine<double>;         // x ↦ d + c·x; compose(then, first): `first` is applied first

// a thread's EPT rows [t0, t0 + EPT) ∩ [0, n): d[e] = r + g·c, a[e] = g·k_{row−1}; rows past n are the identity.
// vec: the pointers are 16-/8-byte aligned (t0 is a multiple of 8), so a full thread reads two float4s and two
// 8-byte flag words instead of 24 scalars.
struct Rows { double a[EPT], d[EPT]; };

__device__ __forceinline__ Rows load_rows(const float* __restrict__ r, const uint8_t* __restrict__ term,
                                          const uint8_t* __restrict__ trunc, long t0, long n, double g, int seg_len,
                                          const double* __restrict__ carry_in, int vec) {
    Rows o;
    float rr[EPT];
    bool end[EPT + 1];                    // end[e + 1]: row t0 + e ends an episode; end[0]: the row before t0
    end[0] = t0 > 0 && t0 <= n ? (term[t0 - 1] || trunc[t0 - 1]) : true;
    if (vec && t0 + EPT <= n) {
        const float4 lo = *reinterpret_cast<const float4*>(r + t0), hi = *reinterpret_cast<const float4*>(r + t0 + 4);
        rr[0] = lo.x; rr[1] = lo.y; rr[2] = lo.z; rr[3] = lo.w;
        rr[4] = hi.x; rr[5] = hi.y; rr[6] = hi.z; rr[7] = hi.w;
        const unsigned long long f = *reinterpret_cast<const unsigned long long*>(term + t0) |
                                     *reinterpret_cast<const unsigned long long*>(trunc + t0);
#pragma unroll
        for (int e = 0; e < EPT; ++e) end[e + 1] = ((f >> (8 * e)) & 0xFFull) != 0;
    } else {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const long t = t0 + e;
            rr[e] = t < n ? r[t] : 0.f;
            end[e + 1] = t < n ? (term[t] || trunc[t]) : true;
        }
    }
    long seg = 0;
    int rem = 1;                          // rem == 0: the row is the first of a segment
    if (seg_len > 0) { seg = t0 / seg_len; rem = (int)(t0 - seg * seg_len); }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        if (t0 + e < n) {
            double c = 0.0;
            if (seg_len > 0) {
                if (rem == 0) c = carry_in[seg];
                if (++rem == seg_len) { rem = 0; ++seg; }
            }
            o.a[e] = end[e] ? 0.0 : g;
            o.d[e] = (double)rr[e] + g * c;
        } else {
            o.a[e] = 1.0;
            o.d[e] = 0.0;
        }
    }
    return o;
}

__device__ __forceinline__ Aff thread_transform(const Rows& w) {
    Aff T{1.0, 0.0};
#pragma unroll
    for (int e = 0; e < EPT; ++e) T = compose(Aff{w.a[e], w.d[e]}, T);
    return T;
}

// exclusive left-to-right scan inside the workgroup: all EARLIER threads composed; *block_total: the whole block
__device__ __forceinline__ Aff block_prefix_exclusive(Aff T, Aff* wave_tot, Aff* block_total) {
    return ppo::block_scan_exclusive<LeftToRight, TPB>(T, wave_tot, block_total);
}

__global__ void __launch_bounds__(TPB) ret_block_kernel(const float* __restrict__ r, const uint8_t* __restrict__ term,
                                                        const uint8_t* __restrict__ trunc, long n, double g,
                                                        int seg_len, const double* __restrict__ carry_in, int vec,
                                                        double2* __restrict__ agg) {
    __shared__ Aff wave_tot[TPB / 64];
    const long t0 = (long)blockIdx.x * CHUNK + (long)threadIdx.x * EPT;
    const Rows w = load_rows(r, term, trunc, t0, n, g, seg_len, carry_in, vec);
    Aff tot;
    block_prefix_exclusive(thread_transform(w), wave_tot, &tot);
    if (threadIdx.x == 0) agg[blockIdx.x] = make_double2(tot.c, tot.d);
}

// carry[b] = the return entering workgroup b from the left (carry[0] = 0): one wave scans the aggregates 64 at
// a time, left to right
__global__ void __launch_bounds__(64) ret_carry_kernel(const double2* __restrict__ agg, double* __restrict__ carry,
                                                       int nblocks) {
    const int lane = threadIdx.x;
    double x = 0.0;                       // the return entering block `base`
    for (int base = 0; base < nblocks; base += 64) {
        const int b = base + lane;
        Aff inc{1.0, 0.0};
        if (b < nblocks) { const double2 v = agg[b]; inc = Aff{v.x, v.y}; }
        inc = ppo::wave_scan_inclusive<LeftToRight>(inc);
        const Aff excl = ppo::wave_scan_exclusive<LeftToRight>(inc);
        if (b < nblocks) carry[b] = excl.d + excl.c * x;
        const double last_c = __shfl(inc.c, 63, 64), last_d = __shfl(inc.d, 63, 64);
        x = last_d + last_c * x;
    }
}

__global__ void __launch_bounds__(TPB) ret_apply_kernel(const float* __restrict__ r, const uint8_t* __restrict__ term,
                                                        const uint8_t* __restrict__ trunc, long n, double g,
                                                        int seg_len, const double* __restrict__ carry_in,
                                                        const uint8_t* __restrict__ cont, int vec,
                                                        const double* __restrict__ carry, double* __restrict__ returns,
                                                        double* __restrict__ carry_out, double* __restrict__ wpart) {
    __shared__ Aff wave_tot[TPB / 64];
    __shared__ double red[TPB / 64];
    __shared__ int red_n[TPB / 64];
    const long t0 = (long)blockIdx.x * CHUNK + (long)threadIdx.x * EPT;
    const Rows w = load_rows(r, term, trunc, t0, n, g, seg_len, carry_in, vec);
    Aff tot;
    const Aff P = block_prefix_exclusive(thread_transform(w), wave_tot, &tot);
    double x = P.d + P.c * carry[blockIdx.x];         // the return of the row before this thread's first
    double R[EPT];
    int cnt = 0;
    double sum = 0.0;
    long seg = 0;
    int rem = 0;
    if (seg_len > 0) { seg = t0 / seg_len; rem = (int)(t0 - seg * seg_len); }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const long t = t0 + e;
        R[e] = 0.0;
        if (t < n) {
            x = w.a[e] != 0.0 ? w.d[e] + w.a[e] * x : w.d[e];
            R[e] = x;
            if (returns) returns[t] = x;
            if (seg_len > 0 && ++rem == seg_len) {    // the last row of segment `seg`
                if (carry_out) carry_out[seg] = cont[seg] ? x : 0.0;
                rem = 0;
                ++seg;
            }
            sum += x;
            cnt++;
        }
    }
    ppo::block_two_pass_triple<TPB>(sum, cnt, R, n - t0, red, red_n, wpart + 3 * (long)blockIdx.x);
}

// One workgroup.  `count` triples (workgroup partials, or rank triples in rank order; count may be 0) combined
// in a fixed order → batch (may be null); folded into the running triple `run` (may be null); the fp32 scale of
// `run` refreshed (scale may be null; needs run); counts (may be null) cleared.
__global__ void __launch_bounds__(TPB) ret_finish_kernel(const double* __restrict__ parts, int count,
                                                         double* __restrict__ batch, double* __restrict__ run,
                                                         float* __restrict__ scale, unsigned long long* counts) {
    __shared__ ppo::Triple s[TPB];
    const ppo::Triple b = ppo::fold_runs_tree<TPB>(s, count, ppo::Triple{0.0, 0.0, 0.0}, ppo::TripleAt{parts},
                                                   ppo::TripleMerge<ppo::chan>{});
    if (threadIdx.x != 0) return;
    if (batch) { batch[0] = b.n; batch[1] = b.mean; batch[2] = b.m2; }
    if (counts) { counts[0] = 0ull; counts[1] = 0ull; }
    if (!run) return;
    double nr = run[0], mr = run[1], Mr = run[2];
    if (count > 0) {
        ppo::chan(nr, mr, Mr, b.n, b.mean, b.m2);
        run[0] = nr; run[1] = mr; run[2] = Mr;
    }
    if (scale) scale[0] = nr > 0.0 ? (float)(1.0 / sqrt(Mr / nr + 1e-8)) : 1.f;
}

__device__ __forceinline__ float scale1(float r, float s, float c, unsigned& clamped) {
    const float t = r * s;
    const float y = t < -c ? -c : (t > c ? c : t);
    clamped += (y != t && t == t) ? 1u : 0u;
    return y;
}

// y[0:n] ← clamp(r[0:n]·s, ±clip); run[0] == 0: no clamp (s is 1 then: the identity); counts: [0] += clamped
// elements, [1] += n.  vec: both pointers 16-byte aligned — float4 body, scalar tail.
__global__ void __launch_bounds__(TPB) ret_scale_kernel(const float* __restrict__ r, float* __restrict__ y, long n,
                                                        const float* __restrict__ scale, float clip,
                                                        const double* __restrict__ run, int vec,
                                                        unsigned long long* counts) {
    __shared__ unsigned long long s_clamped;
    if (threadIdx.x == 0) s_clamped = 0ull;
    __syncthreads();
    const float s = scale[0];
    const float c = run[0] > 0.0 ? clip : INFINITY;
    unsigned clamped = 0;
    const long tid = (long)blockIdx.x * TPB + threadIdx.x, nth = (long)gridDim.x * TPB;
    const long n4 = vec ? n / 4 : 0;
    for (long q = tid; q < n4; q += nth) {
        float4 v = reinterpret_cast<const float4*>(r)[q];
        v.x = scale1(v.x, s, c, clamped);
        v.y = scale1(v.y, s, c, clamped);
        v.z = scale1(v.z, s, c, clamped);
        v.w = scale1(v.w, s, c, clamped);
        reinterpret_cast<float4*>(y)[q] = v;
    }
    for (long i = 4 * n4 + tid; i < n; i += nth) y[i] = scale1(r[i], s, c, clamped);
    if (!counts) return;                      // uniform over the launch
    if (clamped) atomicAdd(&s_clamped, (unsigned long long)clamped);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_clamped) atomicAdd(&counts[0], s_clamped);
        if (blockIdx.x == 0) atomicAdd(&counts[1], (unsigned long long)n);
    }
}

// workspace (grow-only, one per process and never freed, as gae.hip's): aggregates, carries, Welford partials.
// libppo's launchers are called from one host thread and these launches go to libppo's main stream only, so
// consecutive scans are stream-ordered and may share it.
double2* g_agg = nullptr;
double*  g_carry = nullptr;
double*  g_wpart = nullptr;
int      g_cap_blocks = 0;

void ensure_ws(int nb) {
    if (nb <= g_cap_blocks) return;
    if (g_agg) { phip_free(g_agg); phip_free(g_carry); phip_free(g_wpart); }
    g_cap_blocks = nb + 64;
    g_agg = (double2*)phip_malloc(sizeof(double2) * g_cap_blocks);
    g_carry = (double*)phip_malloc(sizeof(double) * g_cap_blocks);
    g_wpart = (double*)phip_malloc(sizeof(double) * 3 * g_cap_blocks);
}

bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

void phip_ret_scan(const float* reward, const uint8_t* term, const uint8_t* trunc, long n, float gamma, int seg_len,
                   const double* carry_in, const uint8_t* cont, double* returns, double* carry_out, double* batch,
                   double* run, float* scale, unsigned long long* counts) {
    PPO_REQUIRE(n >= 0 && seg_len >= 0 && batch && ((reward && term && trunc) || n == 0), "phip_ret_scan: operands");
    PPO_REQUIRE(seg_len == 0 || (n % seg_len == 0 && carry_in && (cont || !carry_out)), "phip_ret_scan: segments");
    PPO_REQUIRE(n <= (long)CHUNK * 0x7FFFFF00L, "phip_ret_scan: too many rows");
    hipStream_t s = ppo::stream();
    const int nb = ppo_divup(n, CHUNK);
    if (nb > 0) {
        ensure_ws(nb);
        const double g = (double)gamma;
        const int vec = aligned(reward, 16) && aligned(term, 8) && aligned(trunc, 8);
        {
            ppo::ProfScope ps(PPO_K_GAE, 6.0 * n);
            hipLaunchKernelGGL(ret_block_kernel, dim3(nb), dim3(TPB), 0, s, reward, term, trunc, n, g, seg_len,
                               carry_in, vec, g_agg);
            PPO_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(ret_carry_kernel, dim3(1), dim3(64), 0, s, g_agg, g_carry, nb);
        PPO_LAUNCH_CHECK();
        {
            ppo::ProfScope ps(PPO_K_GAE, (returns ? 14.0 : 6.0) * n);
            hipLaunchKernelGGL(ret_apply_kernel, dim3(nb), dim3(TPB), 0, s, reward, term, trunc, n, g, seg_len,
                               carry_in, cont, vec, g_carry, returns, carry_out, g_wpart);
            PPO_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(ret_finish_kernel, dim3(1), dim3(TPB), 0, s, g_wpart, nb, batch, run, scale, counts);
    PPO_LAUNCH_CHECK();
}

void phip_ret_fold(const double* triples, int count, double* run, float* scale, unsigned long long* counts) {
    PPO_REQUIRE(run && count >= 0 && (triples || count == 0), "phip_ret_fold: operands");
    hipLaunchKernelGGL(ret_finish_kernel, dim3(1), dim3(TPB), 0, ppo::stream(), triples, count, (double*)nullptr, run,
                       scale, counts);
    PPO_LAUNCH_CHECK();
}

void phip_ret_scale(const float* reward, float* y, long n, const float* scale, float clip, const double* run,
                    unsigned long long* counts) {
    PPO_REQUIRE(n >= 0 && scale && run && ((reward && y) || n == 0), "phip_ret_scale: operands");
    if (n == 0) return;
    int g = ppo_divup(n, TPB * 8);
    if (g > 2048) g = 2048;
    const int vec = aligned(reward, 16) && aligned(y, 16);
    ppo::ProfScope ps(PPO_K_GAE, 8.0 * n);
    hipLaunchKernelGGL(ret_scale_kernel, dim3(g), dim3(TPB), 0, ppo::stream(), reward, y, n, scale, clip, run, vec,
                       counts);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
