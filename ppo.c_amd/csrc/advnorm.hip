// advnorm.hip — per-minibatch advantage normalisation (no counterpart in the reference; Stable-Baselines3's
// normalize_advantage, CleanRL's norm_adv; ppo_ext.h ppo_set_adv_norm).  advnorm.h holds the definition.
//
// One launch whatever the number of segments: workgroup s (256 threads, four waves) owns segment s, the B floats at
// s·B.  Thread t takes the elements i ≡ t (mod 256) in ascending order — consecutive lanes read consecutive floats, so
// every load and store is coalesced; they are scalar dword accesses, because a segment is 16-byte aligned only when
// B % 4 == 0.  The first ADVNORM_REG = 16 of a thread's elements (B <= 4096: all of them) stay in registers across
// the three passes (sum, squared deviations, write); the rest of a longer segment is read again in passes two and
// three, from L2: a segment of the benchmark's B = 32768 is 128 KiB.  In-place calls are safe for the same reason
// out-of-place ones are: a thread reads x_i for the last time before it writes y_i, and no other thread touches i.
//
// Occupancy: the compiler reports 78 VGPRs and no scratch (the 16 floats, the double-precision division sequences),
// which allows six waves per SIMD, so six workgroups share a CU; the 256 doubles of LDS (2 KiB per workgroup) limit
// nothing.  That residency is what hides the two barrier trees at small B, where a launch is tens of thousands of
// short workgroups.  No atomics: lane partials, then the pairwise tree of advnorm.h
// in LDS; the order is a function of B alone.  The multiply and the add of Σ d·d round separately: the pragma below
// and the Makefile's -ffp-contract=off both forbid a fused multiply-add.
#include "dev.h"
#include "advnorm.h"
#include "reduce.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = ADVNORM_LANES;
constexpr int REG = ADVNORM_REG;

// the tree of advnorm.h over s[0 … 255] (reduce.h's tree_fold under __dadd_rn); every thread gets s[0].  Ends with
// a barrier, so s may be rewritten
__device__ __forceinline__ double tree_sum(double* s, int t, double lane) {
    s[t] = lane;
    const double total = ppo::tree_fold<TPB>(s, t, ppo::DaddRn{});
    __syncthreads();
    return total;
}

__global__ void __launch_bounds__(TPB) adv_normalize_kernel(const float* in, float* out, int B,
                                                            float* __restrict__ stats) {
    __shared__ double s_part[TPB];
    const int t = threadIdx.x;
    const long base = (long)blockIdx.x * B;
    const float* x = in + base;
    float* y = out + base;
    const long tail = (long)TPB * REG + t;        // the thread's first element beyond its registers

    float r[REG];
#pragma unroll
    for (int k = 0; k < REG; ++k) {
        const int i = k * TPB + t;
        r[k] = i < B ? x[i] : 0.f;
    }

    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < REG; ++k)
        if (k * TPB + t < B) acc = __dadd_rn(acc, (double)r[k]);
    for (long i = tail; i < B; i += TPB) acc = __dadd_rn(acc, (double)x[i]);
    const double mean = tree_sum(s_part, t, acc) / (double)B;

    acc = 0.0;
#pragma unroll
    for (int k = 0; k < REG; ++k)
        if (k * TPB + t < B) {
            const double d = __dsub_rn((double)r[k], mean);
            acc = __dadd_rn(acc, __dmul_rn(d, d));
        }
    for (long i = tail; i < B; i += TPB) {
        const double d = __dsub_rn((double)x[i], mean);
        acc = __dadd_rn(acc, __dmul_rn(d, d));
    }
    const double Q = tree_sum(s_part, t, acc);
    const float sd = (float)__dsqrt_rn(Q / (double)(B > 1 ? B - 1 : 1));
    const float m = (float)mean;
    if (stats && t == 0) {
        stats[2 * (long)blockIdx.x] = m;
        stats[2 * (long)blockIdx.x + 1] = sd;
    }

    const double den = (double)sd + 1e-8;
#pragma unroll
    for (int k = 0; k < REG; ++k) {
        const int i = k * TPB + t;
        if (i < B) y[i] = (float)((double)__fsub_rn(r[k], m) / den);
    }
    for (long i = tail; i < B; i += TPB) y[i] = (float)((double)__fsub_rn(x[i], m) / den);
}

}  // namespace

extern "C" {

void phip_adv_normalize(const float* in, float* out, long n_seg, int B, float* stats) {
    PPO_REQUIRE(in && out && n_seg > 0 && n_seg <= 0x7fffffffL && B > 0, "phip_adv_normalize: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 8.0 * (double)n_seg * B);
    hipLaunchKernelGGL(adv_normalize_kernel, dim3((unsigned)n_seg), dim3(TPB), 0, ppo::stream(), in, out, B, stats);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
