// clip.hip — global gradient-norm clipping for the device PPO update (no counterpart in the reference).
//
// One launch per minibatch step, between the gradient all-reduce and the step's Adam:
//   norm = grad_scale · sqrt(Σ g²)   over a flat gradient span (+ a small side span: the policy's log σ)
//   coef = min(1, max_norm / (norm + 1e-6))                       (torch.nn.utils.clip_grad_norm_)
// left in a device record the Adam kernels read through a pointer (adam.hip: g · fl32(scale · coef)).
//
// Deterministic by construction: the grid is a function of n (and the span's alignment) only, every
// thread sums its grid-stride elements in double in index order, a workgroup folds its 256 sums by a
// fixed LDS tree, and the last workgroup to arrive folds the ≤ 256 workgroup partials by the same fixed
// tree — no floating-point atomic anywhere, so the same gradient bits give the same coef bits whatever
// order the workgroups ran in.  No grid barrier: the tree (block_sum_halving) and the hand-off (ticket_publish /
// ticket_load, one 8-byte partial per workgroup) are reduce.h's, which holds the ordering argument.
#include "dev.h"
#include "reduce.h"

namespace {

constexpr int TPB = 256;
constexpr int UNROLL = 4;

// reduce.h's halving tree over the workgroup's 256 doubles
__device__ __forceinline__ double block_sum(double v, double* s) { return ppo::block_sum_halving<TPB>(v, s); }

// vec: a is 16-B aligned (float4 body, scalar tail for n % 4); else every element takes the scalar loop
__global__ void __launch_bounds__(TPB) grad_norm_kernel(const float* __restrict__ a, long n,
                                                        const float* __restrict__ b, long nb, int vec,
                                                        float grad_scale, float max_norm, PhipClipRec* rec) {
    __shared__ double s[TPB + 1];             // s[TPB]: "this workgroup drew the last ticket"
    const long gtid = blockIdx.x * (long)TPB + threadIdx.x, gsz = (long)gridDim.x * TPB;
    const long n4 = vec ? n >> 2 : 0;
    double acc = 0.0;
    // UNROLL independent 16-B loads in flight per thread before the first add (the span was just written
    // by other CUs: every load is a trip beyond this CU's L2 slice); indices past the end re-read the
    // thread's first element and add nothing, so no load sits behind a branch
    for (long i = gtid; i < n4; i += UNROLL * gsz) {
        float4 g[UNROLL];
#pragma unroll
        for (int k = 0; k < UNROLL; ++k) {
            const long ik = i + k * gsz;
            g[k] = reinterpret_cast<const float4*>(a)[ik < n4 ? ik : i];
        }
#pragma unroll
        for (int k = 0; k < UNROLL; ++k) {
            const double w = i + k * gsz < n4 ? 1.0 : 0.0;
            acc += w * ((double)g[k].x * (double)g[k].x);
            acc += w * ((double)g[k].y * (double)g[k].y);
            acc += w * ((double)g[k].z * (double)g[k].z);
            acc += w * ((double)g[k].w * (double)g[k].w);
        }
    }
    for (long j = 4 * n4 + gtid; j < n; j += gsz) acc += (double)a[j] * (double)a[j];
    if (blockIdx.x == 0)
        for (long j = threadIdx.x; j < nb; j += TPB) acc += (double)b[j] * (double)b[j];
    const double part = block_sum(acc, s);

    const double part1[1] = {part};
    if (!ppo::ticket_publish(&rec->partial[blockIdx.x], part1, &rec->ticket, &s[TPB])) return;

    // the last workgroup: every partial of this launch is visible; fold them in index order
    const double p = threadIdx.x < gridDim.x ? ppo::ticket_load(&rec->partial[threadIdx.x]) : 0.0;
    const double total = block_sum(p, s);
    if (threadIdx.x == 0) {
        const double norm = (double)grad_scale * sqrt(total);
        const double c = (double)max_norm / (norm + 1e-6);
        const float coef = c < 1.0 ? (float)c : 1.0f;      // NaN or +inf: 1
        rec->norm = norm;
        rec->coef = coef;
        if (coef < 1.0f) rec->clipped += 1u;
        __hip_atomic_store(&rec->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch's
    }
}

int grid_for(long n, int vec) {
    const long work = vec ? (n + 3) / 4 : n;
    long g = (work + TPB - 1) / TPB;
    if (g < 1) g = 1;
    if (g > PHIP_CLIP_PARTS) g = PHIP_CLIP_PARTS;
    return (int)g;
}

}  // namespace

extern "C" {

void phip_grad_norm(const float* g, long n, const float* side, long n_side, float grad_scale, float max_norm,
                    PhipClipRec* rec) {
    static_assert(PHIP_CLIP_PARTS <= TPB, "the last workgroup folds one partial per thread");
    PPO_REQUIRE(n >= 0 && n_side >= 0 && rec, "phip_grad_norm: spans");
    const int vec = ((uintptr_t)g & 15u) == 0;
    ppo::ProfScope ps(PPO_K_ADAM, 4.0 * (double)(n + n_side));
    hipLaunchKernelGGL(grad_norm_kernel, dim3(grid_for(n, vec)), dim3(TPB), 0, ppo::stream(), g, n, side, n_side, vec,
                       grad_scale, max_norm, rec);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
