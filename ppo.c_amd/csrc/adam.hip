// adam.hip — Adam as one streaming pass over a flat parameter span (HBM-bound, 28 B/param).
//
// Reference: adam_update (adam.cu:53-74) and adam_update_kernel (adam.cu:138-169, K10), which
// finds each element's layer by a linear search over prefix lengths through a device float**.
// libppo networks keep W and b of every layer in one contiguous buffer, so the update is a
// single float4-vectorised kernel; a multi-tensor variant covers arbitrary tensor lists.
//
// Arithmetic is the reference's, operation for operation (compiled without FMA contraction):
//   m = β1·m + (1−β1)·g;  v = β2·v + (1−β2)·g²;
//   denom = (float)(sqrtf(v/bc2) + 1e-8)   (double add, as in C);   p −= step·m/denom
// so that, given identical gradients, parameters, m and v match the oracle bit for bit — over the whole
// fp32 range of g (subnormals, ±inf, NaN up to its payload): tests/test_gpu_adam.py.
//
// One definition of each kernel, a template over where the step's (step, bc2) come from (RateValue, RateWord,
// RateTable below): an instantiation holds its own source's kernel arguments and no branch on the others'.
#include "dev.h"
#include "ppo_math.h"

namespace {

constexpr int TPB = 256;

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float step, float b1, float b2,
                                          float bc2, float scale) {
    g = g * scale;
    ppo::adam_elem(p, g, m, v, step, b1, b2, bc2);
}

// a step's bias-corrected step size lr / (1 − β1^t) and second-moment correction 1 − β2^t
struct StepBc { float step, bc2; };

// by value: the host divided lr / bias_correction1
struct RateValue {
    float step, bc2;
    __device__ __forceinline__ StepBc operator()() const { return {step, bc2}; }
    static RateValue of(PhipAdamRate r, float bc1, float bc2) { return {r.lr / bc1, bc2}; }
};

// The learning rate through a device word (the KL-adaptive schedule, kl.hip: decide() wrote it in a launch before
// this one): step = *lr / bias_correction1, the fp32 division the host does for RateValue, so an equal rate gives
// equal bits.
struct RateWord {
    const float* lr; float bc1, bc2;
    __device__ __forceinline__ StepBc operator()() const { return {*lr / bc1, bc2}; }
    static RateWord of(PhipAdamRate r, float bc1, float bc2) { return {r.d_lr, bc1, bc2}; }
};

// the step table of graph replay, at the device step counter; which = 0: the network's Adam, 1: the entropy Adam
struct RateTable {
    const PhipStepArgs* tab; int* ctr; int which;
    __device__ __forceinline__ StepBc operator()() const {
        const PhipStepArgs& s = tab[*ctr];
        return which ? StepBc{s.step_ls, s.bc2_ls} : StepBc{s.step, s.bc2};
    }
};

// n elements: float4 body plus a scalar tail (a network's span ends with its unpadded output bias).
// w16 (bf16 mode): the parameters' bf16 shadow for the first n16 elements, written in the same pass.
// zero_g: the gradient is cleared once read (ppo_update: the next backward's split-K atomics then
// accumulate into zeros without a memset launch per minibatch step).
__device__ __forceinline__ void adam_vec_body(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, long n, float step, float b1, float b2,
                                              float bc2, float scale, __bf16* __restrict__ w16, long n16,
                                              int zero_g) {
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < n4; i += (long)gridDim.x * TPB) {
        float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        adam_elem(pp.x, gg.x, mm.x, vv.x, step, b1, b2, bc2, scale);
        adam_elem(pp.y, gg.y, mm.y, vv.y, step, b1, b2, bc2, scale);
        adam_elem(pp.z, gg.z, mm.z, vv.z, step, b1, b2, bc2, scale);
        adam_elem(pp.w, gg.w, mm.w, vv.w, step, b1, b2, bc2, scale);
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
        if (zero_g) reinterpret_cast<float4*>(g)[i] = float4{0.f, 0.f, 0.f, 0.f};
        if (w16 && 4 * i < n16) {
            if (4 * i + 4 <= n16) {
                bf16x4 o = {(__bf16)pp.x, (__bf16)pp.y, (__bf16)pp.z, (__bf16)pp.w};
                reinterpret_cast<bf16x4*>(w16)[i] = o;
            } else {
                const float e[4] = {pp.x, pp.y, pp.z, pp.w};
                for (long j = 4 * i; j < n16; ++j) w16[j] = (__bf16)e[j - 4 * i];
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long j = 4 * n4 + threadIdx.x;
        float pp = p[j], mm = m[j], vv = v[j];
        adam_elem(pp, g[j], mm, vv, step, b1, b2, bc2, scale);
        p[j] = pp; m[j] = mm; v[j] = vv;
        if (zero_g) g[j] = 0.f;
        if (w16 && j < n16) w16[j] = (__bf16)pp;
    }
}

__device__ __forceinline__ void clear_vec_body(float* __restrict__ g, long n) {
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < n4; i += (long)gridDim.x * TPB)
        reinterpret_cast<float4*>(g)[i] = float4{0.f, 0.f, 0.f, 0.f};
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) g[4 * n4 + threadIdx.x] = 0.f;
}

// The early part of every kernel that takes skip and coef; false: the step is not taken.
// skip — target-KL early stopping (kl.hip wrote the stop word in a launch before this one): while it is set p, m, v
// and the bf16 shadow stay as they are, but the gradient is still cleared where the step would have cleared it,
// since the next backward accumulates into it.  skip == nullptr: off.
// coef — the device clip coefficient when clipping is on (clip.hip wrote it in the launch before this one), folded
// into the gradient scale(s); scale2 is the pair kernel's side span: one coefficient for both spans (one optimiser
// group).  coef == nullptr leaves g · scale as it was.
__device__ __forceinline__ bool step_begin(const unsigned* __restrict__ skip, const float* __restrict__ coef,
                                           float* __restrict__ g, long n, int zero_g, float& scale, float& scale2) {
    if (skip && *skip != 0u) {
        if (zero_g) clear_vec_body(g, n);
        return false;
    }
    if (coef) {
        const float c = *coef;
        scale = scale * c;
        scale2 = scale2 * c;
    }
    return true;
}

template <class Rate>
__global__ void adam_flat_vec_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                     float* __restrict__ v, long n, Rate rate, float b1, float b2, float scale,
                                     __bf16* __restrict__ w16, long n16, int zero_g, const float* __restrict__ coef,
                                     const unsigned* __restrict__ skip) {
    float none = 0.f;
    if (!step_begin(skip, coef, g, n, zero_g, scale, none)) return;
    const StepBc s = rate();
    adam_vec_body(p, g, m, v, n, s.step, b1, b2, s.bc2, scale, w16, n16, zero_g);
}

// a second, small flat span in the same launch (the policy step's entropy Adam beside the network's,
// ppo.cu:440-442 — independent parameters) with a rate of its own: the last workgroup's first n threads, scalar
template <class Rate>
struct SideSpan {
    float* p; float* g; float* m; float* v; int n; Rate rate; float scale; int zero_g;
};
template <class Rate>
__global__ void adam_flat_vec_pair_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, long n, Rate rate, float b1, float b2, float scale,
                                          __bf16* __restrict__ w16, long n16, int zero_g, SideSpan<Rate> side,
                                          const float* __restrict__ coef, const unsigned* __restrict__ skip) {
    const bool on_side = blockIdx.x == gridDim.x - 1 && threadIdx.x < side.n;
    if (!step_begin(skip, coef, g, n, zero_g, scale, side.scale)) {    // neither span steps; both cleared as asked
        if (on_side && side.zero_g) side.g[threadIdx.x] = 0.f;
        return;
    }
    if (on_side) {
        const int j = threadIdx.x;
        const StepBc s = side.rate();
        float pp = side.p[j], mm = side.m[j], vv = side.v[j];
        adam_elem(pp, side.g[j], mm, vv, s.step, b1, b2, s.bc2, side.scale);
        side.p[j] = pp; side.m[j] = mm; side.v[j] = vv;
        if (side.zero_g) side.g[j] = 0.f;
    }
    const StepBc s = rate();
    adam_vec_body(p, g, m, v, n, s.step, b1, b2, s.bc2, scale, w16, n16, zero_g);
}

// the flat Adam with its step size / bias correction from the step table (graph replay); which = 0
// (the network's Adam) also advances the step counter: its last workgroup to finish, after every
// workgroup has read the entry (a workgroup takes its ticket only at its end)
__global__ void adam_flat_tab_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                     float* __restrict__ v, long n, RateTable rate, unsigned* ticket, float b1,
                                     float b2, float scale, __bf16* __restrict__ w16, long n16, int zero_g) {
    const StepBc s = rate();
    adam_vec_body(p, g, m, v, n, s.step, b1, b2, s.bc2, scale, w16, n16, zero_g);
    if (rate.which == 0) {
        __syncthreads();                                   // every wave of this workgroup read the entry
        if (threadIdx.x == 0) {
            const unsigned t = atomicAdd(ticket, 1u);
            if (t == gridDim.x - 1) {                      // the last workgroup: all have read it
                *ticket = 0u;
                *rate.ctr += 1;
            }
        }
    }
}

// spans the float4 kernels cannot take (a caller's unaligned tensors): no shadow, no clear
template <class Rate>
__global__ void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                 float* __restrict__ v, long n, Rate rate, float b1, float b2, float scale,
                                 const float* __restrict__ coef, const unsigned* __restrict__ skip) {
    float none = 0.f;
    if (!step_begin(skip, coef, nullptr, 0, 0, scale, none)) return;
    const StepBc s = rate();
    for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) {
        float pp = p[i], mm = m[i], vv = v[i];
        adam_elem(pp, g[i], mm, vv, s.step, b1, b2, s.bc2, scale);
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
}

constexpr int MAXT = 24;
struct TensorTable {
    float* p[MAXT];
    const float* g[MAXT];
    long start[MAXT + 1];        // prefix offsets into the flat m / v
    int count;
};

template <class Rate>
__global__ void adam_multi_kernel(TensorTable t, float* __restrict__ m, float* __restrict__ v, Rate rate, float b1,
                                  float b2, float scale) {
    const StepBc s = rate();
    const long total = t.start[t.count];
    for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        int k = 0;
        while (i >= t.start[k + 1]) ++k;           // ≤ 24 tensors, uniform-ish
        const long j = i - t.start[k];
        float pp = t.p[k][j], mm = m[i], vv = v[i];
        adam_elem(pp, t.g[k][j], mm, vv, s.step, b1, b2, s.bc2, scale);
        t.p[k][j] = pp; m[i] = mm; v[i] = vv;
    }
}

int grid_for(long n) {
    long g = (n + TPB - 1) / TPB;
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;
    return (int)g;
}

// the float4 kernels' spans: p, g, m, v 16-B aligned, the bf16 shadow (when there is one) 8-B
bool span_vec_ok(const float* p, const float* g, const float* m, const float* v, const unsigned short* w16) {
    return (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15u) == 0 && ((uintptr_t)w16 & 7u) == 0;
}

// f(the rate's functor): the instantiation is picked here, on the host
template <class F>
void with_rate(PhipAdamRate rate, float bc1, float bc2, F&& f) {
    if (rate.d_lr) f(RateWord::of(rate, bc1, bc2));
    else f(RateValue::of(rate, bc1, bc2));
}

}  // namespace

extern "C" {

void phip_adam_flat(const PhipAdamSpan* span, PhipAdamRate rate, float beta1, float beta2, unsigned short* w16,
                    long n16, const float* coef, const unsigned* skip) {
    const PhipAdamSpan& s = *span;
    if (s.n <= 0) return;
    ppo::ProfScope ps(PPO_K_ADAM, 28.0 * s.n + (w16 ? 2.0 * n16 : 0.0) + (s.zero_g ? 4.0 * s.n : 0.0));
    const bool vec = span_vec_ok(s.p, s.g, s.m, s.v, w16);
    PPO_REQUIRE(vec || (!w16 && !s.zero_g), "phip_adam_flat: unaligned span with a bf16 shadow or gradient clear");
    with_rate(rate, s.bc1, s.bc2, [&](auto r) {
        if (vec)
            hipLaunchKernelGGL(adam_flat_vec_kernel<decltype(r)>, dim3(grid_for((s.n + 3) / 4)), dim3(TPB), 0,
                               ppo::stream(), s.p, s.g, s.m, s.v, s.n, r, beta1, beta2, s.grad_scale,
                               reinterpret_cast<__bf16*>(w16), n16, s.zero_g, coef, skip);
        else
            hipLaunchKernelGGL(adam_flat_kernel<decltype(r)>, dim3(grid_for(s.n)), dim3(TPB), 0, ppo::stream(), s.p,
                               s.g, s.m, s.v, s.n, r, beta1, beta2, s.grad_scale, coef, skip);
    });
    PPO_LAUNCH_CHECK();
}

void phip_adam_flat_pair(const PhipAdamSpan* span, PhipAdamRate rate, const PhipAdamSpan* side_span,
                         PhipAdamRate side_rate, float beta1, float beta2, unsigned short* w16, long n16,
                         const float* coef, const unsigned* skip) {
    const PhipAdamSpan &s = *span, &s2 = *side_span;
    PPO_REQUIRE(s.n > 0 && s2.n >= 0 && s2.n <= TPB && !rate.d_lr == !side_rate.d_lr, "phip_adam_flat_pair: spans");
    PPO_REQUIRE(span_vec_ok(s.p, s.g, s.m, s.v, w16), "phip_adam_flat_pair: the network span must be 16-B aligned");
    ppo::ProfScope ps(PPO_K_ADAM, 28.0 * (s.n + s2.n) + (w16 ? 2.0 * n16 : 0.0) + (s.zero_g ? 4.0 * s.n : 0.0));
    with_rate(rate, s.bc1, s.bc2, [&](auto r) {
        using Rate = decltype(r);
        SideSpan<Rate> side{s2.p, s2.g, s2.m, s2.v, (int)s2.n, Rate::of(side_rate, s2.bc1, s2.bc2), s2.grad_scale,
                            s2.zero_g};
        hipLaunchKernelGGL(adam_flat_vec_pair_kernel<Rate>, dim3(grid_for((s.n + 3) / 4)), dim3(TPB), 0, ppo::stream(),
                           s.p, s.g, s.m, s.v, s.n, r, beta1, beta2, s.grad_scale, reinterpret_cast<__bf16*>(w16), n16,
                           s.zero_g, side, coef, skip);
    });
    PPO_LAUNCH_CHECK();
}

void phip_adam_flat_tab(const PhipAdamSpan* span, const PhipStepArgs* tab, int* ctr, unsigned* ticket, int which,
                        float beta1, float beta2, unsigned short* w16, long n16) {
    const PhipAdamSpan& s = *span;
    if (s.n <= 0) return;
    PPO_REQUIRE(span_vec_ok(s.p, s.g, s.m, s.v, w16), "phip_adam_flat_tab: unaligned span");
    hipLaunchKernelGGL(adam_flat_tab_kernel, dim3(grid_for((s.n + 3) / 4)), dim3(TPB), 0, ppo::stream(), s.p, s.g, s.m,
                       s.v, s.n, RateTable{tab, ctr, which}, ticket, beta1, beta2, s.grad_scale,
                       reinterpret_cast<__bf16*>(w16), n16, s.zero_g);
    PPO_LAUNCH_CHECK();
}

void phip_adam_multi(float* const* params, float* const* grads, const int* lengths, int num_tensors, float* m,
                     float* v, PhipAdamRate rate, float beta1, float beta2, float bias_correction1,
                     float bias_correction2, float grad_scale) {
    long base = 0;
    for (int t0 = 0; t0 < num_tensors; t0 += MAXT) {
        TensorTable t{};
        t.count = num_tensors - t0 < MAXT ? num_tensors - t0 : MAXT;
        t.start[0] = 0;
        for (int k = 0; k < t.count; ++k) {
            t.p[k] = params[t0 + k];
            t.g[k] = grads[t0 + k];
            t.start[k + 1] = t.start[k] + lengths[t0 + k];
        }
        const long total = t.start[t.count];
        if (total > 0) {
            ppo::ProfScope ps(PPO_K_ADAM, 28.0 * total);
            with_rate(rate, bias_correction1, bias_correction2, [&](auto r) {
                hipLaunchKernelGGL(adam_multi_kernel<decltype(r)>, dim3(grid_for(total)), dim3(TPB), 0, ppo::stream(),
                                   t, m + base, v + base, r, beta1, beta2, grad_scale);
            });
            PPO_LAUNCH_CHECK();
        }
        base += total;
    }
}

}  // extern "C"
