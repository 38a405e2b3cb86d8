// layernorm.hip — layer normalisation of the hidden pre-activations (ppo_ext.h ppo_set_layer_norm; DESIGN.md §4
// "Layer normalisation"): per row of z [m, l], ẑ = (z − mean)·rstd and h = act(ẑ), no learnable scale or shift, and
// the backward that turns g = ∂loss/∂h into ∂loss/∂z in place.  The row arithmetic is dev.h's ln_* atoms, the row
// sums reduce.h's wave_sum_xor_f32; this file is how the rows are split, held and moved.
//
// Split: a row belongs to one group of LANES lanes and never leaves their registers — no LDS, no barrier, no atomics.
//   l > 128:   LANES = 64, a wave per row, four rows per 256-thread workgroup, NV = ⌈l/256⌉ rounded up to 1, 2, 4, 8 or
//              16 float4 per lane.
//   l <= 128:  LANES = 16, a quarter-wave per row, four rows per wave and sixteen per workgroup, NV = 1 or 2 — the
//              rollout's small forwards and the 64- and 128-wide networks keep all 64 lanes busy.
//   Workgroups stride over the rows.  A group whose row is past m loads zeros and stores nothing (it is never
//   pointed at a live row); its lanes still take part in the shuffles, which stay inside the group.
// Lane mapping: element j is held by lane (j / 4) % LANES of its group in slot j / (4·LANES), component j % 4; NV is
//   a template parameter, so every register array is indexed statically.  Elements at or past l hold +0: they add
//   nothing to a sum and are not stored.
// Sums: a lane adds its own elements in ascending j, then the xor butterfly over the group (32 … 1, or 8 … 1).  The
//   order depends on l alone, so a row's bits are a function of its contents, l, eps and the activation — not of m,
//   of where the row stands, or of the arrays' alignment.
// Memory: when l % 4 == 0 and every base pointer is 16-byte aligned the lanes move dwordx4, four consecutive lanes
//   a 64-byte segment; otherwise the same lanes move the same elements as single dwords.  The forward reads z once
//   and holds it over both passes (mean, then Σ d and Σ d²); the backward reads z and g once each, and h (tanh, ELU only)
//   once, consumed as it arrives: two rows' worth of registers at most, 128 floats a lane at NV = 16.
// Fusing the statistics into the GEMM epilogue is out of scope: a tile would have to own whole rows, and the x3
// tiles are 64 – 256 columns wide.  γ / β would be two more operands of the same loops (h = act(γ·ẑ + β)) and two
// column sums in the backward; nothing here stands in their way.
#include "dev.h"
#include "reduce.h"

namespace {

using namespace ppo;

constexpr int TPB = 256;
constexpr int MAX_L = 4096;

// one row's elements of this lane: in-range ones from p (the row's base), the rest +0; `live`: the row exists
template <int NV, int LANES>
__device__ __forceinline__ void load_row(float (&v)[NV][4], const float* __restrict__ p, int l, int sub, bool vec,
                                         bool live) {
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        const int j = (s * LANES + sub) * 4;
        if (vec) {                                        // l % 4 == 0: j < l covers j + 3
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live && j < l) q = *reinterpret_cast<const float4*>(p + j);
            v[s][0] = q.x; v[s][1] = q.y; v[s][2] = q.z; v[s][3] = q.w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[s][c] = (live && j + c < l) ? p[j + c] : 0.f;
        }
    }
}

template <int NV, int LANES>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float (&v)[NV][4], int l, int sub, bool vec,
                                          bool live) {
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        const int j = (s * LANES + sub) * 4;
        if (vec) {
            if (live && j < l) *reinterpret_cast<float4*>(p + j) = make_float4(v[s][0], v[s][1], v[s][2], v[s][3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (live && j + c < l) p[j + c] = v[s][c];
        }
    }
}

// the lane's elements in ascending j, then the group's butterfly
template <int NV, int LANES>
__device__ __forceinline__ float row_sum(const float (&v)[NV][4]) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) s += v[k][c];
    return wave_sum_xor_f32<LANES>(s);
}

template <int ACT, int NV, int LANES>
__global__ __launch_bounds__(TPB) void ln_fwd(const float* __restrict__ z, float* __restrict__ h,
                                              float* __restrict__ stat, int m, int l, float eps, int vec) {
    constexpr int RPW = 64 / LANES, RPB = (TPB / 64) * RPW;
    const int lane = threadIdx.x & 63, sub = lane % LANES;
    const int rb = (threadIdx.x >> 6) * RPW + lane / LANES;
    for (long base = (long)blockIdx.x * RPB; base < m; base += (long)gridDim.x * RPB) {
        const long row = base + rb;
        const bool live = row < m;
        const size_t at = live ? (size_t)row * (size_t)l : 0;
        float v[NV][4];
        load_row<NV, LANES>(v, z + at, l, sub, vec != 0, live);
        const float mean = ln_mean(row_sum<NV, LANES>(v), l);
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int c = 0; c < 4; ++c) v[s][c] = (s * LANES + sub) * 4 + c < l ? v[s][c] - mean : 0.f;
        float q[NV][4];
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int c = 0; c < 4; ++c) q[s][c] = v[s][c] * v[s][c];
        const float dsum = row_sum<NV, LANES>(v);             // Σ d: the mean's own rounding error, times −l
        const float rstd = ln_rstd(row_sum<NV, LANES>(q), dsum, l, eps);
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int c = 0; c < 4; ++c) v[s][c] = ln_act_fwd<ACT>(v[s][c] * rstd);
        store_row<NV, LANES>(h + at, v, l, sub, vec != 0, live);
        if (live && sub == 0) {
            stat[2 * row] = mean;
            stat[2 * row + 1] = rstd;
        }
    }
}

// g ← ∂loss/∂z in place.  h is read for tanh and ELU only (it may be NULL otherwise)
template <int ACT, int NV, int LANES>
__global__ __launch_bounds__(TPB) void ln_bwd(float* __restrict__ g, const float* __restrict__ z,
                                              const float* __restrict__ h, const float* __restrict__ stat, int m, int l,
                                              int vec) {
    constexpr int RPW = 64 / LANES, RPB = (TPB / 64) * RPW;
    constexpr bool NEEDS_H = ACT > PHIP_ACT_RELU;
    const int lane = threadIdx.x & 63, sub = lane % LANES;
    const int rb = (threadIdx.x >> 6) * RPW + lane / LANES;
    for (long base = (long)blockIdx.x * RPB; base < m; base += (long)gridDim.x * RPB) {
        const long row = base + rb;
        const bool live = row < m;
        const size_t at = live ? (size_t)row * (size_t)l : 0;
        const float mean = live ? stat[2 * row] : 0.f, rstd = live ? stat[2 * row + 1] : 0.f;
        float zh[NV][4], a[NV][4];
        load_row<NV, LANES>(zh, z + at, l, sub, vec != 0, live);
        load_row<NV, LANES>(a, g + at, l, sub, vec != 0, live);
#pragma unroll
        for (int s = 0; s < NV; ++s) {
            float hv[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (NEEDS_H) {                       // slot s of h alone: four floats, consumed here
                const int j = (s * LANES + sub) * 4;
                if (vec) {
                    if (live && j < l) {
                        const float4 t = *reinterpret_cast<const float4*>(h + at + j);
                        hv[0] = t.x; hv[1] = t.y; hv[2] = t.z; hv[3] = t.w;
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (live && j + c < l) hv[c] = h[at + j + c];
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool in = (s * LANES + sub) * 4 + c < l;
                zh[s][c] = in ? ln_zhat(zh[s][c], mean, rstd) : 0.f;
                a[s][c] = in ? ln_act_bwd<ACT>(a[s][c], zh[s][c], hv[c]) : 0.f;
            }
        }
        const float s1 = ln_mean(row_sum<NV, LANES>(a), l);
        float p[NV][4];
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int c = 0; c < 4; ++c) p[s][c] = a[s][c] * zh[s][c];
        const float s2 = ln_mean(row_sum<NV, LANES>(p), l);
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int c = 0; c < 4; ++c) a[s][c] = ln_dz(a[s][c], zh[s][c], s1, s2, rstd);
        store_row<NV, LANES>(g + at, a, l, sub, vec != 0, live);
    }
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// enough workgroups to cover the rows, at most eight resident per CU's worth of a 256-CU device
template <int LANES>
int grid_for(int m) {
    constexpr int RPB = (TPB / 64) * (64 / LANES);
    const long want = ((long)m + RPB - 1) / RPB;
    return (int)(want < 2048 ? want : 2048);
}

template <int ACT, int NV, int LANES>
void launch_fwd(const float* z, float* h, float* stat, int m, int l, float eps, int vec) {
    hipLaunchKernelGGL((ln_fwd<ACT, NV, LANES>), dim3(grid_for<LANES>(m)), dim3(TPB), 0, ppo::stream(), z, h, stat, m, l,
                       eps, vec);
}
template <int ACT, int NV, int LANES>
void launch_bwd(float* g, const float* z, const float* h, const float* stat, int m, int l, int vec) {
    hipLaunchKernelGGL((ln_bwd<ACT, NV, LANES>), dim3(grid_for<LANES>(m)), dim3(TPB), 0, ppo::stream(), g, z, h, stat, m,
                       l, vec);
}

// the row's register footprint by width: a quarter-wave up to 128, then ⌈l/256⌉ rounded up to a power of two
#define LN_BY_WIDTH(FN, ACT, ...)                                         \
    do {                                                                  \
        if (l <= 64) FN<ACT, 1, 16>(__VA_ARGS__);                         \
        else if (l <= 128) FN<ACT, 2, 16>(__VA_ARGS__);                   \
        else if (l <= 256) FN<ACT, 1, 64>(__VA_ARGS__);                   \
        else if (l <= 512) FN<ACT, 2, 64>(__VA_ARGS__);                   \
        else if (l <= 1024) FN<ACT, 4, 64>(__VA_ARGS__);                  \
        else if (l <= 2048) FN<ACT, 8, 64>(__VA_ARGS__);                  \
        else FN<ACT, 16, 64>(__VA_ARGS__);                                \
    } while (0)
#define LN_BY_ACT(FN, ...)                                                                   \
    do {                                                                                     \
        switch (act) {                                                                       \
            case PHIP_ACT_NONE: LN_BY_WIDTH(FN, PHIP_ACT_NONE, __VA_ARGS__); break;          \
            case PHIP_ACT_RELU: LN_BY_WIDTH(FN, PHIP_ACT_RELU, __VA_ARGS__); break;          \
            case PHIP_ACT_TANH: LN_BY_WIDTH(FN, PHIP_ACT_TANH, __VA_ARGS__); break;          \
            default: LN_BY_WIDTH(FN, PHIP_ACT_ELU, __VA_ARGS__); break;                      \
        }                                                                                    \
    } while (0)

}  // namespace

extern "C" {

int phip_ln_shape_ok(int l, int act) { return l >= 1 && l <= MAX_L && act >= PHIP_ACT_NONE && act <= PHIP_ACT_ELU; }

void phip_ln_fwd(const float* z, float* h, float* stat, int m, int l, int act, float eps) {
    if (m <= 0) return;
    PPO_REQUIRE(phip_ln_shape_ok(l, act), "phip_ln_fwd: width or activation outside the limits");
    const int vec = l % 4 == 0 && al16(z) && al16(h);
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * (2.0 * l + 2));
    LN_BY_ACT(launch_fwd, z, h, stat, m, l, eps, vec);
    PPO_LAUNCH_CHECK();
}

void phip_ln_bwd(float* g, const float* z, const float* h, const float* stat, int m, int l, int act) {
    if (m <= 0) return;
    PPO_REQUIRE(phip_ln_shape_ok(l, act), "phip_ln_bwd: width or activation outside the limits");
    const bool needs_h = act > PHIP_ACT_RELU;
    PPO_REQUIRE(!needs_h || h, "phip_ln_bwd: tanh and ELU read the stored post-activation");
    const int vec = l % 4 == 0 && al16(g) && al16(z) && (!needs_h || al16(h));
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * ((needs_h ? 4.0 : 3.0) * l + 2));
    LN_BY_ACT(launch_bwd, g, z, h, stat, m, l, vec);
    PPO_LAUNCH_CHECK();
}

// average device µs of one launch over `iters` back-to-back launches between two events (ppo_bench_gemm's method):
// op 0 = ln_fwd, 1 = ln_bwd, 2 = hipMemcpyDtoD of `bytes_like` = 0 / 1's byte count (the yardstick of the same visit).
// *bytes_out (may be NULL): the bytes one launch moves.  −1 for a shape the kernels decline.
double ppo_bench_layer_norm(int op, int m, int l, int act, int iters, int bytes_like, double* bytes_out) {
    if (m <= 0 || !phip_ln_shape_ok(l, act) || op < 0 || op > 2 || iters <= 0) return -1.0;
    ppo::ensure_device();
    const size_t n = (size_t)m * l, big = 2 * n + 2 * (size_t)m;      // the largest copy: half of 4·m·(4l + 2) bytes
    const int like = op == 2 ? bytes_like : op;
    const double bytes = 4.0 * m * (like == 0 ? 2.0 * l + 2 : (act > PHIP_ACT_RELU ? 4.0 : 3.0) * l + 2);
    if (bytes_out) *bytes_out = bytes;
    float* z = (float*)phip_malloc(sizeof(float) * n);
    float* h = (float*)phip_malloc(sizeof(float) * n);
    float* g = (float*)phip_malloc(sizeof(float) * big);         // the gradient, and the copy's destination
    float* src = op == 2 ? (float*)phip_malloc(sizeof(float) * big) : nullptr;
    float* st = (float*)phip_malloc(sizeof(float) * 2 * (size_t)m);
    phip_fill_uniform(z, (long)n, 1, -1.f, 1.f);
    phip_fill_uniform(g, (long)big, 2, -1.f, 1.f);
    if (src) phip_fill_uniform(src, (long)big, 3, -1.f, 1.f);
    phip_ln_fwd(z, h, st, m, l, act, 1e-5f);
    const size_t half = (size_t)(bytes / 2) & ~(size_t)15;       // a copy of b bytes reads b/2 and writes b/2
    auto run = [&]() {
        if (op == 0) phip_ln_fwd(z, h, st, m, l, act, 1e-5f);
        else if (op == 1) phip_ln_bwd(g, z, h, st, m, l, act);
        else PPO_CHECK(hipMemcpyDtoDAsync(g, src, half, ppo::stream()));
    };
    for (int i = 0; i < 3; ++i) run();
    hipEvent_t e0, e1;
    PPO_CHECK(hipEventCreate(&e0));
    PPO_CHECK(hipEventCreate(&e1));
    PPO_CHECK(hipEventRecord(e0, ppo::stream()));
    for (int i = 0; i < iters; ++i) run();
    PPO_CHECK(hipEventRecord(e1, ppo::stream()));
    PPO_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    PPO_CHECK(hipEventElapsedTime(&ms, e0, e1));
    PPO_CHECK(hipEventDestroy(e0));
    PPO_CHECK(hipEventDestroy(e1));
    phip_free(z); phip_free(h); phip_free(g); phip_free(st); phip_free(src);
    return 1000.0 * ms / iters;
}

}  // extern "C"
