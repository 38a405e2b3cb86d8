// obsnorm.hip — running observation normalisation for the device PPO update (no counterpart in the
// reference; VecNormalize / CleanRL NormalizeObservation semantics, ppo_ext.h ppo_set_obs_norm).
//
// Running state per observation column j, in double: a shared count n, mean[j], M2[j] (the sum of squared
// deviations; population variance M2/n) — one device array {n, mean[S], M2[S]}.  The fp32 affine pair
//     m[j] = (float)mean[j],   r[j] = (float)(1 / sqrt(M2[j]/n + 1e-8))        (n = 0: m = 0, r = 1)
// is refreshed by obs_affine_kernel after every change of the triple, and one element normalises as
//     t = (x − m[j]) · r[j];   y = t < −c ? −c : (t > c ? c : t)               (fp32, no contraction)
// with NaN propagating; while n = 0 the clamp is ignored, so an un-warmed normaliser is the identity.
//
// All kernels are pure streaming.  Rows are [n, S] row-major fp32 with S arbitrary: a thread owns one
// column unit — four consecutive columns read as one 16-byte access when S % 4 = 0 and the base is 16-byte
// aligned, one column otherwise — and walks down the rows, so its per-column vectors (m, r, the running
// sums) live in registers and consecutive threads touch consecutive addresses.  A row's units are split
// into equal tiles of at most 64 threads (S = 376: two tiles of 47 float4s), the rest of the 256-thread
// workgroup takes further rows.
//
// Statistics are deterministic: no floating-point atomic anywhere.  A thread sums its rows in the shifted
// form (K = its first element; Σ(x − K), Σ(x − K)² in double — never Σx²), the workgroup folds its row
// threads by Chan's pairwise combine (reduce.h's chan) in thread order through LDS, each workgroup writes one partial
// (mean, M2) per column, and a second launch folds the ≤ 512 partials of a column in a fixed two-level order
// (16 groups of consecutive partials in index order, then the groups in order).  The grid
// is a function of (n, S, alignment) only, so the same rows give the same bits.  The clamped-element
// counter is an integer atomic: exact in any order.
#include "dev.h"
#include "reduce.h"

namespace {

constexpr int TPB = 256;
constexpr int MAX_PARTS = 512;      // row blocks of the statistics kernel (partials per column)
constexpr int MAX_NORM_PARTS = 2048;
constexpr int UNR_STATS = 8;        // independent row loads in flight per thread
constexpr int UNR_NORM = 4;

struct Tile {
    int U, CU, tiles, bx, by;       // columns per unit, units per row, tiles per row, block = (bx, by)
};

Tile tile_for(int S, bool vec) {
    Tile t;
    t.U = vec ? 4 : 1;
    t.CU = S / t.U;
    t.tiles = (t.CU + 63) / 64;
    t.bx = (t.CU + t.tiles - 1) / t.tiles;
    t.by = TPB / t.bx;
    return t;
}

using ppo::chan;                    // (na, ma, Ma) ← (na, ma, Ma) ⊕ (nb, mb, Mb), reduce.h

template <int U> struct Vec;
template <> struct Vec<4> { using T = float4; };
template <> struct Vec<1> { using T = float; };

template <int U>
__device__ __forceinline__ void unpack(const typename Vec<U>::T& v, float* o);
template <>
__device__ __forceinline__ void unpack<4>(const float4& v, float* o) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
template <>
__device__ __forceinline__ void unpack<1>(const float& v, float* o) { o[0] = v; }

// one partial (mean, M2) per column and row block: part_mean / part_m2 [gridDim.y][S]; the block's count is
// its row count (rows [by·R, min(n, (by+1)·R)), known to the fold)
template <int U>
__global__ void __launch_bounds__(TPB) obs_stats_kernel(const float* __restrict__ x, long n, int S, int CU, long R,
                                                        double* __restrict__ part_mean,
                                                        double* __restrict__ part_m2) {
    using V = typename Vec<U>::T;
    __shared__ double s_mean[TPB * U], s_m2[TPB * U], s_cnt[TPB];
    const int tx = threadIdx.x, ty = threadIdx.y, by = blockDim.y;
    const int cu = blockIdx.x * blockDim.x + tx;
    const long r0 = (long)blockIdx.y * R, r1 = r0 + R < n ? r0 + R : n;
    const bool active = cu < CU;
    double K[U], s1[U], s2[U];
#pragma unroll
    for (int u = 0; u < U; ++u) K[u] = s1[u] = s2[u] = 0.0;
    long cnt = 0;
    if (active && r0 + ty < r1) {
        const V* __restrict__ xv = reinterpret_cast<const V*>(x);
        const long first = r0 + ty;
        float f[U];
        unpack<U>(xv[first * CU + cu], f);
#pragma unroll
        for (int u = 0; u < U; ++u) K[u] = (double)f[u];
        // rows past the block re-read the thread's first row and add nothing: no load behind a branch
        for (long r = first; r < r1; r += (long)by * UNR_STATS) {
            V v[UNR_STATS];
#pragma unroll
            for (int k = 0; k < UNR_STATS; ++k) {
                const long rk = r + (long)k * by;
                v[k] = xv[(rk < r1 ? rk : first) * CU + cu];
            }
#pragma unroll
            for (int k = 0; k < UNR_STATS; ++k) {
                if (r + (long)k * by < r1) {
                    unpack<U>(v[k], f);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const double d = (double)f[u] - K[u];
                        s1[u] += d;
                        s2[u] += d * d;
                    }
                    ++cnt;
                }
            }
        }
    }
    const int slot = ty * blockDim.x + tx;
    s_cnt[slot] = (double)cnt;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        double mean = 0.0, m2 = 0.0;
        if (cnt > 0) {
            const double c = (double)cnt, a = s1[u] / c;
            mean = K[u] + a;
            m2 = s2[u] - s1[u] * a;
            if (!(m2 >= 0.0) && m2 == m2) m2 = 0.0;       // rounding below zero (NaN stays)
        }
        s_mean[slot * U + u] = mean;
        s_m2[slot * U + u] = m2;
    }
    __syncthreads();
    if (ty != 0 || !active) return;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        double na = 0.0, ma = 0.0, Ma = 0.0;
        for (int j = 0; j < by; ++j) {
            const int sj = j * blockDim.x + tx;
            chan(na, ma, Ma, s_cnt[sj], s_mean[sj * U + u], s_m2[sj * U + u]);
        }
        const long o = (long)blockIdx.y * S + (long)cu * U + u;
        part_mean[o] = ma;
        part_m2[o] = Ma;
    }
}

// the G row-block partials of each column → triple {n, mean[S], M2[S]}, in a fixed two-level order: thread
// (column, group q) folds the consecutive partials [q·per, (q+1)·per) in index order, then group 0 folds the
// PARTS_GROUPS group results in group order through LDS — a dependent chain of G/16 + 16 combines per column
// instead of G.  Block = (PARTS_COLS columns, PARTS_GROUPS groups).
constexpr int PARTS_COLS = 16, PARTS_GROUPS = 16;
__global__ void __launch_bounds__(PARTS_COLS* PARTS_GROUPS)
    obs_parts_kernel(const double* __restrict__ part_mean, const double* __restrict__ part_m2, int G, long R, long n,
                     int S, double* __restrict__ triple) {
    __shared__ double s_n[PARTS_GROUPS][PARTS_COLS], s_mean[PARTS_GROUPS][PARTS_COLS], s_m2[PARTS_GROUPS][PARTS_COLS];
    const int tx = threadIdx.x, q = threadIdx.y;
    const int j = blockIdx.x * PARTS_COLS + tx;
    const int per = (G + PARTS_GROUPS - 1) / PARTS_GROUPS;
    double na = 0.0, ma = 0.0, Ma = 0.0;
    if (j < S) {
        const int g1 = (q + 1) * per < G ? (q + 1) * per : G;
        for (int g = q * per; g < g1; ++g) {
            const long r0 = (long)g * R, r1 = r0 + R < n ? r0 + R : n;
            chan(na, ma, Ma, (double)(r1 - r0), part_mean[(long)g * S + j], part_m2[(long)g * S + j]);
        }
    }
    s_n[q][tx] = na;
    s_mean[q][tx] = ma;
    s_m2[q][tx] = Ma;
    __syncthreads();
    if (q != 0 || j >= S) return;
    for (int k = 1; k < PARTS_GROUPS; ++k) chan(na, ma, Ma, s_n[k][tx], s_mean[k][tx], s_m2[k][tx]);
    triple[1 + j] = ma;
    triple[1 + S + j] = Ma;
    if (j == 0) triple[0] = (double)n;
}

// `count` triples of 1 + 2S doubles (ranks in rank order; empty ones skipped) combined, then folded into the
// running triple.  One workgroup: every thread reads the running count before thread 0 replaces it.
__global__ void __launch_bounds__(TPB) obs_fold_kernel(const double* __restrict__ triples, int count, int S,
                                                       double* __restrict__ run) {
    const long stride = 1 + 2L * S;
    const double n_run = run[0];
    double n_new = 0.0;
    for (int r = 0; r < count; ++r) {
        const double nb = triples[r * stride];
        if (nb > 0.0) n_new += nb;
    }
    for (int j = threadIdx.x; j < S; j += TPB) {
        double na = 0.0, ma = 0.0, Ma = 0.0;
        for (int r = 0; r < count; ++r) {
            const double* t = triples + r * stride;
            chan(na, ma, Ma, t[0], t[1 + j], t[1 + S + j]);
        }
        double nr = n_run, mr = run[1 + j], Mr = run[1 + S + j];
        chan(nr, mr, Mr, na, ma, Ma);
        run[1 + j] = mr;
        run[1 + S + j] = Mr;
    }
    __syncthreads();
    if (threadIdx.x == 0) run[0] = n_run + n_new;
}

__global__ void __launch_bounds__(TPB) obs_affine_kernel(const double* __restrict__ run, int S, float* __restrict__ m,
                                                         float* __restrict__ r) {
    const int j = blockIdx.x * TPB + threadIdx.x;
    if (j >= S) return;
    const double n = run[0];
    if (!(n > 0.0)) { m[j] = 0.f; r[j] = 1.f; return; }
    m[j] = (float)run[1 + j];
    r[j] = (float)(1.0 / sqrt(run[1 + S + j] / n + 1e-8));
}

__device__ __forceinline__ float norm1(float x, float m, float r, float c) {
    const float t = (x - m) * r;
    return t < -c ? -c : (t > c ? c : t);
}
// the same, counting the element when it was clamped (y != t and t is not NaN)
__device__ __forceinline__ float norm1(float x, float m, float r, float c, unsigned& clamped) {
    const float t = (x - m) * r;
    const float y = t < -c ? -c : (t > c ? c : t);
    clamped += (y != t && t == t) ? 1u : 0u;
    return y;
}

// y[0:n] ← norm(x[0:n]); y may be x (every element is read and written by the same thread).  run: the
// running triple (its count 0: no clamp); counts (may be null): [0] += clamped, [1] += elements
template <int U>
__global__ void __launch_bounds__(TPB) obs_norm_kernel(const float* x, float* y, long n, int S, int CU, long R,
                                                       const float* __restrict__ m, const float* __restrict__ r,
                                                       float clip, const double* __restrict__ run,
                                                       unsigned long long* counts) {
    using V = typename Vec<U>::T;
    __shared__ unsigned long long s_clamped;
    const int tx = threadIdx.x, ty = threadIdx.y, by = blockDim.y;
    if (tx == 0 && ty == 0) s_clamped = 0ull;
    __syncthreads();
    const int cu = blockIdx.x * blockDim.x + tx;
    const long r0 = (long)blockIdx.y * R, r1 = r0 + R < n ? r0 + R : n;
    const float c = run[0] > 0.0 ? clip : INFINITY;
    unsigned clamped = 0;
    if (cu < CU && r0 + ty < r1) {
        const V* xv = reinterpret_cast<const V*>(x);
        V* yv = reinterpret_cast<V*>(y);
        float mv[U], rv[U];
        unpack<U>(reinterpret_cast<const V*>(m)[cu], mv);
        unpack<U>(reinterpret_cast<const V*>(r)[cu], rv);
        const long first = r0 + ty;
        for (long row = first; row < r1; row += (long)by * UNR_NORM) {
            V v[UNR_NORM];
#pragma unroll
            for (int k = 0; k < UNR_NORM; ++k) {
                const long rk = row + (long)k * by;
                v[k] = xv[(rk < r1 ? rk : first) * CU + cu];
            }
#pragma unroll
            for (int k = 0; k < UNR_NORM; ++k) {
                const long rk = row + (long)k * by;
                if (rk < r1) {
                    float f[U];
                    unpack<U>(v[k], f);
#pragma unroll
                    for (int u = 0; u < U; ++u) f[u] = norm1(f[u], mv[u], rv[u], c, clamped);
                    if constexpr (U == 4) yv[rk * CU + cu] = make_float4(f[0], f[1], f[2], f[3]);
                    else yv[rk * CU + cu] = f[0];
                }
            }
        }
    }
    if (!counts) return;                      // uniform over the launch
    if (clamped) atomicAdd(&s_clamped, (unsigned long long)clamped);
    __syncthreads();
    if (tx == 0 && ty == 0) {
        if (s_clamped) atomicAdd(&counts[0], s_clamped);
        if (blockIdx.x == 0 && blockIdx.y == 0) atomicAdd(&counts[1], (unsigned long long)n * (unsigned long long)S);
    }
}

// dst[dst_rows[i]] ← norm(src[src_rows[i]]) for i < rows (a null list: the identity); one workgroup per row.
// Rollout and next_state rows are not counted: the clamp counters describe the update's state normalisation.
__global__ void __launch_bounds__(64) obs_norm_rows_kernel(const float* src, const int* __restrict__ src_rows,
                                                           float* dst, const int* __restrict__ dst_rows, int rows,
                                                           int S, int vec, const float* __restrict__ m,
                                                           const float* __restrict__ r, float clip,
                                                           const double* __restrict__ run) {
    const float c = run[0] > 0.0 ? clip : INFINITY;
    for (int i = blockIdx.x; i < rows; i += gridDim.x) {
        const long sr = src_rows ? src_rows[i] : i, dr = dst_rows ? dst_rows[i] : i;
        const float* xs = src + sr * S;
        float* yd = dst + dr * S;
        if (vec) {
            for (int q = threadIdx.x; q < S / 4; q += 64) {
                const float4 v = reinterpret_cast<const float4*>(xs)[q];
                const float4 mv = reinterpret_cast<const float4*>(m)[q], rv = reinterpret_cast<const float4*>(r)[q];
                reinterpret_cast<float4*>(yd)[q] =
                    make_float4(norm1(v.x, mv.x, rv.x, c), norm1(v.y, mv.y, rv.y, c), norm1(v.z, mv.z, rv.z, c),
                                norm1(v.w, mv.w, rv.w, c));
            }
        } else {
            for (int j = threadIdx.x; j < S; j += 64) yd[j] = norm1(xs[j], m[j], r[j], c);
        }
    }
}

// the statistics kernel's partials: [2][G][S], grow-only, one per process and never freed (as gae.hip's and
// ppo.c's GAE scratch).  By contract libppo's launchers are called from one host thread and these launches go
// to libppo's main stream only, so consecutive statistics launches are stream-ordered and may share it.
double* g_parts = nullptr;
size_t g_parts_cap = 0;

bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

void phip_obs_stats(const float* x, long n, int S, double* triple) {
    PPO_REQUIRE(n >= 0 && S > 0 && triple && (x || n == 0), "phip_obs_stats: operands");
    if (n == 0) {                   // an empty shard: the zero triple (n = 0 is skipped by every combine)
        phip_memset(triple, 0, sizeof(double) * (size_t)(1 + 2L * S));
        return;
    }
    const bool vec = S % 4 == 0 && al16(x);
    const Tile t = tile_for(S, vec);
    long G = (n + (long)t.by * UNR_STATS - 1) / ((long)t.by * UNR_STATS);
    if (G > MAX_PARTS) G = MAX_PARTS;
    const long R = (n + G - 1) / G;
    G = (n + R - 1) / R;            // no empty row block
    const size_t need = 2 * (size_t)G * (size_t)S;
    if (need > g_parts_cap) {
        phip_free(g_parts);
        g_parts = (double*)phip_malloc(sizeof(double) * need);
        g_parts_cap = need;
    }
    double* pm = g_parts;
    double* pM = g_parts + (size_t)G * S;
    {
        ppo::ProfScope ps(PPO_K_OTHER, 4.0 * (double)n * S);
        const dim3 grid(t.tiles, (unsigned)G), block(t.bx, t.by);
        if (vec) hipLaunchKernelGGL(obs_stats_kernel<4>, grid, block, 0, ppo::stream(), x, n, S, t.CU, R, pm, pM);
        else hipLaunchKernelGGL(obs_stats_kernel<1>, grid, block, 0, ppo::stream(), x, n, S, t.CU, R, pm, pM);
        PPO_LAUNCH_CHECK();
    }
    // the small combines (partials, rank triples, affine refresh) are timed with the GAE class, like the
    // advantage statistics' welford_combine, so a profile separates them from the streaming launch above
    ppo::ProfScope ps(PPO_K_GAE, 16.0 * (double)G * S);
    hipLaunchKernelGGL(obs_parts_kernel, dim3(ppo_divup(S, PARTS_COLS)), dim3(PARTS_COLS, PARTS_GROUPS), 0,
                       ppo::stream(), pm, pM, (int)G, R, n, S, triple);
    PPO_LAUNCH_CHECK();
}

void phip_obs_fold(const double* triples, int count, int S, double* run) {
    PPO_REQUIRE(triples && run && count > 0 && S > 0, "phip_obs_fold: operands");
    ppo::ProfScope ps(PPO_K_GAE, 8.0 * (double)(count + 2) * (1 + 2.0 * S));
    hipLaunchKernelGGL(obs_fold_kernel, dim3(1), dim3(TPB), 0, ppo::stream(), triples, count, S, run);
    PPO_LAUNCH_CHECK();
}

void phip_obs_affine(const double* run, int S, float* m, float* r) {
    PPO_REQUIRE(run && m && r && S > 0, "phip_obs_affine: operands");
    ppo::ProfScope ps(PPO_K_GAE, 24.0 * S);
    hipLaunchKernelGGL(obs_affine_kernel, dim3(ppo_divup(S, TPB)), dim3(TPB), 0, ppo::stream(), run, S, m, r);
    PPO_LAUNCH_CHECK();
}

void phip_obs_normalize(const float* x, float* y, long n, int S, const float* m, const float* r, float clip,
                        const double* run, unsigned long long* counts) {
    PPO_REQUIRE(n >= 0 && S > 0 && m && r && run && ((x && y) || n == 0), "phip_obs_normalize: operands");
    if (n == 0) return;
    const bool vec = S % 4 == 0 && al16(x) && al16(y) && al16(m) && al16(r);
    const Tile t = tile_for(S, vec);
    long G = (n + (long)t.by * UNR_NORM - 1) / ((long)t.by * UNR_NORM);
    const long cap = MAX_NORM_PARTS / t.tiles > 0 ? MAX_NORM_PARTS / t.tiles : 1;
    if (G > cap) G = cap;
    const long R = (n + G - 1) / G;
    G = (n + R - 1) / R;
    ppo::ProfScope ps(PPO_K_OTHER, 8.0 * (double)n * S);
    const dim3 grid(t.tiles, (unsigned)G), block(t.bx, t.by);
    if (vec) hipLaunchKernelGGL(obs_norm_kernel<4>, grid, block, 0, ppo::stream(), x, y, n, S, t.CU, R, m, r, clip, run, counts);
    else hipLaunchKernelGGL(obs_norm_kernel<1>, grid, block, 0, ppo::stream(), x, y, n, S, t.CU, R, m, r, clip, run, counts);
    PPO_LAUNCH_CHECK();
}

void phip_obs_normalize_rows(const float* src, const int* src_rows, float* dst, const int* dst_rows, int rows, int S,
                             const float* m, const float* r, float clip, const double* run) {
    PPO_REQUIRE(rows >= 0 && S > 0 && m && r && run && ((src && dst) || rows == 0), "phip_obs_normalize_rows: operands");
    if (rows == 0) return;
    const int vec = S % 4 == 0 && al16(src) && al16(dst) && al16(m) && al16(r);
    ppo::ProfScope ps(PPO_K_OTHER, 8.0 * (double)rows * S);
    hipLaunchKernelGGL(obs_norm_rows_kernel, dim3(rows < 4096 ? rows : 4096), dim3(64), 0, ppo::stream(), src, src_rows,
                       dst, dst_rows, rows, S, vec, m, r, clip, run);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
