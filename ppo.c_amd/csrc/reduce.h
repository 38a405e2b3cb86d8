// reduce.h — the fixed-order reductions behind libppo's statistics, each written once ("One
// definition per arithmetic").  Device code only.  The kernels of gae.hip, retnorm.hip, obsnorm.hip, episode.hip,
// advnorm.hip, kl.hip and clip.hip keep their loops and call these; their contract is "the same input gives the
// same bits", so the written expression and the order ARE the definition.  Two of the families below come in two
// orders that round differently — Chan's combine (chan / chan_ref_order) and the tree over a workgroup's threads
// (tree_fold / block_sum_halving): each has its own users, and a kernel never moves from one to the other.
#pragma once
#include "dev.h"

namespace ppo {

// ---- Chan et al.'s combine of two (n, mean, M2) triples --------------------------------------------------------
// (na, ma, Ma) ← (na, ma, Ma) ⊕ (nb, mb, Mb); an empty b leaves a as it is.  The order of obsnorm.hip, retnorm.hip
// and episode.hip: f = nb/n first, then ma + δ·f and (Ma + Mb) + (δ·δ)·(na·f).  tests/obsnorm_ref.py restates it.
__device__ __forceinline__ void chan(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
    if (!(nb > 0.0)) return;
    if (!(na > 0.0)) { na = nb; ma = mb; Ma = Mb; return; }
    const double n = na + nb, delta = mb - ma;
    ma = ma + delta * (nb / n);
    Ma = (Ma + Mb) + delta * delta * (na * (nb / n));
    na = n;
}

// The same combine in the order of the reference's welford_var.h, which gae.hip's advantage statistics keep:
// mean + (δ·nb)/nn and M2 + (M2b + (((δ·δ)·n)·nb)/nn) — the products first, one division at the end of each —
// with `<= 0` guards.  NOT interchangeable with chan above: the two round differently, so swapping them would
// move every normalised advantage.  tests/gae_ref.py restates this one.
__device__ __forceinline__ void chan_ref_order(double& n, double& mean, double& m2, double nb, double mb,
                                               double m2b) {
    if (nb <= 0.0) return;
    if (n <= 0.0) { n = nb; mean = mb; m2 = m2b; return; }
    const double nn = n + nb, d = mb - mean;
    mean += d * nb / nn;
    m2 += m2b + d * d * n * nb / nn;
    n = nn;
}

struct Triple { double n, mean, m2; };
struct TripleAt {                         // triple i of a packed array of triples
    const double* p;
    __device__ Triple operator()(int i) const { return Triple{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
};
using ChanFn = void(double&, double&, double&, double, double, double);
template <ChanFn F> struct TripleMerge {  // chan or chan_ref_order as a fold's operation
    __device__ Triple operator()(Triple a, const Triple& b) const { F(a.n, a.mean, a.m2, b.n, b.mean, b.m2); return a; }
};
struct DaddRn { __device__ double operator()(double a, double b) const { return __dadd_rn(a, b); } };

// ---- runs, then a pairwise tree over the threads ---------------------------------------------------------------
// The pairwise tree over s[0 … T) of a T-thread workgroup: stride 1, 2, 4, …, thread t, a multiple of 2·stride,
// does s[t] = op(s[t], s[t + stride]).  Thread t has stored s[t]; every thread calls this and gets s[0].  NOT the
// halving tree of block_sum_halving below, which pairs t with t + T/2 first.
template <int T, class A, class Op>
__device__ __forceinline__ A tree_fold(A* s, int t, Op op) {
    __syncthreads();
#pragma unroll
    for (int stride = 1; stride < T; stride *= 2) {
        if ((t & (2 * stride - 1)) == 0) s[t] = op(s[t], s[t + stride]);
        __syncthreads();
    }
    return s[0];
}

// `count` aggregates folded by one T-thread workgroup in an order that is a function of count alone: thread t
// folds the contiguous run [t·per, (t+1)·per), per = ⌈count/T⌉, in index order from `zero`, then tree_fold.
// load(i) supplies aggregate i; s: T aggregates of LDS.
template <int T, class A, class Load, class Op>
__device__ __forceinline__ A fold_runs_tree(A* s, int count, A zero, Load load, Op op) {
    const int t = threadIdx.x;
    const int per = (count + T - 1) / T;
    A a = zero;
    for (int i = t * per; i < min(count, (t + 1) * per); ++i) a = op(a, load(i));
    s[t] = a;
    return tree_fold<T>(s, t, op);
}

// ---- a workgroup's (n, mean, M2) over the values its threads hold in registers ---------------------------------
// Two passes, in double: the wave xor-butterfly of the thread sums and counts, the T/64 wave totals added wave
// ascending through LDS, mean = Σ/n; then Σ(x − mean)² the same way.  The thread's `sum` over its valid values is
// accumulated by the caller, in the caller's order; x[e] is valid iff e < valid.  Thread 0 stores the triple to
// out[0 … 2].  red: T/64 doubles, red_n: T/64 ints of LDS.  Every thread of the workgroup calls it.
template <int T, int EPT, class X>
__device__ __forceinline__ void block_two_pass_triple(double sum, int cnt, const X (&x)[EPT], long valid, double* red,
                                                      int* red_n, double* out) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double s = sum;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    int c_tot = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c_tot += __shfl_xor(c_tot, o, 64);
    if (lane == 0) { red[w] = s; red_n[w] = c_tot; }
    __syncthreads();
    double bs = 0.0; long bn = 0;
    for (int k = 0; k < T / 64; ++k) { bs += red[k]; bn += red_n[k]; }
    const double mean = bn > 0 ? bs / (double)bn : 0.0;
    double m2 = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e)
        if (e < valid) { const double d = (double)x[e] - mean; m2 += d * d; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m2 += __shfl_xor(m2, o, 64);
    __syncthreads();
    if (lane == 0) red[w] = m2;
    __syncthreads();
    if (threadIdx.x == 0) {
        double bm2 = 0.0;
        for (int k = 0; k < T / 64; ++k) bm2 += red[k];
        out[0] = (double)bn; out[1] = mean; out[2] = bm2;
    }
}

// ---- affine maps x ↦ d + c·x and their scan ---------------------------------------------------------------------
template <class T> struct Affine { T c, d; };
// a ∘ b: b is applied first
template <class T>
__device__ __forceinline__ Affine<T> compose(Affine<T> a, Affine<T> b) { return Affine<T>{a.c * b.c, a.d + a.c * b.d}; }

// Direction of a scan.  RightToLeft: element l is applied after l + 1 (gae.hip: A_t from A_{t+1}); LeftToRight:
// after l − 1 (retnorm.hip: R_i from R_{i−1}).  `toward(v, o)` fetches the value o lanes nearer the scan's start.
struct RightToLeft {
    static constexpr int start = 63, end = 0;
    template <class T> static __device__ __forceinline__ T toward(T v, int o) { return __shfl_down(v, o, 64); }
    static __device__ __forceinline__ bool has(int lane, int o) { return lane + o < 64; }
};
struct LeftToRight {
    static constexpr int start = 0, end = 63;
    template <class T> static __device__ __forceinline__ T toward(T v, int o) { return __shfl_up(v, o, 64); }
    static __device__ __forceinline__ bool has(int lane, int o) { return lane >= o; }
};

// inclusive scan over a wave: lane l ← T_l ∘ … ∘ T_start (Hillis–Steele, offsets 1, 2, … 32)
template <class Dir, class T>
__device__ __forceinline__ Affine<T> wave_scan_inclusive(Affine<T> inc) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const Affine<T> other{Dir::toward(inc.c, o), Dir::toward(inc.d, o)};
        if (Dir::has(lane, o)) inc = compose(inc, other);
    }
    return inc;
}
// the exclusive scan from the inclusive one: the neighbour's value, the identity at the scan's start
template <class Dir, class T>
__device__ __forceinline__ Affine<T> wave_scan_exclusive(Affine<T> inc) {
    Affine<T> excl{Dir::toward(inc.c, 1), Dir::toward(inc.d, 1)};
    if ((threadIdx.x & 63) == Dir::start) excl = Affine<T>{(T)1, (T)0};
    return excl;
}

// Exclusive scan of the per-thread maps of a TPB-thread workgroup: the composition of the threads between the scan's
// start and this one (the identity for the first); *block_total: the whole workgroup's.  wave_tot: TPB/64 maps of LDS.
template <class Dir, int TPB, class T>
__device__ __forceinline__ Affine<T> block_scan_exclusive(Affine<T> m, Affine<T>* wave_tot, Affine<T>* block_total) {
    constexpr int W = TPB / 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const Affine<T> inc = wave_scan_inclusive<Dir>(m);
    const Affine<T> excl = wave_scan_exclusive<Dir>(inc);
    if (lane == Dir::end) wave_tot[w] = inc;
    __syncthreads();
    constexpr int first = Dir::start ? W - 1 : 0, step = Dir::start ? -1 : 1;     // the waves in scan order
    Affine<T> before{(T)1, (T)0};
    for (int k = first; k != w; k += step) before = compose(wave_tot[k], before);
    Affine<T> tot{(T)1, (T)0};
    for (int k = first; k != first + step * W; k += step) tot = compose(wave_tot[k], tot);
    *block_total = tot;
    return compose(excl, before);
}

// ---- the halving tree ------------------------------------------------------------------------------------------
// Sum of one double per thread of a T-thread workgroup, to every thread: w = T/2, T/4, … 1: s[t] += s[t + w] for
// t < w.  s: T doubles of LDS; ends with a barrier, so s may be rewritten.  NOT tree_fold's pairwise order: that
// one adds neighbours first, this one adds halves, and the sums round differently.
template <int T>
__device__ __forceinline__ double block_sum_halving(double v, double* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = T / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// ---- ticket hand-off: the last workgroup of a launch to arrive reads what the others left ----------------------
// No grid barrier and no release fence.  Thread 0 of each workgroup stores its K 8-byte partials with agent-scope
// atomic stores — write-through on gfx950, so they leave this CU for the agent's coherence point — and drains
// them (vmcnt(0)) BEFORE its ticket add: whoever observes the add finds the partials there.  A release fence
// would say the same and write back the whole L2 slice.  The workgroup that draws the last ticket acquires once
// and reads the partials with agent-scope loads (ticket_load).  Returns, uniformly over the workgroup, whether this
// one is the last arriver; flag: one double of LDS.  Its deciding thread resets *ticket last, for the next launch.
template <int K>
__device__ __forceinline__ bool ticket_publish(double* slots, const double (&v)[K], unsigned* ticket, double* flag) {
    if (threadIdx.x == 0) {
        unsigned long long* slot = reinterpret_cast<unsigned long long*>(slots);
#pragma unroll
        for (int k = 0; k < K; ++k)
            __hip_atomic_store(slot + k, (unsigned long long)__double_as_longlong(v[k]), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the write-through stores have left this CU
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag = last ? 1.0 : 0.0;
    }
    __syncthreads();
    return *flag != 0.0;
}
__device__ __forceinline__ double ticket_load(const double* slot) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(slot),
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

}  // namespace ppo
