// gauss_sd.hip — the state-dependent-σ Gaussian policy's head and sampler (ppo_set_action_gaussian_sd; no
// counterpart in the reference).  A row of μ's A outputs z is Aa = A / 2 means followed by Aa raw log σ, clamped to
// [ls_min, ls_max] where it is read.  The per-row arithmetic is ppo_math.h's (the sd_* atoms over the Gaussian
// ones), called, never restated; the KL monitor's mode of it is kl.hip's.
//
// HEAD.  One launch per policy step: z [m, A] and the action rows read once, the gradient [m, A] written once, all
// three by coalesced 16-byte accesses (scalar ones where a pointer is not 16-byte aligned, and for the < 4 floats at
// the end of the last tile).  A workgroup is one wave and owns tiles of 64 rows, a lane per row (Aa <= 32):
//   1. the tile's nr × A outputs go to LDS at the odd row pitch A | 1, the first Aa columns of its action rows at the
//      odd pitch Aa | 1 (an action row is A floats in memory: its zero half shares the 128-byte lines of the other
//      half, so reading whole rows costs no more traffic than reading half of each);
//   2. lane r walks row r of both tiles (its LDS addresses differ from its neighbours' by the odd pitch: no bank
//      conflict): sd_row gives lp, H and the clamped count, surrogate gives g, and the second walk overwrites the
//      tile with the gradient — a clamped column gets +0, written;
//   3. the tile is stored the way it was loaded.
// LDS: 64·((A | 1) + (Aa | 1)) floats — 13.3 KB at Aa = 17, 25 KB at Aa = 32.  Traffic: 3·m·A·4 bytes plus 8 per row.
// The grid is min(⌈m / 64⌉, PHIP_SD_PARTS) workgroups, a function of m alone; workgroup b takes tiles b, b + grid, ….
// The two cross-row sums are deterministic (reduce.h): every lane adds its rows' surrogate and entropy in double in
// tile order, the workgroup folds its 64 lanes by the halving tree, leaves two partials and draws a ticket; the last
// workgroup to arrive folds the partials by fold_runs_tree — an order that is a function of the grid alone — and
// writes the step's loss and entropy sum into the record, and adds the loss to the update's running loss word (one
// thread, a plain add: launches on one stream are ordered).  No floating-point atomic.  The clamped log-σ elements and
// the elements m·Aa are two integer atomics per workgroup.
//
// SAMPLER.  One lane per row through sd_sample_row: a_j = μ_j + normal_at(e·Aa + j, offset, key)·expf(ls_j), columns
// Aa … A−1 ← +0, the log-prob through sd_lp_step as the head's, so both give the same bits on the same (z, a).  The
// dense form and the rollout's (rows[e] of the buffer, offset = kNoise + step) are one kernel; the deterministic
// action is the mean half with zeros after it.  rng.h lists the stream.
#include "dev.h"
#include "ppo_math.h"
#include "reduce.h"
#include "rng.h"

#include <cmath>

namespace {

using namespace ppo_rng;

constexpr int TPB = 64;                              // one wave: a lane per row of a 64-row tile
constexpr int STPB = 256;                            // the sampler's workgroup

// n floats from src (16-byte aligned when VEC) into an LDS tile [rows][pitch], columns < keep only; A floats a row
template <bool VEC>
__device__ __forceinline__ void tile_load(float* tile, int pitch, const float* __restrict__ src, int n, int A,
                                          int keep, int tid) {
    int done = 0;
    if (VEC) {
        const int n4 = n >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        for (int q = tid; q < n4; q += TPB) {
            const float4 v = s4[q];
            const float c[4] = {v.x, v.y, v.z, v.w};
            int row = (4 * q) / A, k = 4 * q - row * A;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (k < keep) tile[row * pitch + k] = c[i];
                if (++k == A) { k = 0; ++row; }
            }
        }
        done = n4 << 2;
    }
    for (int e = done + tid; e < n; e += TPB) {
        const int row = e / A, k = e - row * A;
        if (k < keep) tile[row * pitch + k] = src[e];
    }
}

template <bool VEC>
__device__ __forceinline__ void tile_store(const float* tile, int pitch, float* __restrict__ dst, int n, int A,
                                           int tid) {
    int done = 0;
    if (VEC) {
        const int n4 = n >> 2;
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int q = tid; q < n4; q += TPB) {
            float c[4];
            int row = (4 * q) / A, k = 4 * q - row * A;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                c[i] = tile[row * pitch + k];
                if (++k == A) { k = 0; ++row; }
            }
            d4[q] = make_float4(c[0], c[1], c[2], c[3]);
        }
        done = n4 << 2;
    }
    for (int e = done + tid; e < n; e += TPB) {
        const int row = e / A, k = e - row * A;
        dst[e] = tile[row * pitch + k];
    }
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void sd_head_kernel(const float* __restrict__ z, const float* __restrict__ action,
                                                      const float* __restrict__ adv, const float* __restrict__ old_lp,
                                                      int m, int A, float lo, float hi, float eps, float ent_coeff,
                                                      float* __restrict__ grad, float* __restrict__ lp_out,
                                                      float* __restrict__ ent_out, PhipSdRec* rec,
                                                      float* d_loss_accum) {
    extern __shared__ float lds[];
    __shared__ double red[TPB + 1];                  // red[TPB]: "this workgroup drew the last ticket"
    const int Aa = A >> 1, pitch = A | 1, apitch = Aa | 1;
    float* tile = lds;                               // [64][pitch]: z, then the gradient
    float* at = tile + TPB * pitch;                  // [64][apitch]: the action half
    const int tid = threadIdx.x;
    const int ntiles = (m + TPB - 1) / TPB;
    const float cm = ent_coeff / m;
    double sur_sum = 0.0, ent_sum = 0.0;
    unsigned clamped = 0, elems = 0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long r0 = (long)t * TPB;
        const int nr = (int)min((long)TPB, (long)m - r0);
        const long base = r0 * A;
        tile_load<VEC>(tile, pitch, z + base, nr * A, A, A, tid);
        tile_load<VEC>(at, apitch, action + base, nr * A, A, Aa, tid);
        __syncthreads();
        if (tid < nr) {
            float* zr = tile + tid * pitch;
            const float* ar = at + tid * apitch;
            const ppo::SdRow r = ppo::sd_row(zr, ar, Aa, lo, hi);
            const long i = r0 + tid;
            float g;
            const float sur = ppo::surrogate(adv[i], r.lp, old_lp[i], eps, m, &g);
            for (int j = 0; j < Aa; ++j) {
                const float mu = zr[j], tj = zr[Aa + j];
                zr[j] = ppo::sd_grad_mu(ar[j], mu, ppo::sd_clamp(tj, lo, hi), g);
                zr[Aa + j] = ppo::sd_grad_ls(ar[j], mu, tj, lo, hi, g, cm);
            }
            if (lp_out) lp_out[i] = r.lp;
            if (ent_out) ent_out[i] = r.H;
            sur_sum += (double)sur;
            ent_sum += (double)r.H;
            clamped += (unsigned)r.clamped;
            elems += (unsigned)Aa;
        }
        __syncthreads();
        tile_store<VEC>(tile, pitch, grad + base, nr * A, A, tid);
        __syncthreads();                             // the next tile's loads overwrite what the stores read
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        clamped += __shfl_xor(clamped, o, 64);
        elems += __shfl_xor(elems, o, 64);
    }
    if (tid == 0) {
        atomicAdd(&rec->counts[0], (unsigned long long)clamped);
        atomicAdd(&rec->counts[1], (unsigned long long)elems);
    }
    const double part_s = ppo::block_sum_halving<TPB>(sur_sum, red);
    const double part_h = ppo::block_sum_halving<TPB>(ent_sum, red);
    const double part[2] = {part_s, part_h};
    if (!ppo::ticket_publish(&rec->partial[2 * blockIdx.x], part, &rec->ticket, &red[TPB])) return;

    // the last workgroup: every partial of this launch is visible; fold them in an order fixed by the grid
    const double* slots = rec->partial;
    const double S = ppo::fold_runs_tree<TPB>(red, (int)gridDim.x, 0.0,
                                              [&](int i) { return ppo::ticket_load(&slots[2 * i]); }, ppo::DaddRn());
    __syncthreads();
    const double Hs = ppo::fold_runs_tree<TPB>(red, (int)gridDim.x, 0.0,
                                               [&](int i) { return ppo::ticket_load(&slots[2 * i + 1]); },
                                               ppo::DaddRn());
    if (tid == 0) {
        const double loss = -(S / m) - (double)ent_coeff * (Hs / m);
        rec->loss = loss;
        rec->ent_sum = Hs;
        if (d_loss_accum) *d_loss_accum += (float)loss;
        __hip_atomic_store(&rec->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch's
    }
}

// one row by one thread: the sampled action (DET: the mean) into ar[0 … Aa), +0 after it; returns the log-prob of
// what it wrote through the head's atoms (DET: unused)
template <bool DET>
__device__ __forceinline__ float sd_sample_row(const float* __restrict__ zr, float* __restrict__ ar, int A, float lo,
                                               float hi, uint64_t e, uint64_t key, uint64_t offset) {
    const int Aa = A >> 1;
    float lp = ppo::log_prob_start(Aa);
    for (int j = 0; j < Aa; ++j) {
        if (DET) {
            ar[j] = zr[j];
        } else {
            const float ls = ppo::sd_clamp(zr[Aa + j], lo, hi);
            const float a = zr[j] + normal_at(e * (uint64_t)Aa + j, offset, key) * expf(ls);
            ar[j] = a;
            lp = ppo::sd_lp_step(lp, a, zr[j], ls);
        }
    }
    for (int k = Aa; k < A; ++k) ar[k] = 0.f;
    return lp;
}

// row e of z; the action and the log-prob (may be NULL) go to row rows[e] (NULL: e)
template <bool DET>
__global__ void sd_sample_kernel(const float* __restrict__ z, const int* __restrict__ rows,
                                 float* __restrict__ action, float* __restrict__ logprob, int m, int A, float lo,
                                 float hi, uint64_t key, uint64_t offset) {
    const long e = (long)blockIdx.x * STPB + threadIdx.x;
    if (e >= m) return;
    const long row = rows ? rows[e] : e;
    const float lp = sd_sample_row<DET>(z + e * A, action + row * A, A, lo, hi, (uint64_t)e, key, offset);
    if (!DET && logprob) logprob[row] = lp;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int phip_sd_shape_ok(int A) { return A >= 2 && (A & 1) == 0 && A / 2 <= PHIP_SD_MAX_AA; }

void phip_sd_head(const float* z, const float* action, const float* adv, const float* old_lp, int m, int A,
                  float ls_min, float ls_max, float epsilon, float ent_coeff, float* grad, float* lp_out,
                  float* ent_out, PhipSdRec* rec, float* d_loss_accum) {
    if (m <= 0) return;
    PPO_REQUIRE(phip_sd_shape_ok(A), "phip_sd_head: A must be even with A / 2 <= 32");
    PPO_REQUIRE(z && action && adv && old_lp && grad && rec, "phip_sd_head: operands");
    const int Aa = A / 2;
    const size_t lds = sizeof(float) * (size_t)TPB * ((A | 1) + (Aa | 1));
    const int tiles = ppo_divup(m, TPB);
    const int grid = tiles < PHIP_SD_PARTS ? tiles : PHIP_SD_PARTS;
    ppo::ProfScope ps(PPO_K_HEAD, 4.0 * m * (3.0 * A + 2));
    // a tile starts 64·A floats after the last one, a multiple of 16 bytes: the bases decide
    if (aligned16(z) && aligned16(action) && aligned16(grad))
        hipLaunchKernelGGL(sd_head_kernel<true>, dim3(grid), dim3(TPB), lds, ppo::stream(), z, action, adv, old_lp, m,
                           A, ls_min, ls_max, epsilon, ent_coeff, grad, lp_out, ent_out, rec, d_loss_accum);
    else
        hipLaunchKernelGGL(sd_head_kernel<false>, dim3(grid), dim3(TPB), lds, ppo::stream(), z, action, adv, old_lp, m,
                           A, ls_min, ls_max, epsilon, ent_coeff, grad, lp_out, ent_out, rec, d_loss_accum);
    PPO_LAUNCH_CHECK();
}

void phip_sd_sample(const float* z, const int* rows, float* action, float* logprob, int m, int A, float ls_min,
                    float ls_max, uint64_t key, uint64_t offset) {
    if (m <= 0) return;
    PPO_REQUIRE(phip_sd_shape_ok(A) && z && action, "phip_sd_sample: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * (2.0 * A + 1));
    hipLaunchKernelGGL(sd_sample_kernel<false>, dim3(ppo_divup(m, STPB)), dim3(STPB), 0, ppo::stream(), z, rows, action,
                       logprob, m, A, ls_min, ls_max, key, offset);
    PPO_LAUNCH_CHECK();
}

void phip_sd_sample_rows(const float* z, const int* rows, float* action, float* logprob, int E, int A, float ls_min,
                         float ls_max, uint64_t key, uint64_t step) {
    phip_sd_sample(z, rows, action, logprob, E, A, ls_min, ls_max, key, kNoise + step);
}

void phip_sd_mean(const float* z, float* action, int m, int A) {
    if (m <= 0) return;
    PPO_REQUIRE(phip_sd_shape_ok(A) && z && action, "phip_sd_mean: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * 1.5 * A);
    hipLaunchKernelGGL(sd_sample_kernel<true>, dim3(ppo_divup(m, STPB)), dim3(STPB), 0, ppo::stream(), z, nullptr,
                       action, nullptr, m, A, 0.f, 0.f, (uint64_t)0, (uint64_t)0);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
