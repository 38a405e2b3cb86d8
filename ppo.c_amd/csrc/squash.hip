// squash.hip — the squashed (tanh) Gaussian policy's head and sampler (ppo_set_action_squashed_gaussian; no
// counterpart in the reference).  A row of μ's A outputs z is Aa = A / 2 means followed by Aa raw log σ, clamped to
// [ls_min, ls_max] where it is read, as under the state-dependent-σ Gaussian; a stored action row holds
// a_j = tanhf(u_j) in columns 0 … Aa−1 and the pre-squash sample u_j in columns Aa … A−1.  The per-row arithmetic is
// ppo_math.h's (the sq_* atoms over the sd_* ones), called, never restated; the KL monitor's mode of it is kl.hip's.
//
// HEAD.  One launch per policy step.  The entropy has no closed form: it is estimated per row from one fresh
// reparameterised sample u′ = μ + σ·ε, so an element costs a Philox block, a Box–Muller, a tanhf and two softplus on
// top of the Gaussian terms, and the work is split by element, not by row: a 256-thread workgroup owns tiles of 32
// rows and passes over a tile three times.
//   0. z [32, A] and the action rows [32, A] go to LDS at the odd row pitch A | 1 by coalesced 16-byte loads
//      (tile_io.h; scalar ones where a pointer is not 16-byte aligned).  Only the u half of an action row is read; its
//      a half shares the same 128-byte lines, so loading whole rows costs no extra traffic;
//   1. a lane per (row, component), strided over the tile's nr·Aa elements: ε = normal_at(i·Aa + j, offset, key),
//      q = expf(ls)·ε, u′ = μ + q; ldj(u), ldj(u′), tanhf(u′) and q go to four float tiles at the odd pitch Aa | 1;
//   2. a lane per row (the first nr threads): sd_row over (z, u) gives the base Gaussian's lp, Σ ls and the clamped
//      count; J and Σ ldj(u′) are the sums of the row's elements, j ascending, by this one lane — a row's outputs do
//      not depend on the tile shape; surrogate gives g; lp, H and g leave;
//   3. a lane per (row, component) again: the z tile ← the gradient (sq_grad_mu, sq_grad_ls; a clamped column +0);
//   4. the tile is stored the way it was loaded.
// LDS: 32·(2·(A | 1) + 4·(Aa | 1)) floats — 17.5 KiB at Aa = 17, 32.75 KiB at Aa = 32 — plus 2.2 KiB of reduction
// space.  Traffic: 3·m·A·4 bytes plus 8 per row, the state-dependent-σ head's.  The grid is min(⌈m / 32⌉,
// PHIP_SD_PARTS) workgroups, a function of m alone; workgroup b takes tiles b, b + grid, ….  The cross-row sums are
// deterministic (reduce.h): the row lanes add their rows' surrogate and entropy in double in tile order, the workgroup
// folds its 256 lanes by the halving tree, leaves two partials and draws a ticket; the last workgroup to arrive folds
// the partials by fold_runs_tree and writes the loss and the entropy sum into the record (the state-dependent-σ
// head's PhipSdRec), and adds the loss to the update's running loss word (one thread, a plain add).  No
// floating-point atomic.  The clamped log-σ elements and the elements m·Aa are two integer atomics per workgroup.
//
// SAMPLER.  One kernel; a lane per (row, component), a workgroup owning 256 / Aa whole rows:
// u_j = μ_j + normal_at(e·Aa + j, offset, key)·expf(ls_j), a_j = tanhf(u_j), both stored.  The lanes leave u_j and
// ldj(u_j) in LDS and the row's first lane takes sd_row and the sum J as the head's row lane does, so the stored
// log-prob is the head's lp bit for bit on the same (z, action) and stays finite where tanhf rounds to ±1.  The dense
// form and the rollout's (rows[e] of the buffer, offset = kNoise + step) are one kernel; the deterministic action has
// u = μ.  rng.h lists the streams.
#include "dev.h"
#include "ppo_math.h"
#include "reduce.h"
#include "rng.h"
#include "tile_io.h"

#include <cmath>

namespace {

using namespace ppo_rng;

constexpr int HT = 256;                              // the head's workgroup
constexpr int ROWS = 32;                             // rows of a tile
constexpr int ST = 256;                              // the sampler's workgroup

constexpr size_t head_lds_bytes(int Aa) {
    return sizeof(float) * (size_t)ROWS * (2 * (size_t)((2 * Aa) | 1) + 4 * (size_t)(Aa | 1));
}
static_assert(head_lds_bytes(PHIP_SD_MAX_AA) + sizeof(double) * (HT + 1) + 256 <= 64 * 1024,
              "squash head: the widest tile exceeds the 64 KiB of LDS a launch gets unasked");

template <bool VEC>
__global__ __launch_bounds__(HT) void sq_head_kernel(const float* __restrict__ z, const float* __restrict__ action,
                                                     const float* __restrict__ adv, const float* __restrict__ old_lp,
                                                     int m, int A, float lo, float hi, float eps, float ent_coeff,
                                                     uint64_t key, uint64_t offset, float* __restrict__ grad,
                                                     float* __restrict__ lp_out, float* __restrict__ ent_out,
                                                     PhipSdRec* rec, float* d_loss_accum) {
    extern __shared__ float lds[];
    __shared__ double red[HT + 1];                   // red[HT]: "this workgroup drew the last ticket"
    __shared__ float grow[ROWS];                     // the rows' g = ∂loss/∂lp
    const int Aa = A >> 1, pitch = A | 1, apitch = Aa | 1;
    float* tile = lds;                               // [32][pitch]: z, then the gradient
    float* at = tile + ROWS * pitch;                 // [32][pitch]: the action rows; u is columns Aa … A−1
    float* lju = at + ROWS * pitch;                  // [32][apitch]: ldj(u)
    float* ljp = lju + ROWS * apitch;                // [32][apitch]: ldj(u′)
    float* tht = ljp + ROWS * apitch;                // [32][apitch]: tanhf(u′)
    float* qt = tht + ROWS * apitch;                 // [32][apitch]: q = expf(ls)·ε
    const int tid = threadIdx.x;
    const int ntiles = (m + ROWS - 1) / ROWS;
    const float cm = ent_coeff / m;
    double sur_sum = 0.0, ent_sum = 0.0;
    unsigned clamped = 0, elems = 0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long r0 = (long)t * ROWS;
        const int nr = (int)min((long)ROWS, (long)m - r0);
        const long base = r0 * A;
        ppo::tile_load<HT, VEC>(tile, pitch, z + base, nr * A, A, A, tid);
        ppo::tile_load<HT, VEC>(at, pitch, action + base, nr * A, A, A, tid);
        __syncthreads();
        for (int el = tid; el < nr * Aa; el += HT) {             // 1. a lane per (row, component)
            const int r = el / Aa, j = el - r * Aa;
            const float ls = ppo::sd_clamp(tile[r * pitch + Aa + j], lo, hi);
            const float e = normal_at((uint64_t)(r0 + r) * (uint64_t)Aa + (uint64_t)j, offset, key);
            const float q = ppo::sq_fresh(ls, e), up = tile[r * pitch + j] + q;
            lju[r * apitch + j] = ppo::sq_ldj(at[r * pitch + Aa + j]);
            ljp[r * apitch + j] = ppo::sq_ldj(up);
            tht[r * apitch + j] = tanhf(up);
            qt[r * apitch + j] = q;
        }
        __syncthreads();
        if (tid < nr) {                                          // 2. a lane per row
            const ppo::SdRow s = ppo::sd_row(tile + tid * pitch, at + tid * pitch + Aa, Aa, lo, hi);
            float J = 0.f, Jp = 0.f;
            for (int j = 0; j < Aa; ++j) {
                J += lju[tid * apitch + j];
                Jp += ljp[tid * apitch + j];
            }
            const float lp = ppo::sq_lp(s.lp, J), H = ppo::sq_entropy(s.H, Jp);
            const long i = r0 + tid;
            float g;
            const float sur = ppo::surrogate(adv[i], lp, old_lp[i], eps, m, &g);
            grow[tid] = g;
            if (lp_out) lp_out[i] = lp;
            if (ent_out) ent_out[i] = H;
            sur_sum += (double)sur;
            ent_sum += (double)H;
            clamped += (unsigned)s.clamped;
            elems += (unsigned)Aa;
        }
        __syncthreads();
        for (int el = tid; el < nr * Aa; el += HT) {             // 3. a lane per (row, component): the gradient
            const int r = el / Aa, j = el - r * Aa;
            float* zr = tile + r * pitch;
            const float mu = zr[j], tj = zr[Aa + j], u = at[r * pitch + Aa + j], g = grow[r];
            const float th = tht[r * apitch + j];
            zr[j] = ppo::sq_grad_mu(u, mu, ppo::sd_clamp(tj, lo, hi), g, cm, th);
            zr[Aa + j] = ppo::sq_grad_ls(u, mu, tj, lo, hi, g, cm, th, qt[r * apitch + j]);
        }
        __syncthreads();
        ppo::tile_store<HT, VEC>(tile, pitch, grad + base, nr * A, A, tid);
        __syncthreads();                             // the next tile's loads overwrite what the stores read
    }
    if (tid < 64) {                                  // the row lanes are the first 32 threads: one wave holds them all
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            clamped += __shfl_xor(clamped, o, 64);
            elems += __shfl_xor(elems, o, 64);
        }
        if (tid == 0) {
            atomicAdd(&rec->counts[0], (unsigned long long)clamped);
            atomicAdd(&rec->counts[1], (unsigned long long)elems);
        }
    }
    const double part_s = ppo::block_sum_halving<HT>(sur_sum, red);
    const double part_h = ppo::block_sum_halving<HT>(ent_sum, red);
    const double part[2] = {part_s, part_h};
    if (!ppo::ticket_publish(&rec->partial[2 * blockIdx.x], part, &rec->ticket, &red[HT])) return;

    // the last workgroup: every partial of this launch is visible; fold them in an order fixed by the grid
    const double* slots = rec->partial;
    const double S = ppo::fold_runs_tree<HT>(red, (int)gridDim.x, 0.0,
                                             [&](int i) { return ppo::ticket_load(&slots[2 * i]); }, ppo::DaddRn());
    __syncthreads();
    const double Hs = ppo::fold_runs_tree<HT>(red, (int)gridDim.x, 0.0,
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

// row e of z; the action row [a | u] and the log-prob (may be NULL) go to row rows[e] (NULL: e).  rpw = ST / Aa rows
// a workgroup; DET: u = μ, no log-prob
template <bool DET>
__global__ __launch_bounds__(ST) void sq_sample_kernel(const float* __restrict__ z, const int* __restrict__ rows,
                                                       float* __restrict__ action, float* __restrict__ logprob, int m,
                                                       int A, float lo, float hi, uint64_t key, uint64_t offset) {
    __shared__ float us[ST], lj[ST];
    const int Aa = A >> 1, rpw = ST / Aa;
    const int lr = threadIdx.x / Aa, j = threadIdx.x - lr * Aa;
    const long e = (long)blockIdx.x * rpw + lr;
    const bool live = lr < rpw && e < m;
    long row = 0;
    if (live) {
        row = rows ? rows[e] : e;
        const float* zr = z + e * A;
        float u = zr[j];
        if (!DET)
            u = zr[j] + normal_at((uint64_t)e * (uint64_t)Aa + (uint64_t)j, offset, key) *
                            expf(ppo::sd_clamp(zr[Aa + j], lo, hi));
        action[row * A + j] = tanhf(u);
        action[row * A + Aa + j] = u;
        if (!DET) {
            us[threadIdx.x] = u;
            lj[threadIdx.x] = ppo::sq_ldj(u);
        }
    }
    if (DET || !logprob) return;
    __syncthreads();
    if (live && j == 0) {
        float J = 0.f;
        for (int k = 0; k < Aa; ++k) J += lj[threadIdx.x + k];
        logprob[row] = ppo::sq_lp(ppo::sd_row(z + e * A, us + threadIdx.x, Aa, lo, hi).lp, J);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

void phip_sq_head(const float* z, const float* action, const float* adv, const float* old_lp, int m, int A,
                  float ls_min, float ls_max, float epsilon, float ent_coeff, uint64_t key, uint64_t offset,
                  float* grad, float* lp_out, float* ent_out, PhipSdRec* rec, float* d_loss_accum) {
    if (m <= 0) return;
    PPO_REQUIRE(phip_sd_shape_ok(A), "phip_sq_head: A must be even with A / 2 <= 32");
    PPO_REQUIRE(z && action && adv && old_lp && grad && rec, "phip_sq_head: operands");
    const size_t lds = head_lds_bytes(A / 2);
    const int tiles = ppo_divup(m, ROWS);
    const int grid = tiles < PHIP_SD_PARTS ? tiles : PHIP_SD_PARTS;
    ppo::ProfScope ps(PPO_K_HEAD, 4.0 * m * (3.0 * A + 2));
    // a tile starts 32·A floats after the last one, a multiple of 16 bytes: the bases decide
    if (aligned16(z) && aligned16(action) && aligned16(grad))
        hipLaunchKernelGGL(sq_head_kernel<true>, dim3(grid), dim3(HT), lds, ppo::stream(), z, action, adv, old_lp, m, A,
                           ls_min, ls_max, epsilon, ent_coeff, key, offset, grad, lp_out, ent_out, rec, d_loss_accum);
    else
        hipLaunchKernelGGL(sq_head_kernel<false>, dim3(grid), dim3(HT), lds, ppo::stream(), z, action, adv, old_lp, m,
                           A, ls_min, ls_max, epsilon, ent_coeff, key, offset, grad, lp_out, ent_out, rec,
                           d_loss_accum);
    PPO_LAUNCH_CHECK();
}

void phip_sq_sample(const float* z, const int* rows, float* action, float* logprob, int m, int A, float ls_min,
                    float ls_max, uint64_t key, uint64_t offset) {
    if (m <= 0) return;
    PPO_REQUIRE(phip_sd_shape_ok(A) && z && action, "phip_sq_sample: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * (2.0 * A + 1));
    hipLaunchKernelGGL(sq_sample_kernel<false>, dim3(ppo_divup(m, ST / (A / 2))), dim3(ST), 0, ppo::stream(), z, rows,
                       action, logprob, m, A, ls_min, ls_max, key, offset);
    PPO_LAUNCH_CHECK();
}

void phip_sq_sample_rows(const float* z, const int* rows, float* action, float* logprob, int E, int A, float ls_min,
                         float ls_max, uint64_t key, uint64_t step) {
    phip_sq_sample(z, rows, action, logprob, E, A, ls_min, ls_max, key, kNoise + step);
}

void phip_sq_mean(const float* z, float* action, int m, int A) {
    if (m <= 0) return;
    PPO_REQUIRE(phip_sd_shape_ok(A) && z && action, "phip_sq_mean: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * 2.0 * A);
    hipLaunchKernelGGL(sq_sample_kernel<true>, dim3(ppo_divup(m, ST / (A / 2))), dim3(ST), 0, ppo::stream(), z, nullptr,
                       action, nullptr, m, A, 0.f, 0.f, (uint64_t)0, (uint64_t)0);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
