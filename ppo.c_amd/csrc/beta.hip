// beta.hip — the Beta policy's head and sampler (ppo_set_action_beta; no counterpart in the reference).  A row of μ's
// A outputs z is Aa = A / 2 raw α-logits followed by Aa raw β-logits, clamped to [−z_max, z_max] where it is read;
// α = 1 + softplus, β likewise; the action row holds x_j ∈ (0, 1) and zeros after them.  The arithmetic is
// ppo_math.h's (the beta_* atoms, in double), called, never restated; the KL monitor's mode of it is kl.hip's.
//
// HEAD.  One launch per policy step.  An element costs three lnΓ, three ψ and three ψ′ in double — two orders of
// magnitude above a Gaussian element — so the work is split by element, not by row: a 256-thread workgroup owns tiles
// of 64 rows and passes over a tile three times.
//   0. z [64, A] goes to LDS at the odd row pitch A | 1 and the first Aa columns of the action rows at the odd pitch
//      Aa | 1, both by coalesced 16-byte loads (tile_io.h; scalar ones where a pointer is not 16-byte aligned);
//   1. a lane per (row, component), strided over the tile's nr·Aa elements: beta_component gives lp_j and H_j, kept in
//      double in LDS, and the four partial derivatives; ∂lp/∂z of both logits goes to a second float tile and
//      (ent_coeff/m)·∂H/∂z overwrites the two logits in the z tile — a clamped logit gets +0 in both;
//   2. a lane per row (the first nr threads): lp and H are the sums of the row's lp_j and H_j, j ascending, in double —
//      one lane, one order, no cross-lane floating-point reduction — then surrogate gives g; lp, H and g leave;
//   3. a lane per logit, strided over the tile's nr·A elements: the z tile ← g·∂lp/∂z − (ent_coeff/m)·∂H/∂z, +0 where
//      both terms are zero (a clamped logit, whatever g is);
//   4. the tile is stored the way it was loaded.
// LDS: 64·(8·(A | 1) + 20·(Aa | 1)) bytes of tiles — 38.75 KiB at Aa = 17, 73.75 KiB at Aa = 32, the widest (checked
// against the CU's 160 KiB below) — plus 2.3 KiB of reduction space.  Traffic: 3·m·A·4 bytes plus 8 per row; the
// special functions, not the bytes, set the time.  The grid is min(⌈m / 64⌉, PHIP_SD_PARTS) workgroups, a function of
// m alone; workgroup b takes tiles b, b + grid, ….  The cross-row sums are deterministic (reduce.h): the row lanes add
// their rows' surrogate and entropy in double in tile order, the workgroup folds its 256 lanes by the halving tree,
// leaves two partials and draws a ticket; the last workgroup to arrive folds the partials by fold_runs_tree and writes
// the loss and the entropy sum into the record (the state-dependent-σ head's PhipSdRec), and adds the loss to the
// update's running loss word (one thread, a plain add).  No floating-point atomic.  The clamped logits and the logits
// m·A are two integer atomics per workgroup.
//
// SAMPLER.  One kernel, one device function (beta_draw); a lane per (row, component), a workgroup owning 256 / Aa
// whole rows.  x = Ga / (Ga + Gb) in fp32, Ga ~ Gamma(α), Gb ~ Gamma(β) by Marsaglia–Tsang (shape >= 1: no boost):
// d = shape − 1/3, c = 1/√(9d); an attempt takes ONE Philox block at counter (e·Aa + j) | (2·attempt + sel) << 56
// (sel 0 for α, 1 for β): n = Box–Muller of .x .y, v = (1 + c·n)³, accepted when v > 0 and
// ln u01(.z) < n²/2 + d − d·v + d·ln v; the variate is d·v.  Attempts are capped at 16: acceptance is >= 0.95 per
// attempt for shape >= 1, so the cap is reached with probability <= 0.05¹⁶ ≈ 1.5e−21, and then the variate is d
// (v = 1, the mode's neighbourhood).  x is clamped to [2⁻²⁴, 1 − 2⁻²⁴].  The draw is a pure function of (key, offset,
// row, component).  The lanes leave lp_j = beta_lp in LDS and the row's first lane adds them j ascending — the head's
// terms in the head's order, so the stored log-prob is the head's lp bit for bit on the same (z, x).  The dense form
// and the rollout's (rows[e] of the buffer, offset = kNoise + step) are one kernel; the deterministic action is the
// mean α / (α + β).  rng.h lists the stream.
#include "dev.h"
#include "ppo_math.h"
#include "reduce.h"
#include "rng.h"
#include "tile_io.h"

#include <cmath>

namespace {

using namespace ppo_rng;

constexpr int HT = 256;                              // the head's workgroup
constexpr int ROWS = 64;                             // rows of a tile
constexpr int ST = 256;                              // the sampler's workgroup
constexpr int MAX_ATTEMPTS = 16;

constexpr size_t head_lds_bytes(int Aa) {
    return (size_t)ROWS * (8 * (size_t)((2 * Aa) | 1) + 20 * (size_t)(Aa | 1));
}
static_assert(head_lds_bytes(PHIP_SD_MAX_AA) + sizeof(double) * (HT + 1) + 64 <= 160 * 1024,
              "beta head: the widest tile exceeds a CU's 160 KiB of LDS");

template <bool VEC>
__global__ __launch_bounds__(HT) void beta_head_kernel(const float* __restrict__ z, const float* __restrict__ action,
                                                       const float* __restrict__ adv, const float* __restrict__ old_lp,
                                                       int m, int A, float zmax, float eps, float ent_coeff,
                                                       float* __restrict__ grad, float* __restrict__ lp_out,
                                                       float* __restrict__ ent_out, PhipSdRec* rec,
                                                       float* d_loss_accum) {
    extern __shared__ double lds[];
    __shared__ double red[HT + 1];                   // red[HT]: "this workgroup drew the last ticket"
    __shared__ float grow[ROWS];                     // the rows' g = ∂loss/∂lp
    __shared__ unsigned wg_clamped;
    const int Aa = A >> 1, pitch = A | 1, apitch = Aa | 1;
    double* lpj = lds;                               // [64][apitch]: lp_j
    double* Hj = lpj + ROWS * apitch;                // [64][apitch]: H_j
    float* tile = reinterpret_cast<float*>(Hj + ROWS * apitch);   // [64][pitch]: z, then cm·∂H/∂z, then the gradient
    float* dl = tile + ROWS * pitch;                 // [64][pitch]: ∂lp/∂z
    float* at = dl + ROWS * pitch;                   // [64][apitch]: x
    const int tid = threadIdx.x;
    const int ntiles = (m + ROWS - 1) / ROWS;
    const double cm = (double)ent_coeff / m;
    double sur_sum = 0.0, ent_sum = 0.0;
    unsigned clamped = 0;
    unsigned long long elems = 0;
    if (tid == 0) wg_clamped = 0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long r0 = (long)t * ROWS;
        const int nr = (int)min((long)ROWS, (long)m - r0);
        const long base = r0 * A;
        ppo::tile_load<HT, VEC>(tile, pitch, z + base, nr * A, A, A, tid);
        ppo::tile_load<HT, VEC>(at, apitch, action + base, nr * A, A, Aa, tid);
        __syncthreads();
        for (int el = tid; el < nr * Aa; el += HT) {             // 1. a lane per (row, component)
            const int r = el / Aa, j = el - r * Aa;
            float* zr = tile + r * pitch;
            const float za = zr[j], zb = zr[Aa + j];
            const float ca = ppo::beta_clamp(za, zmax), cb = ppo::beta_clamp(zb, zmax);
            const ppo::BetaComp c = ppo::beta_component(ppo::beta_shape(ca), ppo::beta_shape(cb), at[r * apitch + j]);
            const bool ina = ppo::beta_inside(za, zmax), inb = ppo::beta_inside(zb, zmax);
            const double sa = ppo::beta_dshape(za, zmax), sb = ppo::beta_dshape(zb, zmax);
            lpj[r * apitch + j] = c.lp;
            Hj[r * apitch + j] = c.H;
            // a clamped logit: +0 in both terms, whatever the rest of the row holds
            dl[r * pitch + j] = ina ? (float)(c.dlp_a * sa) : 0.f;
            dl[r * pitch + Aa + j] = inb ? (float)(c.dlp_b * sb) : 0.f;
            zr[j] = ina ? (float)(cm * (c.dH_a * sa)) : 0.f;
            zr[Aa + j] = inb ? (float)(cm * (c.dH_b * sb)) : 0.f;
            clamped += (unsigned)!ina + (unsigned)!inb;
        }
        __syncthreads();
        if (tid < nr) {                                          // 2. a lane per row
            double lp = 0.0, H = 0.0;
            for (int j = 0; j < Aa; ++j) {
                lp += lpj[tid * apitch + j];
                H += Hj[tid * apitch + j];
            }
            const long i = r0 + tid;
            const float lpf = (float)lp;
            float g;
            const float sur = ppo::surrogate(adv[i], lpf, old_lp[i], eps, m, &g);
            grow[tid] = g;
            if (lp_out) lp_out[i] = lpf;
            if (ent_out) ent_out[i] = (float)H;
            sur_sum += (double)sur;
            ent_sum += H;
        }
        if (tid == 0) elems += (unsigned long long)nr * A;
        __syncthreads();
        for (int el = tid; el < nr * A; el += HT) {              // 3. a lane per logit
            const int r = el / A, k = el - r * A;
            const float d = dl[r * pitch + k], h = tile[r * pitch + k];
            // a clamped logit left +0 in both terms: its gradient is +0 whatever g is, a NaN row's included
            tile[r * pitch + k] = (d == 0.f && h == 0.f) ? 0.f : (float)((double)grow[r] * (double)d - (double)h);
        }
        __syncthreads();
        ppo::tile_store<HT, VEC>(tile, pitch, grad + base, nr * A, A, tid);
        __syncthreads();                             // the next tile's loads overwrite what the stores read
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) clamped += __shfl_xor(clamped, o, 64);
    __syncthreads();                                 // wg_clamped's zero is visible (a workgroup with no tile: grid <= tiles)
    if ((tid & 63) == 0) atomicAdd(&wg_clamped, clamped);        // LDS, integer
    __syncthreads();
    if (tid == 0) {
        atomicAdd(&rec->counts[0], (unsigned long long)wg_clamped);
        atomicAdd(&rec->counts[1], elems);
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

// Gamma(shape, 1), shape >= 1, by Marsaglia–Tsang; attempt a reads the Philox block at counter idx | (2a + sel) << 56
__device__ __forceinline__ float gamma_draw(float shape, uint64_t idx, int sel, uint64_t offset, uint64_t key) {
    const float d = shape - 1.f / 3.f, c = 1.f / sqrtf(9.f * d);
    for (int a = 0; a < MAX_ATTEMPTS; ++a) {
        const u32x4 r = philox(idx | ((uint64_t)(2 * a + sel) << 56), offset, key);
        const float n = sqrtf(-2.f * logf(u01(r.x))) * cosf(2.f * (float)M_PI * u01(r.y));
        const float t = 1.f + c * n, v = t * t * t;
        if (v > 0.f && logf(u01(r.z)) < 0.5f * n * n + d - d * v + d * logf(v)) return d * v;
    }
    return d;                                        // the cap: probability <= 0.05¹⁶
}

// component j of row e under the clamped logits za, zb: the drawn x (DET: the mean), clamped to [2⁻²⁴, 1 − 2⁻²⁴]
template <bool DET>
__device__ __forceinline__ float beta_draw(double a, double b, uint64_t idx, uint64_t key, uint64_t offset) {
    if (DET) return (float)(a / (a + b));
    const float ga = gamma_draw((float)a, idx, 0, offset, key), gb = gamma_draw((float)b, idx, 1, offset, key);
    const float x = ga / (ga + gb);
    const float lo = 1.f / 16777216.f, hi = 1.f - lo;
    return x < lo ? lo : (x > hi ? hi : x);          // a NaN (a NaN logit) passes through
}

// row e of z; the action and the log-prob (may be NULL) go to row rows[e] (NULL: e).  rpw = ST / Aa rows a workgroup
template <bool DET>
__global__ __launch_bounds__(ST) void beta_sample_kernel(const float* __restrict__ z, const int* __restrict__ rows,
                                                         float* __restrict__ action, float* __restrict__ logprob,
                                                         int m, int A, float zmax, uint64_t key, uint64_t offset) {
    __shared__ double lpj[ST];
    const int Aa = A >> 1, rpw = ST / Aa;
    const int lr = threadIdx.x / Aa, j = threadIdx.x - lr * Aa;
    const long e = (long)blockIdx.x * rpw + lr;
    const bool live = lr < rpw && e < m;
    long row = 0;
    if (live) {
        row = rows ? rows[e] : e;
        const float* zr = z + e * A;
        const double a = ppo::beta_shape(ppo::beta_clamp(zr[j], zmax));
        const double b = ppo::beta_shape(ppo::beta_clamp(zr[Aa + j], zmax));
        const float x = beta_draw<DET>(a, b, (uint64_t)e * (uint64_t)Aa + (uint64_t)j, key, offset);
        action[row * A + j] = x;
        action[row * A + Aa + j] = 0.f;
        if (!DET) lpj[threadIdx.x] = ppo::beta_lp(a, b, x);
    }
    if (DET || !logprob) return;
    __syncthreads();
    if (live && j == 0) {
        double lp = 0.0;
        for (int k = 0; k < Aa; ++k) lp += lpj[threadIdx.x + k];
        logprob[row] = (float)lp;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool VEC>
void launch_head(int grid, size_t lds, const float* z, const float* action, const float* adv, const float* old_lp,
                 int m, int A, float zmax, float eps, float ent_coeff, float* grad, float* lp_out, float* ent_out,
                 PhipSdRec* rec, float* d_loss_accum) {
    auto kern = beta_head_kernel<VEC>;
    // past the 64 KiB a launch gets unasked (Aa >= 28): asked for at every such launch, so it holds on whichever
    // device the call runs and from any thread
    if (lds > 64 * 1024)
        PPO_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(HT), lds, ppo::stream(), z, action, adv, old_lp, m, A, zmax, eps,
                       ent_coeff, grad, lp_out, ent_out, rec, d_loss_accum);
}

}  // namespace

extern "C" {

void phip_beta_head(const float* z, const float* action, const float* adv, const float* old_lp, int m, int A,
                    float z_max, float epsilon, float ent_coeff, float* grad, float* lp_out, float* ent_out,
                    PhipSdRec* rec, float* d_loss_accum) {
    if (m <= 0) return;
    PPO_REQUIRE(phip_sd_shape_ok(A), "phip_beta_head: A must be even with A / 2 <= 32");
    PPO_REQUIRE(z && action && adv && old_lp && grad && rec && z_max > 0.f, "phip_beta_head: operands");
    const size_t lds = head_lds_bytes(A / 2);
    PPO_REQUIRE(lds <= 160 * 1024, "phip_beta_head: LDS");
    const int tiles = ppo_divup(m, ROWS);
    const int grid = tiles < PHIP_SD_PARTS ? tiles : PHIP_SD_PARTS;
    ppo::ProfScope ps(PPO_K_HEAD, 4.0 * m * (3.0 * A + 2));
    // a tile starts 64·A floats after the last one, a multiple of 16 bytes: the bases decide
    if (aligned16(z) && aligned16(action) && aligned16(grad))
        launch_head<true>(grid, lds, z, action, adv, old_lp, m, A, z_max, epsilon, ent_coeff, grad, lp_out, ent_out, rec,
                          d_loss_accum);
    else
        launch_head<false>(grid, lds, z, action, adv, old_lp, m, A, z_max, epsilon, ent_coeff, grad, lp_out, ent_out,
                           rec, d_loss_accum);
    PPO_LAUNCH_CHECK();
}

void phip_beta_sample(const float* z, const int* rows, float* action, float* logprob, int m, int A, float z_max,
                      uint64_t key, uint64_t offset) {
    if (m <= 0) return;
    PPO_REQUIRE(phip_sd_shape_ok(A) && z && action && z_max > 0.f, "phip_beta_sample: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * (2.0 * A + 1));
    hipLaunchKernelGGL(beta_sample_kernel<false>, dim3(ppo_divup(m, ST / (A / 2))), dim3(ST), 0, ppo::stream(), z, rows,
                       action, logprob, m, A, z_max, key, offset);
    PPO_LAUNCH_CHECK();
}

void phip_beta_sample_rows(const float* z, const int* rows, float* action, float* logprob, int E, int A, float z_max,
                           uint64_t key, uint64_t step) {
    phip_beta_sample(z, rows, action, logprob, E, A, z_max, key, kNoise + step);
}

void phip_beta_mean(const float* z, float* action, int m, int A, float z_max) {
    if (m <= 0) return;
    PPO_REQUIRE(phip_sd_shape_ok(A) && z && action && z_max > 0.f, "phip_beta_mean: operands");
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * m * 2.0 * A);
    hipLaunchKernelGGL(beta_sample_kernel<true>, dim3(ppo_divup(m, ST / (A / 2))), dim3(ST), 0, ppo::stream(), z, nullptr,
                       action, nullptr, m, A, z_max, (uint64_t)0, (uint64_t)0);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
