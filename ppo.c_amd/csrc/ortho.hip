// ortho.hip — orthogonal weight initialisation (ppo_ext.h ppo_init_orthogonal; DESIGN.md §4 "Orthogonal
// initialisation"): torch.nn.init.orthogonal_ restated in double, one launch for every layer of both networks.
//
// For W [rows][cols] and a Gaussian G of the same shape: M = G (rows >= cols) or Gᵀ, T × S with T >= S; M = Q·R by
// Householder reflections; Q ← Q·diag(sign R_jj) (+1 for a zero); W = (float)(gain · Q), transposed back.  Everything
// between the fp32 G and the one fp32 rounding at the store is double.
//
// Split: the grid is the number of matrices, one 1024-thread workgroup (16 waves) each.  A matrix is a chain of S
// dependent reflections and no reflection here has work for more than one CU.
//
// Data movement: two column-major T × S double workspaces per matrix in global memory (L2-resident at the sizes the
// networks have) — `fac`, the factor (R above the diagonal, the reflectors v_j below it, the diagonal left as the
// column's own head), and `q`.  The current reflector (<= T doubles), every τ_j and every sign live in LDS.
//   factor, step j:  every thread reads the column's head α and Σ_{i>=j} a_i² (one LDS double) and forms β = −sign(α)‖a‖,
//                    τ = (β − α)/β;  the threads write v = a/(α − β) (v_j = 1) to LDS and, below the diagonal, back to
//                    fac;  barrier;  wave w takes the trailing columns j+1+w, j+17+w, …: lanes stride the rows
//                    (coalesced), vᵀa by a fixed-order wave sum, a −= τ(vᵀa)v — a column of <= 512 live rows stays in
//                    registers between the two passes.  The wave that owns column j+1 also sums its new squares below
//                    row j: the next step's norm costs no pass and no barrier;  barrier.  Two barriers a reflection.
//   q:               H_0 … H_{S−1} applied to the first S columns of the identity, j descending (H_j moves columns
//                    >= j only), with the same column routine.
//   store:           W's own layout, lanes along cols: sign, gain, the transpose back and the cast.
// A column whose squares sum to zero gets no reflection (τ = 0, v = e_j): no NaN.  No floating-point atomics and no
// order that depends on timing: W is a function of (G, shape, gain) alone, so every rank of a data-parallel run
// draws identical bits from one seed.
#include "dev.h"
#include "reduce.h"
#include "rng.h"

#include <cmath>

namespace {

using namespace ppo;

constexpr int TPB = 1024, WAVES = TPB / 64;
constexpr int MAX_S = 1024, MAX_T = 4096;   // phip_ortho_shape_ok
constexpr int REG_ROWS = 8;                 // a column of <= 64·REG_ROWS live rows is held in registers

struct Smem {
    double v[MAX_T];        // the current reflector, indexed by row
    double tau[MAX_S];
    float sign[MAX_S];      // sign(R_jj), +1 for a zero
    double next_sq;         // Σ of the squares of the next column at and below its diagonal
};
static_assert(sizeof(Smem) <= 64 * 1024, "static LDS");

// Σ_{i >= from} col[i]² over one wave: lane l adds rows from + l, from + l + 64, … ascending, then the butterfly
__device__ __forceinline__ double wave_sumsq(const double* col, int from, int T) {
    double s = 0.0;
    for (int i = from + (threadIdx.x & 63); i < T; i += 64) s += col[i] * col[i];
    return wave_sum_xor_f64(s);
}

// col ← (I − τ v vᵀ) col over rows j … T−1 by one wave (v in LDS, v[j] = 1).  NEXT: returns the sum of the new
// squares of rows > j.  Both forms add in the same order: a lane's rows ascending, then the butterfly.
template <bool NEXT>
__device__ __forceinline__ double reflect_col(double* col, const double* v, int j, int T, double tau) {
    const int lane = threadIdx.x & 63;
    double sq = 0.0;
    if (T - j <= 64 * REG_ROWS) {
        double a[REG_ROWS], dot = 0.0;
#pragma unroll
        for (int k = 0; k < REG_ROWS; ++k) {
            const int i = j + lane + 64 * k;
            a[k] = i < T ? col[i] : 0.0;
            if (i < T) dot += v[i] * a[k];
        }
        const double f = tau * wave_sum_xor_f64(dot);
#pragma unroll
        for (int k = 0; k < REG_ROWS; ++k) {
            const int i = j + lane + 64 * k;
            if (i < T) {
                const double n = a[k] - f * v[i];
                col[i] = n;
                if (NEXT && i > j) sq += n * n;
            }
        }
    } else {
        double dot = 0.0;
        for (int i = j + lane; i < T; i += 64) dot += v[i] * col[i];
        const double f = tau * wave_sum_xor_f64(dot);
        for (int i = j + lane; i < T; i += 64) {
            const double n = col[i] - f * v[i];
            col[i] = n;
            if (NEXT && i > j) sq += n * n;
        }
    }
    return NEXT ? wave_sum_xor_f64(sq) : 0.0;
}

__global__ __launch_bounds__(TPB) void ortho_kernel(const PhipOrthoJob* __restrict__ jobs) {
    __shared__ Smem sm;
    const PhipOrthoJob job = jobs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int rows = job.rows, cols = job.cols;
    const bool tall = rows >= cols;
    const int T = tall ? rows : cols, S = tall ? cols : rows;
    double* fac = job.work;
    double* q = job.work + (size_t)T * S;

    // G into the factor workspace (element e = r·cols + c of W's layout is M[r][c] or M[c][r]); q ← I; the biases
    for (int e = tid; e < rows * cols; e += TPB) {
        const int r = e / cols, c = e - r * cols;
        const float g = job.fill ? ppo_rng::normal_at((uint64_t)e, job.offset, job.key) : job.W[e];
        fac[tall ? (size_t)c * T + r : (size_t)r * T + c] = (double)g;
    }
    for (int e = tid; e < T * S; e += TPB) q[e] = (e % T == e / T) ? 1.0 : 0.0;
    for (int e = tid; e < job.n_bias; e += TPB) job.bias[e] = 0.f;
    __syncthreads();
    if (w == 0) {
        const double s = wave_sumsq(fac, 0, T);
        if (lane == 0) sm.next_sq = s;
    }
    __syncthreads();

    for (int j = 0; j < S; ++j) {
        double* colj = fac + (size_t)j * T;
        const double alpha = colj[j], n2 = sm.next_sq;
        double beta = 0.0, tau = 0.0, denom = 1.0;           // a zero column: H = I, v = e_j (its rows are zeros)
        if (n2 > 0.0) {
            beta = -copysign(__dsqrt_rn(n2), alpha);
            tau = (beta - alpha) / beta;
            denom = alpha - beta;
        }
        for (int i = j + 1 + tid; i < T; i += TPB) {
            const double vi = colj[i] / denom;
            sm.v[i] = vi;
            colj[i] = vi;
        }
        if (tid == 0) {
            sm.v[j] = 1.0;
            sm.tau[j] = tau;
            sm.sign[j] = beta < 0.0 ? -1.f : 1.f;
        }
        __syncthreads();
        for (int c = j + 1 + w; c < S; c += WAVES) {
            double* col = fac + (size_t)c * T;
            if (c == j + 1) {
                const double s = reflect_col<true>(col, sm.v, j, T, tau);
                if (lane == 0) sm.next_sq = s;
            } else {
                reflect_col<false>(col, sm.v, j, T, tau);
            }
        }
        __syncthreads();
    }

    for (int j = S - 1; j >= 0; --j) {
        const double tau = sm.tau[j];
        if (tau == 0.0) continue;                             // uniform over the workgroup
        const double* colj = fac + (size_t)j * T;
        for (int i = j + 1 + tid; i < T; i += TPB) sm.v[i] = colj[i];
        if (tid == 0) sm.v[j] = 1.0;
        __syncthreads();
        for (int c = j + w; c < S; c += WAVES) reflect_col<false>(q + (size_t)c * T, sm.v, j, T, tau);
        __syncthreads();
    }

    const double gain = (double)job.gain;
    for (int e = tid; e < rows * cols; e += TPB) {
        const int r = e / cols, c = e - r * cols;
        const double x = tall ? (double)sm.sign[c] * q[(size_t)c * T + r] : (double)sm.sign[r] * q[(size_t)r * T + c];
        job.W[e] = (float)(gain * x);
    }
}

}  // namespace

extern "C" {

int phip_ortho_shape_ok(int rows, int cols) {
    return rows >= 1 && cols >= 1 && (rows < cols ? rows : cols) <= MAX_S && (rows > cols ? rows : cols) <= MAX_T;
}

void phip_ortho(PhipOrthoJob* jobs, int n) {
    if (n <= 0) return;
    size_t doubles = 0;
    for (int i = 0; i < n; ++i) {
        PPO_REQUIRE(phip_ortho_shape_ok(jobs[i].rows, jobs[i].cols), "phip_ortho: shape outside the limits");
        doubles += 2 * (size_t)jobs[i].rows * jobs[i].cols;
    }
    ppo::ensure_device();
    double* work = nullptr;
    PhipOrthoJob* d_jobs = nullptr;
    PPO_CHECK(hipMalloc(&work, sizeof(double) * doubles));
    PPO_CHECK(hipMalloc(&d_jobs, sizeof(PhipOrthoJob) * (size_t)n));
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        jobs[i].work = work + at;
        at += 2 * (size_t)jobs[i].rows * jobs[i].cols;
    }
    phip_h2d(d_jobs, jobs, sizeof(PhipOrthoJob) * (size_t)n);
    {
        ppo::ProfScope ps(PPO_K_OTHER, 8.0 * (double)doubles);
        hipLaunchKernelGGL(ortho_kernel, dim3(n), dim3(TPB), 0, ppo::stream(), d_jobs);
        PPO_LAUNCH_CHECK();
    }
    phip_sync();
    PPO_CHECK(hipFree(d_jobs));
    PPO_CHECK(hipFree(work));
    for (int i = 0; i < n; ++i) jobs[i].work = nullptr;
}

}  // extern "C"
