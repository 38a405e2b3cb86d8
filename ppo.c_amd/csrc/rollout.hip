// rollout.hip — batched on-device rollout: all E environments step together.
//
// Reference collect_trajectories (ppo.cu:54-79) steps ONE environment on the host: policy sgemv
// (m = 1), rand()-Box–Muller noise (policy.cu:46-89), a gymnasium step through CPython.  Here one
// rollout step for E environments is: the μ forward over E rows (the buffer rows e·T + t read
// through the GEMM's row indirection), one sampling kernel that writes action / log-prob straight
// into the buffer rows, and one environment kernel.  Buffer layout is the env-major convention of
// ppo.cu:70-74: transition (e, t) at row e·T + t, every segment ending with truncated = 1.
//
// Environments (device, per-env state in HBM):
//   kind 0 — Pendulum-v1 (S = 3, A = 1): gymnasium classic_control dynamics as restated in
//            host/env.c (g = 10, m = l = 1, dt = 0.05, max speed 8, max torque 2, 200-step limit);
//            reset θ ~ U(−π, π), θ̇ ~ U(−1, 1) from Philox.
//   kind 1 — synthetic (any S, A): o' = clip(0.95·o + 0.05·tanh(a[j mod A]) +
//            0.05·ε, −1, 1); r = −0.01·mean(a²) + 0.1·ε; terminated ~ Bernoulli(1/500), reset
//            o ~ U(−1, 1).  With a categorical policy (ppo_set_action_dist 1) the action row holds an index
//            in column 0: every element reads tanh's argument as c = 2·index/(A − 1) − 1, whatever j, and
//            the reward's action term becomes −0.01·c²; the noise, the done draw and the reset are unchanged.
//            With a multi-discrete policy (ppo_set_action_multidiscrete) columns 0 … D−1 hold D indices: element
//            j reads component d = j mod D as c_d = 2·a_d/(n_d − 1) − 1 and the reward's action term is
//            −0.01·(Σ_d c_d²)/D, d ascending — at D = 1 the categorical arithmetic bit for bit.
//   kind 2 — CartPole-v1 (S = 4, A = 2, categorical policy only): gymnasium's constants (g = 9.8, cart 1.0, pole
//            0.1, half-length 0.5, force 10, τ = 0.02) and explicit Euler, in fp32 in the order of
//            cartpole_advance below; action index 1 pushes right.  Terminated when |x| > 2.4 or |θ| > 12·2π/360
//            after the step; reward 1 on every step, the terminating one included; TimeLimit at 500 steps sets
//            truncated.  Per-env state (x, ẋ, θ, θ̇, steps); a reset draws the four U(−0.05, 0.05) from
//            .x .y .z .w of one Philox draw at counter e.
#include "dev.h"
#include "ppo_math.h"
#include "rng.h"

#include <cmath>

namespace {

using namespace ppo_rng;

constexpr int TPB = 256;

// `step` below is the rollout's global step counter (it advances with every step of every
// ppo_rollout_device call): the position in the policy-noise, env and reset streams of rng.h.  `t`
// is the step inside this call: row addressing and the segment-end truncation only.

// a = μ + ε·σ written to buffer row rows[e]; log π(a) from the atoms of ppo_math.h log_prob_row
__global__ void sample_rows_kernel(const float* __restrict__ mu, const float* __restrict__ log_std,
                                   const int* __restrict__ rows, float* __restrict__ action,
                                   float* __restrict__ logprob, int E, int A, uint64_t seed, uint64_t step) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= E) return;
    const float* mr = mu + (long)e * A;
    float* ar = action + (long)rows[e] * A;
    float lp = ppo::log_prob_start(A);
    for (int j = 0; j < A; ++j) {
        const float a = mr[j] + normal_at((uint64_t)e * A + j, kNoise + step, seed) * expf(log_std[j]);
        ar[j] = a;
        const float z = (a - mr[j]) / expf(log_std[j]);
        lp = ppo::log_prob_sub(lp, ppo::log_prob_term(log_std[j], z));
    }
    logprob[rows[e]] = lp;
}

__device__ __forceinline__ float angle_normalize(float x) {
    const float two_pi = 2.f * (float)M_PI;
    float y = fmodf(x + (float)M_PI, two_pi);
    if (y < 0.f) y += two_pi;
    return y - (float)M_PI;
}

// One Pendulum-v1 step of environment e from (θ, θ̇, steps) under action a: the transition's reward and next
// observation; on return (θ, θ̇, steps) is what the next step starts from — the TimeLimit reset drawn where
// `limit`.  The training and the evaluation kernels both step through this, so the two cannot drift.
struct PendulumStep { float reward, next[3]; bool limit; };

__device__ __forceinline__ PendulumStep pendulum_advance(float& th, float& thdot, float& steps, float a, uint64_t e,
                                                         uint64_t step, uint64_t seed) {
    PendulumStep o;
    const float u = fminf(fmaxf(a, -2.f), 2.f);
    const float an = angle_normalize(th);
    const float cost = an * an + 0.1f * thdot * thdot + 0.001f * u * u;
    float nthdot = thdot + (3.f * 10.f / 2.f * sinf(th) + 3.f * u) * 0.05f;
    nthdot = fminf(fmaxf(nthdot, -8.f), 8.f);
    th = th + nthdot * 0.05f;
    thdot = nthdot;
    steps += 1.f;
    o.next[0] = cosf(th);
    o.next[1] = sinf(th);
    o.next[2] = thdot;
    o.reward = -cost;
    o.limit = steps >= 200.f;
    if (o.limit) {                                       // TimeLimit reset
        const u32x4 r = philox(e, kReset + step, seed);
        th = -(float)M_PI + 2.f * (float)M_PI * u01(r.x);
        thdot = -1.f + 2.f * u01(r.y);
        steps = 0.f;
    }
    return o;
}

// Pendulum-v1: env state (θ, θ̇, steps) in es[3e .. 3e+2]
__global__ void pendulum_step_kernel(float* __restrict__ es, float* __restrict__ state,
                                     const float* __restrict__ action, float* __restrict__ next_state,
                                     float* __restrict__ reward, uint8_t* __restrict__ term,
                                     uint8_t* __restrict__ trunc, uint8_t* __restrict__ cont, int E, int T, int t,
                                     uint64_t step, uint64_t seed, int A) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= E) return;
    const long row = (long)e * T + t;
    float th = es[3 * e], thdot = es[3 * e + 1];
    float steps = es[3 * e + 2];
    // the torque is column 0 of the action row (A = 2: the state-dependent-σ Gaussian's row, a zero after it)
    const PendulumStep o = pendulum_advance(th, thdot, steps, action[row * A], (uint64_t)e, step, seed);
    next_state[3 * row] = o.next[0];
    next_state[3 * row + 1] = o.next[1];
    next_state[3 * row + 2] = o.next[2];
    reward[row] = o.reward;
    term[row] = 0;
    trunc[row] = (o.limit || t == T - 1) ? 1 : 0;
    if (cont && t == T - 1) cont[e] = o.limit ? 0 : 1;   // not reset: the next rollout continues this episode
    es[3 * e] = th;
    es[3 * e + 1] = thdot;
    es[3 * e + 2] = steps;
    if (t + 1 < T) {
        state[3 * (row + 1)] = cosf(th);
        state[3 * (row + 1) + 1] = sinf(th);
        state[3 * (row + 1) + 2] = thdot;
    }
}

// the evaluation's form: obs [E, 3] is the current observation, replaced in place; action [E]
__global__ void pendulum_eval_kernel(float* __restrict__ es, float* __restrict__ obs, const float* __restrict__ action,
                                     float* __restrict__ reward, uint8_t* __restrict__ term,
                                     uint8_t* __restrict__ trunc, uint8_t* __restrict__ cont, int E, int T, int t,
                                     uint64_t step, uint64_t seed, int A) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= E) return;
    const long row = (long)e * T + t;
    float th = es[3 * e], thdot = es[3 * e + 1];
    float steps = es[3 * e + 2];
    const PendulumStep o = pendulum_advance(th, thdot, steps, action[(long)e * A], (uint64_t)e, step, seed);
    reward[row] = o.reward;
    term[row] = 0;
    trunc[row] = (o.limit || t == T - 1) ? 1 : 0;
    if (t == T - 1) cont[e] = o.limit ? 0 : 1;
    es[3 * e] = th;
    es[3 * e + 1] = thdot;
    es[3 * e + 2] = steps;
    obs[3 * e] = cosf(th);
    obs[3 * e + 1] = sinf(th);
    obs[3 * e + 2] = thdot;
}

// One synthetic step of observation element k = e·S + j under the action row ar: o2 the transition's next
// observation, nxt what the next step starts from (the reset drawn where done), the reward for j == 0 only.  The
// reward / done decision per env is taken by every thread of the env identically (same Philox draw).
struct SynthStep { float o2, nxt, reward; bool done; };

// multi-discrete: component d's index (column d of the action row) mapped onto [−1, 1]
__device__ __forceinline__ float md_centre(const float* __restrict__ ar, const int* __restrict__ md_off, int d) {
    const int n = md_off[d + 1] - md_off[d];
    return 2.f * (float)ppo::cat_index(ar[d], n) / (float)(n - 1) - 1.f;
}

// A: the action columns in use (the state-dependent-σ Gaussian's row holds A / 2 of them and zeros after)
__device__ __forceinline__ SynthStep synth_advance(float o, const float* __restrict__ ar, long k, int e, int j, int A,
                                                   uint64_t step, uint64_t seed, int cat,
                                                   const int* __restrict__ md_off, int D) {
    SynthStep s;
    const u32x4 d = philox((uint64_t)e, kEnv + 2 * step, seed);
    s.done = u01(d.z) < 1.f / 500.f;
    const float eps = normal_at((uint64_t)k, kEnv + 2 * step + 1, seed);
    // categorical: the index of column 0 mapped onto [−1, 1]
    float c = cat ? 2.f * (float)ppo::cat_index(ar[0], A) / (float)(A - 1) - 1.f : 0.f;
    if (md_off) c = md_centre(ar, md_off, j % D);    // multi-discrete: this element's component
    float o2 = 0.95f * o + 0.05f * tanhf(cat ? c : ar[j % A]) + 0.05f * eps;
    o2 = fminf(fmaxf(o2, -1.f), 1.f);
    s.o2 = o2;
    s.reward = 0.f;
    if (j == 0) {
        float ss = 0.f;
        for (int q = 0; q < A; ++q) ss += ar[q] * ar[q];
        float act_term = cat ? -0.01f * (c * c) : -0.01f * ss / (float)A;
        if (md_off) {
            float cc = 0.f;
            for (int d = 0; d < D; ++d) {
                const float cd = md_centre(ar, md_off, d);
                cc += cd * cd;
            }
            act_term = -0.01f * cc / (float)D;
        }
        s.reward = act_term + 0.1f * sqrtf(-2.f * logf(u01(d.x))) * cosf(2.f * (float)M_PI * u01(d.y));
    }
    s.nxt = s.done ? -1.f + 2.f * u01(philox((uint64_t)k, kReset + step, seed).x) : o2;
    return s;
}

// synthetic env: one thread per (env, obs element); no cross-thread exchange
__global__ void synth_step_kernel(float* __restrict__ es, float* __restrict__ state, const float* __restrict__ action,
                                  float* __restrict__ next_state, float* __restrict__ reward,
                                  uint8_t* __restrict__ term, uint8_t* __restrict__ trunc,
                                  uint8_t* __restrict__ cont, int E, int T, int t, uint64_t step, int S, int A,
                                  uint64_t seed, int cat, const int* __restrict__ md_off, int D, int Au) {
    const long k = (long)blockIdx.x * TPB + threadIdx.x;
    if (k >= (long)E * S) return;
    const int e = (int)(k / S), j = (int)(k % S);
    const long row = (long)e * T + t;
    const SynthStep s = synth_advance(es[k], action + row * A, k, e, j, Au, step, seed, cat, md_off, D);
    next_state[row * S + j] = s.o2;
    if (j == 0) {
        reward[row] = s.reward;
        term[row] = s.done ? 1 : 0;
        trunc[row] = (!s.done && t == T - 1) ? 1 : 0;
        if (cont && t == T - 1) cont[e] = s.done ? 0 : 1;
    }
    es[k] = s.nxt;
    if (t + 1 < T) state[(row + 1) * S + j] = s.nxt;
}

// the evaluation's form: obs [E, S] is the current observation, replaced in place; action [E, A]
__global__ void synth_eval_kernel(float* __restrict__ es, float* __restrict__ obs, const float* __restrict__ action,
                                  float* __restrict__ reward, uint8_t* __restrict__ term, uint8_t* __restrict__ trunc,
                                  uint8_t* __restrict__ cont, int E, int T, int t, uint64_t step, int S, int A,
                                  uint64_t seed, int cat, const int* __restrict__ md_off, int D, int Au) {
    const long k = (long)blockIdx.x * TPB + threadIdx.x;
    if (k >= (long)E * S) return;
    const int e = (int)(k / S), j = (int)(k % S);
    const long row = (long)e * T + t;
    const SynthStep s = synth_advance(es[k], action + (long)e * A, k, e, j, Au, step, seed, cat, md_off, D);
    if (j == 0) {
        reward[row] = s.reward;
        term[row] = s.done ? 1 : 0;
        trunc[row] = (!s.done && t == T - 1) ? 1 : 0;
        if (t == T - 1) cont[e] = s.done ? 0 : 1;
    }
    es[k] = s.nxt;
    obs[k] = s.nxt;
}

// One CartPole-v1 step of environment e from (x, ẋ, θ, θ̇, steps) under the action index a (1 pushes right), fp32
// in exactly this order (tests/categorical_ref.py mirrors it): the transition's next observation and flags; on
// return the state is what the next step starts from — the reset drawn where the episode ended.  The training
// and the evaluation kernels both step through this, so the two cannot drift.
struct CartPoleStep { float next[4]; bool term, limit; };

__device__ __forceinline__ void cartpole_reset(float* st, uint64_t e, uint64_t offset, uint64_t seed) {
    const u32x4 r = philox(e, offset, seed);
    st[0] = -0.05f + 0.1f * u01(r.x);
    st[1] = -0.05f + 0.1f * u01(r.y);
    st[2] = -0.05f + 0.1f * u01(r.z);
    st[3] = -0.05f + 0.1f * u01(r.w);
    st[4] = 0.f;
}

__device__ __forceinline__ CartPoleStep cartpole_advance(float* st, int a, uint64_t e, uint64_t step, uint64_t seed) {
    CartPoleStep o;
    const float x = st[0], xd = st[1], th = st[2], thd = st[3];
    const float force = a == 1 ? 10.f : -10.f;
    const float ct = cosf(th), sn = sinf(th);
    const float temp = (force + 0.05f * (thd * thd) * sn) / 1.1f;                  // polemass_length 0.05, total mass 1.1
    const float thacc = (9.8f * sn - ct * temp) / (0.5f * (4.f / 3.f - 0.1f * (ct * ct) / 1.1f));
    const float xacc = temp - 0.05f * thacc * ct / 1.1f;
    o.next[0] = x + 0.02f * xd;
    o.next[1] = xd + 0.02f * xacc;
    o.next[2] = th + 0.02f * thd;
    o.next[3] = thd + 0.02f * thacc;
    const float steps = st[4] + 1.f;
    o.term = fabsf(o.next[0]) > 2.4f || fabsf(o.next[2]) > 12.f * 2.f * (float)M_PI / 360.f;
    o.limit = steps >= 500.f;
    if (o.term || o.limit) {
        cartpole_reset(st, e, kReset + step, seed);
    } else {
        for (int q = 0; q < 4; ++q) st[q] = o.next[q];
        st[4] = steps;
    }
    return o;
}

// CartPole-v1: env state (x, ẋ, θ, θ̇, steps) in es[5e .. 5e+4]
__global__ void cartpole_step_kernel(float* __restrict__ es, float* __restrict__ state,
                                     const float* __restrict__ action, float* __restrict__ next_state,
                                     float* __restrict__ reward, uint8_t* __restrict__ term,
                                     uint8_t* __restrict__ trunc, uint8_t* __restrict__ cont, int E, int T, int t,
                                     uint64_t step, uint64_t seed) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= E) return;
    const long row = (long)e * T + t;
    float st[5];
    for (int q = 0; q < 5; ++q) st[q] = es[5 * e + q];
    const CartPoleStep o = cartpole_advance(st, ppo::cat_index(action[2 * row], 2), (uint64_t)e, step, seed);
    for (int q = 0; q < 4; ++q) next_state[4 * row + q] = o.next[q];
    reward[row] = 1.f;
    term[row] = o.term ? 1 : 0;
    trunc[row] = (o.limit || t == T - 1) ? 1 : 0;
    if (cont && t == T - 1) cont[e] = (o.term || o.limit) ? 0 : 1;
    for (int q = 0; q < 5; ++q) es[5 * e + q] = st[q];
    if (t + 1 < T)
        for (int q = 0; q < 4; ++q) state[4 * (row + 1) + q] = st[q];
}

// the evaluation's form: obs [E, 4] is the current observation, replaced in place; action [E, 2]
__global__ void cartpole_eval_kernel(float* __restrict__ es, float* __restrict__ obs, const float* __restrict__ action,
                                     float* __restrict__ reward, uint8_t* __restrict__ term,
                                     uint8_t* __restrict__ trunc, uint8_t* __restrict__ cont, int E, int T, int t,
                                     uint64_t step, uint64_t seed) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= E) return;
    const long row = (long)e * T + t;
    float st[5];
    for (int q = 0; q < 5; ++q) st[q] = es[5 * e + q];
    const CartPoleStep o = cartpole_advance(st, ppo::cat_index(action[2 * e], 2), (uint64_t)e, step, seed);
    reward[row] = 1.f;
    term[row] = o.term ? 1 : 0;
    trunc[row] = (o.limit || t == T - 1) ? 1 : 0;
    if (t == T - 1) cont[e] = (o.term || o.limit) ? 0 : 1;
    for (int q = 0; q < 5; ++q) es[5 * e + q] = st[q];
    for (int q = 0; q < 4; ++q) obs[4 * e + q] = st[q];
}

// reset every env; write row e·T (t = 0) of the buffer
__global__ void env_reset_kernel(int kind, float* __restrict__ es, float* __restrict__ state, int E, int T, int S,
                                 uint64_t seed) {
    const long k = (long)blockIdx.x * TPB + threadIdx.x;
    if (kind == 0) {
        if (k >= E) return;
        const u32x4 r = philox((uint64_t)k, kReset - 1, seed);
        const float th = -(float)M_PI + 2.f * (float)M_PI * u01(r.x), thdot = -1.f + 2.f * u01(r.y);
        es[3 * k] = th; es[3 * k + 1] = thdot; es[3 * k + 2] = 0.f;
        return;
    }
    if (kind == 2) {
        if (k >= E) return;
        float st[5];
        cartpole_reset(st, (uint64_t)k, kReset - 1, seed);
        for (int q = 0; q < 5; ++q) es[5 * k + q] = st[q];
        return;
    }
    if (k >= (long)E * S) return;
    es[k] = -1.f + 2.f * u01(philox((uint64_t)k, kReset - 1, seed).x);
}

// first row of each segment from the persistent env state (episodes continue across rollouts)
__global__ void env_obs_kernel(int kind, const float* __restrict__ es, float* __restrict__ state, int E, int T,
                               int S) {
    const long k = (long)blockIdx.x * TPB + threadIdx.x;
    if (k >= (long)E * S) return;
    const int e = (int)(k / S), j = (int)(k % S);
    float v;
    if (kind == 0) v = j == 0 ? cosf(es[3 * e]) : (j == 1 ? sinf(es[3 * e]) : es[3 * e + 1]);
    else if (kind == 2) v = es[5 * e + j];
    else v = es[k];
    state[(long)e * T * S + j] = v;
}

__global__ void rows_kernel(int* __restrict__ rows, int E, int T) {
    const long k = (long)blockIdx.x * TPB + threadIdx.x;     // k = t·E + e
    if (k >= (long)E * T) return;
    const int t = (int)(k / E), e = (int)(k % E);
    rows[k] = e * T + t;
}

// The dense forms (ppo_ext.h ppo_env_step_device): the same advance functions over caller-owned arrays — action
// [E, A] in, the transition's next observation, the observation the next step starts from, reward and the
// environment's own flags out, each [E, ·].  trunc is the TimeLimit alone: a segment end belongs to the store.
__global__ void pendulum_dense_kernel(float* __restrict__ es, const float* __restrict__ action,
                                      float* __restrict__ next_obs, float* __restrict__ obs_after,
                                      float* __restrict__ reward, uint8_t* __restrict__ term,
                                      uint8_t* __restrict__ trunc, int E, uint64_t step, uint64_t seed) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= E) return;
    float th = es[3 * e], thdot = es[3 * e + 1];
    float steps = es[3 * e + 2];
    const PendulumStep o = pendulum_advance(th, thdot, steps, action[e], (uint64_t)e, step, seed);
    next_obs[3 * e] = o.next[0];
    next_obs[3 * e + 1] = o.next[1];
    next_obs[3 * e + 2] = o.next[2];
    reward[e] = o.reward;
    term[e] = 0;
    trunc[e] = o.limit ? 1 : 0;
    es[3 * e] = th;
    es[3 * e + 1] = thdot;
    es[3 * e + 2] = steps;
    obs_after[3 * e] = cosf(th);
    obs_after[3 * e + 1] = sinf(th);
    obs_after[3 * e + 2] = thdot;
}

__global__ void synth_dense_kernel(float* __restrict__ es, const float* __restrict__ action,
                                   float* __restrict__ next_obs, float* __restrict__ obs_after,
                                   float* __restrict__ reward, uint8_t* __restrict__ term,
                                   uint8_t* __restrict__ trunc, int E, uint64_t step, int S, int A, uint64_t seed,
                                   int cat) {
    const long k = (long)blockIdx.x * TPB + threadIdx.x;
    if (k >= (long)E * S) return;
    const int e = (int)(k / S), j = (int)(k % S);
    const SynthStep s = synth_advance(es[k], action + (long)e * A, k, e, j, A, step, seed, cat, nullptr, 0);
    next_obs[k] = s.o2;
    if (j == 0) {
        reward[e] = s.reward;
        term[e] = s.done ? 1 : 0;
        trunc[e] = 0;
    }
    es[k] = s.nxt;
    obs_after[k] = s.nxt;
}

__global__ void cartpole_dense_kernel(float* __restrict__ es, const float* __restrict__ action,
                                      float* __restrict__ next_obs, float* __restrict__ obs_after,
                                      float* __restrict__ reward, uint8_t* __restrict__ term,
                                      uint8_t* __restrict__ trunc, int E, uint64_t step, uint64_t seed) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= E) return;
    float st[5];
    for (int q = 0; q < 5; ++q) st[q] = es[5 * e + q];
    const CartPoleStep o = cartpole_advance(st, ppo::cat_index(action[2 * e], 2), (uint64_t)e, step, seed);
    for (int q = 0; q < 4; ++q) next_obs[4 * e + q] = o.next[q];
    reward[e] = 1.f;
    term[e] = o.term ? 1 : 0;
    trunc[e] = o.limit ? 1 : 0;
    for (int q = 0; q < 5; ++q) es[5 * e + q] = st[q];
    for (int q = 0; q < 4; ++q) obs_after[4 * e + q] = st[q];
}

// The open rollout (ppo_ext.h ppo_rollout_act / ppo_rollout_store).  One thread per (e, j), j along the row.
// dense[e, :] = action[rows[e], :]
__global__ void action_rows_out_kernel(const float* __restrict__ action, const int* __restrict__ rows,
                                       float* __restrict__ dense, int E, int A) {
    const long k = (long)blockIdx.x * TPB + threadIdx.x;
    if (k >= (long)E * A) return;
    const int e = (int)(k / A), j = (int)(k % A);
    dense[k] = action[(long)rows[e] * A + j];
}

// One external step into row e·T + t: the store rule of ppo_ext.h.  obs_after (NULL: next_obs) is what the next
// step starts from: it goes to state[row + 1] and to cur, the PPO's current observations.  The flags, the reward
// and cont[e] are thread j == 0's; no thread reads what another writes.  next_obs and obs_after may be one array.
__global__ void ext_store_kernel(const float* next_obs, const float* obs_after, const float* __restrict__ reward_in,
                                 const uint8_t* __restrict__ term_in, const uint8_t* __restrict__ trunc_in,
                                 float* __restrict__ state, float* __restrict__ next_state,
                                 float* __restrict__ reward, uint8_t* __restrict__ term, uint8_t* __restrict__ trunc,
                                 uint8_t* __restrict__ cont, float* __restrict__ cur, int E, int T, int t, int S) {
    const long k = (long)blockIdx.x * TPB + threadIdx.x;
    if (k >= (long)E * S) return;
    const int e = (int)(k / S), j = (int)(k % S);
    const long row = (long)e * T + t;
    next_state[row * S + j] = next_obs[k];
    const float after = obs_after ? obs_after[k] : next_obs[k];
    if (t + 1 < T) state[(row + 1) * S + j] = after;
    cur[k] = after;
    if (j == 0) {
        const bool tm = term_in[e] != 0, tr = trunc_in[e] != 0;
        reward[row] = reward_in[e];
        term[row] = tm ? 1 : 0;
        trunc[row] = (tr || (t == T - 1 && !tm)) ? 1 : 0;
        if (t == T - 1) cont[e] = (tm || tr) ? 0 : 1;
    }
}

}  // namespace

extern "C" {

void phip_rollout_rows(int* rows, int E, int T) {
    const long n = (long)E * T;
    hipLaunchKernelGGL(rows_kernel, dim3(ppo_divup(n, TPB)), dim3(TPB), 0, ppo::stream(), rows, E, T);
    PPO_LAUNCH_CHECK();
}

void phip_env_reset(int kind, float* env_state, float* state, int E, int T, int S, uint64_t seed) {
    const long n = (kind == 0 || kind == 2) ? E : (long)E * S;
    PPO_REQUIRE(kind != 2 || S == 4, "phip_env_reset: CartPole-v1 needs S = 4");
    hipLaunchKernelGGL(env_reset_kernel, dim3(ppo_divup(n, TPB)), dim3(TPB), 0, ppo::stream(), kind, env_state, state,
                       E, T, S, seed);
    PPO_LAUNCH_CHECK();
}

void phip_env_first_obs(int kind, const float* env_state, float* state, int E, int T, int S) {
    const long n = (long)E * S;
    PPO_REQUIRE(kind != 2 || S == 4, "phip_env_first_obs: CartPole-v1 needs S = 4");
    hipLaunchKernelGGL(env_obs_kernel, dim3(ppo_divup(n, TPB)), dim3(TPB), 0, ppo::stream(), kind, env_state, state,
                       E, T, S);
    PPO_LAUNCH_CHECK();
}

void phip_sample_rows(const float* mu, const float* log_std, const int* rows, float* action, float* logprob, int E,
                      int A, uint64_t seed, uint64_t step) {
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * E * (2 * A + 1));
    hipLaunchKernelGGL(sample_rows_kernel, dim3(ppo_divup(E, TPB)), dim3(TPB), 0, ppo::stream(), mu, log_std, rows,
                       action, logprob, E, A, seed, step);
    PPO_LAUNCH_CHECK();
}

void phip_env_step(int kind, float* env_state, float* state, const float* action, float* next_state, float* reward,
                   uint8_t* term, uint8_t* trunc, uint8_t* cont, int E, int T, int t, uint64_t step, int S, int A,
                   uint64_t seed, int cat, const int* md_off, int D, int Au) {
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * E * (3 * S + A + 2));
    PPO_REQUIRE(Au == A || (!cat && 2 * Au == A), "phip_env_step: the action columns in use");
    PPO_REQUIRE(!md_off || (cat && D >= 1 && 2 * D <= A), "phip_env_step: multi-discrete offsets");
    if (kind == 0) {
        PPO_REQUIRE(S == 3 && Au == 1, "phip_env_step: Pendulum-v1 needs S = 3 and one action column");
        hipLaunchKernelGGL(pendulum_step_kernel, dim3(ppo_divup(E, TPB)), dim3(TPB), 0, ppo::stream(), env_state,
                           state, action, next_state, reward, term, trunc, cont, E, T, t, step, seed, A);
    } else if (kind == 2) {
        PPO_REQUIRE(S == 4 && A == 2 && cat, "phip_env_step: CartPole-v1 needs S = 4, A = 2 and categorical actions");
        hipLaunchKernelGGL(cartpole_step_kernel, dim3(ppo_divup(E, TPB)), dim3(TPB), 0, ppo::stream(), env_state,
                           state, action, next_state, reward, term, trunc, cont, E, T, t, step, seed);
    } else {
        hipLaunchKernelGGL(synth_step_kernel, dim3(ppo_divup((long)E * S, TPB)), dim3(TPB), 0, ppo::stream(),
                           env_state, state, action, next_state, reward, term, trunc, cont, E, T, t, step, S, A,
                           seed, cat, md_off, D, Au);
    }
    PPO_LAUNCH_CHECK();
}

void phip_env_step_eval(int kind, float* env_state, float* obs, const float* action, float* reward, uint8_t* term,
                        uint8_t* trunc, uint8_t* cont, int E, int T, int t, uint64_t step, int S, int A,
                        uint64_t seed, int cat, const int* md_off, int D, int Au) {
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * E * (2 * S + A + 2));
    PPO_REQUIRE(Au == A || (!cat && 2 * Au == A), "phip_env_step_eval: the action columns in use");
    PPO_REQUIRE(!md_off || (cat && D >= 1 && 2 * D <= A), "phip_env_step_eval: multi-discrete offsets");
    PPO_REQUIRE(env_state && obs && action && reward && term && trunc && cont && E > 0 && t >= 0 && t < T,
                "phip_env_step_eval: operands");
    if (kind == 0) {
        PPO_REQUIRE(S == 3 && Au == 1, "phip_env_step_eval: Pendulum-v1 needs S = 3 and one action column");
        hipLaunchKernelGGL(pendulum_eval_kernel, dim3(ppo_divup(E, TPB)), dim3(TPB), 0, ppo::stream(), env_state, obs,
                           action, reward, term, trunc, cont, E, T, t, step, seed, A);
    } else if (kind == 2) {
        PPO_REQUIRE(S == 4 && A == 2 && cat,
                    "phip_env_step_eval: CartPole-v1 needs S = 4, A = 2 and categorical actions");
        hipLaunchKernelGGL(cartpole_eval_kernel, dim3(ppo_divup(E, TPB)), dim3(TPB), 0, ppo::stream(), env_state, obs,
                           action, reward, term, trunc, cont, E, T, t, step, seed);
    } else {
        hipLaunchKernelGGL(synth_eval_kernel, dim3(ppo_divup((long)E * S, TPB)), dim3(TPB), 0, ppo::stream(),
                           env_state, obs, action, reward, term, trunc, cont, E, T, t, step, S, A, seed, cat, md_off,
                           D, Au);
    }
    PPO_LAUNCH_CHECK();
}

void phip_env_step_dense(int kind, float* env_state, const float* action, float* next_obs, float* obs_after,
                         float* reward, uint8_t* term, uint8_t* trunc, int E, uint64_t step, int S, int A,
                         uint64_t seed, int cat) {
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * E * (3 * S + A + 2));
    PPO_REQUIRE(env_state && action && next_obs && obs_after && reward && term && trunc && E > 0,
                "phip_env_step_dense: operands");
    if (kind == 0) {
        PPO_REQUIRE(S == 3 && A == 1, "phip_env_step_dense: Pendulum-v1 needs S = 3, A = 1");
        hipLaunchKernelGGL(pendulum_dense_kernel, dim3(ppo_divup(E, TPB)), dim3(TPB), 0, ppo::stream(), env_state,
                           action, next_obs, obs_after, reward, term, trunc, E, step, seed);
    } else if (kind == 2) {
        PPO_REQUIRE(S == 4 && A == 2 && cat,
                    "phip_env_step_dense: CartPole-v1 needs S = 4, A = 2 and categorical actions");
        hipLaunchKernelGGL(cartpole_dense_kernel, dim3(ppo_divup(E, TPB)), dim3(TPB), 0, ppo::stream(), env_state,
                           action, next_obs, obs_after, reward, term, trunc, E, step, seed);
    } else {
        hipLaunchKernelGGL(synth_dense_kernel, dim3(ppo_divup((long)E * S, TPB)), dim3(TPB), 0, ppo::stream(),
                           env_state, action, next_obs, obs_after, reward, term, trunc, E, step, S, A, seed, cat);
    }
    PPO_LAUNCH_CHECK();
}

void phip_action_rows_out(const float* action, const int* rows, float* dense, int E, int A) {
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * E * (2 * A + 1));
    hipLaunchKernelGGL(action_rows_out_kernel, dim3(ppo_divup((long)E * A, TPB)), dim3(TPB), 0, ppo::stream(), action,
                       rows, dense, E, A);
    PPO_LAUNCH_CHECK();
}

void phip_ext_store(const float* next_obs, const float* obs_after, const float* reward_in, const uint8_t* term_in,
                    const uint8_t* trunc_in, float* state, float* next_state, float* reward, uint8_t* term,
                    uint8_t* trunc, uint8_t* cont, float* cur, int E, int T, int t, int S) {
    ppo::ProfScope ps(PPO_K_OTHER, 4.0 * E * (4 * S + 3));
    PPO_REQUIRE(next_obs && reward_in && term_in && trunc_in && cont && cur && E > 0 && t >= 0 && t < T,
                "phip_ext_store: operands");
    hipLaunchKernelGGL(ext_store_kernel, dim3(ppo_divup((long)E * S, TPB)), dim3(TPB), 0, ppo::stream(), next_obs,
                       obs_after, reward_in, term_in, trunc_in, state, next_state, reward, term, trunc, cont, cur, E,
                       T, t, S);
    PPO_LAUNCH_CHECK();
}

}  // extern "C"
