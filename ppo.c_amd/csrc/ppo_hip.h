/*
 * ppo_hip.h — the thin C ABI between libppo's plain-C host code (ppo.c_amd/host)
 * and its hand-written gfx950 HIP kernels (ppo.c_amd/csrc).
 *
 * All pointers named d_* / device arrays are HBM pointers; every launch goes to
 * libppo's single stream and is asynchronous unless stated.  Shapes follow the
 * reference (row-major, W is [out, in]).  No function here allocates per call.
 */
#ifndef PPO_HIP_H
#define PPO_HIP_H

#include <stddef.h>
#include <stdint.h>

/* splitmix64: libppo's key derivation (Feistel round keys, RNG stream keys) on the host, and the replica
 * hash's mixer on the device (comm.hip) */
#define PHIP_GOLDEN64 0x9E3779B97F4A7C15ULL
#ifdef __HIPCC__
__host__ __device__
#endif
static inline uint64_t splitmix64(uint64_t z) {
    z += PHIP_GOLDEN64;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- runtime / memory ---------------- */
void  phip_init(void);                     /* select device, create stream; abort without a GPU */
void* phip_malloc(size_t bytes);           /* zero-filled, 256-B aligned */
void  phip_free(void* p);
void  phip_h2d(void* dst, const void* src, size_t bytes);   /* completes before return */
void  phip_d2h(void* dst, const void* src, size_t bytes);   /* completes before return */
void  phip_d2d(void* dst, const void* src, size_t bytes);   /* async */
void  phip_memset(void* dst, int value, size_t bytes);      /* async */
void  phip_sync(void);                     /* both queues */
/* a second queue for independent work: fork = the side queue waits for everything issued so far on
 * the main queue; use(1) routes launches to the side queue until use(0); join = the main queue
 * waits for everything issued so far on the side queue */
void  phip_side_fork(void);
void  phip_side_use(int on);
int   phip_comm_inline(void);   /* gradient all-reduces in stream order, one per step (comm.hip) */
int   phip_side_active(void);   /* 1 while launches go to the side stream */
void  phip_side_join(void);
void  phip_record_error(const char* msg);
void  phip_drain(void);                 /* synchronise both streams, ignoring errors (before a fatal exit) */

/* ---------------- PPO2 value-loss clipping (vclip.h) ---------------- */
/* what every form of the value head takes (ppo_ext.h ppo_set_value_clip; csrc/vclip.h value_head_row holds
 * the arithmetic once): row i of the minibatch reads its old value at v_old[rows[i]].  A NULL PhipVClip*,
 * or v_old == NULL, is "off": today's arithmetic and launches. */
typedef struct {
    const float* v_old;             /* old values indexed by buffer row (device); NULL: off */
    const int* rows;                /* minibatch slot -> buffer row (device); NULL: the identity */
    float eps;                      /* the clip range eps_v > 0 */
    unsigned long long* counts;     /* device [2]: += clipped rows, += rows (integer atomics: exact) */
} PhipVClip;

/* ---------------- dense layers (gemm.hip) ---------------- */
/* activation kinds of the forward launchers' `act` argument (host: nn_act_kind); the value is uniform over a
 * launch.  PHIP_ACT_TANH applies tanhf after the bias and writes no mask bits: tanh′ = 1 − h² needs only the
 * stored post-activation h, which the grad_x launchers take as their `h` operand */
enum { PHIP_ACT_NONE = 0, PHIP_ACT_RELU = 1, PHIP_ACT_TANH = 2 };
/* y[m,l] = act(x[m,n]·W[l,n]ᵀ + b[l]) (mat_mul.cu:132-163 + K1/K5 fused) */
void phip_linear_fwd(float* y, const float* x, const float* W, const float* b, int m, int n, int l, int act);
/* same, and (act = relu) writes the ReLU′ mask as bits: word (row, c/32) bit c%32 = y[row, c] > 0,
 * ⌈l/32⌉ words per row — 1/32 of the bytes the float mask costs the backward */
void phip_linear_fwd_bits(float* y, const float* x, const float* W, const float* b, int m, int n, int l, int act,
                          unsigned* bits);
/* gx[m,n] = g[m,l]·W[l,n]; if mask: gx = (mask > 0) ? gx : 0 (K3 + K6 fused) */
void phip_linear_bwd_x(float* gx, const float* g, const float* W, const float* mask, int m, int n, int l);
/* forward whose input row r is x[ridx[r]] (the minibatch gather fused into layer 0); the gathered
 * rows are also written to xcopy[m, n] (for the layer's grad_W) when xcopy != NULL */
void phip_linear_fwd_gather(float* y, const float* x, const int* ridx, float* xcopy, const float* W, const float* b,
                            int m, int n, int l, int act, unsigned* bits);
/* same with the mask given as bits (phip_linear_fwd_bits layout, ⌈n/32⌉ words per row); or, for a tanh
 * layer below, h [m, n] (ld = n) its stored post-activation: gx = acc − (acc·h)·h in fp32 (mask and bits
 * are then NULL) */
void phip_linear_bwd_x_bits(float* gx, const float* g, const float* W, const float* mask, const unsigned* bits,
                            const float* h, int m, int n, int l);
/* gW[l,n] = g[m,l]ᵀ·x[m,n] and gb[l] = Σ_m g[m,l] (K4 + K7 fused); overwrites */
void phip_linear_bwd_w(float* gW, float* gb, const float* g, const float* x, int m, int n, int l);
/* same, with gW/gb already zero on entry when `zeroed` (one memset per backward instead of two per layer) */
/* grad_W (+ bias) and grad_x ⊙ ReLU′(bits) of one layer, one launch when the shapes allow */
void phip_linear_bwd_pair(float* gW, float* gb, float* gx, const float* g, const float* x, const float* W,
                          const unsigned* bits, int m, int n, int l, int zeroed);
void phip_linear_bwd_w_ex(float* gW, float* gb, const float* g, const float* x, int m, int n, int l, int zeroed);

/* ---------------- bf16-MFMA dense layers (gemm16.hip) ---------------- */
/* dtype codes t*: 0 = fp32 storage, 1 = bf16 storage; W16 = bf16 shadow of W [l, n]; fp32 accumulation.
 * forward (optional fused gather: ridx / bf16 copy of the gathered rows in xcopy16) */
void phip_linear16_fwd(void* y, int ty, const void* x, int tx, const int* ridx, void* xcopy16, const void* W16,
                       const float* b, int m, int n, int l, int relu, unsigned* bits);
/* gx = (g·W) ⊙ bits (bits may be NULL: no mask) */
void phip_linear16_bwd_x(void* gx, int tgx, const void* g, int tg, const void* W16, const unsigned* bits, int m,
                         int n, int l);
/* gW[l,n] (+)= gᵀ·x, gb (+)= Σ g in fp32 (zeroed != 0: outputs already zero) */
void phip_linear16_bwd_w(float* gW, float* gb, const void* g, int tg, const void* x, int tx, int m, int n, int l,
                         int zeroed);
/* fp32-accurate products on the bf16 MFMA (gemm_x3.hip, the "x3" engine of fp32 mode): every fp32
 * operand splits exactly into three bf16 planes on its way into LDS, six plane products, fp32
 * accumulation.  Forward with optional fused gather (xcopy = fp32 copy of the gathered rows) +
 * bias/ReLU/ReLU' bits; grad_x with the bit mask; grad_W (+gb) split-K. */
int  phip_x3_supported(int op, int m, int n, int l);
void phip_x3_fwd(float* y, const float* x, const int* ridx, float* xcopy, const float* W, const float* b, int m,
                 int n, int l, int act, unsigned* bits);
/* the next phip_x3_bwd_w(_fold) leaves its split-K slab reduce to the next phip_x3_bwd_x(_fold) on the same
 * stream (extra workgroups of that launch) — the caller guarantees grad_x follows */
void phip_x3_defer_reduce(int on);
/* bits: the ReLU′ mask of the layer below (NULL: none); h: a tanh layer below's post-activation [m, n], read
 * at gx's own coordinates — gx = acc − (acc·h)·h (NULL: none) */
void phip_x3_bwd_x(float* gx, const float* g, const float* W, const unsigned* bits, const float* h, int m, int n,
                   int l);
void phip_x3_bwd_w(float* gW, float* gb, const float* g, const float* x, int m, int n, int l, int zeroed);
/* value-head fold (nn_value_fold_step): forward partial y dots (returns ypart slots); backward with the
 * upper gradient g·w·1[h > 0] applied as the 0/1 mask of h with g, w as row / column scales (grad_x:
 * W pre-scaled by w) and the output layer's gW */
int  phip_x3_fwd_vhead(float* y, const float* x, const int* ridx, float* xcopy, const float* W, const float* b, int m,
                       int n, int l, int act, unsigned* bits, const float* ydot, float* ypart);
void phip_x3_bwd_x_fold(float* gx, const float* g, const unsigned* fold_bits, const float* fold_g, const float* fold_w,
                        const float* W, const unsigned* bits, int m, int n, int l);
void phip_x3_bwd_w_fold(float* gW, float* gb, const float* h, const float* fold_g, const float* fold_w, float* fold_gw,
                        const float* x, int m, int n, int l, int zeroed);
/* phip_x3_bwd_w_fold carrying the value head: g (into fold_g) from the forward's partial dots ypart [slots][m]
 * + b against tgt, y, the output bias gradient gb_out and loss_accum (+= loss / m) — value_head_kernel's work;
 * vc: value-loss clipping of that head (NULL: off) */
void phip_x3_bwd_w_vhead(float* gW, float* gb, const float* h, float* fold_g, const float* fold_w, float* fold_gw,
                         const float* x, int m, int n, int l, int zeroed, const float* ypart, int slots, const float* b,
                         const float* tgt, float* y, float* gb_out, float* loss_accum, const PhipVClip* vc);
/* dst[i, :] = bf16(src[rows[i], :]) for i < m (S % 4 == 0): layer 0's gather in bf16 mode */
void phip_gather_rows_bf16(unsigned short* dst, const float* src, const int* rows, int m, int S);
void phip_f32_to_bf16(unsigned short* dst, const float* src, long count);

/* ---------------- batched device rollout (rollout.hip) ---------------- */
/* env kinds: 0 = Pendulum-v1 (S = 3, A = 1), 1 = synthetic (any S, A), 2 = CartPole-v1 (S = 4, A = 2, categorical
 * actions).  env_state holds PHIP_ENV_STATE(S) floats per environment.  cat != 0 (the step functions): column 0
 * of an action row is a categorical index (kind 1 reads it as 2·index/(A − 1) − 1; kind 2 requires it).
 * md_off != NULL (phip_env_step, phip_env_step_eval; cat != 0): the multi-discrete policy's D + 1 offsets — kind
 * 1 reads columns 0 … D−1 as D indices (rollout.hip) */
#define PHIP_ENV_STATE(S) ((S) > 5 ? (S) : 5)
void phip_rollout_rows(int* rows, int E, int T);             /* rows[t·E + e] = e·T + t */
void phip_env_reset(int kind, float* env_state, float* state, int E, int T, int S, uint64_t seed);
void phip_env_first_obs(int kind, const float* env_state, float* state, int E, int T, int S);
void phip_sample_rows(const float* mu, const float* log_std, const int* rows, float* action, float* logprob, int E,
                      int A, uint64_t seed, uint64_t step);
/* cont (may be NULL) [E], written at t = T − 1: 1 when the environment was not reset after that step — the next
 * rollout's first observation continues the episode — 0 otherwise.  t addresses the row and ends the segment;
 * step, the same global counter phip_sample_rows takes, is the position in the env and reset streams (rng.h).
 * Au (phip_env_step, phip_env_step_eval): the action columns in use — A, or A / 2 under the state-dependent-σ
 * Gaussian, whose rows hold zeros after them: kind 0 then takes A = 2 and reads column 0, kind 1 reads column
 * j mod Au and averages the action term over Au columns */
void phip_env_step(int kind, float* env_state, float* state, const float* action, float* next_state, float* reward,
                   uint8_t* term, uint8_t* trunc, uint8_t* cont, int E, int T, int t, uint64_t step, int S, int A,
                   uint64_t seed, int cat, const int* md_off, int D, int Au);
/* the evaluation's step (ppo_eval_device): the same dynamics (shared __device__ functions) over compact arrays —
 * obs [E, S] is the current observation, read and replaced in place, action [E, A]; reward / term / trunc are
 * written at row e·T + t and cont as phip_env_step writes them; nothing else is kept */
void phip_env_step_eval(int kind, float* env_state, float* obs, const float* action, float* reward, uint8_t* term,
                        uint8_t* trunc, uint8_t* cont, int E, int T, int t, uint64_t step, int S, int A,
                        uint64_t seed, int cat, const int* md_off, int D, int Au);
/* the dense step (ppo_env_step_device): the same dynamics again over [E, ·] arrays the caller owns — action in;
 * the transition's next observation, the observation the next step starts from (the reset one where the episode
 * ended), reward, terminated and the environment's own TimeLimit out.  No segment end, no cont */
void phip_env_step_dense(int kind, float* env_state, const float* action, float* next_obs, float* obs_after,
                         float* reward, uint8_t* term, uint8_t* trunc, int E, uint64_t step, int S, int A,
                         uint64_t seed, int cat);
/* the open rollout (ppo_rollout_begin … _end): ro_kind of a rollout whose environment the caller steps */
#define PHIP_ENV_EXTERNAL 3
void phip_action_rows_out(const float* action, const int* rows, float* dense, int E, int A);  /* dense[e] = action[rows[e]] */
/* one external step into buffer row e·T + t by the store rule of ppo_ext.h; obs_after may be NULL (= next_obs);
 * cur [E, S] ← the observation the next step starts from; cont [E] written at t = T − 1 */
void phip_ext_store(const float* next_obs, const float* obs_after, const float* reward_in, const uint8_t* term_in,
                    const uint8_t* trunc_in, float* state, float* next_state, float* reward, uint8_t* term,
                    uint8_t* trunc, uint8_t* cont, float* cur, int E, int T, int t, int S);

/* ---------------- episode statistics (episode.hip) ---------------- */
/* The scan of ppo_ext.h ppo_episode_scan_device plus its fold, two launches: E segments of T rows, cont (may be
 * NULL) [E]; state_in (NULL: fresh) and state_out (NULL: not written) [E][4] doubles, may be the same array;
 * row_ret / row_disc (may be NULL) [E·T]; out [8] ← the batch aggregate (PPO_EP_NBATCH doubles) and, at [7], the
 * number of environments left mid-episode; window (may be NULL) [8] ← window ⊕ batch, [7] ← out[7]. */
void phip_episode_scan(const float* reward, const uint8_t* term, const uint8_t* trunc, const uint8_t* cont, int E,
                       int T, float gamma, const double* state_in, double* state_out, double* row_ret,
                       double* row_disc, double* out, double* window);
void phip_mean_action(const float* mu, float* action, long n);      /* action[0:n] ← mu[0:n], bit for bit */

/* ---------------- per-minibatch advantage normalisation (advnorm.hip) ---------------- */
/* The map of advnorm.h over n_seg segments of B floats, one launch, one 256-thread workgroup per segment: segment s
 * is in[s·B, (s+1)·B) → out likewise (out == in is legal; any other overlap is not); stats (may be NULL)
 * [n_seg][2] ← (m, sd).  n_seg <= 2^31 − 1. */
void phip_adv_normalize(const float* in, float* out, long n_seg, int B, float* stats);

/* ---------------- single-workgroup update phase for small networks (tiny.hip) ---------------- */
typedef struct {
    int L;                          /* linear layers (≤ 8) */
    int sizes[9];                   /* widths (≤ 128; output ≤ 32) */
    int relu[8];
    long woff[8], boff[8];          /* offsets of W_l / b_l in params / grads */
    float *params, *grads, *m, *v;  /* flat parameter / gradient buffers, the network's Adam moments */
    long span;                      /* floats the network's Adam updates */
    float *log_std, *log_std_grad, *m_ls, *v_ls;   /* policy: log σ and its Adam (entropy) state */
    float* wt; long wt_cap;         /* scratch for the transposed weights (Σ in·out floats) */
} PhipTinyNet;
typedef struct {
    int policy;                     /* 0 = value epochs (MSE), 1 = policy epochs (clipped surrogate) */
    const float *state, *action, *logprob, *adv, *adv_target;   /* device buffer arrays */
    int limit, B, num_batches, n_epochs;        /* n_epochs ≤ 16 */
    long max_steps;                 /* ≤ 0: every step of the n_epochs; else the first max_steps */
    const int* perms;               /* [n_epochs][limit] permutations, or NULL: device Feistel */
    uint32_t feistel_k[64];         /* per epoch, 4 round keys (when perms == NULL) */
    const float *steps, *steps_ls;  /* device [n_steps][2] = {lr/bc1, bc2} per Adam step */
    float b1, b2, eps, ent_coeff;
    float* stats;                   /* device [0] Σ value loss, [1] Σ policy loss */
} PhipTinyPhase;
/* runs every minibatch step of the phase in one workgroup; returns −1 (nothing launched) when the
 * network or minibatch does not fit */
int phip_tiny_update(const PhipTinyNet* net, const PhipTinyPhase* ph);
/* the same phase for S → 256 → 256 → O networks (S ≤ 20, O ≤ 16) at B = 64 on 8 cooperating
 * workgroups (cluster.hip; net->wt unused); −1 when it does not fit, −2 after an earlier timeout */
int phip_cluster_update(const PhipTinyNet* net, const PhipTinyPhase* ph);
int phip_cluster_error(void);          /* nonzero: a cluster barrier timed out */
void phip_cluster_report(void);        /* PPO_CLUSTER_STAMPS: print the joined phases' sub-phase means */
/* S → 512 → 512 → 512 → O (S ≤ 380, S % 4 = 0, O ≤ 20) at B = 64 on 32 cooperating workgroups
 * (cluster_deep.hip); phip_cluster_update dispatches 4-layer networks here */
int phip_cluster_deep_update(const PhipTinyNet* net, const PhipTinyPhase* ph);
unsigned* phip_cluster_err_dev(void);  /* device pointer of the shared error word (NULL: already set) */

/* ---------------- element-wise / heads (kernels.hip) ---------------- */
void phip_relu(float* x, long count);
void phip_relu_bwd(const float* y, float* g, long count);
/* x ← tanhf(x); g ← g − (g·y)·y with y the post-activation (tanh′ = 1 − y²) */
void phip_tanh(float* x, long count);
void phip_tanh_bwd(const float* y, float* g, long count);
/* y += x (host-pointer API: the reference's CPU backward accumulates, mat_mul.cu:67,79) */
void phip_axpy(float* y, const float* x, long count);
/* d_loss[0] = Σ(t−y)²/count (written), d_loss_accum[0] += same (if non-NULL);
 * grad = 2(y−t)/count (if non-NULL).  loss.cu:25-83 fused, no host sync. */
void phip_mse(const float* y, const float* t, long count, float* grad, float* d_loss, float* d_loss_accum);
/* the same kernel as the update's plain value head: value-loss clipping per vc (NULL: off), the loss into
 * d_loss_accum only */
void phip_mse_vclip(const float* y, const float* t, long count, float* grad, float* d_loss_accum, const PhipVClip* vc);
/* the folded value head (kernels.hip): y = Σ ypart slots + b, loss += Σ(t−y)²/m, g = 2(y−t)/m, gb += Σ g;
 * and Ws = diag(w)·W for the hidden layer's grad_x (W [l][n], w [l]) */
void phip_value_head(const float* ypart, int slots, const float* b, const float* tgt, int m, float* y, float* g,
                     float* gb, float* d_loss_accum, const PhipVClip* vc);
/* out_head.hip: output layer forward + loss head + output-layer backward in one pass (ppo_update;
 * head 0 = value, A = 1, MSE against tgt; 1 = policy, clipped surrogate); gW / gb / grad_log_std
 * accumulated into zeroed outputs, loss into loss_accum; widths 64…1024, A ∈ {1, 6}; bf16 != 0:
 * x, W and gx stored bf16 (bf16 compute mode, value head); vc: the value head's loss clipping (NULL: off) */
int  phip_out_head_supported(int head, int n, int A);
/* gemm.hip: 1 when ppo_gemm_tune(·, 1) asked for atomic-free (deterministic) gradient products */
int  phip_gemm_deterministic(void);
/* out_head.hip: the backward of a wide output layer (A = 17, n = 512 / 256, fp32) in one pass over the
 * rows — gx = (g·W) ⊙ 1[x > 0] (relu_in) and gW = gᵀ·x, gb = Σ g through per-workgroup partials;
 * gb must follow gW in memory (the flat gradient layout); returns 0 when the shape is not taken */
/* 1 when the wide pass takes (m rows, width n, A outputs; head: the fused policy head too) */
int  phip_out_bwd_wide_ok(int m, int n, int A, int head);
int  phip_out_bwd_wide(float* gW, float* gb, float* gx, const float* g, const float* x, const float* W, int relu_in,
                       int m, int n, int A);
/* the same pass with the policy head (kernels.hip policy_head_tiled_kernel's arithmetic) computed from μ
 * first: ∂/∂log σ (+ −c_ent) and the loss accumulated into grad_log_std / loss_accum (atomics) */
int  phip_policy_out_fused(const float* x, const float* W, const float* b, float* mu, const float* log_std,
                           const float* action, const float* adv, const float* old_lp, float eps, float ent_coeff,
                           float* grad_log_std, float* loss_accum, int relu_in, float* gW, float* gb, float* gx,
                           int m, int n, int A);
int  phip_policy_head_bwd_wide(const float* mu, const float* log_std, const float* action, const float* adv,
                               const float* old_lp, float eps, float ent_coeff, float* grad_log_std,
                               float* loss_accum, const float* x, const float* W, int relu_in, float* gW, float* gb,
                               float* gx, int m, int n, int A);
void phip_out_head(int head, int bf16, const void* x, int relu_in, const void* W, const float* b, int m, int n,
                   int A, const float* tgt, const float* log_std, const float* action, const float* adv,
                   const float* old_lp, float eps, float ent_coeff, float* y, void* gx, float* gW, float* gb,
                   float* grad_log_std, float* loss_accum, const PhipVClip* vc);
void phip_log_prob(const float* mu, const float* log_std, const float* action, float* out, int m, int A);
void phip_log_prob_bwd(const float* mu, const float* log_std, const float* action, const float* grad_in,
                       float* grad_mu, float* grad_log_std, int m, int A);
/* d_out[0] = A·½(1+log 2π) + Σ log_std */
void phip_entropy(const float* log_std, int A, float* d_out);
/* clipped surrogate (ppo.cu:82-107): grad_lp[i], d_loss[0] = loss incl. −c·H (H from d_entropy) */
void phip_policy_loss(const float* adv, const float* lp, const float* old_lp, float* grad_lp, int m,
                      float epsilon, float ent_coeff, const float* d_entropy, float* d_loss, float* d_loss_accum);
/* fused policy head for the update: log-prob, ratio/clip, grad_lp, grad_mu, grad_log_std
 * (+ −ent_coeff, ppo.cu:436-438); loss accumulated into d_loss_accum; ls_zeroed: grad_log_std
 * already holds zeros (cleared by the previous entropy Adam step), else it is cleared first. */
void phip_policy_head(const float* mu, const float* log_std, const float* action, const float* adv,
                      const float* old_lp, int m, int A, float epsilon, float ent_coeff,
                      float* grad_mu, float* grad_log_std, float* d_loss_accum,
                      int ls_zeroed);

/* ---------------- categorical policy: the unmasked head (categorical.hip) ---------------- */
#define PHIP_CAT_MAX_A 4096
/* the clipped-surrogate head over logits [m, A] (2 <= A <= PHIP_CAT_MAX_A), the chosen index in column 0 of
 * action [m, A]: grad [m, A] = ∂loss/∂logits written, lp_out / ent_out (may be NULL) [m] = the row's log-prob /
 * entropy written, d_loss_accum (may be NULL) += −Σ surrogate/m − ent_coeff·Σ H/m, d_ent_accum (may be NULL)
 * += Σ H (both one floating-point atomic per workgroup).  One launch; log σ is not involved. */
void phip_cat_head(const float* logits, const float* action, const float* adv, const float* old_lp, int m, int A,
                   float epsilon, float ent_coeff, float* grad, float* lp_out, float* ent_out, float* d_loss_accum,
                   float* d_ent_accum);

/* ---------------- discrete policies, masked or not: tile head, sampler, greedy action (discrete.hip) ---------- */
#define PHIP_MD_MAX_D 256
/* D softmaxes side by side over logits [m, A]: component d owns [d_off[d], d_off[d + 1]), d_off (device, D + 1
 * ints) ascending from 0 to A, every width >= 2; max_n the widest component (the launcher's choice of form).  The
 * chosen indices are columns 0 … D−1 of action [m, A].  The categorical policy is D = 1, d_off = {0, A}.
 * A row's mask is W = (A + 31) / 32 words, bit k & 31 of word k >> 5 = logit column k allowed (ppo_math.h "Action
 * masking": a component with no stored bit set is fully allowed; the head also allows the chosen column).  mask NULL
 * selects the unmasked kernels; a full mask gives their bits.
 * The head: outputs as phip_cat_head's, lp / ent the joint ones.  With a mask, minibatch row i reads its W words at
 * mask[rows[i]·W] (rows NULL: i; unread without a mask); a masked column's gradient is +0 and its logit never read
 * into arithmetic. */
void phip_disc_head(const float* logits, const float* action, const float* adv, const float* old_lp,
                    const uint32_t* mask, const int* rows, int m, int A, const int* d_off, int D, int max_n,
                    float epsilon, float ent_coeff, float* grad, float* lp_out, float* ent_out, float* d_loss_accum,
                    float* d_ent_accum);
/* component d of row e from u01 of word d & 3 of philox(e | (d >> 2) << 32, offset, key), inverse CDF over the
 * allowed columns of the dense mask [m, W] (row e of the mask for row e of the logits; NULL: every column); the
 * action row (indices in columns 0 … D−1, zeros after) and the joint log-prob (may be NULL) go to row rows[e] (rows
 * NULL: e); mask_out (may be NULL; needs a mask): row rows[e]'s W words ← the mask sampled under */
void phip_disc_sample(const float* logits, const uint32_t* mask, const int* rows, const int* d_off, float* action,
                      float* logprob, uint32_t* mask_out, int m, int A, int D, uint64_t key, uint64_t offset);
/* the rollout's form, as phip_sample_rows: the "policy noise" stream at the global step counter `step` */
void phip_disc_sample_rows(const float* logits, const uint32_t* mask, const int* rows, const int* d_off, float* action,
                           float* logprob, uint32_t* mask_out, int E, int A, int D, uint64_t key, uint64_t step);
/* action[e] ← per component the lowest allowed index holding the maximum over the allowed columns, in columns
 * 0 … D−1, zeros after; mask dense [m, W] (NULL: every column) */
void phip_disc_argmax(const float* logits, const uint32_t* mask, const int* d_off, float* action, int m, int A,
                      int D);
/* mask[rows[e]·W + j] ← all ones for e < E: the rows a step laid with the unmasked sampler */
void phip_mask_fill_rows(uint32_t* mask, const int* rows, int E, int A);

/* ---------------- state-dependent-σ Gaussian policy: head and sampler (gauss_sd.hip) ---------------- */
#define PHIP_SD_MAX_AA 32
#define PHIP_SD_PARTS 1024
/* the head's record: zero-initialised (phip_malloc); the caller clears everything ahead of `ticket` before a launch,
 * the kernel leaves the ticket at zero again */
typedef struct {
    double loss;                    /* −Σ surrogate/m − ent_coeff·Σ H/m of the last launch */
    double ent_sum;                 /* Σ of its row entropies */
    unsigned long long counts[2];   /* [0] clamped log-σ elements, [1] elements m·Aa of the last launch */
    unsigned ticket;
    unsigned pad;
    double partial[2 * PHIP_SD_PARTS];
} PhipSdRec;
int phip_sd_shape_ok(int A);        /* A even, 1 <= A / 2 <= PHIP_SD_MAX_AA */
/* the clipped-surrogate head over z [m, A]: columns 0 … Aa−1 the mean, Aa … A−1 the raw log σ, clamped to
 * [ls_min, ls_max] on read (ppo_math.h sd_*); the action in columns 0 … Aa−1 of action [m, A].  grad [m, A] =
 * ∂loss/∂z written (a clamped log-σ column: +0), lp_out / ent_out (may be NULL) [m] = the row's log-prob / entropy.
 * rec: loss, Σ H and the two counters of this launch; d_loss_accum (may be NULL) += (float)loss by one thread.
 * One launch, deterministic: no floating-point atomics, grid a function of m, no host read. */
void phip_sd_head(const float* z, const float* action, const float* adv, const float* old_lp, int m, int A,
                  float ls_min, float ls_max, float epsilon, float ent_coeff, float* grad, float* lp_out,
                  float* ent_out, PhipSdRec* rec, float* d_loss_accum);
/* a_j = μ_j + normal_at(e·Aa + j, offset, key)·expf(ls_j) for row e of z; the action row (zeros in columns Aa … A−1)
 * and the log-prob (may be NULL) go to row rows[e] (rows NULL: e) */
void phip_sd_sample(const float* z, const int* rows, float* action, float* logprob, int m, int A, float ls_min,
                    float ls_max, uint64_t key, uint64_t offset);
/* the rollout's form, as phip_sample_rows: the "policy noise" stream at the global step counter `step` */
void phip_sd_sample_rows(const float* z, const int* rows, float* action, float* logprob, int E, int A, float ls_min,
                         float ls_max, uint64_t key, uint64_t step);
/* the deterministic action: action [m, A] ← the mean half, zeros after it */
void phip_sd_mean(const float* z, float* action, int m, int A);

/* ---------------- GAE + normalisation (gae.hip) ---------------- */
/* advantages and targets by an exact segmented reverse scan; d_welford[0..2] =
 * (n, mean, M2) in double for this shard.  Then normalise with the (global)
 * statistics held in d_welford. */
void phip_gae_scan(const float* v, const float* v_next, const float* reward, const uint8_t* term,
                   const uint8_t* trunc, int n, float gamma, float lambda, float* adv, float* adv_target,
                   double* d_welford);
/* vn[t] = v[t+1] wherever next_state[t] == state[t+1] bit for bit; every other t is written to
 * own[0, count) (any order).  Returns count (synchronises). */
int phip_next_value_map(const float* next_state, const float* state, const float* v, float* vn, int* own, int n,
                        int S);
/* vn[own[i]] = vals[i] */
void phip_scatter_values(float* vn, const int* own, const float* vals, int m);
/* d_welford_all holds `world` triples; combine them into d_welford (3 doubles) */
void phip_welford_combine(const double* d_welford_all, int world, double* d_welford);
/* adv = (adv − mean)/(σ_pop + 1e-8); d_stats_out (optional) = {mean, std} as float */
void phip_normalize(float* adv, int n, const double* d_welford, float* d_stats_out);

/* ---------------- buffer (buffer.hip) ---------------- */
/* minibatch gather: row i ← perm[(offset+i) % limit] (perm != NULL) or
 * feistel((offset+i) % limit, limit, key) (perm == NULL).  Any dst may be NULL. */
/* phip_gather that also (or, with states == NULL, instead of copying states) writes each slot's
 * source row to rows[batch] — for layer 0's fused gather (phip_linear_fwd_gather) */
void phip_gather_rows(const int* perm, uint64_t key, int offset, int limit, int batch, int S, int A,
                      const float* state, const float* action, const float* logprob, const float* advantage,
                      const float* adv_target, float* states, float* actions, float* logprobs, float* advs,
                      float* adv_targets, int* rows);
void phip_gather(const int* perm, uint64_t key, int offset, int limit, int batch, int S, int A,
                 const float* state, const float* action, const float* logprob,
                 const float* advantage, const float* adv_target,
                 float* states, float* actions, float* logprobs, float* advs, float* adv_targets);

/* ---------------- Adam (adam.hip) ---------------- */
/* one flat span: p, g, m, v over n floats, the step's bias corrections 1 − β1^t and 1 − β2^t, the gradient
 * scale; zero_g: g is cleared once read (the next backward accumulates into it without a memset) */
typedef struct {
    float *p, *g, *m, *v;
    long n;
    float bc1, bc2, grad_scale;
    int zero_g;
} PhipAdamSpan;
/* the learning rate: by value, or — d_lr != NULL — read from that device word by the kernel (lr is then unused):
 * step = *d_lr / bc1, the fp32 division the host does for a rate by value, so an equal rate gives equal bits */
typedef struct {
    float lr;
    const float* d_lr;
} PhipAdamRate;
/* ---- launch-free minibatch steps (hipGraph replay with a device step table) ----
 * One minibatch step is captured once as a graph whose per-step arguments — the gather's
 * permutation offset / Feistel round keys and row offset, the Adam step sizes — live in a device
 * table indexed by a device step counter; the network's Adam kernel advances the counter (its last
 * workgroup to finish), so every replay of the same graph performs the next step. */
typedef struct {
    long perm_off;                  /* ≥ 0: host-rand permutation at perm_base + perm_off; −1: Feistel */
    unsigned fk[4];                 /* Feistel round keys of the epoch */
    unsigned fhalf, fmask, fn;      /* Feistel domain (the buffer's limit) */
    int offset;                     /* k·B: the minibatch's first position in the epoch order */
    float step, bc2;                /* the network Adam's lr / (1 − β1^t) and 1 − β2^t */
    float step_ls, bc2_ls;          /* the entropy Adam's (policy log σ) */
} PhipStepArgs;
void phip_step_feistel(PhipStepArgs* s, unsigned long long key, int limit);   /* fills fk / fhalf / fmask / fn */
void phip_gather_rows_tab(const PhipStepArgs* tab, const int* ctr, const int* perm_base, int limit, int batch, int A,
                          const float* action, const float* logprob, const float* advantage,
                          const float* adv_target, float* actions, float* logprobs, float* advs, float* adv_targets,
                          int* rows);
/* which = 0: the network's Adam (step / bc2; advances *ctr); 1: the entropy Adam (step_ls / bc2_ls);
 * span->bc1 / bc2 are unused (the table holds the step's), the span is 16-B aligned */
void phip_adam_flat_tab(const PhipAdamSpan* span, const PhipStepArgs* tab, int* ctr, unsigned* ticket, int which,
                        float beta1, float beta2, unsigned short* w16, long n16);
int  phip_graph_begin(void);                 /* capture the current stream's launches (returns 0 on success) */
void* phip_graph_end(void);                  /* → instantiated executable graph (NULL on failure) */
void phip_graph_launch(void* exec);          /* replay on the current stream */
void phip_graph_destroy(void* exec);
const char* phip_graph_error(void);         /* why the last capture failed (warning text) */
int  phip_capturing(void);                   /* 1 while a capture is open (profiling scopes stay out) */

/* One launch over a span: float4 where p, g, m, v are 16-B aligned (and w16 8-B), else scalar (then without
 * shadow or clear).  w16 != NULL: bf16(p) is also written into w16[0, n16) (bf16 mode's parameter shadow).
 * coef (NULL: off, the arithmetic is g · grad_scale): the device clip coefficient of this step (clip.hip,
 * PhipClipRec.coef) — the gradient is scaled by fl32(grad_scale · *coef).
 * skip (NULL: off): the device stop word of target-KL early stopping (kl.hip, PhipKlRec.stopped) — while
 * *skip != 0 the step is not taken: p, m, v and w16 stay untouched (both spans of the pair), the gradients are
 * still cleared where zero_g asks */
void phip_adam_flat(const PhipAdamSpan* span, PhipAdamRate rate, float beta1, float beta2, unsigned short* w16,
                    long n16, const float* coef, const unsigned* skip);
/* the same for a network span (16-B aligned) plus a small second span (≤ 256 floats, any alignment: the policy
 * step's entropy Adam) with its own rate, in one launch; both rates by value or both through device words */
void phip_adam_flat_pair(const PhipAdamSpan* span, PhipAdamRate rate, const PhipAdamSpan* side_span,
                         PhipAdamRate side_rate, float beta1, float beta2, unsigned short* w16, long n16,
                         const float* coef, const unsigned* skip);
/* multi-tensor: ptrs/lengths are HOST arrays describing device tensors; m/v are flat */
void phip_adam_multi(float* const* params, float* const* grads, const int* lengths, int num_tensors, float* m,
                     float* v, PhipAdamRate rate, float beta1, float beta2, float bias_correction1,
                     float bias_correction2, float grad_scale);

/* ---------------- global gradient-norm clipping (clip.hip) ---------------- */
#define PHIP_CLIP_PARTS 256
/* one per loop (the value and policy loops run concurrently): the result, the ticket and the
 * per-workgroup partials of the norm kernel.  Zero-initialised (phip_malloc); the kernel leaves the
 * ticket at zero again. */
typedef struct {
    double norm;                    /* grad_scale · sqrt(Σ g²) of the last launch (before clipping) */
    float coef;                     /* min(1, max_norm / (norm + 1e-6)) */
    unsigned clipped;               /* launches with coef < 1 since the record was cleared */
    unsigned ticket;
    unsigned pad;
    double partial[PHIP_CLIP_PARTS];
} PhipClipRec;
/* norm and coef of g[0, n) plus side[0, n_side) (n_side may be 0) into rec; one launch, deterministic
 * (no floating-point atomics, grid a function of n), no host read */
void phip_grad_norm(const float* g, long n, const float* side, long n_side, float grad_scale, float max_norm,
                    PhipClipRec* rec);

/* ---------------- target-KL early stopping (kl.hip) ---------------- */
#define PHIP_KL_PARTS 256
#define PHIP_KL_HIST 4096
/* the policy loop's record: zero-initialised (phip_malloc); the sum kernel leaves the ticket at zero again.
 * Everything ahead of `ticket` is the head the host reads at policy-epoch boundaries. */
typedef struct {
    float sums[4];                  /* [0] Σ KL terms, [1] clipped rows of this rank's minibatch (16-B aligned:
                                     * all-reduced under data parallelism), [2] Σ closed-form KL of its rows (zero
                                     * without that estimator), [3] zero */
    float kl, clip_frac;            /* of the last decided step, over the global minibatch */
    unsigned stopped;               /* sticky within one update: the Adam kernels take no step while set */
    unsigned step;                  /* policy steps decided in this update */
    int stop_step;                  /* index of the step that tripped it, −1 if none */
    unsigned applied;               /* steps whose Adam ran, since the record was cleared */
    unsigned ticket;
    unsigned pad;
    double partial[2 * PHIP_KL_PARTS];
    float hist[PHIP_KL_HIST];       /* KL per decided step of the current update (later steps are not recorded) */
    /* the KL-adaptive learning rate (ppo_set_lr_schedule, PPO_LR_ADAPTIVE), behind everything the record held
     * before: with lr_kl == 0 (off) decide() neither reads nor writes anything below */
    float lr;                       /* the policy rate: the policy and entropy Adams read it through a pointer */
    float lr_v;                     /* the value rate under coupling (phip_lr_couple), read by the value Adam */
    float lr_kl, lr_min, lr_max;    /* desired_kl (0: off) and the clamp range */
    unsigned lr_raised, lr_lowered; /* steps that raised / lowered the rate since the counters were cleared */
    unsigned lr_pad;
    float lr_hist[PHIP_KL_HIST];    /* the rate each decided step's Adam used */
    /* the closed-form estimator (ppo_set_kl_estimator, PPO_KL_EXACT), behind everything the record held before: a
     * launch without it neither reads nor writes anything below */
    double partial_x[3 * PHIP_KL_PARTS]; /* its launches' three partials per workgroup (`partial` keeps the two) */
    float hist_other[PHIP_KL_HIST]; /* the estimator that did NOT decide (k3), per decided step */
    float kl_other;                 /* … and of the last decided step */
    unsigned x_pad;
} PhipKlRec;
/* the closed-form estimator's inputs of one launch (by value; NULL at phip_policy_kl: the k3 launch and its bits) */
typedef struct {
    const float* old_dist;          /* the behaviour distribution's A outputs per row: minibatch row i reads
                                     * old_dist[rows[i]·A] (rows NULL: i) — means (Gaussian) or logits (discrete) */
    const float* old_log_std;       /* Gaussian: the behaviour log σ [A]; unread otherwise */
    const int* rows;
    const int* off;                 /* discrete: device offsets (D + 1) of the components, the categorical policy as */
    int D;                          /* {0, A}; NULL: Gaussian */
    int wide;                       /* discrete: some component is wider than 32 — a wave walks each row */
    double* row_kl;                 /* NULL, or [m] ← every row's KL (the test entry) */
} PhipKlExact;
/* Σ (expm1(x) − x) and the clipped-row count of one policy minibatch (x = log-prob − old log-prob, rows of
 * μ [m, A]) into rec->sums; one launch, deterministic (no floating-point atomics, grid a function of m), no
 * host read.  decide_here != 0: the same launch also decides (below) from the local sums */
/* dist: 0 = Gaussian; 1 = categorical — μ holds the logits, column 0 of the action the index, log σ is unread;
 * 2 = multi-discrete — md_off (device, D + 1 offsets) splits the logits, columns 0 … D−1 hold the indices, lp is
 * the joint one (md_off and D are unread otherwise).  mask (NULL: today's path and bits; needs dist 2, the
 * categorical policy passing the offsets {0, A}): minibatch row i reads its (A + 31) / 32 words at mask[rows[i]·W]
 * (rows NULL: i) and lp is the masked joint log-prob (ppo_math.h md_log_prob_row over MaskRow) */
/* ex (NULL: the launch above, bit for bit): the same launch also sums the closed-form KL(old ‖ new) of every row
 * (ppo_math.h kl_gauss_row / kl_cat_row under the launch's mask) into rec->sums[2], a third partial per workgroup
 * through the same tree and ticket; the k3 sum and the clipped count keep their bits.  The decision then takes
 * sums[2] and keeps k3 in hist_other / kl_other.  old_lp NULL (with ex only: the test entry): k3 and the count are
 * skipped and left 0, action is read under a mask alone */
/* dist 3 = the state-dependent-σ Gaussian (gauss_sd.hip): μ holds [mean | raw log σ], sd (host, {ls_min, ls_max};
 * unread otherwise) the clamp, lp is ppo_math.h's sd_row and, with ex, the row KL is sd_kl_row over old_dist's raw
 * rows, clamped on read (old_log_std and off are unread); log σ is unread */
void phip_policy_kl(const float* mu, const float* log_std, const float* action, const float* old_lp, int m, int A,
                    int dist, float eps, float target_kl, long rows_global, int decide_here, PhipKlRec* rec,
                    const int* md_off, int D, const uint32_t* mask, const int* rows, const PhipKlExact* ex,
                    const float* sd);
/* kl = sums[0] / rows_global (exact != 0: sums[2] / rows_global, and kl_other = hist_other[step] = the former),
 * clip_frac = sums[1] / rows_global; stop when kl > 1.5 · target_kl (NaN never
 * stops); hist[step] = kl, step += 1, applied += !stopped.  Under data parallelism it runs after the
 * all-reduce of rec->sums, with rows_global = m · world: every rank must hold the same target_kl setting, so
 * that all ranks issue the same order of collectives */
void phip_kl_decide(PhipKlRec* rec, float target_kl, long rows_global, int exact);
/* rec->lr_v = lr_V · (rec->lr / base) in fp32, one thread (value-rate coupling of the adaptive schedule) */
void phip_lr_couple(PhipKlRec* rec, float lr_V, float base);
/* the host waits for the launches issued so far on the current stream only (an event recorded there) */
void phip_stream_wait(void);

/* ---------------- observation normalisation (obsnorm.hip) ---------------- */
/* A triple is 1 + 2S device doubles {n, mean[S], M2[S]} (M2: the sum of squared deviations per column).
 * triple ← the exact-in-double statistics of x [n, S] (n = 0: the zero triple); deterministic (no
 * floating-point atomics, partials per workgroup folded in a fixed order, shifted sums); two launches */
void phip_obs_stats(const float* x, long n, int S, double* triple);
/* `count` triples (consecutive, rank order; empty ones skipped) combined, then folded into `run` (Chan) */
void phip_obs_fold(const double* triples, int count, int S, double* run);
/* the fp32 affine pair of a running triple: m = (float)mean, r = (float)(1/sqrt(M2/n + 1e-8)); n = 0: (0, 1) */
void phip_obs_affine(const double* run, int S, float* m, float* r);
/* y[0:n] ← clamp((x − m)·r, ±clip) per column (y may be x); run[0] == 0: no clamp; counts (may be NULL):
 * [0] += clamped elements, [1] += n·S (integer atomics) */
void phip_obs_normalize(const float* x, float* y, long n, int S, const float* m, const float* r, float clip,
                        const double* run, unsigned long long* counts);
/* dst[dst_rows[i]] ← the same map of src[src_rows[i]], i < rows (a NULL list: the identity) */
void phip_obs_normalize_rows(const float* src, const int* src_rows, float* dst, const int* dst_rows, int rows, int S,
                             const float* m, const float* r, float clip, const double* run);

/* ---------------- return-based reward normalisation (retnorm.hip) ---------------- */
/* The segmented forward scan of the discounted returns R_i = r_i + g·(k_{i-1}·R_{i-1} + c_i) over reward[0:n]
 * (g = (double)gamma, k = !(term ∨ trunc), double throughout; seg_len > 0: n % seg_len == 0 and row e·seg_len
 * takes c = carry_in[e]; seg_len = 0: no carry, carry_in / cont / carry_out unused) and what follows it, four
 * launches (block aggregates, carry, apply, finish; n = 0: the finish alone), none with a host read:
 * returns (may be NULL) ← the n returns; carry_out (may be NULL; needs cont) [n / seg_len] ← cont[e] ?
 * R_{e·seg_len + seg_len − 1} : 0; batch ← the exact-in-double triple {n, mean, M2} of the returns,
 * deterministic (no floating-point atomics, per-workgroup partials folded in a fixed order); run (may be NULL)
 * ← run ⊕ batch (Chan); scale (may be NULL; needs run) ← (float)(1/sqrt(M2/n + 1e-8)) of run, 1 for n = 0;
 * counts (may be NULL) [2] ← 0 */
void phip_ret_scan(const float* reward, const uint8_t* term, const uint8_t* trunc, long n, float gamma, int seg_len,
                   const double* carry_in, const uint8_t* cont, double* returns, double* carry_out, double* batch,
                   double* run, float* scale, unsigned long long* counts);
/* the finish alone: `count` triples (consecutive, rank order; empty ones skipped; count = 0: none) folded into
 * run, scale (may be NULL) refreshed, counts (may be NULL) cleared */
void phip_ret_fold(const double* triples, int count, double* run, float* scale, unsigned long long* counts);
/* y[0:n] ← clamp(reward·scale[0], ±clip) in fp32 (y may be reward); run[0] == 0: no clamp; counts (may be NULL):
 * [0] += clamped elements, [1] += n (integer atomics) */
void phip_ret_scale(const float* reward, float* y, long n, const float* scale, float clip, const double* run,
                    unsigned long long* counts);

/* ---------------- sampling / synthetic data (sample.hip) ---------------- */
void phip_sample(const float* mu, const float* log_std, float* action, float* logprob, int m, int A,
                 uint64_t seed, uint64_t offset);
/* same with caller-supplied noise ε[m·A] (host rand() Box–Muller in the reference API path) */
void phip_sample_noise(const float* mu, const float* log_std, const float* noise, float* action, float* logprob,
                       int m, int A);
void phip_fill_uniform(float* p, long n, uint64_t seed, float lo, float hi);
void phip_fill_normal(float* p, long n, uint64_t seed, float scale);
void phip_fill_rollout_flags(uint8_t* term, uint8_t* trunc, int n_envs, int horizon, float p_term, uint64_t seed);
/* next_state[t] = state[t+1] inside an env segment when not terminated (else fresh U(−1,1)) */
void phip_link_next_state(float* next_state, const float* state, const uint8_t* term, int n_envs,
                          int horizon, int S, uint64_t seed);

/* ---------------- data parallel (comm.hip, RCCL) ---------------- */
int  phip_comm_world(void);
int  phip_comm_rank(void);
int  phip_comm_min_i32(int v);      /* min over ranks (synchronous); identity at world 1 */
/* a communicator is up (world > 1, the PPO_COMM_SELF one-rank rehearsal, or the loopback) */
int  phip_comm_active(void);
void phip_allreduce_sum_f32(float* d_buf, long n);
/* gradient bucket: queued behind the issuing stream's work, which does not wait for it;
 * phip_allreduce_join() makes the issuing stream wait for every bucket queued so far */
void phip_allreduce_sum_f32_async(float* d_buf, long n);
void phip_allreduce_join(void);
void phip_allgather_f64(const double* d_send, double* d_recv, long n_per_rank);
/* bounded host wait for every libppo stream (PPO_COMM_TIMEOUT_S, RCCL async errors polled): a stall
 * or an RCCL error aborts the communicators and fails loudly, naming `what` */
void phip_comm_wait(const char* what);
/* replica check: this rank's parameter hash into a device word (Σ mix(index, bits) over the spans,
 * indices running on across spans), then an all-gather over ranks, a bounded wait and the comparison —
 * 0 if every rank's hash equals rank 0's, −1 with the differing ranks in msg; own ← this rank's hash */
void phip_param_hash(const float* const* spans, const long* lens, int nspans);
int  phip_comm_check_hash(int gather, unsigned long long* own, char* msg, int cap);   /* gather 0: own only */

/* ---------------- profiling ---------------- */
/* host C wrappers bracket launches: slot = phip_prof_begin(cls, work); ...; phip_prof_end(slot) */
int  phip_prof_begin(int cls, double work);
int  phip_prof_begin_key(int cls, double work, long long key);
void phip_prof_end(int slot);

#ifdef __cplusplus
}
#endif
#endif /* PPO_HIP_H */
