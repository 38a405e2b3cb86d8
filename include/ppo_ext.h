/*
 * ppo_ext.h — libppo exports beyond the reference API (additive only).
 *
 * None of these exist in cube1324/ppo.c; they expose what the MI355X build
 * adds: device selection and error reporting (SURVEY §8b "Errors"), the
 * device-resident PPO update over an already-filled buffer (the hot path of
 * reference ppo.cu:479-539 without the host rollout), the batched sampler,
 * the env-sharded data-parallel communicator (RCCL over xGMI),
 * a seeded synthetic rollout generator and kernel timing.
 */
#ifndef PPO_EXT_H
#define PPO_EXT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* PPO / GaussianPolicy objects are passed as void* so this header stands alone. */

/* ---------------- device & errors ----------------
 * Fatal errors (a failed HIP/RCCL call, a grid-barrier timeout of the B = 64 phases, a replica-check
 * mismatch, a stalled collective past PPO_COMM_TIMEOUT_S) END THE EMBEDDING PROCESS with status 1, as
 * the reference's checks do (cuda_helper.h:4-16, exit(1)) — but through _exit(1): after a device fault
 * the HIP runtime's own teardown can hang, so atexit handlers and buffered stdio of the host language
 * (e.g. Python's) do not run.  libppo prints the message to stderr and records it for ppo_last_error
 * first.  Callers that must decide for themselves use the entry points that return a status
 * (ppo_comm_init, ppo_comm_check_replicas, ppo_set_device, …). */
int         ppo_device_count(void);              /* HIP devices visible (0 without a GPU) */
int         ppo_set_device(int device);          /* 0 on success */
const char* ppo_last_error(void);                /* first HIP/RCCL error recorded, "" if none */
void        ppo_clear_error(void);               /* forget it (after a status-returning call the caller handled) */
void        ppo_synchronize(void);               /* drain libppo's stream */
const char* ppo_build_info(void);                /* offload arch, compiler, kernel list */
/* sizeof of the API structs, for FFI layout checks: Layer, NeuralNetwork,
 * GaussianPolicy, TrajectoryBuffer, Adam, PPO, Env (no GPU needed) */
int         ppo_struct_sizes(long* out, int n);

/* raw device memory helpers (tests, bench) */
void* ppo_dev_alloc(size_t bytes);
void  ppo_dev_free(void* p);
void  ppo_h2d(void* dst, const void* src, size_t bytes);
void  ppo_d2h(void* dst, const void* src, size_t bytes);
void  ppo_d2d(void* dst, const void* src, size_t bytes);
void  ppo_dev_memset(void* dst, int value, size_t bytes);

/* ---------------- data parallel (RCCL) ---------------- */
int  ppo_comm_unique_id(unsigned char* out, int cap);   /* returns id size (128) */
int  ppo_comm_init(int rank, int world, const unsigned char* id);  /* 0 on success */
int  ppo_comm_rank(void);
int  ppo_comm_world(void);
void ppo_comm_finalize(void);
/* sum-all-reduce of n floats in place on libppo's stream (no-op at world 1) */
void ppo_comm_allreduce_f32(float* d_buf, long n);
/* host-synchronous helpers over the communicator (identity at world 1): a barrier (every rank's
 * queued work drained, then one collective), and the max over ranks of a host double */
void   ppo_comm_barrier(void);
double ppo_comm_max_f64(double v);
/* the advantage-statistics combine after the all-gather: `count` device triples (n, mean, M2) in
 * double → one triple (Chan et al. pairwise combine; empty parts skipped).  Synchronises. */
void ppo_welford_combine(const double* d_parts, int count, double* d_out);
/* PPO_COMM_LOOPBACK=k (one process standing in for k ranks, tests): the other ranks' contributions,
 * so rank 0 of a k-rank job whose shards DIFFER runs in one process.  welford: host [(k−1)·3]
 * (n, mean, M2) triples of ranks 1…k−1, delivered by the all-gather after the local one; limits: host
 * [k−1] buffer limits for the empty-shard agreement (min over ranks); either may be NULL.  Returns
 * 0, or −1 outside loopback mode or for count ≠ k − 1. */
int  ppo_comm_loopback_peers(const double* welford, const int* limits, int count);
/* an all-reduce of a span inside [d_local_base, d_local_base + n) adds the peers' values at the same
 * offset from d_peers (device, [k−1][n], rank order) instead of the k-fold identical sum; ≤ 4 spans */
int  ppo_comm_loopback_peer_grads(const float* d_local_base, const float* d_peers, long n);
/* the parameter hashes of ranks 1…k−1 for the replica check (host [k−1]) */
int  ppo_comm_loopback_peer_hash(const unsigned long long* hashes, int count);
void ppo_comm_loopback_clear(void);                      /* forget every registered peer contribution */
/* the gradient all-reduce form in use: "none", "inline: …" (default: one all-reduce per step in each
 * loop's stream, a communicator per loop) or "bucketed: …" (PPO_COMM_ASYNC=1, or after a failed split) */
const char* ppo_comm_mode(void);
/* Replica check (SURVEY §8e "verify with a periodic checksum all-reduce"): every rank hashes its
 * parameters (μ, log σ, V: 64-bit, bit-exact), the hashes are all-gathered and compared.  Returns 0
 * when every rank holds rank 0's parameters, −1 otherwise (ppo_last_error names the ranks).
 * Synchronises (bounded: PPO_COMM_TIMEOUT_S).  ppo_update runs it at world > 1 after every
 * PPO_REPLICA_CHECK-th update (default 1; 0 = off) and ends the process on a mismatch. */
int  ppo_comm_check_replicas(void* ppo);
/* this rank's parameter hash (as the replica check computes it; synchronises) */
unsigned long long ppo_param_hash(void* ppo);

/* ---------------- the PPO update ---------------- */
enum { PPO_SHUFFLE_HOST_RAND = 0,   /* reference shuffle_buffer: swap(i, rand()%N), host rand() */
       PPO_SHUFFLE_DEVICE   = 1 };  /* device Feistel bijection, seeded, no host work */

/* One PPO update over the device-resident buffer (limit = full ? capacity : idx):
 * compute_gae_cuda, then n_epochs_value value epochs and n_epochs_policy policy
 * epochs of ⌊limit/batch_size⌋ minibatches (reference ppo.cu:487-533).  With
 * ppo_comm_world() > 1 every rank holds its own env shard; gradients are
 * all-reduced (mean over the global minibatch) and advantage statistics are
 * global.  Asynchronous: nothing is read back to the host — except after the multi-workgroup
 * B = 64 phases (cluster.hip), which synchronise once at the end to check their grid barriers
 * (a timeout ends the process with status 1: the phase's state is incomplete), and, only while
 * target-KL early stopping is on (ppo_set_target_kl), after the last step of each policy epoch, where the
 * host waits for the policy loop's stream and reads 40 bytes to stop issuing steps the device skips. */
void ppo_update(void* ppo, float gamma, int batch_size, int n_epochs_policy, int n_epochs_value,
                int shuffle_mode, unsigned long long seed);

/* stats accumulated by ppo_update since the last reset (synchronises):
 * out[0]=Σ value loss, out[1]=#value steps, out[2]=Σ policy loss,
 * out[3]=#policy steps, out[4]=entropy, out[5]=advantage mean, out[6]=advantage std,
 * out[7]=rows of the last GAE's own V(next_state) forward (those not reused from V(state[t+1])),
 * out[8]=minibatch steps replayed from captured graphs (PPO_GRAPH=1),
 * out[9] / out[10]=pre-clip gradient norm of the last value / policy step, out[11] / out[12]=value /
 * policy steps whose clip coefficient was < 1 since the last reset (all four 0 while gradient
 * clipping is off; callers passing n <= 9 see no change),
 * out[13]=approximate KL of the last decided policy step, out[14]=its clip fraction, out[15]=policy steps
 * whose Adam ran since the last reset, out[16]=stop step of the last update (−1: none) (all four 0 while
 * target-KL early stopping is off; callers passing n <= 13 see no change),
 * out[17]=Σ clipped rows over the value steps since the last reset, out[18]=Σ rows of those steps (value-loss
 * clipping, ppo_set_value_clip: exact integer counts, under data parallelism THIS RANK's rows; both 0 while it
 * is off; callers passing n <= 17 see no change).  While value-loss clipping is on, out[0] accumulates the
 * clipped loss.
 * out[19]=the observation normaliser's running count, out[20]=elements clamped by the last update's state
 * normalisation (an exact integer: integer atomics only; under data parallelism THIS RANK's rows),
 * out[21]=elements it normalised (limit·S) (observation normalisation, ppo_set_obs_norm: all three 0 while it
 * is off; callers passing n <= 19 see no change).
 * out[22]=the reward normaliser's running count, out[23]=rewards clamped by the last update's scaling (an exact
 * integer: integer atomics only; under data parallelism THIS RANK's rows), out[24]=rewards it scaled (limit)
 * (reward normalisation, ppo_set_reward_norm: all three 0 while it is off; callers passing n <= 22 see no
 * change).
 * out[25]=the policy learning rate in use, out[26]=the value learning rate in use (ppo_get_lr), out[27]=policy steps
 * that raised the rate, out[28]=policy steps that lowered it, both since the last reset (the adaptive schedule,
 * ppo_set_lr_schedule: both 0 under the other schedules; callers passing n <= 25 see no change).
 * out[29]=the advantage-normalisation mode (ppo_set_adv_norm), out[30] / out[31]=the smallest / largest segment sd of
 * the last update's per-minibatch normalisation (NaN if a segment's sd is NaN; under data parallelism THIS RANK's
 * segments) (all three 0 while it is off; callers passing n <= 29 see no change).
 * out[32]=the KL monitor's estimator (ppo_set_kl_estimator; out[13] is the DECIDING estimator's value), out[33]=the
 * other estimator's value of the same step — k3 while the closed-form estimator decides; 0 while the monitor is off
 * and 0 under PPO_KL_K3, which does not evaluate the closed form (callers passing n <= 32 see no change).
 * With the categorical policy (ppo_set_action_dist 1) — or the multi-discrete one, its joint row entropy — out[4] is the
 * mean row entropy of the last policy step's
 * minibatch (Σ H / rows as the head accumulated it; 0 before the first policy step; under data parallelism THIS
 * RANK's rows), not the Gaussian entropy of log σ. */
void ppo_read_stats(void* ppo, double* out, int n);
void ppo_reset_stats(void* ppo);

/* Global gradient-norm clipping (off by default; not in the reference).  With max_norm > 0 and finite,
 * every minibatch step computes on the device, after the gradient all-reduce and before its Adam,
 *     norm = grad_scale · sqrt(Σ g²)              (grad_scale = 1/world: the norm of the mean gradient)
 *     coef = min(1, max_norm / (norm + 1e-6))     (torch.nn.utils.clip_grad_norm_)
 * and Adam scales the gradient by fl32(grad_scale · coef).  A value step sums over V's gradients; a
 * policy step over μ's gradients and the log σ gradient jointly (one optimiser group: the same coef
 * feeds the policy Adam and the entropy Adam).  The norm is deterministic (no floating-point atomics),
 * so replicas stay bit-identical under data parallelism.  While clipping is on, ppo_update runs the
 * multi-launch loop: the single-workgroup / cluster phases (small networks, B = 64) and graph replay do
 * not clip and are not taken.  The setting is not part of a checkpoint (save_ppo's, which keeps the reference's
 * byte layout; ppo_save_state keeps it): set it again after load_ppo.
 * max_norm <= 0 or +inf: off.  Returns 0, or −1 for NaN (setting unchanged). */
int    ppo_set_max_grad_norm(void* ppo, float max_norm);
float  ppo_get_max_grad_norm(void* ppo);                  /* 0 when off */
/* L2 norm of a device span plus an optional second span (d_b may be NULL with nb = 0), by the update's
 * own norm kernel; synchronises */
double ppo_grad_norm_device(const float* d_a, long na, const float* d_b, long nb);

/* Target-KL early stopping (off by default; not in the reference).  While it is on, every policy minibatch
 * step measures on the device, after its forward and before its Adam, with x = log-prob − old log-prob of
 * the minibatch's rows (the log-prob by the loss's own expression),
 *     kl        = mean(expm1(x) − x)               (in double; Schulman's k3 estimator of KL(old ‖ new))
 *     clip_frac = mean(|exp(x) − 1| > epsilon)
 * and stops the policy loop of this update once kl > 1.5 · target_kl (Stable-Baselines3, CleanRL,
 * Spinning Up): the step that tripped it and every later policy step of the update take no Adam step (μ,
 * log σ and both Adams' moments stay; the gradients are still cleared).  A NaN kl never stops.  The value
 * loop is untouched.  The decision is taken on the device, per step; ppo_update synchronises the policy
 * loop's stream after the last step of each policy epoch — only while this feature is on — to stop
 * issuing steps that would be no-ops, and sets the policy and entropy Adams' time_step back by the skipped
 * steps, so they count the steps that were applied.  The sums are deterministic (no floating-point
 * atomics).  Under data parallelism the two sums are all-reduced (one extra 16-byte collective per policy
 * step behind the gradient's, same stream and communicator) and kl is the mean over the global minibatch:
 * EVERY RANK MUST HOLD THE SAME target_kl SETTING, or the ranks issue different sequences of collectives.
 * While it is on, ppo_update runs the multi-launch loop (no single-workgroup / cluster phases, no graph
 * replay), as with gradient clipping, and works together with it.  Not part of a checkpoint (save_ppo's; ppo_save_state keeps it):
 * set it again after load_ppo.
 * target_kl > 0: on; +inf: measure only, never stop; <= 0: off.  Returns 0, or −1 for NaN (unchanged). */
int    ppo_set_target_kl(void* ppo, float target_kl);
float  ppo_get_target_kl(void* ppo);                      /* 0 when off */
/* KL of every decided policy step of the last ppo_update, in step order, into out[0, min(n, steps, 4096));
 * returns the number of decided steps (0 while the feature is off); synchronises */
int    ppo_kl_history(void* ppo, double* out, int n);
/* the update's KL kernel on caller-supplied device arrays: μ [m, A], log σ [A], action [m, A], old log-prob
 * [m] → out2 = {approximate KL, clip fraction}; returns 0, −1 for bad arguments; synchronises */
int    ppo_policy_kl_device(const float* d_mu, const float* d_log_std, const float* d_action, const float* d_old_lp,
                            int m, int A, float eps, double* out2);
/* The KL monitor's estimator (PPO_KL_K3 by default: everything above, bit for bit, nothing allocated or launched).
 * PPO_KL_EXACT: while the monitor runs (a target KL, or the adaptive schedule), the kl that stops the loop, moves the
 * adaptive rate, fills ppo_kl_history and out[13] is the CLOSED-FORM KL(old ‖ new) between the behaviour distribution
 * and the current one, averaged over the minibatch's rows — what rl_games and rsl_rl drive their adaptive rule with:
 * non-negative, free of sampling variance, and defined for every policy here.  Per row, fp32 inputs, double arithmetic
 * (csrc/ppo_math.h, which this quotes), j / k / d ascending:
 *   Gaussian, old (μo, lso), new (μn, lsn), ls = log σ:    d = lso_j − lsn_j
 *       KL = Σ_j (0.5·expm1(2d) − d) + 0.5·(μo_j − μn_j)²·exp(−2·lsn_j)
 *     the textbook diagonal-Gaussian KL in a form that does not cancel near d = 0.  rsl_rl adds 1e-5 inside its log
 *     (log(σn/σo + 1e-5)); libppo does not.
 *   categorical / multi-discrete / masked, per component d over its EFFECTIVE allowed columns only (ppo_set_action_mask's
 *     three rules: the stored bits; none set → all allowed; the chosen column OR-ed in):
 *       lo_k = (zo_k − Mo) − log Σ_k exp(zo_k − Mo),  ln_k likewise from the new logits
 *       s = Σ_k exp(lo_k)·(lo_k − ln_k),   KL_d = s < 0 ? 0 : s (a NaN stays NaN),   KL = Σ_d KL_d
 *     A masked column is read in neither the old nor the new logits: a NaN or 1e30 there changes no output bit.
 * The behaviour distribution needs no rollout plumbing: policy parameters do not change between a rollout and its
 * ppo_update, so at the head of every update (only while PPO_KL_EXACT is set AND the monitor is on) μ is forwarded over
 * state[0, limit) — the normalised shadow while observation normalisation is on — in chunks of at most 16384 rows into
 * a PPO-owned device store [capacity, A] (means or logits; allocated on first use, freed with the PPO), and log σ is
 * snapshotted.  That serves every way of filling the buffer (device and open rollouts, ppo_fill_synthetic, caller-laid
 * rows).  The policy steps' one KL launch then reads the store in place through the step's row indices and sums the
 * row KLs beside k3 and the clip fraction, which keep their bits (no launch added per step, no floating-point
 * atomics).  A chunk's forward may pick another GEMM configuration than a minibatch's, so the first policy step's
 * exact KL is tiny but NEED NOT BE 0.  The store is a function of (parameters, buffer): ppo_save_state keeps the
 * setting alone (files and ppo_state_hash of PPOs that never set it are unchanged), save_ppo nothing.  Under data
 * parallelism the sum rides in the monitor's existing 16-byte all-reduce: no collective is added and the order of
 * collectives does not depend on the setting, but EVERY RANK MUST HOLD THE SAME ESTIMATOR, or the ranks decide from
 * different numbers.  With PPO_KL_EXACT and the monitor off nothing is allocated or launched either.
 * Returns 0, or −1 with the setting unchanged for a NULL ppo or an unknown estimator. */
enum { PPO_KL_K3 = 0, PPO_KL_EXACT = 1 };
int    ppo_set_kl_estimator(void* ppo, int estimator);
int    ppo_get_kl_estimator(void* ppo);                   /* the estimator; 0 for NULL */
/* ppo_kl_history for either estimator: the deciding one's values, or — while PPO_KL_EXACT decides — k3's of the same
 * steps; returns 0 steps for PPO_KL_EXACT while the estimator is PPO_KL_K3 (never evaluated) and for an unknown
 * estimator; synchronises */
int    ppo_kl_history_est(void* ppo, int estimator, double* out, int n);
/* the device store [limit, A] the last ppo_update filled (means or logits by buffer row) and, through d_log_std_old
 * (may be NULL), its log σ snapshot [A] (Gaussian policy); NULL / NULL if no update has filled it */
const float* ppo_kl_old_dist(void* ppo, const float** d_log_std_old);
/* the update's KL launch on caller-supplied device arrays (a test entry): dist 0 = Gaussian (both log σ [A] needed,
 * nvec / D / d_mask unused), 1 = categorical (nvec = {A}), 2 = multi-discrete over nvec[D].  d_new [m, A]; minibatch row
 * i reads d_old[d_rows[i]·A] (d_rows NULL: i) and, under a mask (dist 1 / 2, d_mask not NULL), its (A + 31) / 32 words
 * at d_mask[d_rows[i]·W] as ppo_masked_head_device does; d_action [m, A] is needed only under a mask (rule 3).
 * d_row_kl (may be NULL) [m] ← every row's KL in double; *out_mean = (double)(float)Σ / m, the sum as the record keeps
 * it.  Returns 0, or −1 with nothing launched for bad arguments; synchronises */
int    ppo_policy_kl_exact_device(int dist, const float* d_new, const float* d_log_std_new, const float* d_old,
                                  const float* d_log_std_old, const int* d_rows, const float* d_action,
                                  const uint32_t* d_mask, int m, int A, const int* nvec, int D, double* d_row_kl,
                                  double* out_mean);
/* Per-minibatch advantage normalisation (off by default; not in the reference, whose gae normalises once per update
 * over the whole buffer: A ← (A − μ)/(σ_pop + 1e-8), which libppo keeps doing in every mode; Stable-Baselines3
 * normalize_advantage = True and CleanRL norm_adv = True, both their defaults).  With PPO_ADV_NORM_MINIBATCH every
 * policy minibatch's advantages are normalised again over that minibatch alone before its head reads them.  The
 * definition (csrc/advnorm.h, which this quotes): a segment x_0 … x_{B−1} — the B advantages of one policy
 * minibatch, as GAE's global normalisation left them — becomes
 *     p_t  = Σ_{i ≡ t (mod 256), i ascending} (double)x_i          t = 0 … 255
 *     S    = pairwise tree over p (stride 1, 2, 4 … 128: p_t += p_{t+stride} for t a multiple of 2·stride)
 *     mean = S / B                                                  (double)
 *     q_t, Q likewise over d_i·d_i,  d_i = (double)x_i − mean       (product rounded, then added: no FMA)
 *     sd   = (float)sqrt(Q / max(B − 1, 1))                         (the unbiased std of torch.Tensor.std)
 *     m    = (float)mean
 *     y_i  = (float)((double)(x_i − m) / ((double)sd + 1e-8))       (the form of gae.hip's normalize_kernel)
 * A NaN propagates within its own segment only; a constant segment gives y = 0; B == 1 gives y = 0.  Because the map
 * is invariant under the global affine map GAE applied first, y equals Stable-Baselines3's / CleanRL's
 * (a − a.mean())/(a.std() + 1e-8) of the raw minibatch advantages a up to rounding and the two 1e-8 terms — it is not
 * bit-equal to them.
 * The work is one launch per ppo_update (csrc/advnorm.hip: one 256-thread workgroup per segment, no floating-point
 * atomics, the outputs a function of (B, data) alone), ahead of the value and policy loops, over the copy of the
 * policy phase's advantages the update gathers up front: the trajectory buffer's `advantage` array is never written,
 * and every form of the policy head (fused, wide, plain, categorical, multi-discrete, masked; fp32 on both GEMM
 * engines, bf16 mode) reads the rewritten segment unchanged.  While it is on, ppo_update runs the multi-launch loop
 * (no single-workgroup / cluster phases, no graph replay — they gather for themselves), as with value-loss clipping,
 * and works together with gradient clipping, target KL (segments normalised for steps it leaves unissued are never
 * read), value clipping, both normalisers, the schedules and the step limit.  Under data parallelism each rank
 * normalises its own minibatch shard (CleanRL under DDP does the same): no collective is added, the order of
 * collectives does not depend on the setting, and the replicas stay identical because the gradients are still
 * all-reduced; EVERY RANK SHOULD HOLD THE SAME SETTING, or the ranks train one model on differently scaled
 * advantages.  With the mode global no launch is added, nothing is allocated and every path gives the bits it
 * always gave.  Not part of a checkpoint (save_ppo's; ppo_save_state keeps it): set it again after load_ppo.
 * Returns 0, or −1 (setting unchanged) for a NULL ppo or an unknown mode. */
enum { PPO_ADV_NORM_GLOBAL = 0, PPO_ADV_NORM_MINIBATCH = 1 };
int ppo_set_adv_norm(void* ppo, int mode);
int ppo_get_adv_norm(void* ppo);             /* the mode; 0 for NULL */
/* the update's kernel on caller-supplied device arrays: n_seg segments of B floats, segment s at [s·B, (s+1)·B);
 * d_out may be d_in (no other overlap); d_stats (may be NULL) [n_seg][2] ← (m, sd).  Returns 0, or −1 for a NULL
 * array, n_seg <= 0 (or above 2^31 − 1) or B <= 0; synchronises */
int ppo_adv_normalize_device(const float* d_in, float* d_out, long n_seg, int B, float* d_stats);
/* (m, sd) of every policy segment the last ppo_update normalised, in step order, into out[0, 2·min(n, steps));
 * returns steps — the update's policy steps after ppo_set_step_limit's cap, those target KL left unissued
 * included (0 while the mode is global); synchronises */
int ppo_adv_norm_history(void* ppo, float* out, int n);
/* host copies of policy step `step` of the last ppo_update: its B buffer row indices and the B advantages its head
 * read — normalised while the mode is minibatch, the gathered ones while it is global (rows / adv may be NULL).
 * Returns B, or −1 for a bad step, cap < B, or an update that kept no gather (the single-workgroup / cluster phases,
 * graph replay); synchronises */
int ppo_adv_norm_read(void* ppo, long step, int* rows, float* adv, int cap);

/* Learning-rate schedules (constant by default; not in the reference).  kind picks one; p0 … p2 are its parameters.
 *   PPO_LR_CONSTANT  today's behaviour on today's code path, bit for bit: ppo->lr_policy and ppo->lr_V are read from
 *                    the struct by every update and passed to the Adam kernels by value.  p0 … p2 are ignored.
 *   PPO_LR_LINEAR    linear decay (CleanRL anneal_lr, Stable-Baselines3 linear_schedule).  p0 = total updates N >= 1,
 *                    p1 = final fraction f in [0, 1], p2 unused.  Update number u counts the ppo_update calls since
 *                    the setter, from 0; update u runs with
 *                        lr = (float)((double)base · (1 − (1 − f)·(min(u, N)/N)))   (double, rounded once, on the host;
 *                                                                                    u >= N gives (float)(base·f))
 *                    for base = ppo->lr_policy and base = ppo->lr_V alike, passed by value: no kernel differs, and
 *                    every update path (single-workgroup / cluster phases, graph replay) stays available.
 *   PPO_LR_ADAPTIVE  the KL-adaptive rate of rl_games and rsl_rl (schedule = "adaptive", desired_kl).  p0 = desired_kl
 *                    > 0, p1 = lr_min > 0, p2 = lr_max >= lr_min, all finite.  The policy rate is one fp32 word on
 *                    the device, set by the setter to clamp(ppo->lr_policy, lr_min, lr_max); the struct field is
 *                    the base and is never written.  While the schedule is on, the KL monitor runs exactly as under
 *                    ppo_set_target_kl(ppo, +inf) (a finite target keeps working alongside), and every policy
 *                    minibatch step, once its kl is known and before the stop test, applies in fp32 (IEEE division
 *                    and product):
 *                        if      (kl > 2.0f · desired_kl)               lr = fmaxf(lr_min, lr / 1.5f);   lowered += 1
 *                        else if (kl < 0.5f · desired_kl && kl > 0.0f)  lr = fminf(lr_max, lr · 1.5f);   raised  += 1
 *                    A NaN kl changes nothing; once target-KL early stopping has stopped the update, the rate no
 *                    longer changes.  The step's own policy and entropy Adams read the new word through a pointer
 *                    (step = lr / bias_correction1 computed by the kernel: the fp32 division the host does otherwise,
 *                    so an equal rate gives equal bits); the host never reads the rate inside an epoch.  kl is the
 *                    monitor's estimator (ppo_set_kl_estimator): by default k3 of ppo_set_target_kl above —
 *                    mean(expm1(x) − x) over the minibatch — which is NOT the closed-form KL rsl_rl evaluates, so a
 *                    desired_kl tuned there carries over only roughly; with PPO_KL_EXACT it is that closed-form KL,
 *                    and an rsl_rl desired_kl carries over up to the 1e-5 rsl_rl adds inside its log.
 *                    The value rate stays ppo->lr_V by value unless coupled (below).  As target KL, the schedule
 *                    takes the multi-launch loop (no single-workgroup / cluster phases, no graph replay) and works
 *                    with clipping, both normalisers, the discrete policies and bf16 mode.  Under data parallelism
 *                    the rule runs on the all-reduced sums, so every rank takes the same decision from the same bits
 *                    and no collective is added; EVERY RANK MUST HOLD THE SAME SCHEDULE, and ppo_param_hash /
 *                    ppo_comm_check_replicas cover the two rate words while it is on.
 * The setter restarts the schedule (u = 0, the adaptive rate back at the clamped base, both counters 0).  Not part of a
 * checkpoint (save_ppo's; ppo_save_state keeps the kind, the parameters, the coupling, u, the rate words and the
 * counters): set it again after load_ppo.
 * Returns 0, or −1 with the setting unchanged for an unknown kind, a NaN parameter or a parameter outside the
 * ranges above. */
enum { PPO_LR_CONSTANT = 0, PPO_LR_LINEAR = 1, PPO_LR_ADAPTIVE = 2 };
int  ppo_set_lr_schedule(void* ppo, int kind, float p0, float p1, float p2);
/* returns the kind; out4 (may be NULL) = {p0, p1, p2, couple_value}: p0 … p2 are zeros for the constant schedule,
 * couple_value is the flag as ppo_lr_couple_value left it, whatever the schedule */
int  ppo_get_lr_schedule(void* ppo, float* out4);
/* Value-rate coupling of the adaptive schedule (off by default; without that schedule the flag is kept and unused).
 * The value loop runs beside the policy loop on its own stream, so nothing changes its rate inside an update: with
 * coupling on, one one-thread launch at the start of each ppo_update, ahead of the loops' fork, sets
 *     lr_v = lr_V · (lr / clamp(lr_policy, lr_min, lr_max))          (fp32: one division, one product)
 * from the policy rate as the previous update left it, and the value Adam reads that word for the whole update —
 * deterministic, no cross-stream read.  Returns the previous value, −1 for a NULL ppo. */
int  ppo_lr_couple_value(void* ppo, int on);
/* out2 = {policy lr, value lr} in use now: what an update starting now would pass (constant, linear) or the device
 * words as they stand (adaptive; the value word only under coupling, where it is the last update's).  Returns 0, −1
 * for a NULL argument; synchronises */
int  ppo_get_lr(void* ppo, double* out2);
/* the rate each decided policy step of the last ppo_update ran its Adam with (adaptive schedule), in step order,
 * into out[0, min(n, steps, 4096)); returns the number of decided steps (0 under the other schedules); synchronises */
int  ppo_lr_history(void* ppo, float* out, int n);
/* One adam_update_cuda step of a device Adam with the rate read from the device word d_lr, through the Adam kernels'
 * pointer variants (a test entry: the update calls them through the adaptive schedule).  Returns 0, −1 for a NULL or
 * host Adam or a NULL d_lr */
int  ppo_adam_update_lr_device(void* adam, const float* d_lr);

/* PPO2 value-loss clipping (off by default; not in the reference; baselines PPO2, CleanRL clip_vloss,
 * Stable-Baselines3 clip_range_vf).  For a value minibatch of m rows, with y the network's value of a row, t its
 * target (adv_target), v_old its old value and eps_v > 0 the clip range, every form of the value head (the plain
 * MSE kernel, the fused output layer in fp32 and bf16 storage, the folded head and the head carried by the x3
 * grad_W launch — one device function, csrc/vclip.h) computes in fp32, in this order:
 *     d      = y − v_old
 *     inside = !(|d| > eps_v)                      (NaN counts as inside: it propagates exactly as with clipping off)
 *     lu     = (t − y)²
 *     if inside:      l = lu, g = 2·(y − t)/m      (bit for bit the head with clipping off)
 *     else:  yc = v_old + copysignf(eps_v, d)
 *            lc = (t − yc)²
 *            if lu >= lc:  l = lu, g = 2·(y − t)/m (max() picks the unclipped term; ties go here)
 *            else:         l = lc, g = 0, the row counts as "clipped"
 *     loss = Σ l / m                               (the reference's MSE convention, no ½)
 * — mean(max((y − t)², (v_old + clamp(y − v_old, ±eps_v) − t)²)) with the sub-gradient fixed; an inside row
 * never depends on whether v_old + (y − v_old) rounds back to y.  The gradient stays one scalar per row, and no
 * launch is added to a value step.  While it is on, ppo_update runs the multi-launch loop (no single-workgroup /
 * cluster phases, no graph replay), as with gradient clipping and target-KL early stopping, and works together
 * with both and with data parallelism: the head is element-wise, so no collective is added and the order of
 * collectives does not depend on the setting.  Not part of a checkpoint (save_ppo's; ppo_save_state keeps it): set it
 * again after load_ppo.
 * eps_v > 0 and finite: on; <= 0 or +inf: off.  Returns 0, or −1 for NaN (setting unchanged). */
int    ppo_set_value_clip(void* ppo, float eps_v);
float  ppo_get_value_clip(void* ppo);                     /* 0 when off */
/* The old values.  By default they are the V(state) of every buffer row that the update's own GAE has just
 * computed (with them the first value step of an update has y ≈ v_old, so nothing clips yet).  Callers who
 * stored values at rollout time pass them here: a caller-owned device array indexed by BUFFER ROW, which must
 * stay valid while it is set.  Returns −1 (unchanged) when n is smaller than the buffer capacity; NULL restores
 * the default. */
int    ppo_value_clip_old_values(void* ppo, const float* d_v_old, long n);
/* the update's own head arithmetic (the plain head's kernel) on caller-supplied device arrays: y [m], old values
 * read at d_v_old[d_rows[i]] (d_rows NULL: the identity), targets [m] → d_g [m] = ∂loss/∂y and out3 = {loss,
 * clipped rows, rows}; returns 0, −1 for bad arguments (a NULL array, m <= 0, eps_v not > 0); synchronises */
int    ppo_value_clip_head_device(const float* d_y, const float* d_v_old, const int* d_rows, const float* d_tgt, int m,
                                  float eps_v, float* d_g, double* out3);
/* One form of the clipped-surrogate / Gaussian policy head on caller-supplied device arrays (a test entry: the
 * update never calls it).  The head exists in five forms, all of the same per-row arithmetic:
 *     form 0 "separate"  log_prob_kernel → policy_loss_kernel → log_prob_bwd_kernel (the reference-API kernels); any A
 *     form 1 "head"      phip_policy_head: the tiled kernel for A <= 32, the generic one above; A <= 4096
 *     form 2 "out_head"  phip_out_head(head = 1): output layer + head + its backward; A ∈ {1, 6}, n ∈ {64 … 512}
 *     form 3 "wide"      phip_policy_head_bwd_wide: head + output-layer backward; A = 17, n ∈ {256, 512}
 *     form 4 "fused"     phip_policy_out_fused: output layer + head + its backward; A = 17, n ∈ {256, 512}
 * Inputs: log σ [A], action [m, A], adv [m], old log-prob [m], and μ [m, A] for forms 0, 1 and 3.  Forms 2 and 4
 * compute μ = x·Wᵀ + b from x [m, n], W [A, n], b [A] and WRITE it to d_mu; form 3 reads x and W for its backward
 * (d_b unused).  relu_in != 0 masks gx by x > 0.  Outputs: forms 0 and 1 d_grad_mu [m, A] (and form 0 d_lp [m]);
 * forms 2–4 d_gx [m, n] and d_gW, ONE allocation of A·n + A floats, gW [A, n] followed by gb [A]; every form
 * d_grad_log_std [A] and *loss (the loss word read back).  Forms 1–4 add −ent_coeff to every column of
 * d_grad_log_std (ppo.cu:436-438), form 0's kernels leave that to their host caller, so form 0 returns the bare
 * sum; every form's loss includes −ent_coeff · entropy once.  The entry zeroes what the kernels accumulate into
 * (gW, gb, grad log σ, the loss word), calls the form's phip_* function and synchronises.  Arrays a form does not
 * use may be NULL; x, W, gx and gW must be 16-byte aligned.
 * Returns 0 when the form ran; 1 when the form does not take the shape (by the kernels' own predicates; no
 * kernel was launched); −1 for bad arguments (form outside 0–4, a NULL or misaligned array the form needs,
 * m <= 0, A <= 0, n <= 0 for forms 2–4, NaN eps), with nothing recorded for ppo_last_error. */
int    ppo_policy_head_device(int form, int m, int A, int n, int relu_in, float eps, float ent_coeff,
                              const float* d_log_std, const float* d_action, const float* d_adv,
                              const float* d_old_lp, float* d_mu, const float* d_x, const float* d_W, const float* d_b,
                              float* d_lp, float* d_grad_mu, float* d_gx, float* d_gW, float* d_grad_log_std,
                              double* loss);
/* The action distribution (default 0; not in the reference).  dist 0 is the diagonal Gaussian — today's behaviour,
 * every path bit for bit.  dist 1 is a categorical policy over A = action_size choices: μ's A outputs are the logits
 * z, log σ is unused.  The per-row arithmetic is written once (csrc/ppo_math.h cat_*), fp32, in this order:
 *     M = max_k z_k;  e_k = expf(z_k − M);  s = Σ_k e_k;  lp = (z_a − M) − logf(s);  p_k = e_k / s
 *     H = logf(s) − (Σ_k e_k·(z_k − M)) / s
 *     g = ∂loss/∂lp of the clipped surrogate (the Gaussian head's own function)
 *     ∂loss/∂z_k = g·([k == a] − p_k) + (ent_coeff / m)·p_k·((z_k − M) − logf(s) + H)
 *     loss = −Σ_rows surrogate / m − ent_coeff·(Σ_rows H) / m
 * ACTIONS keep their storage: a row's action stays A floats in the trajectory buffer, column 0 the chosen index as
 * an exact float, columns 1 … A−1 written as 0; no buffer layout, gather or struct changes.  SAMPLING is inverse-CDF
 * from one uniform per row: u = u01(philox(counter, offset, key).x) ∈ (0, 1], c_k = Σ_{j<=k} e_j (fp32, k ascending),
 * a = min{k : u·c_{A−1} <= c_k} (csrc/rng.h lists the streams).  ppo_rollout_device, ppo_eval_device and
 * ppo_fill_synthetic sample this way; ppo_eval_device with deterministic != 0 takes argmax_k z_k, the lowest index
 * on ties.
 * THE UPDATE.  While it is on, a policy step is forward → the categorical head (one launch, csrc/categorical.hip) →
 * backward, and ppo_update runs the multi-launch loop (no single-workgroup / cluster phases, no graph replay, no
 * fused output-layer kernels: those embed the Gaussian head), as with gradient clipping.  It works together with
 * gradient clipping, value-loss clipping, target-KL early stopping (x = lp − old log-prob with the categorical lp),
 * both normalisers, tanh networks, both fp32 GEMM engines and data parallelism: no collective is added and the order
 * of collectives does not depend on the setting.  The head writes no gradient to log σ; the entropy Adam still runs
 * each step, on a zero gradient, which leaves log σ bit-identical.
 * The reference-API entry points that have only a policy or only host data stay Gaussian: sample_action,
 * compute_log_prob*, ppo_sample_action_device, policy_loss_and_grad*, and ppo_policy_kl_device — to act on
 * caller-supplied observations under the PPO's distribution (and its observation normaliser) use ppo_act_device, and
 * to train against a caller-stepped environment the open rollout (ppo_rollout_begin … _end).  The host rollout
 * has no discrete form: train_ppo_epoch / eval_ppo END THE PROCESS with a message while it is on.
 * The setting lives with the PPO, not in GaussianPolicy (whose layout is the reference's).  Not part of a
 * checkpoint (save_ppo's; ppo_save_state keeps it): set it again after load_ppo.
 * Returns 0, or −1 with the setting unchanged for an unknown dist, and for dist 1 with A < 2, A > 4096 or bf16
 * compute mode (ppo_set_compute_dtype(ppo, 1) in turn returns −1 while dist is 1).  nn_set_compute_dtype called on
 * the policy network itself has no handle to the PPO and is not declined: ppo_update ENDS THE PROCESS with a message
 * when it finds a categorical policy whose μ is in bf16 mode. */
int    ppo_set_action_dist(void* ppo, int dist);
int    ppo_get_action_dist(void* ppo);                    /* 0 for a NULL ppo */
/* The categorical head on caller-supplied device arrays (a test entry: the update calls the same launcher):
 * logits [m, A], action [m, A] (column 0 the index), adv [m], old log-prob [m] → d_grad [m, A] = ∂loss/∂logits,
 * d_lp [m], d_ent [m] = the row entropies, *loss.  2 <= A <= 4096.  Synchronises.  Returns 0, or −1 for bad
 * arguments (a NULL array, m <= 0, A out of range, NaN eps) with nothing recorded for ppo_last_error. */
int    ppo_categorical_head_device(const float* d_logits, const float* d_action, const float* d_adv,
                                   const float* d_old_lp, int m, int A, float eps, float ent_coeff, float* d_grad,
                                   float* d_lp, float* d_ent, double* loss);
/* The categorical sampler on caller-supplied device arrays: logits [m, A], row i's uniform from
 * philox(i, offset, key).x → d_action [m, A] (index, 0, …, 0) and d_log_prob [m].  Synchronises.  Returns 0, or −1
 * for bad arguments, as above. */
int    ppo_categorical_sample_device(const float* d_logits, int m, int A, unsigned long long key,
                                     unsigned long long offset, float* d_action, float* d_log_prob);
/* The multi-discrete policy (off by default; not in the reference; gymnasium's MultiDiscrete space): a step's action
 * is D independent choices, and μ's A = action_size outputs are D softmaxes side by side.  nvec = (n_0 … n_{D−1})
 * with every n_d >= 2, Σ n_d == A, 2 <= A <= 4096 and 1 <= D <= PPO_MD_MAX_D; component d owns the logits
 * [o_d, o_d + n_d), o_d = Σ_{j<d} n_j.  It is action distribution 2 and generalises dist 1, which is the case D = 1.
 * A row's stored action stays A floats: columns 0 … D−1 hold the chosen indices a_d ∈ [0, n_d) as exact floats,
 * columns D … A−1 are written as +0; reads clamp into [0, n_d).  Per row, fp32, in this order (csrc/ppo_math.h):
 *     per component d: M_d, e_k, s_d, t_d, ls_d = logf(s_d), lp_d = (z_{o_d + a_d} − M_d) − ls_d, H_d = ls_d − t_d / s_d
 *     lp = ((lp_0 + lp_1) + lp_2) + …     H = ((H_0 + H_1) + H_2) + …        d ascending
 *     g  = ∂loss/∂lp of the clipped surrogate on the JOINT lp (one ratio per row)
 *     ∂loss/∂z_k, k in component d = g·([k == o_d + a_d] − p_k) + (ent_coeff / m)·p_k·((z_k − M_d) − ls_d + H_d)
 *     loss = −Σ_rows surrogate / m − ent_coeff·(Σ_rows H) / m
 * The entropy term of a logit's gradient takes its own component's H_d (∂H/∂z_k = ∂H_d/∂z_k).  A component with
 * n_d <= 32 is summed k ascending by one lane, a wider one by lane partials combined in a fixed tree, so a row's
 * outputs are bit-reproducible; with nvec = {A}, A <= 32, lp, H and every gradient element are dist 1's bits.
 * SAMPLING draws one uniform per (row, component): component d of row e takes u01 of word d & 3 (.x .y .z .w) of
 * philox(e | ((uint64)(d >> 2) << 32), offset, key), key and offset exactly those dist 1 uses at each call site, and
 * inverts its own CDF as dist 1 does; d = 0 is dist 1's draw, so D = 1 samples what dist 1 samples bit for bit.  The
 * stored log-prob is the joint lp.  The deterministic action is the per-component argmax, lowest index on ties.
 * While it is on: ppo_get_action_dist returns 2; everything said of dist 1 above holds — the multi-launch update loop
 * with the multi-discrete head (one launch, csrc/discrete.hip), the KL monitor on the joint lp, ppo_read_stats
 * out[4] = the mean joint row entropy, ppo_rollout_device / ppo_eval_device / ppo_fill_synthetic / the open rollout /
 * ppo_act_device, the options it composes with, the entry points that stay Gaussian, train_ppo_epoch / eval_ppo ending
 * the process.  The synthetic environment reads component d = j mod D for observation element j as
 * c_d = 2·a_d/(n_d − 1) − 1, its reward's action term is −0.01·(Σ_d c_d²)/D; CartPole-v1 accepts nvec = {2} and then
 * fills the buffers dist 1 fills.  ppo_env_step_device keeps its Gaussian and dist-1 forms only; invalid
 * actions are masked with ppo_set_action_mask (below).  ppo_set_action_dist(ppo, 0 | 1) switches away from it; ppo_set_action_dist(ppo, 2) returns −1 (it
 * has no nvec).  Not part of a checkpoint (save_ppo's; ppo_save_state keeps it): set it again after load_ppo.
 * ppo_set_action_multidiscrete returns 0, or −1 with the setting unchanged for a NULL argument, D out of range, an
 * n_d < 2, Σ n_d != A, A > 4096 or bf16 compute mode (ppo_set_compute_dtype(ppo, 1) returns −1 while it is on).
 * ppo_get_action_nvec returns D (0 unless the distribution is 2) and fills min(D, cap) entries of out. */
#define PPO_MD_MAX_D 256
int    ppo_set_action_multidiscrete(void* ppo, const int* nvec, int D);
int    ppo_get_action_nvec(void* ppo, int* out, int cap);
/* The multi-discrete head and sampler on caller-supplied device arrays (test entries: the update and the rollouts
 * call the same launchers), as their categorical counterparts above; nvec is a HOST array of D widths summing to A.
 * d_lp / d_ent [m] are the joint log-prob and entropy.  They synchronise.  Return 0, or −1 for bad arguments (a NULL
 * array, m <= 0, an nvec the setter would decline, NaN eps) with nothing recorded for ppo_last_error. */
int    ppo_multidiscrete_head_device(const float* d_logits, const float* d_action, const float* d_adv,
                                     const float* d_old_lp, int m, int A, const int* nvec, int D, float eps,
                                     float ent_coeff, float* d_grad, float* d_lp, float* d_ent, double* loss);
int    ppo_multidiscrete_sample_device(const float* d_logits, int m, int A, const int* nvec, int D,
                                       unsigned long long key, unsigned long long offset, float* d_action,
                                       float* d_log_prob);
/* INVALID-ACTION MASKING for the categorical and the multi-discrete policy (off by default; not in the reference;
 * Stable-Baselines3-contrib MaskablePPO, CleanRL ppo_*_mask): state-dependent illegal actions are taken out of the
 * softmax everywhere it is evaluated — the head (log-prob, entropy, gradient), the sampler, the greedy action and the
 * target-KL monitor — and the mask is stored per transition, so the update sees the distribution the rollout sampled
 * from.  The definition (csrc/ppo_math.h "Action masking"):
 * MASK STORAGE.  A row's mask is W = (A + 31) / 32 uint32 words; bit k & 31 of word k >> 5 set = logit column k is
 * allowed, k the column in the row of A logits counted across the components; bits at k >= A are ignored.
 * EFFECTIVE MASK of component d (columns [o_d, o_d + n_d); d = 0, n_0 = A for dist 1), in this order: 1. its stored
 * bits; 2. none of them set: the component reads as fully allowed — nothing is NaN, nothing aborts; 3. only where a
 * chosen action exists (head, KL): the chosen column is OR-ed in, so a caller-filled buffer whose action contradicts
 * its mask still gives a finite log-prob.
 * ARITHMETIC.  Per component, fp32, k ascending over the allowed columns only: M_d = max z_k, e_k = expf(z_k − M_d),
 * s_d = Σ e_k, t_d = Σ e_k·(z_k − M_d); ls_d, lp_d, H_d, the joint lp and H, the surrogate on the joint ratio, the
 * gradient of an allowed column and the loss exactly as above.  A masked column contributes to no max and no sum, its
 * gradient element is written as +0 and its logit is never read into arithmetic: a NaN, an infinity or 1e30 there
 * changes no output bit.  With every bit set, lp, H and the gradient are the unmasked multi-discrete head's bits for
 * the same nvec; masked dist 1 is masked dist 2 with nvec = {A} (for A <= 32 also the categorical head's bits).
 * SAMPLING inverts the CDF over the allowed columns only — c accumulates e_k over allowed k ascending, the action is
 * the first allowed k with u·s_d <= c, the fallback the last allowed k — with the same Philox word per (row,
 * component) as without masking: under a full mask it draws the unmasked action and log-prob bit for bit.  The greedy
 * action is the lowest allowed index holding the maximum over the allowed columns.
 * ppo_set_action_mask(ppo, on): on allocates a PPO-owned device store of capacity × W words, every bit set, freed
 * with the PPO (or when turned off); row r's words are at r·W.  Returns 0, or −1 with the setting unchanged for a
 * NULL ppo or while the distribution is Gaussian; ppo_set_action_dist(ppo, 0) turns it off, and changing the
 * distribution or nvec through the setters sets every bit of the store again.  ppo_action_mask_words returns W (0 for
 * a NULL ppo), ppo_action_mask_buffer the device store — NULL while masking is off — for callers who lay the buffer
 * themselves.  TrajectoryBuffer and every reference layout are untouched; the setting and the store are not part of a
 * checkpoint (save_ppo's; ppo_save_state keeps it) and not hashed by ppo_param_hash, and no collective is added under data parallelism.
 * While it is on, ppo_update's policy step runs the masked head (one launch, csrc/discrete.hip) for both discrete
 * distributions: minibatch row i reads the mask of its buffer row in place, through the row indices the minibatch
 * gather already produces — no gather launch is added — and the KL monitor takes the masked joint lp; everything else
 * in the step and the options it composes with are unchanged.  With masking off, or on with full masks, every
 * discrete path gives the bits it gives without this feature.
 * ppo_rollout_act_masked is ppo_rollout_act with d_mask [E, W] (dense, environment e's words at e·W): it samples
 * under the masks and writes them to the step's rows of the store in the same launch; −1 while masking is off or for
 * a NULL mask.  While masking is on, plain ppo_rollout_act, ppo_rollout_device and ppo_fill_synthetic write full masks
 * for the rows they lay (the built-in environments have no illegal actions; their sampled bits are unchanged).
 * ppo_act_device_masked is ppo_act_device with d_mask [m, W], in the sampled and the deterministic case; −1 while
 * masking is off or for a NULL mask.  ppo_eval_device stays unmasked. */
int       ppo_set_action_mask(void* ppo, int on);
int       ppo_get_action_mask(void* ppo);                 /* 0 for a NULL ppo */
int       ppo_action_mask_words(void* ppo);
uint32_t* ppo_action_mask_buffer(void* ppo);
long long ppo_rollout_act_masked(void* ppo, const uint32_t* d_mask, float* d_action);
int       ppo_act_device_masked(void* ppo, const float* d_obs, const uint32_t* d_mask, int m, int deterministic,
                                unsigned long long seed, unsigned long long step, float* d_action,
                                float* d_log_prob);
/* The masked head, sampler and greedy action on caller-supplied device arrays (test entries: the update, the rollouts
 * and ppo_act_device_masked call the same launchers), as their multi-discrete counterparts; nvec is a HOST array
 * (dist 1: nvec = {A}).  Head: d_mask holds W words per row, minibatch row i's at d_mask[d_rows[i]·W] (d_rows NULL:
 * i).  Sampler / argmax: d_mask dense [m, W].  They synchronise.  Return 0, or −1 for bad arguments (a NULL array
 * other than d_rows, m <= 0, an nvec the setter would decline, NaN eps) with nothing recorded for ppo_last_error. */
int       ppo_masked_head_device(const float* d_logits, const float* d_action, const float* d_adv,
                                 const float* d_old_lp, const uint32_t* d_mask, const int* d_rows, int m, int A,
                                 const int* nvec, int D, float eps, float ent_coeff, float* d_grad, float* d_lp,
                                 float* d_ent, double* loss);
int       ppo_masked_sample_device(const float* d_logits, const uint32_t* d_mask, int m, int A, const int* nvec, int D,
                                   unsigned long long key, unsigned long long offset, float* d_action,
                                   float* d_log_prob);
int       ppo_masked_argmax_device(const float* d_logits, const uint32_t* d_mask, int m, int A, const int* nvec, int D,
                                   float* d_action);
/* Running observation normalisation (off by default; not in the reference; Stable-Baselines3 VecNormalize,
 * CleanRL NormalizeObservation).  Per observation column j the running state is, in double, a shared count n,
 * mean[j] and M2[j] (the sum of squared deviations; population variance M2/n, as SB3's RunningMeanStd).  The
 * fp32 affine pair is refreshed on the device after every change of that state,
 *     m[j] = (float)mean[j]
 *     r[j] = (float)(1.0 / sqrt(M2[j]/n + 1e-8))        (double arithmetic, one rounding to fp32)
 * and one element normalises, in fp32 and in this order, as
 *     t = (x − m[j]) · r[j]
 *     y = t < −c ? −c : (t > c ? c : t)                  (NaN propagates; c = clip, +inf = no clamp)
 * An element counts as "clamped" when y != t and t is not NaN.  While n == 0 the map is the exact identity
 * (m = 0, r = 1, the clamp ignored): an un-warmed normaliser never truncates raw observations.
 * While it is on, ppo_update — stream-ordered, ahead of GAE — (1) writes norm(state[0:limit]) under the pair as
 * it stands on entry (the pair the rollout that filled the buffer sampled under) into a shadow of `state`
 * (capacity × S floats, allocated on first use), (2) unless frozen, folds the statistics of the RAW
 * state[0:limit] into the running state (Chan's combine) and refreshes the pair — nothing later in that
 * update reads it, the next rollout does — and (3) GAE, the single-workgroup / cluster phases, both loops and
 * captured graphs read the shadow.  Of next_state only the rows GAE forwards on their own are normalised, into
 * a compact scratch (PPO_GAE_FULL=1: every row).  The caller's buffer is never written.  The statistics are
 * deterministic (no floating-point atomics, shifted sums in double).  ppo_rollout_device normalises each
 * step's observations into the shadow and forwards μ from there; ppo_fill_synthetic samples from
 * μ(norm(state)).  compute_gae_cuda / compute_gae called on their own have no PPO and stay un-normalised, and
 * the host rollout (collect_trajectories) has no handle to the normaliser: train_ppo_epoch / eval_ppo END THE
 * PROCESS with a message while the feature is on.  Unlike the options above this one keeps the
 * single-workgroup / cluster phases and PPO_GRAPH=1 replay available.
 * Under data parallelism each rank's batch triple (1 + 2S doubles; n = 0 for an empty shard) is all-gathered
 * right behind GAE's own all-gather, combined in rank order and folded, so every rank holds bit-identical
 * statistics: EVERY RANK MUST HOLD THE SAME on/off AND frozen SETTING, or the ranks issue different sequences
 * of collectives.  While it is on, ppo_param_hash and the replica check also cover the 1 + 2S doubles.
 * Not part of a checkpoint (save_ppo's, which keeps the reference's byte layout; ppo_save_state keeps it): with load_ppo,
 * save and restore the state with
 * ppo_obs_norm_get_state / _set_state and set the option again after load_ppo.  Turning it off keeps the state.
 * clip > 0: on (+inf: normalise, never clamp); <= 0: off.  Returns 0, or −1 for NaN (setting unchanged). */
int    ppo_set_obs_norm(void* ppo, float clip);
float  ppo_get_obs_norm(void* ppo);                       /* 0 when off */
/* evaluation: normalise, never fold; returns the previous value */
int    ppo_obs_norm_freeze(void* ppo, int frozen);
/* fold the device buffer's current rows (state[0:limit]) now — warm-up after a random rollout; the collective
 * included at world > 1 (every rank calls it); asynchronous.  Returns 0, or −1 when off or frozen */
int    ppo_obs_norm_fold_buffer(void* ppo);
/* The five below synchronise.  out = {n, mean[S], M2[S]}; returns 1 + 2S, or −1 when n (the doubles out
 * holds) is too small */
int    ppo_obs_norm_get_state(void* ppo, double* out, long n);
/* returns 0, or −1 (state unchanged) for n != 1 + 2S, a negative count or M2, NaN or infinity */
int    ppo_obs_norm_set_state(void* ppo, const double* in, long n);
/* the fp32 pair in use, to the host (either may be NULL); −1 when S is not the buffer's state size */
int    ppo_obs_norm_affine(void* ppo, float* mean, float* rstd, int S);
/* the update's normalisation kernel on caller-supplied device rows, m rows × S, under the current pair and
 * clip; d_out may be d_in.  Nothing is counted: ppo_read_stats out[20] / out[21] keep describing the last
 * update.  Returns 0, or −1 while the feature is off or for bad arguments */
int    ppo_obs_normalize_device(void* ppo, const float* d_in, float* d_out, long m);
/* the update's statistics kernel alone: d_x [n, S] → out = {n, mean[S], M2[S]} (host, 1 + 2S doubles);
 * returns 0, −1 for bad arguments */
int    ppo_obs_stats_device(const float* d_x, long n, int S, double* out);
/* Running return-based reward normalisation (off by default; not in the reference; the reward half of
 * Stable-Baselines3's VecNormalize): rewards are divided by the running standard deviation of the discounted
 * return and clamped; they are not centred.  Per PPO the running state is three doubles {n, mean, M2} of the
 * discounted returns (population variance M2/n, as SB3's RunningMeanStd; the mean is kept only because Chan's
 * combine needs it).  With g = (double)gamma — the gamma argument of this ppo_update — and the rows of
 * reward[0:limit] in buffer order,
 *     k_i = !(terminated[i] || truncated[i])                 (k_{-1} = 0)
 *     R_i = (double)r_i + g · (k_{i-1} · R_{i-1} + c_i)      (double throughout)
 * where c_i is a carried return, non-zero only at the first row of an environment's segment (below) and 0 for
 * every buffer ppo_rollout_device did not fill.  While it is on, ppo_update — stream-ordered, ahead of GAE's
 * forwards, no read back to the host —
 *   1. scans the RAW rewards into R_0 … R_{limit−1} and their exact-in-double triple (deterministic: no
 *      floating-point atomics, per-workgroup partials folded in a fixed order; csrc/retnorm.hip);
 *   2. unless frozen, folds that triple into the running state (Chan's combine);
 *   3. refreshes the scale  s = (float)(1.0 / sqrt(M2/n + 1e-8))  (double arithmetic, one rounding to fp32;
 *      n == 0: s = 1 and the clamp ignored, the exact identity, as for observations);
 *   4. writes a shadow of the rewards (capacity floats, allocated on first use), per element in fp32 and in
 *      this order:  t = r · s;  y = t < −c ? −c : (t > c ? c : t)  (NaN propagates; an element counts as
 *      "clamped" when y != t and t is not NaN);
 *   5. points GAE at the shadow.  The caller's buffer is never written: train_ppo_epoch's printed J / R stay
 *      raw, and a second update over the same buffer does not scale twice.
 * ORDER: this option folds first and scales with the refreshed state, as SB3 does (the step's own return
 * enters the variance before its reward is divided), so the first update already sees scaled rewards.
 * Observation normalisation does the opposite — it normalises under the pair on entry and folds afterwards —
 * because a rollout sampled under that pair; nothing samples under the reward scale.  While frozen the update
 * scales under the state as it stands and neither scans nor folds.
 * Only GAE reads rewards, so the minibatch loops, the single-workgroup / cluster phases and PPO_GRAPH=1 replay
 * all stay available.  compute_gae_cuda / compute_gae called on their own have no PPO and stay raw.
 * train_ppo_epoch keeps working: its buffer is scanned with no carry (collect_trajectories resets the
 * environment at each call).
 * CARRY ACROSS DEVICE ROLLOUTS: ppo_rollout_device lays transition (e, t) at row e·T + t and ends every segment
 * with truncated = 1 although episodes continue across calls.  It records cont[e] = 1 when environment e was
 * not reset after its last step (whether or not the feature is on, so it may be turned on between a rollout
 * and its update).  The scan of such a buffer (limit == E·T) adds g·carry_in[e] at row e·T — c_{e·T} above —
 * and writes carry_out[e] = cont[e] ? R_{e·T+T−1} : 0.  Carries change at rollout time only: at the start of
 * ppo_rollout_device carry_out becomes carry_in if an update has scanned the rollout just before it, otherwise
 * carry_in is zeroed; an environment reset (a change of n_envs or env_kind) zeroes it.  Repeated updates over
 * one rollout read the same carry_in: idempotent apart from the fold.  ppo_fill_synthetic, train_ppo_epoch and
 * a limit that is not E·T mean "not rollout-laid": one stream, no carry.  (A buffer the caller refills through
 * the device pointers after a rollout keeps the rollout's layout and carry; the open rollout, ppo_rollout_begin …
 * _end below, is the supported way to lay a caller-stepped environment with all of it.)  Carries are per rank, not hashed.
 * Under data parallelism each rank's 3-double batch triple (the zero triple for an empty shard) is all-gathered
 * at one fixed point ahead of GAE's forwards — every rank reaches it, empty shard or not — combined in rank
 * order and folded, so every rank holds bit-identical state: EVERY RANK MUST HOLD THE SAME on/off AND frozen
 * SETTING, or the ranks issue different sequences of collectives.  While it is on, ppo_param_hash and the
 * replica check also cover the three doubles (a function of the state only).  Loopback caveat
 * (PPO_COMM_LOOPBACK=k): the loopback all-gather hands the peers registered by ppo_comm_loopback_peers to any
 * gather of their length, and this triple has the length of GAE's Welford triple — registered peers would feed
 * both gathers, so do not combine them with this option.
 * Not part of a checkpoint (save_ppo's; ppo_save_state keeps it): with load_ppo, save and restore the state with
 * ppo_reward_norm_get_state / _set_state.  Turning
 * it off keeps the state.
 * clip > 0: on (+inf: scale, never clamp); <= 0: off.  Returns 0, or −1 for NaN (setting unchanged). */
int    ppo_set_reward_norm(void* ppo, float clip);
float  ppo_get_reward_norm(void* ppo);                    /* 0 when off */
/* scale, never scan or fold; returns the previous value */
int    ppo_reward_norm_freeze(void* ppo, int frozen);
/* The three below synchronise.  out3 = {n, mean, M2} */
void   ppo_reward_norm_get_state(void* ppo, double* out3);
/* returns 0, or −1 (state unchanged) for a negative count or M2, NaN or infinity */
int    ppo_reward_norm_set_state(void* ppo, const double* in3);
/* the fp32 scale s in use */
float  ppo_reward_norm_scale(void* ppo);
/* the update's scan alone, on caller-supplied device arrays (synchronises).  seg_len = 0: one stream, no carry
 * (d_carry_in / d_cont / d_carry_out unused, may be NULL); seg_len = T > 0: n must be a multiple of T, row e·T
 * takes d_carry_in[e] and d_carry_out[e] (may be NULL) = d_cont[e] ? R_{e·T+T−1} : 0.  d_returns (may be
 * NULL) ← the n returns in double; out3 (host) ← their triple {n, mean, M2}.  Returns 0 (n = 0: the zero
 * triple), −1 for bad arguments.  PPO_RET_CHUNK: the rows one workgroup of the scan composes. */
#define PPO_RET_CHUNK 2048
int    ppo_reward_returns_device(const float* d_reward, const unsigned char* d_term, const unsigned char* d_trunc,
                                 long n, float gamma, int seg_len, const double* d_carry_in,
                                 const unsigned char* d_cont, double* d_returns, double* d_carry_out, double* out3);
/* Episode-return statistics of device rollouts and device evaluation (always on; not in the reference; what
 * Stable-Baselines3's Monitor / evaluate_policy and CleanRL's episodic_return report; csrc/episode.hip).
 * THE SCAN.  A rollout-laid buffer is E segments of T rows, transition (e, t) at row e·T + t.  Row (e, t) ENDS AN
 * EPISODE iff
 *     terminated || (truncated && (t < T−1 || cont == NULL || !cont[e]))
 * (cont[e] = 1: environment e was not reset after the segment's last step, so the truncation ppo_rollout_device
 * writes there ends nothing).  Each environment carries four doubles {ret, disc, w, len}, fresh = {0, 0, 1, 0},
 * and its rows are taken in row order, in double, with g = (double)gamma and r the row's fp32 reward:
 *     ret  = ret + (double)r
 *     disc = disc + w·(double)r            (the product rounded, then the sum: no fused multiply-add — libppo is
 *     w    = w·g                            built with -ffp-contract=off and episode.hip repeats it as a pragma)
 *     len  = len + 1
 *     at an end row: the episode (ret, disc, len) is emitted and the state set fresh
 * d_row_ret / d_row_disc receive ret / disc after each row's update, before an end row's reset.
 * THE AGGREGATE of a set of episodes is PPO_EP_NBATCH doubles
 *     {n, mean of ret, M2 of ret (Σ squared deviations), min ret, max ret, Σ len, mean of disc}
 * — all zero for the empty set — and two aggregates combine as a ⊕ b (Chan et al.; an empty side returns the
 * other unchanged):
 *     n = na + nb;  f = nb / n;  δ = mean_b − mean_a
 *     mean = mean_a + δ·f;   M2 = (M2a + M2b) + (δ·δ)·(na·f);   mdisc = mdisc_a + (mdisc_b − mdisc_a)·f
 *     min = b.min < a.min ? b.min : a.min;  max likewise;  Σlen = Σlen_a + Σlen_b
 * The batch aggregate of one scan: environment e's aggregate P_e starts empty and takes each episode it emits, in
 * the order they end, as P_e ← P_e ⊕ {1, ret, 0, ret, ret, len, disc}; then 256 partials
 * Q_i = P_{i·per} ⊕ … ⊕ P_{min(E, (i+1)·per) − 1} (left to right from the empty aggregate, per = ⌈E/256⌉) are folded
 * by a pairwise tree: for stride = 1, 2, 4, …, 128, every i that is a multiple of 2·stride takes Q_i ← Q_i ⊕
 * Q_{i+stride}; Q_0 is the batch.  No floating-point atomics; the order depends on E alone, never on the grid or
 * on scheduling.  The scan and its fold are two launches whatever E and T are.
 * THE TRACKER.  ppo_rollout_device runs the scan once behind its step loop, stream-ordered and with no host
 * read, over the rows it has just laid, with the cont[] it has just written, the PPO's per-environment state and
 * the tracker's gamma.  The batch becomes "the last rollout's" and is folded into a running window, window ←
 * window ⊕ batch: "since the last reset".  The per-environment state lives exactly as long as cont[]: it is
 * allocated and set fresh on the first call and on a change of n_envs, env_kind or state_size, which drops the
 * episodes in progress and keeps the window.  ppo_fill_synthetic, the host rollout and ppo_update do not touch the
 * tracker.  Under data parallelism the statistics are THIS RANK's environments; no collective is added.  Not
 * hashed (ppo_param_hash) and not part of a checkpoint (save_ppo's; ppo_save_state keeps it).
 * ppo_episode_stats: out[0..7] since the last reset, out[8..15] the last rollout, each
 *     {episodes n, mean return, population std sqrt(M2/n), min, max, mean length Σlen/n, mean discounted
 *      return, M2}                          (host double arithmetic on the aggregate; all 0 where n == 0) */
#define PPO_EP_NBATCH 7
#define PPO_EP_NSTAT 16
/* returns the values written (min(n, 16), 0 for n <= 0 or a NULL out); synchronises */
int    ppo_episode_stats(void* ppo, double* out, int n);
/* clears the window, NOT the episodes in progress (nor the last rollout's out[8..15]); stream-ordered */
void   ppo_episode_reset_stats(void* ppo);
/* the discount of `disc`; returns the previous value; NaN or a value outside [0, 1] only queries; default 0.99;
 * applies from the next row scanned (the w carried by an episode in progress keeps its earlier factors) */
float  ppo_episode_gamma(void* ppo, float gamma);
/* The scan alone, on caller-supplied device arrays; synchronises.  d_cont may be NULL; d_state [E][4] doubles in
 * and out (NULL: every environment fresh, nothing written back); d_row_ret / d_row_disc [E·T] doubles, may be
 * NULL; out (host) ← the batch aggregate, PPO_EP_NBATCH doubles.  Returns 0, or −1 — nothing recorded for
 * ppo_last_error, no device work — for a NULL d_reward / d_term / d_trunc / out, E <= 0 or T <= 0. */
int    ppo_episode_scan_device(const float* d_reward, const unsigned char* d_term, const unsigned char* d_trunc,
                               const unsigned char* d_cont, int E, int T, float gamma, double* d_state,
                               double* d_row_ret, double* d_row_disc, double* out);
/* DEVICE EVALUATION.  Steps n_envs fresh environments for `horizon` steps without touching the training state:
 * the environments are reset exactly as a fresh PPO's first ppo_rollout_device(…, seed) resets them, the Philox
 * keys are derived from `seed` as there, and the step counter is local and starts at 0 — so with deterministic
 * == 0 a fresh PPO's evaluation sees, bit for bit, the trajectory of that PPO's first training rollout.
 * deterministic != 0: the action is μ's output bit for bit (no noise drawn, no log-prob) — with the categorical
 * policy, argmax over the logits, the lowest index on ties.  Rewards and flags go
 * to an n_envs × horizon scratch (written as the rollout writes the buffer's, the segment-end truncation and
 * cont[] included) and are scanned once at the end by the scan above with `gamma`, from fresh states:
 * out[0..7] has the layout of ppo_episode_stats over the episodes completed within the horizon, out[8] is the
 * number of environments whose last episode was still running (unfinished episodes are not counted).  While
 * observation normalisation is on, observations are normalised under the pair as it stands, as if frozen:
 * nothing is folded and the clamp counters of ppo_read_stats out[20] / out[21] keep describing the last update;
 * reward normalisation does not apply (returns are raw).  The trajectory buffer, the training environments, the
 * rollout's step counter and cont[], both return carries, the tracker, both normalisers and every parameter and
 * Adam state are left bit-identical; only μ's forward workspaces (its activations of the last forward) change.
 * Scratch is O(n_envs·(S + A) + n_envs·horizon·6 B), kept for the next call and freed by free_ppo.
 * Returns the values written (9), synchronising once to fill out; or −1 — no die, nothing run — for a NULL ppo or
 * out, n_envs <= 0, horizon <= 0, env_kind not 0, 1 or 2, Pendulum with S != 3 or A != 1, CartPole with S != 4,
 * A != 2 or the Gaussian policy, a NaN gamma or n < 9. */
int    ppo_eval_device(void* ppo, int n_envs, int horizon, int env_kind, unsigned long long seed, int deterministic,
                       float gamma, double* out, int n);
/* the last GAE's state (compute_gae_cuda / ppo_update; synchronises): welford (may be NULL) ← the
 * (n, mean, M2) triple the normalisation used (global at world > 1; out[3..5] the local triple);
 * v / v_next (may be NULL) ← the first n values of V(state) and V(next_state) the scan read.
 * Returns the number of transitions of that GAE. */
long ppo_gae_state(double* welford, float* v, float* v_next, long n);
/* Parity testing at full size: cap the value / policy minibatch steps of the following ppo_update
 * calls (−1 = no cap).  GAE, the shuffles and their rand() consumption are unchanged; only the
 * loops stop early (so one step of a 1M-row, B = 32768 update can be checked against the oracle). */
void ppo_set_step_limit(void* ppo, long max_value_steps, long max_policy_steps);

/* Batched policy sample on device: a = μ(s) + σ·ε, ε ~ N(0,1) (counter-based
 * Philox + Box–Muller), log_prob per row.  d_* are device pointers. */
void ppo_sample_action_device(void* policy, float* d_state, float* d_action, float* d_log_prob, int m,
                              unsigned long long seed, unsigned long long offset);

/* Seeded synthetic rollout written straight into the device buffer
 * (SURVEY §8d): n_envs env-major segments of `horizon` steps, obs ~ U(−1,1),
 * actions sampled from the current policy, rewards 0.1·N(0,1),
 * terminated ~ Bernoulli(p_terminate), truncated at each segment end. */
void ppo_fill_synthetic(void* ppo, int n_envs, int horizon, unsigned long long seed, float p_terminate);

/* Batched on-device rollout: `horizon` steps of all `n_envs` environments — μ forward
 * over the E current observations, Gaussian sampling (Philox), one environment step — written
 * env-major into the device buffer (transition (e, t) at row e·horizon + t; each segment ends
 * truncated), ready for ppo_update.  env_kind 0 = Pendulum-v1 (S = 3, A = 1; gymnasium dynamics),
 * 1 = synthetic (any S, A; with the categorical policy the chosen index i acts as 2·i/(A − 1) − 1),
 * 2 = CartPole-v1 (S = 4, A = 2, the categorical policy only — ppo_set_action_dist; gymnasium's constants, explicit
 * Euler, reward 1 per step, terminated at |x| > 2.4 or |θ| > 12°, truncated at 500 steps; index 1 pushes right);
 * any other combination ends the process with a message.  Episodes continue across calls; the first call (or a change of
 * n_envs / env_kind) resets every environment from `seed`.  `seed` keys the Philox streams of the
 * policy noise, the environment's noise and its resets; the position in them advances with every
 * step of every call (a counter that starts at 0 with the PPO), so passing the same seed to every
 * call is the intended use and a fresh PPO with that seed reproduces the same rollouts. */
void ppo_rollout_device(void* ppo, int n_envs, int horizon, int env_kind, unsigned long long seed);

/* THE OPEN ROLLOUT: ppo_rollout_device with the environment step handed to the caller (DESIGN.md §4 "External
 * environments").  The caller owns a vectorised simulator on the device; libppo owns everything else — the row map,
 * observation normalisation, μ's forward, the sampler and its Philox position, the segment-end truncation, cont[],
 * the return carry, the episode tracker — with the same launches and the same streams as ppo_rollout_device.
 *     ppo_rollout_begin(ppo, E, T, d_obs0 | NULL, seed)
 *     T × { step = ppo_rollout_act(ppo, d_action);   the caller steps its E environments under d_action;
 *           ppo_rollout_store(ppo, d_reward, d_next_obs, d_term, d_trunc, d_obs_after | NULL) }
 *     ppo_rollout_end(ppo);   ppo_update(…)
 * Arrays are dense and device-resident: d_obs0, d_next_obs, d_obs_after [E, S] floats, d_action [E, A] floats,
 * d_reward [E] floats, d_term, d_trunc [E] bytes.  Everything is stream-ordered on libppo's stream and nothing is
 * read back: a simulator on another stream synchronises with libppo's itself (ppo_synchronize, or keep its work on
 * the null stream).  All four return −1 — nothing launched, nothing recorded for ppo_last_error, the state of the
 * rollout unchanged — for a NULL ppo or array (d_obs0 and d_obs_after excepted) or a call out of sequence; none
 * ends the process.
 * begin: 1 <= E·T <= capacity.  d_obs0 != NULL: FRESH EPISODES from these observations, as ppo_rollout_device on a
 * change of n_envs or env_kind — cont[], both return carries and the tracker's per-environment state are
 * reallocated fresh, the statistics window stays; the environment kind becomes "external", so going from a
 * built-in environment to an external one or back is a change of environment in both directions.  d_obs0 == NULL:
 * the environments CONTINUE from the d_obs_after of the last stored step — legal only after an external rollout of
 * the same E and state size that reached its end (T may differ), else −1.  The return-carry swap happens here, as
 * at the start of ppo_rollout_device.  The current observations go to rows e·T of `state`.  `seed` keys the policy
 * noise exactly as ppo_rollout_device's does (splitmix64(seed ^ 0x524F4C4C)) for every act of this rollout.  begin
 * leaves the buffer's limit (idx / full) and its rollout-laid mark alone: A ppo_update ISSUED WHILE A ROLLOUT IS OPEN
 * sees the previous limit over partly new rows — the caller's error.  A begin while one is open abandons it (with
 * d_obs0; with NULL it is out of sequence); ppo_rollout_device, ppo_fill_synthetic and train_ppo_epoch called while
 * one is open simply close it, and nothing can continue from it.
 * act (after begin or store): step t's E rows e·T + t are normalised into the shadow while observation
 * normalisation is on, μ is forwarded over them and the Gaussian or categorical row sampler writes action and
 * log-prob into the buffer rows at the rollout step counter's next position — the counter ppo_rollout_device
 * advances, so internal and external rollouts of one PPO never reuse a position; one more launch copies the E
 * action rows out to d_action.  Returns that position (>= 0), so that the caller can address the same position in
 * streams of its own (ppo_env_step_device takes it).
 * store (once after each act), for row = e·T + t:
 *     next_state[row] = d_next_obs[e]          the transition's own next observation: the terminal one where the
 *                                              episode ended
 *     reward[row]     = d_reward[e]
 *     terminated[row] = d_term[e] != 0
 *     truncated[row]  = d_trunc[e] != 0 || (t == T−1 && !terminated[row])
 *     t == T−1:  cont[e] = !(d_term[e] || d_trunc[e])     the environment's own flags alone decide it
 *     t + 1 < T: state[row + 1] = d_obs_after[e]          what the next step starts from: the reset observation
 *     always:    the PPO's current observations [E, S] ← d_obs_after[e]     where the episode ended
 * d_obs_after == NULL means d_next_obs: an environment that never resets, or that resets on its next step.  (A
 * terminated row at a segment end gets truncated = 0 here; CartPole's built-in kernel writes 1.  Nothing downstream
 * tells the two apart: GAE and both scans read terminated || truncated, and terminated alone masks the bootstrap.)
 * end: legal only after the T-th store (else −1, the rollout stays open).  The tail of ppo_rollout_device: the
 * episode scan with cont[], the advantages zeroed, idx / full, the buffer pointed at the device, rollout-laid.
 * Composes with every option of ppo_update (both normalisers, the categorical policy, clipping, target KL, tanh
 * networks, data parallelism: per rank, no collective added).  The open rollout's own state (step t, the current
 * observations) is not part of a checkpoint (save_ppo's; ppo_save_state keeps an ended rollout's continuation
 * observations, and declines while one is open). */
int       ppo_rollout_begin(void* ppo, int n_envs, int horizon, const float* d_obs0, unsigned long long seed);
long long ppo_rollout_act(void* ppo, float* d_action);
int       ppo_rollout_store(void* ppo, const float* d_reward, const float* d_next_obs, const unsigned char* d_term,
                            const unsigned char* d_trunc, const float* d_obs_after);
int       ppo_rollout_end(void* ppo);
/* A STATELESS ACT, for evaluation and serving against a caller's environment (what ppo_eval_device does for the
 * built-ins): d_obs [m, S] raw → d_action [m, A] (and d_log_prob [m]).  Observations are normalised under the pair
 * as it stands, as if frozen — nothing folded, the clamp counters untouched — into a scratch kept with the PPO; μ is
 * forwarded.  deterministic != 0: the action is μ's output bit for bit — categorical: the lowest argmax index in
 * column 0, zeros after; d_log_prob is not written and may be NULL.  Otherwise row i draws exactly what the rollout's
 * sampler draws for environment i at position `step` under `seed`: on the same observations ppo_rollout_act (begun
 * with that seed, returning that step) and ppo_act_device agree bit for bit; d_log_prob may be NULL.  Leaves
 * bit-identical everything ppo_eval_device leaves so (the rollout's step counter and an open rollout included):
 * only μ's forward workspaces change.  Stream-ordered, no host read.  Returns 0, or −1 — nothing launched — for a
 * NULL ppo, d_obs or d_action or m <= 0. */
int ppo_act_device(void* ppo, const float* d_obs, int m, int deterministic, unsigned long long seed,
                   unsigned long long step, float* d_action, float* d_log_prob);
/* THE BUILT-IN ENVIRONMENTS ON DENSE ARRAYS: ppo_rollout_device's three environments as a caller-stepped simulator
 * — a third form of each step kernel through the same device functions as the training and the evaluation forms, so
 * the three cannot drift.  Driven through the open rollout with the seed begin took and the step act returned, they
 * reproduce ppo_rollout_device bit for bit.  d_env_state holds E · ppo_env_state_floats(env_kind, S) floats (−1 for
 * an unknown kind or an S the kind does not take).  reset: every environment from splitmix64(seed) at the reset
 * stream's first offset, as ppo_rollout_device's first call; d_obs [E, S] ← the first observations.  step: d_action
 * [E, A] in (categorical != 0: column 0 holds an index); d_next_obs [E, S] ← the transition's next observation,
 * d_obs_after [E, S] ← what the next step starts from, d_reward [E], d_term [E] as the training kernels write it,
 * d_trunc [E] ← the environment's own TimeLimit alone (Pendulum 200 steps, CartPole 500, synthetic never): the
 * segment end belongs to ppo_rollout_store.  The key is splitmix64(seed ^ 0x524F4C4C), `step` the position in the
 * environment and reset streams.  Stream-ordered, no host read.  Both return 0, or −1 — nothing launched — for a NULL
 * array, E <= 0 or a shape the kind does not take (Pendulum S = 3, A = 1; CartPole S = 4, A = 2, categorical). */
int ppo_env_state_floats(int env_kind, int S);
int ppo_env_reset_device(int env_kind, float* d_env_state, float* d_obs, int E, int S, unsigned long long seed);
int ppo_env_step_device(int env_kind, float* d_env_state, const float* d_action, float* d_next_obs, float* d_obs_after,
                        float* d_reward, unsigned char* d_term, unsigned char* d_trunc, int E, int S, int A,
                        int categorical, unsigned long long seed, unsigned long long step);

/* ---------------- the state-dependent-σ Gaussian policy (csrc/gauss_sd.hip) ----------------
 * A diagonal Gaussian whose standard deviation is an output of the policy network (RLlib's free_log_std = False,
 * Brax's PPO, rl_games' fixed_sigma: False).  A = action_size, the width of μ's output and of a stored action row,
 * does not change; A must be even and Aa = A / 2 <= 32 is the action dimension.  Columns 0 … Aa−1 of a row z of μ's
 * output are the mean, columns Aa … A−1 the raw log σ.  It is action distribution 3, behind its own setter, as the
 * multi-discrete policy is 2.  Per row, fp32, j ascending (csrc/ppo_math.h, the sd_* atoms over the Gaussian ones):
 *     ls_j  = t < ls_min ? ls_min : (t > ls_max ? ls_max : t),   t = z_{Aa+j}      (NaN propagates)
 *     in_j  = !(t < ls_min) && !(t > ls_max)                                        (NaN counts as inside)
 *     lp    = log_prob_start(Aa), then lp = log_prob_sub(lp, log_prob_term(ls_j, (a_j − μ_j)/expf(ls_j)))
 *             — the Gaussian atoms, so a row whose ls equals a fixed log σ vector gets the Gaussian head's bits
 *     H     = the Gaussian entropy expression over this row's ls (the constant for Aa, then += ls_j ascending)
 *     g     = ∂loss/∂lp from surrogate(adv, lp, old_lp, eps, m, &g)
 *     ∂loss/∂z_j      = the Gaussian head's grad_μ expression with this row's ls_j                 j < Aa
 *     ∂loss/∂z_{Aa+j} = in_j ? (the Gaussian head's per-row ∂/∂log σ term with this row's ls_j) − ent_coeff/m : +0
 *     loss  = −Σ_rows surrogate/m − ent_coeff·(Σ_rows H)/m
 * A clamped column's gradient is +0, written.  A stored action row stays A floats: columns 0 … Aa−1 hold the action,
 * columns Aa … A−1 are +0; the stored log-prob is lp.  Sampling: a_j = μ_j + normal_at(e·Aa + j, kNoise + step, key)
 * ·expf(ls_j), key and offset those of the Gaussian sampler at each call site; the deterministic action is the mean
 * half with zeros after it.  Under PPO_KL_EXACT the row KL is the Gaussian closed form over the clamped halves of the
 * old and the new row.  The recommended bounds are (−20, 2), RLlib's and the SAC implementations'; there is no default.
 *
 * While it is on a policy step is forward → this head → backward in the multi-launch loop (no fused head, wide pass,
 * single-workgroup or cluster phase, no graph replay); the log σ vector gets no gradient and stays bit-identical.
 * ppo_rollout_device, ppo_rollout_act, ppo_act_device, ppo_eval_device and ppo_fill_synthetic sample through it;
 * Pendulum is accepted with A == 2, the synthetic environment reads column j mod Aa, CartPole declines;
 * ppo_env_step_device is not extended.  train_ppo_epoch and eval_ppo end the process with a message.
 * ppo_read_stats: out[4] is the mean row entropy of the last policy step's minibatch, out[34] its clamped log-σ
 * elements and out[35] its elements m·Aa (exact integers, THIS RANK's rows under data parallelism; 0 while off).
 * ppo_save_state keeps the setting and the bounds in a section written only while the distribution is 3; save_ppo
 * keeps nothing.
 * Out of scope: Aa > 32, bf16 compute mode, a tanh squash of the action, an additive log-σ offset, and the fused,
 * cluster and graph paths.
 *
 * The setter returns 0, or −1 with the setting unchanged: NULL ppo, A odd, Aa > 32, NaN, ls_min >= ls_max, either
 * outside [−20, 20], or bf16 compute mode (ppo_set_compute_dtype(ppo, 1) returns −1 while it is on).  While it is on
 * ppo_get_action_dist returns 3; ppo_set_action_dist(ppo, 0 | 1) switches away, ppo_set_action_dist(ppo, 3) returns −1
 * and ppo_set_action_mask returns −1.  The getter returns 1 while on (out2 = {ls_min, ls_max}, may be NULL), else 0. */
int ppo_set_action_gaussian_sd(void* ppo, float ls_min, float ls_max);
int ppo_get_action_gaussian_sd(void* ppo, float* out2);
/* test entries: the head, the sampler and the closed-form KL launch on caller-supplied device arrays.  Each
 * synchronises; each returns −1 with nothing launched and nothing recorded for ppo_last_error on bad arguments.
 * Head: d_grad [m, A], d_lp / d_ent [m], *loss the launch's loss, clamped2 = {clamped log-σ elements, m·Aa}.
 * Sampler: counter e·Aa + j at `offset` under `key`.  KL: row i of d_new against row d_rows[i] (NULL: i) of d_old,
 * d_row_kl (may be NULL) [m] ← every row's KL, *out_mean their mean. */
int ppo_gauss_sd_head_device(const float* d_z, const float* d_action, const float* d_adv, const float* d_old_lp,
                             int m, int A, float ls_min, float ls_max, float eps, float ent_coeff,
                             float* d_grad, float* d_lp, float* d_ent, double* loss, long long* clamped2);
int ppo_gauss_sd_sample_device(const float* d_z, int m, int A, float ls_min, float ls_max, unsigned long long key,
                               unsigned long long offset, float* d_action, float* d_log_prob);
int ppo_gauss_sd_kl_exact_device(const float* d_new, const float* d_old, const int* d_rows, int m, int A,
                                 float ls_min, float ls_max, double* d_row_kl, double* out_mean);

/* layer 0's input of the last device forward of a NeuralNetwork*, m rows × input_size fp32, to the
 * host: the gathered minibatch rows the GEMMs read (NeuralNetwork.d_x0) — for parity tests;
 * synchronises.  bf16 copies (x0_dtype 1) are not converted: returns −1 for them and for m beyond the
 * last forward, else 0. */
int ppo_nn_input_rows(void* nn, float* out, int m);

/* ---------------- training-state checkpoints ----------------
 * save_ppo / load_ppo keep the reference's byte layout: five hyper-parameters, the two networks, log σ and the three
 * Adams.  ppo_save_state keeps THE WHOLE TRAINING STATE, so that a run stopped between two updates and resumed with
 * ppo_load_state is the run that was interrupted, bit for bit: the same rollouts, minibatch orders, parameters,
 * normaliser states and episode statistics as if it had never stopped (DESIGN.md §4 "Training-state checkpoints"
 * gives the file format).  A checkpoint is D2H / H2D copies between updates: no kernel, nothing on the update or
 * rollout path changes.
 * WHAT IS KEPT: save_ppo's byte stream itself; the settings — max_grad_norm, target_kl, value_clip, the
 * advantage-normalisation mode (a section of its own, written only while the mode is not the global one, so images
 * of PPOs that never set it are what they always were), both normalisers' clip and freeze flag, the episode tracker's gamma, the action distribution with nvec, masking, both networks'
 * compute dtype (applied on load through their setters: the distribution before the mask, the dtype last); both
 * normalisers' running triples (the fp32 pair and scale are refreshed on load as _set_state refreshes them); the
 * device shuffle's epoch key; and, once a rollout has run, the rollout's state — the built-in environments' device
 * state, the Philox position, cont[], both return carries and whether an update has scanned the last rollout, the
 * episode tracker's per-environment state and both aggregates, and an ended open rollout's continuation observations
 * (ppo_rollout_begin(…, NULL, seed) continues after the load).
 * PPO_CKPT_BUFFER also stores the rows [0, limit) of the trajectory buffer (state, action, log-prob, reward,
 * next-state and both flags, from wherever the buffer currently points; advantages and targets are not stored: every
 * update recomputes them) and, while masking is on, the mask store's limit · W words: a save taken between a rollout
 * and its update resumes into that update.  Without the flag the buffer's contents are not kept: the loaded PPO has an
 * empty buffer (idx = 0, not full, not rollout-laid, full masks) and must roll out before it updates — the usual place
 * to save is behind an update.  A loaded buffer is device-resident.
 * NOT STATE — after a load these are as on a fresh PPO: the ppo_read_stats accumulators and the KL history, the step
 * limit (ppo_set_step_limit), ppo_value_clip_old_values' caller pointer, every workspace and scratch (the minibatch
 * and phase gathers, ppo_eval_device's and ppo_act_device's scratch, captured graphs), the process-wide GEMM engine
 * and tuning knobs, and an RCCL communicator.
 * PPO_SHUFFLE_HOST_RAND draws from libc rand(), whose state cannot be captured: the bit-for-bit promise holds for
 * PPO_SHUFFLE_DEVICE, and as far as the update itself is reproducible run to run.  The host rollout's
 * Env — like a caller's simulator behind the open rollout — is the caller's object and is not kept either.
 * Under data parallelism every rank saves and loads its own file; no collective is added, and
 * ppo_comm_check_replicas is how a caller checks the ranks after loading.
 * ppo_save_state synchronises libppo's streams, copies to the host, writes path + ".tmp" and renames it, so an
 * interrupted save never leaves a half-written file under path.  Returns 0, or −1 with nothing written and nothing
 * recorded for ppo_last_error: a NULL argument, an unwritable path, or an open rollout in progress (between
 * ppo_rollout_begin and _end: partly laid rows are not a state worth keeping).
 * ppo_load_state validates the whole file on the host — magic, version, bounds, every section's checksum, every
 * section's length against the shapes in the legacy header — before it touches the device, builds the PPO from the
 * legacy section (use_cuda = true) and applies the others.  Any failure (a missing, short or damaged file, a version
 * above 1, a section that contradicts the shapes, an nvec the setter declines) returns NULL with a one-line message in
 * err (err_cap bytes, may be NULL): the process stays alive, nothing leaks, nothing is recorded for ppo_last_error.
 * ppo_state_image serialises to memory what ppo_save_state writes — a pure function of the state: no timestamps, no
 * pointers, every gap zero — and returns its size (out NULL: the size only), or −1 when cap is too small, for a NULL
 * ppo or an open rollout.  ppo_state_hash is FNV-1a-64 over that image (0 where there is none): two PPOs with equal
 * hashes under PPO_CKPT_BUFFER continue identically. */
enum { PPO_CKPT_BUFFER = 1 };   /* also store the trajectory buffer's rows (and the mask store's) */
int   ppo_save_state(void* ppo, const char* path, int flags);
void* ppo_load_state(const char* path, char* err, int err_cap);
unsigned long long ppo_state_hash(void* ppo, int flags);
int   ppo_state_image(void* ppo, int flags, void* out, long cap);

/* ---------------- compute precision ---------------- */
/* 0 = fp32 (default: exact fp32 MFMA GEMMs), 1 = bf16 MFMA GEMMs with fp32 accumulation, fp32
 * master parameters / Adam / heads / GAE, bf16 storage of hidden activations and their gradients
 * (BASELINE config C5).  Returns 0, or −1 for an invalid dtype.  The bf16 kernels know ReLU and identity
 * layers only: dtype 1 on a network with a "tanh" layer (for ppo_set_compute_dtype: in either network)
 * returns −1 and leaves the setting unchanged; tanh networks run in fp32 mode, on both fp32 GEMM engines.
 * ppo_set_compute_dtype(ppo, 1) also returns −1 while the categorical policy is on (ppo_set_action_dist). */
int ppo_set_compute_dtype(void* ppo, int dtype);
int nn_set_compute_dtype(void* nn, int dtype);          /* NeuralNetwork* */

/* ---------------- GEMM tuning utilities ---------------- */
/* force a tile configuration (−1 = automatic) and the split-K workgroup target of grad_W
 * (0 = per-shape automatic, < 0 keeps the current setting); returns the number of tile configurations */
int    ppo_gemm_tune(int force_cfg, int splitk_target);
/* experiment switches of the fp32 tiled GEMM (bit 0: invert the s_setprio default around the MFMA block; bit 2 (value 4): grad_W and grad_x of a layer as two launches instead of one paired launch); flags < 0
 * only queries; returns the previous value */
int    ppo_gemm_flags(int flags);
/* average device µs of one launch: op 0 = forward (bias+ReLU), 1 = grad_x, 2 = grad_W (+bias grad),
 * 3 = forward without activation (output layer), 6 = forward (bias+tanh), 7 = grad_x with a tanh layer's
 * post-activation operand h (ppo_bench_gemm_x3: 4 – 6 are its value-head fold variants, 7 the same grad_x,
 * 8 its forward with tanh);
 * m = batch, n = in, l = out; cfg −1 = automatic */
double ppo_bench_gemm(int op, int m, int n, int l, int iters, int cfg);
/* two independent C4-shaped minibatch GEMM chains (B rows, `out` outputs), `steps` steps each,
 * interleaved on one stream (two = 0) or two streams (two = 1); total device µs */
double ppo_bench_streams(int two, int steps, int B, int out);
/* bf16 GEMMs: force a tile configuration (−1 = automatic); returns the number of configurations */
int    ppo_gemm16_tune(int force_cfg);
/* average device µs of one bf16 launch (op as ppo_bench_gemm: 0 forward+ReLU, 1 grad_x, 2 grad_W, 3 forward to fp32 without activation; bf16 operands); splitk_target 0 = automatic */
double ppo_bench_gemm16(int op, int m, int n, int l, int iters, int cfg, int splitk_target);

/* fp32 GEMM engine of fp32 mode: 0 = exact fp32 MFMA (v_mfma_f32_32x32x2_f32), 1 = "x3": fp32
 * operands split exactly into three bf16 planes, the six plane products with pa + pb <= 2 on the
 * bf16 MFMA, fp32 accumulation (fp32-accurate, 6/16 of the fp32 MFMA cycles).  engine < 0 only
 * queries; returns the previous engine.  Env PPO_F32_GEMM=exact|x3 sets the initial value. */
int    ppo_gemm_f32_engine(int engine);
/* bf16 mode's LDS-DMA GEMM kernel (forward / grad_x with bf16 operands, gemm16.hip): on = 1 / 0
 * sets, −1 queries; returns the previous setting (initially on) */
int    ppo_gemm16_dma(int on);
/* bf16 mode's LDS-DMA grad_W tile width: 128 (256 × 128 tiles, default) or 256 (256 × 256, for
 * n % 256 = 0); other values query; returns the previous width */
int    ppo_gemm16_tn_width(int bn);
/* x3 engine tuning: force a tile configuration (−1 = automatic) and the grad_W split-K workgroup
 * target (0 = automatic, < 0 keeps); returns the number of configurations */
int    ppo_gemm_x3_tune(int force_cfg, int splitk_target);
/* average device µs of one x3 launch (fp32 operands; op as ppo_bench_gemm) */
double ppo_bench_gemm_x3(int op, int m, int n, int l, int iters, int cfg, int splitk_target);

/* ---------------- kernel timing ---------------- */
enum { PPO_K_GEMM = 0, PPO_K_GAE = 1, PPO_K_ADAM = 2, PPO_K_GATHER = 3, PPO_K_HEAD = 4,
       PPO_K_COMM = 5, PPO_K_OTHER = 6, PPO_K_COUNT = 7 };
/* stride > 0: record HIP events around every stride-th launch of each class on libppo's stream
 * (1 = every launch; an event pair costs a few µs of stream time, so throughput runs sample);
 * 0 = off */
void ppo_prof_enable(int stride);
void ppo_prof_reset(void);
/* per class: out_ms[k] = Σ kernel time (ms), out_work[k] = Σ algorithmic FLOPs (GEMM) or bytes,
 * out_launches[k] = launches.  Synchronises. */
void ppo_prof_read(double* out_ms, double* out_work, long* out_launches);
/* on != 0: sampled GEMM launches are timed by events the kernel dispatch itself stamps
 * (hipExtLaunchKernel) instead of event packets around the launch — the kernel's own duration, as
 * rocprofv3 --kernel-trace reports it (default off: event pairs around every sampled launch) */
void ppo_prof_kernel_events(int on);
/* per GEMM shape since the last reset: key = op<<58 | engine<<54 | m<<24 | n<<12 | l (op 0 forward,
 * 1 grad_x, 2 grad_W, 3 paired grad_W + grad_x; engine 0 exact fp32, 1 x3, 2 bf16), Σ ms, sampled
 * launches and Σ algorithmic FLOPs.  Returns the number of shapes (fills at most cap).  Synchronises. */
int  ppo_prof_shapes(long long* keys, double* ms, long* launches, double* work, int cap);
/* per GEMM shape key (as ppo_prof_shapes returns them): launches issued while profiling was enabled,
 * sampled or not — so a sampled average can be weighted by how often the shape really runs.
 * Returns how many of the n keys were seen. */
int  ppo_prof_shape_issued(const long long* keys, long* issued, int n);
/* per class: launches issued while profiling was enabled (sampled or not) */
void ppo_prof_counts(long* out_total);
/* per class: Σ algorithmic work of every launch issued while profiling was enabled */
void ppo_prof_issued_work(double* out_work);

#ifdef __cplusplus
}
#endif
#endif /* PPO_EXT_H */
