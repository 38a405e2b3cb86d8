/*
 * ppo_dev.h — PPO.dev: everything libppo keeps with a PPO beyond the reference's struct (the update's
 * workspaces, the options of ppo_ext.h and their running state, the rollouts' state).
 *
 * Shared by ppo.c, which owns and uses it, and checkpoint.c, which captures and restores the part of it
 * that is training state (DESIGN.md §4 "Training-state checkpoints").
 */
#ifndef PPO_HOST_DEV_H
#define PPO_HOST_DEV_H

#include "internal.h"

/* ------------------------------------------------------------------ */
/* device workspaces                                                   */
/* ------------------------------------------------------------------ */
typedef struct {
    int cap_B, S, A;
    float *states, *actions, *old_lp, *adv, *tgt, *gv, *gmu;
    int* rows;                    /* minibatch slot → buffer row (layer 0's fused gather) */
    int* rows_p;                  /* the policy loop's own rows / gathered states (it runs on the */
    float* states_p;              /* side stream beside the value loop) */
    int* perm[2];                 /* host rand() shuffle: every epoch's permutation (value, policy) */
    long perm_cap[2];
    int* ro_rows;                 /* rollout: rows[t·E + e] = e·T + t */
    float* tiny_steps[3];         /* small-network path: per-step Adam step sizes (value, entropy, policy) */
    int tiny_cap[3];
    float* env_state;             /* rollout: per-environment state */
    int ro_E, ro_T, ro_kind, ro_S;
    unsigned long long ro_step;   /* rollout step counter (Philox stream offset) */
    float* stats;                 /* [0] Σ value loss, [1] Σ policy loss */
    long n_v, n_p;
    long n_graph;                 /* minibatch steps replayed from captured graphs (PPO_GRAPH=1) */
    uint64_t key;                 /* device-shuffle epoch key */
    unsigned long long seed;
    int seeded;
    long max_v, max_p;            /* ppo_set_step_limit: cap on value / policy minibatch steps (−1: none) */
    /* launch-free minibatch steps (graph replay): per phase (0 value, 1 policy) a device step table,
     * its step counter and the Adam kernel's ticket */
    PhipStepArgs* tab[2];
    long tab_cap[2];
    int* ctr;                     /* [2] step counters, [2] tickets (as unsigned) */
    PhipStepArgs* h_tab;
    long h_tab_cap;
    /* phase gathers: every minibatch step's row indices and per-row inputs of a whole phase, gathered
     * by one launch per epoch before the loops (value: rows, targets; policy: rows, actions, old
     * log-probs, advantages) — step iv reads its B rows at iv·B */
    int* ph_rows[2];
    float *ph_tgt, *ph_act, *ph_olp, *ph_adv;
    long ph_cap[2];
    /* global gradient-norm clipping (ppo_set_max_grad_norm; 0 = off): each loop's own device record
     * (norm, coefficient, clipped-step counter, the norm kernel's ticket and partials) — the value and
     * policy loops run concurrently, so they share nothing here */
    float max_grad_norm;
    PhipClipRec* clip[2];
    /* target-KL early stopping (ppo_set_target_kl; 0 = off, +inf = measure only): the policy loop's device
     * record (csrc/kl.hip) — the step's KL and clip fraction, the sticky stop word the policy Adams read,
     * the per-step KL history of the last update */
    float target_kl;
    PhipKlRec* kl;
    /* PPO2 value-loss clipping (ppo_set_value_clip; 0 = off): the clip range, the caller's old values by
     * buffer row (ppo_value_clip_old_values; NULL = the default, the update's own GAE values g_v) and the
     * device counters {clipped rows, rows} of the value steps since the last reset */
    float value_clip;
    const float* v_old_user;
    unsigned long long* vclip_counts;
    /* running observation normalisation (ppo_set_obs_norm; 0 = off; csrc/obsnorm.hip): the clamp, the freeze
     * flag, the running triple {n, mean[S], M2[S]} in double and its fp32 affine pair (m, r = m + S), the
     * shadow of `state` every consumer inside the update reads (capacity × S), the compact scratch of the
     * next_state rows GAE forwards on their own, this rank's batch triple and the all-gathered ones, and the
     * counters {clamped, normalised} of the last state normalisation.  All NULL until first used. */
    float obs_clip;
    int obs_frozen;
    double* obs_run;
    float* obs_m;
    float* obs_shadow;
    float* obs_next;
    long obs_next_cap;
    double* obs_batch;
    double* obs_all;
    int obs_all_world;
    unsigned long long* obs_counts;
    /* running return-based reward normalisation (ppo_set_reward_norm; 0 = off; csrc/retnorm.hip): the clamp,
     * the freeze flag, the running triple {n, mean, M2} of the discounted returns in double, the fp32 scale, the
     * shadow of `reward` GAE reads (capacity floats), this rank's batch triple and the all-gathered ones, and the
     * counters {clamped, scaled} of the last update's scaling.  All NULL until first used. */
    float rew_clip;
    int rew_frozen;
    double* rew_run;
    float* rew_scale;
    float* rew_shadow;
    double* rew_batch;
    double* rew_all;
    int rew_all_world;
    unsigned long long* rew_counts;
    /* the carry of the returns across device rollouts, kept whether or not the feature is on: ro_cont[e] = the
     * last rollout left environment e's episode running; carry_in[e] enters row e·T of the buffer's scan,
     * carry_out[e] is what the last scan left for the next rollout (both [ro_E] doubles).  ro_laid: the buffer
     * holds the last ppo_rollout_device's E × T rows; rew_scanned: an update has scanned that rollout. */
    unsigned char* ro_cont;
    double *rew_carry_in, *rew_carry_out;
    int ro_laid, rew_scanned;
    /* episode statistics (ppo_episode_stats; csrc/episode.hip): the discount of `disc`, the per-environment state
     * {ret, disc, w, len} ([ro_E][4] doubles, living exactly as long as ro_cont) and two aggregates of 8 doubles,
     * [0..7] the window since the last reset, [8..15] the last rollout */
    float ep_gamma;
    int ep_fresh;                 /* the next scan starts every environment fresh (ep_state not yet written) */
    double* ep_state;
    double* ep_agg;
    /* ppo_eval_device's scratch, kept across calls: the environments' state, the current observation and its
     * normalised copy, actions, log-probs and the identity row list ([ev_E] rows), the E × T rewards and flags
     * ([ev_N] rows), cont and the aggregate */
    int ev_E;
    long ev_N;
    float *ev_env, *ev_obs, *ev_obsn, *ev_act, *ev_lp, *ev_reward;
    int* ev_rows;
    unsigned char *ev_term, *ev_trunc, *ev_cont;
    double* ev_agg;
    /* the action distribution (ppo_set_action_dist; 0 = diagonal Gaussian, 1 = categorical over A choices, μ's
     * outputs the logits; csrc/categorical.hip, csrc/discrete.hip) and the discrete heads' entropy word: Σ of the row entropies
     * of the last policy step's minibatch and that minibatch's rows (ppo_read_stats out[4]) */
    int action_dist;
    float* cat_ent;
    int cat_rows;
    /* the multi-discrete policy (ppo_set_action_multidiscrete; action_dist == 2; csrc/discrete.hip): μ's A
     * outputs are md_D softmaxes side by side of widths md_nvec; md_off (device, md_D + 1 ints) their offsets,
     * md_max_n the widest.  cat_off = the device offsets {0, A}, laid when ppo_set_action_dist selects the categorical
     * policy: it samples, takes its greedy action and runs its masked head through the same kernels as nvec = {A} */
    int md_D, md_max_n;
    int md_nvec[PHIP_MD_MAX_D];
    int *md_off, *cat_off;
    /* the open rollout (ppo_rollout_begin / _act / _store / _end; ro_kind == PHIP_ENV_EXTERNAL): ext_open while
     * one is open, ext_t the step the next act takes, ext_acted between an act and its store, ext_done once a
     * rollout has ended and ext_obs [ro_E, ro_S] — the observations the next step starts from, as the stores left
     * them — may continue into begin(NULL); ext_key the policy-noise key of begin's seed */
    int ext_open, ext_t, ext_acted, ext_done;
    uint64_t ext_key;
    float* ext_obs;
    long ext_obs_cap;
    /* ppo_act_device's scratch for act_m rows: the normalised observations, the identity row list, log-probs */
    int act_m;
    float *act_obsn, *act_lp;
    int* act_rows;
    /* invalid-action masking (ppo_set_action_mask; csrc/discrete.hip; a discrete policy only): while mask_on the
     * store `mask` holds capacity × W words, W = (A + 31) / 32, row r's words at r·W, bit k & 31 of word k >> 5 =
     * logit column k allowed — whatever lays buffer rows writes them, the policy step reads them through the
     * minibatch's row indices.  NULL while off.  Not part of save_ppo's checkpoint (ppo_save_state keeps it), not
     * hashed, no collective */
    int mask_on;
    uint32_t* mask;
    /* learning-rate schedules (ppo_set_lr_schedule; 0 = constant: ppo->lr_policy / lr_V by value, as ever): the kind,
     * its three parameters, the value-rate coupling of the adaptive kind and the updates since the setter.  The
     * adaptive kind's rates, its parameters' device copy, its two counters and the per-step rate history live in the
     * KL record (`kl`: lr, lr_v, lr_kl, lr_min, lr_max, lr_raised, lr_lowered, lr_hist).  lr_use: the rates this
     * update passes by value {policy, value} */
    int lr_kind;
    float lr_p[3];
    int lr_couple;
    unsigned long long lr_u;
    float lr_use[2];
    /* per-minibatch advantage normalisation (ppo_set_adv_norm; 0 = GAE's global normalisation alone, as ever;
     * csrc/advnorm.hip): the mode, and the (m, sd) pair of every policy segment of the last update ([adv_cap][2]
     * floats; NULL until an update runs with the mode on).  gat_np / gat_B: the policy steps and the minibatch size
     * of the last update's phase gather (ph_rows[1], ph_adv), 0 when that update kept none (single-workgroup /
     * cluster phases, graph replay) — what ppo_adv_norm_read may read; adv_np: the segments the last update
     * normalised (0 while off) */
    int adv_norm_mode;
    float* adv_stats;
    long adv_cap;
    long gat_np, adv_np;
    int gat_B;
    /* the KL monitor's estimator (ppo_set_kl_estimator; 0 = k3, as ever; 1 = the closed-form KL(old ‖ new)): while
     * it is 1 and the monitor is on, every ppo_update forwards μ over the buffer at its head into kl_old
     * [capacity, A] (means or logits, row r at r·A) and snapshots log σ into kl_old_ls [A]; the policy steps' KL
     * launch reads both in place.  kl_old_rows: the rows the last update filled (0: none).  All NULL until first
     * used; a function of (parameters, buffer), so no checkpoint keeps the store — only the setting */
    int kl_est;
    float *kl_old, *kl_old_ls;
    long kl_old_rows;
    /* the state-dependent-σ Gaussian (ppo_set_action_gaussian_sd; action_dist == 3; csrc/gauss_sd.hip): μ's A outputs
     * are A / 2 means and A / 2 raw log σ, clamped to sd_ls = {ls_min, ls_max} on read.  sd_rec: the head's device
     * record — the last policy step's loss, entropy sum and the counters {clamped log-σ elements, elements};
     * sd_rows: that step's rows.  NULL until the setter first succeeds */
    float sd_ls[2];
    PhipSdRec* sd_rec;
    int sd_rows;
} PPODev;

/* ppo.c: the PPO's PPODev, created on first use (as every setter does) */
PPODev* ppo_dev(PPO* ppo);
/* ppo.c: the rollout's row map for E × T (rows[t·E + e] = e·T + t), as the rollouts build it; sets ro_T */
void ppo_dev_ro_rows(PPODev* d, int E, int T);
/* ppo.c: the rates an update starting now passes by value {policy, value} under the schedule as it stands */
void ppo_dev_lr_now(PPO* ppo, PPODev* d, float* out2);
/* ppo.c: save_ppo's byte stream into an open file, and load_ppo's read of it */
void save_ppo_file(PPO* ppo, FILE* f);
PPO* load_ppo_file(FILE* f, bool use_cuda);

#endif
