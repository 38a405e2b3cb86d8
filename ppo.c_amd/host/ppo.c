/*
 * ppo.c — PPO orchestration (reference /root/reference/src/ppo.cu).
 *
 * The update (GAE → value epochs → policy epochs) is issued entirely on
 * libppo's HIP stream: no per-minibatch allocation, no device→host reads
 * (the reference blocks on 1–2 scalar copies per minibatch), the
 * losses accumulate on the device.  Per value minibatch:
 *     gather → L × fused linear(+bias+ReLU) → MSE+grad → L × bwd_W(+bias grad)
 *     → (L−1) × bwd_x(+ReLU′) → [RCCL all-reduce] → flat Adam
 * and per policy minibatch the same with the fused Gaussian/clipped-surrogate
 * head (csrc/kernels.hip) in place of the MSE.
 */
#include "internal.h"
#include "ppo_dev.h"                  /* PPODev: the device workspaces and the options' state */

#include <math.h>

void buffer_point_device(TrajectoryBuffer* b);

static float* g_v = NULL;         /* V(state), V(next_state) for compute_gae_cuda */
static float* g_vn = NULL;
static int* g_own = NULL;         /* transitions whose V(next_state) needs its own forward */
static long g_v_cap = 0;
static double* g_welford = NULL;  /* (n, mean, M2) */
static double* g_welford_all = NULL;
static int g_welford_world = 0;
static float* g_adv_stats = NULL; /* (mean, std) as used for normalisation */
static long g_gae_own_rows = 0;   /* rows of the last GAE's own V(next_state) forward */
static long g_gae_n = 0;          /* transitions of the last GAE */

static void ensure_gae_ws(long n) {
    if (!g_welford) {
        g_welford = (double*)phip_malloc(4 * sizeof(double));
        g_adv_stats = (float*)phip_malloc(4 * sizeof(float));
    }
    const int world = phip_comm_world();
    if (world > g_welford_world) {
        phip_free(g_welford_all);
        g_welford_all = (double*)phip_malloc(sizeof(double) * 3 * (size_t)world);
        g_welford_world = world;
    }
    if (n > g_v_cap) {
        phip_free(g_v);
        phip_free(g_vn);
        phip_free(g_own);
        g_v = (float*)phip_malloc(sizeof(float) * (size_t)n);
        g_vn = (float*)phip_malloc(sizeof(float) * (size_t)n);
        g_own = (int*)phip_malloc(sizeof(int) * (size_t)n);
        g_v_cap = n;
    }
}

static PPODev* dev_ws(PPO* ppo, int B) {
    PPODev* d = (PPODev*)ppo->dev;
    const int S = ppo->buffer->state_size, A = ppo->buffer->action_size;
    if (!d) {
        d = (PPODev*)xcalloc(1, sizeof(PPODev));
        d->stats = (float*)phip_malloc(4 * sizeof(float));
        d->max_v = d->max_p = -1;
        d->ep_gamma = 0.99f;
        d->clip[0] = (PhipClipRec*)phip_malloc(sizeof(PhipClipRec));
        d->clip[1] = (PhipClipRec*)phip_malloc(sizeof(PhipClipRec));
        d->kl = (PhipKlRec*)phip_malloc(sizeof(PhipKlRec));
        d->vclip_counts = (unsigned long long*)phip_malloc(2 * sizeof(unsigned long long));
        d->cat_ent = (float*)phip_malloc(4 * sizeof(float));
        ppo->dev = d;
    }
    if (B > d->cap_B) {
        phip_free(d->states); phip_free(d->actions); phip_free(d->old_lp); phip_free(d->adv);
        phip_free(d->tgt); phip_free(d->gv); phip_free(d->gmu); phip_free(d->rows);
        phip_free(d->rows_p); phip_free(d->states_p);
        d->rows = (int*)phip_malloc(sizeof(int) * (size_t)B);
        d->rows_p = (int*)phip_malloc(sizeof(int) * (size_t)B);
        d->states = (float*)phip_malloc(sizeof(float) * (size_t)B * S);
        d->states_p = (float*)phip_malloc(sizeof(float) * (size_t)B * S);
        d->actions = (float*)phip_malloc(sizeof(float) * (size_t)B * A);
        d->old_lp = (float*)phip_malloc(sizeof(float) * (size_t)B);
        d->adv = (float*)phip_malloc(sizeof(float) * (size_t)B);
        d->tgt = (float*)phip_malloc(sizeof(float) * (size_t)B);
        d->gv = (float*)phip_malloc(sizeof(float) * (size_t)B);
        d->gmu = (float*)phip_malloc(sizeof(float) * (size_t)B * A);
        d->cap_B = B;
    }
    d->S = S;
    d->A = A;
    return d;
}

PPODev* ppo_dev(PPO* ppo) { return dev_ws(ppo, 1); }

/* learning-rate schedules (ppo_ext.h ppo_set_lr_schedule) */
static int lr_adaptive(const PPODev* d) { return d && d->lr_kind == PPO_LR_ADAPTIVE; }
/* the KL monitor's setting: the caller's target_kl, or — while the adaptive schedule is on and target KL is off —
 * +inf: measure every policy step, never stop */
static float kl_target(const PPODev* d) {
    return d->target_kl > 0.f ? d->target_kl : lr_adaptive(d) ? INFINITY : 0.f;
}
/* the closed-form estimator decides (ppo_set_kl_estimator): it is selected AND the monitor runs */
static int kl_exact(const PPODev* d) { return d->kl_est == PPO_KL_EXACT && kl_target(d) > 0.f; }
static float clampf(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }
/* linear decay: (float)(base · (1 − (1 − f)·(min(u, N)/N))) in double, rounded once; the quotient first, so that
 * u >= N gives exactly (float)(base · f) for every N */
static float lr_linear(float base, const PPODev* d) {
    const double N = (double)d->lr_p[0], f = (double)d->lr_p[1];
    const double u = (double)d->lr_u < N ? (double)d->lr_u : N;
    return (float)((double)base * (1.0 - (1.0 - f) * (u / N)));
}
void ppo_dev_lr_now(PPO* ppo, PPODev* d, float* out2) {
    const int lin = d->lr_kind == PPO_LR_LINEAR;
    out2[0] = lin ? lr_linear(ppo->lr_policy, d) : ppo->lr_policy;
    out2[1] = lin ? lr_linear(ppo->lr_V, d) : ppo->lr_V;
}

static void free_dev_ws(PPO* ppo) {
    PPODev* d = (PPODev*)ppo->dev;
    if (!d) return;
    phip_free(d->states); phip_free(d->actions); phip_free(d->old_lp); phip_free(d->adv);
    phip_free(d->tgt); phip_free(d->gv); phip_free(d->gmu); phip_free(d->stats); phip_free(d->rows);
    phip_free(d->ro_rows); phip_free(d->env_state); phip_free(d->perm[0]); phip_free(d->perm[1]);
    phip_free(d->rows_p); phip_free(d->states_p);
    for (int i = 0; i < 3; i++) phip_free(d->tiny_steps[i]);
    phip_free(d->tab[0]); phip_free(d->tab[1]); phip_free(d->ctr);
    phip_free(d->ph_rows[0]); phip_free(d->ph_rows[1]); phip_free(d->ph_tgt); phip_free(d->ph_act);
    phip_free(d->ph_olp); phip_free(d->ph_adv);
    phip_free(d->clip[0]); phip_free(d->clip[1]);
    phip_free(d->kl);
    phip_free(d->vclip_counts);
    phip_free(d->cat_ent);
    phip_free(d->md_off); phip_free(d->cat_off);
    phip_free(d->obs_run); phip_free(d->obs_m); phip_free(d->obs_shadow); phip_free(d->obs_next);
    phip_free(d->obs_batch); phip_free(d->obs_all); phip_free(d->obs_counts);
    phip_free(d->rew_run); phip_free(d->rew_scale); phip_free(d->rew_shadow); phip_free(d->rew_batch);
    phip_free(d->rew_all); phip_free(d->rew_counts);
    phip_free(d->ro_cont); phip_free(d->rew_carry_in); phip_free(d->rew_carry_out);
    phip_free(d->ep_state); phip_free(d->ep_agg);
    phip_free(d->ev_env); phip_free(d->ev_obs); phip_free(d->ev_obsn); phip_free(d->ev_act); phip_free(d->ev_lp);
    phip_free(d->ev_reward); phip_free(d->ev_rows); phip_free(d->ev_term); phip_free(d->ev_trunc);
    phip_free(d->ev_cont); phip_free(d->ev_agg);
    phip_free(d->ext_obs); phip_free(d->act_obsn); phip_free(d->act_lp); phip_free(d->act_rows);
    phip_free(d->mask);
    phip_free(d->adv_stats);
    phip_free(d->kl_old); phip_free(d->kl_old_ls);
    phip_free(d->sd_rec);
    free(d->h_tab);
    free(d);
    ppo->dev = NULL;
}

/* ------------------------------------------------------------------ */
/* construction (ppo.cu:6-51)                                          */
/* ------------------------------------------------------------------ */
PPO* create_ppo(char** activation_functions, int* layer_sizes, int num_layers, int buffer_size, float lr_policy,
                float lr_v, float lambda, float epsilon, float ent_coeff, float init_std, bool use_cuda) {
    PPO* ppo = (PPO*)xcalloc(1, sizeof(PPO));
    ppo->buffer = create_trajectory_buffer(buffer_size, layer_sizes[0], layer_sizes[num_layers - 1]);
    ppo->policy = create_gaussian_policy(layer_sizes, activation_functions, num_layers, init_std);
    int* sizes_v = (int*)xmalloc(sizeof(int) * (size_t)num_layers);
    memcpy(sizes_v, layer_sizes, sizeof(int) * (size_t)(num_layers - 1));
    sizes_v[num_layers - 1] = 1;                                         /* ppo.cu:12-16 */
    ppo->V = create_neural_network(sizes_v, activation_functions, num_layers);
    free(sizes_v);
    ppo->adam_policy = create_adam_from_nn_cuda(ppo->policy->mu, 0.9f, 0.999f);
    ppo->adam_V = create_adam_from_nn_cuda(ppo->V, 0.9f, 0.999f);
    ppo->adam_entropy = create_adam_cuda(&ppo->policy->d_log_std, &ppo->policy->d_log_std_grad,
                                         &ppo->policy->action_size, 1, ppo->policy->action_size, 0.9f, 0.999f);
    ppo->lambda = lambda;
    ppo->epsilon = epsilon;
    ppo->ent_coeff = ent_coeff;
    ppo->lr_policy = lr_policy;
    ppo->lr_V = lr_v;
    ppo->use_cuda = use_cuda;
    ppo->dev = NULL;
    return ppo;
}

void free_ppo(PPO* ppo) {
    if (!ppo) return;
    free_adam_cuda(ppo->adam_policy);
    free_adam_cuda(ppo->adam_V);
    free_adam_cuda(ppo->adam_entropy);
    free_trajectory_buffer(ppo->buffer, ppo->use_cuda);
    free_gaussian_policy(ppo->policy);
    free_neural_network(ppo->V);
    free_dev_ws(ppo);
    free(ppo);
}

/* ------------------------------------------------------------------ */
/* rollout (ppo.cu:54-79) — host loop over the Env ABI, out of scope of the accelerated path */
/* ------------------------------------------------------------------ */
void collect_trajectories(TrajectoryBuffer* buffer, Env* env, GaussianPolicy* policy, int steps) {
    if (buffer->on_device) buffer_to_host(buffer);
    env->reset_env(buffer->state(buffer, buffer->idx));
    for (int i = 0; i < steps; i++) {
        sample_action(policy, buffer->state(buffer, buffer->idx), buffer->action(buffer, buffer->idx),
                      buffer->logprob(buffer, buffer->idx), 1);
        env->step_env(buffer->action(buffer, buffer->idx), buffer->next_state(buffer, buffer->idx),
                      buffer->reward(buffer, buffer->idx), buffer->terminated(buffer, buffer->idx),
                      buffer->truncated(buffer, buffer->idx), buffer->action_size);
        int new_idx = (buffer->idx + 1) % buffer->capacity;
        if (i < steps - 1) {
            if (*buffer->truncated(buffer, buffer->idx) || *buffer->terminated(buffer, buffer->idx))
                env->reset_env(buffer->state(buffer, new_idx));
            else
                memcpy(buffer->state(buffer, new_idx), buffer->next_state(buffer, buffer->idx),
                       sizeof(float) * (size_t)buffer->state_size);
        } else if (!*buffer->terminated(buffer, buffer->idx)) {
            *buffer->truncated(buffer, buffer->idx) = true;
        }
        buffer->idx = new_idx;
        buffer->full = buffer->full || buffer->idx == 0;
    }
}

/* ------------------------------------------------------------------ */
/* GAE (ppo.cu:261-369)                                                */
/* ------------------------------------------------------------------ */
/* PPO_GAE_FULL=1: evaluate V over every next_state row as the reference does (A/B checks) */
static int gae_full_forwards(void) {
    const char* e = getenv("PPO_GAE_FULL");
    return e && *e && *e != '0';
}

/* ------------------------------------------------------------------ */
/* running observation normalisation (ppo_ext.h ppo_set_obs_norm)      */
/* ------------------------------------------------------------------ */
static int obs_on(const PPODev* d) { return d && d->obs_clip > 0.f; }
/* a discrete policy: categorical (1) or multi-discrete (2) — μ's outputs are logits, log σ is unread */
static int cat_on(const PPODev* d) { return d && (d->action_dist == 1 || d->action_dist == 2); }
static int md_on(const PPODev* d) { return d && d->action_dist == 2; }
/* the state-dependent-σ Gaussian (3): μ's outputs are [mean | raw log σ], the log σ vector is unread */
static int sd_on(const PPODev* d) { return d && d->action_dist == 3; }
/* the multi-discrete offsets for the environment and KL launches: NULL unless it is on */
static const int* md_off(const PPODev* d) { return md_on(d) ? d->md_off : NULL; }

/* the shape the discrete kernels (discrete.hip) run either policy with: the offsets, the component count and the
 * widest component (the categorical policy as nvec = {A}) */
static const int* disc_off(const PPODev* d) { return md_on(d) ? d->md_off : d->cat_off; }
static int disc_D(const PPODev* d) { return md_on(d) ? d->md_D : 1; }
static int disc_max_n(const PPODev* d, int A) { return md_on(d) ? d->md_max_n : A; }
/* action masking: on, and the words of one row */
static int mask_on(const PPODev* d) { return cat_on(d) && d->mask_on && d->mask; }
static int mask_words(int A) { return (A + 31) / 32; }
/* rows [0, n) of the store ← full masks: what an unmasked sampler lays */
static void mask_fill_full(PPODev* d, long n, int A) {
    if (mask_on(d)) phip_memset(d->mask, 0xFF, sizeof(uint32_t) * (size_t)n * (size_t)mask_words(A));
}

/* the running triple and its affine pair (the identity until something is folded or set) */
static void obs_ws(PPO* ppo, PPODev* d) {
    if (d->obs_run) return;
    const int S = ppo->buffer->state_size;
    d->obs_run = (double*)phip_malloc(sizeof(double) * (size_t)(1 + 2L * S));
    d->obs_batch = (double*)phip_malloc(sizeof(double) * (size_t)(1 + 2L * S));
    d->obs_m = (float*)phip_malloc(sizeof(float) * 2 * (size_t)S);
    d->obs_counts = (unsigned long long*)phip_malloc(2 * sizeof(unsigned long long));
    phip_obs_affine(d->obs_run, S, d->obs_m, d->obs_m + S);
}

static float* obs_shadow(PPO* ppo, PPODev* d) {
    obs_ws(ppo, d);
    if (!d->obs_shadow)
        d->obs_shadow = (float*)phip_malloc(sizeof(float) * (size_t)ppo->buffer->capacity * ppo->buffer->state_size);
    return d->obs_shadow;
}

/* this rank's batch triple (d->obs_batch, already queued) into the running triple: all-gathered and combined
 * in rank order at world > 1, so every rank folds the same bits; then the affine pair is refreshed */
static void obs_fold_batch(PPO* ppo, PPODev* d) {
    const int S = ppo->buffer->state_size;
    const int world = phip_comm_world();
    if (world > 1) {
        if (world > d->obs_all_world) {
            phip_free(d->obs_all);
            d->obs_all = (double*)phip_malloc(sizeof(double) * (size_t)(1 + 2L * S) * (size_t)world);
            d->obs_all_world = world;
        }
        phip_allgather_f64(d->obs_batch, d->obs_all, 1 + 2L * S);
        phip_obs_fold(d->obs_all, world, S, d->obs_run);
    } else {
        phip_obs_fold(d->obs_batch, 1, S, d->obs_run);
    }
    phip_obs_affine(d->obs_run, S, d->obs_m, d->obs_m + S);
}

/* steps 1 and 2 of the update while the feature is on, stream-ordered ahead of GAE: the shadow of
 * state[0:limit] under the affine pair as it stands (the pair the rollout sampled under), and — unless
 * frozen — this rank's batch triple over the RAW rows; gae_device folds it behind its own all-gather.
 * Returns the shadow. */
static const float* obs_prepare(PPO* ppo, PPODev* d, int limit) {
    TrajectoryBuffer* buf = ppo->buffer;
    const int S = buf->state_size;
    float* sh = obs_shadow(ppo, d);
    phip_memset(d->obs_counts, 0, 2 * sizeof(unsigned long long));
    phip_obs_normalize(buf->state_p, sh, limit, S, d->obs_m, d->obs_m + S, d->obs_clip, d->obs_run, d->obs_counts);
    if (!d->obs_frozen) phip_obs_stats(buf->state_p, limit, S, d->obs_batch);
    return sh;
}

/* the next_state rows listed in `rows` (NULL: the first m rows) normalised into the compact scratch */
static const float* obs_next_rows(PPODev* d, TrajectoryBuffer* b, const int* rows, int m) {
    const int S = b->state_size;
    if (m > d->obs_next_cap) {
        phip_free(d->obs_next);
        d->obs_next = (float*)phip_malloc(sizeof(float) * (size_t)m * S);
        d->obs_next_cap = m;
    }
    phip_obs_normalize_rows(b->next_state_p, rows, d->obs_next, NULL, m, S, d->obs_m, d->obs_m + S, d->obs_clip,
                            d->obs_run);
    return d->obs_next;
}

/* ------------------------------------------------------------------ */
/* running return-based reward normalisation (ppo_ext.h ppo_set_reward_norm) */
/* ------------------------------------------------------------------ */
static int rew_on(const PPODev* d) { return d && d->rew_clip > 0.f; }

/* the running triple and its scale (the identity, s = 1, until something is folded or set) */
static void rew_ws(PPODev* d) {
    if (d->rew_run) return;
    d->rew_run = (double*)phip_malloc(3 * sizeof(double));
    d->rew_batch = (double*)phip_malloc(3 * sizeof(double));
    d->rew_scale = (float*)phip_malloc(sizeof(float));
    d->rew_counts = (unsigned long long*)phip_malloc(2 * sizeof(unsigned long long));
    phip_ret_fold(NULL, 0, d->rew_run, d->rew_scale, NULL);
}

/* the update's steps 1 to 4 while the feature is on, stream-ordered ahead of GAE's forwards and with no host
 * read: the scan of the raw reward[0:limit] into this rank's batch triple and carry_out, the fold (at world > 1
 * behind the all-gather every rank reaches here, an empty shard with the zero triple), the refreshed scale and
 * the scaled, clamped shadow.  Frozen: the shadow alone, under the scale as it stands.  Returns the shadow. */
static const float* rew_prepare(PPO* ppo, PPODev* d, int limit, float gamma) {
    TrajectoryBuffer* buf = ppo->buffer;
    rew_ws(d);
    if (!d->rew_shadow) d->rew_shadow = (float*)phip_malloc(sizeof(float) * (size_t)buf->capacity);
    if (d->rew_frozen) {
        phip_memset(d->rew_counts, 0, 2 * sizeof(unsigned long long));
    } else {
        /* rows e·T of a buffer ppo_rollout_device laid take carry_in[e]; any other buffer is one stream */
        const int laid = d->ro_laid && limit > 0 && (long)d->ro_E * d->ro_T == limit;
        const int world = phip_comm_world();
        phip_ret_scan(buf->reward_p, (const uint8_t*)buf->terminated_p, (const uint8_t*)buf->truncated_p, limit, gamma,
                      laid ? d->ro_T : 0, laid ? d->rew_carry_in : NULL, laid ? d->ro_cont : NULL, NULL,
                      laid ? d->rew_carry_out : NULL, d->rew_batch, world > 1 ? NULL : d->rew_run,
                      world > 1 ? NULL : d->rew_scale, d->rew_counts);
        if (laid) d->rew_scanned = 1;
        if (world > 1) {
            if (world > d->rew_all_world) {
                phip_free(d->rew_all);
                d->rew_all = (double*)phip_malloc(3 * sizeof(double) * (size_t)world);
                d->rew_all_world = world;
            }
            phip_allgather_f64(d->rew_batch, d->rew_all, 3);
            phip_ret_fold(d->rew_all, world, d->rew_run, d->rew_scale, NULL);
        }
    }
    phip_ret_scale(buf->reward_p, d->rew_shadow, limit, d->rew_scale, d->rew_clip, d->rew_run, d->rew_counts);
    return d->rew_shadow;
}

/* ppo: NULL (compute_gae_cuda / compute_gae: no normaliser, raw states), or the PPO whose update runs this
 * GAE with observation normalisation on (obs_prepare has run): the forwards read the shadow, the own
 * next_state rows are normalised into a compact scratch, and the batch triple is folded behind the scan.
 * reward: the rows the scan reads — the buffer's, or their scaled shadow (rew_prepare) */
static void gae_device(NeuralNetwork* V, TrajectoryBuffer* b, float gamma, float lambda, PPO* ppo,
                       const float* reward) {
    PPODev* od = ppo ? (PPODev*)ppo->dev : NULL;
    const float* state = od ? od->obs_shadow : b->state_p;
    const int n = b->full ? b->capacity : b->idx;
    g_gae_own_rows = 0;                     /* an empty buffer reports no own-row forward */
    g_gae_n = n;
    ensure_gae_ws(n);
    if (n > 0 && gae_full_forwards()) {     /* the reference's two full forwards (ppo.cu:333-336) */
        nn_forward_dev(V, od ? obs_next_rows(od, b, NULL, n) : b->next_state_p, n);
        phip_d2d(g_vn, V->d_output, sizeof(float) * (size_t)n);
        g_gae_own_rows = n;
        nn_forward_dev(V, state, n);
        phip_d2d(g_v, V->d_output, sizeof(float) * (size_t)n);
    } else if (n > 0) {
        /* V(state) once; V(next_state[t]) = V(state[t+1]) wherever the rows are bitwise equal
         * (every transition that did not end an episode); the rest get their own forward */
        nn_forward_dev(V, state, n);
        phip_d2d(g_v, V->d_output, sizeof(float) * (size_t)n);
        /* the raw rows are compared: equal raw rows give equal normalised rows */
        const int own = phip_next_value_map(b->next_state_p, b->state_p, g_v, g_vn, g_own, n, V->layers[0].input_size);
        g_gae_own_rows = own;
        if (own > 0) {
            if (od) nn_forward_dev(V, obs_next_rows(od, b, g_own, own), own);
            else nn_forward_dev_rows(V, b->next_state_p, g_own, NULL, own);
            phip_scatter_values(g_vn, g_own, V->d_output, own);
        }
    }
    phip_gae_scan(g_v, g_vn, reward, (const uint8_t*)b->terminated_p, (const uint8_t*)b->truncated_p, n, gamma,
                  lambda, b->advantage_p, b->adv_target_p, g_welford);
    const int world = phip_comm_world();
    if (world > 1) {       /* global advantage statistics across env shards */
        phip_allgather_f64(g_welford, g_welford_all, 3);
        phip_welford_combine(g_welford_all, world, g_welford);
    }
    /* right behind the Welford all-gather and ahead of the update's empty-shard agreement: every rank
     * reaches this collective (an empty shard contributes the zero triple) */
    if (od && !od->obs_frozen) obs_fold_batch(ppo, od);
    phip_normalize(b->advantage_p, n, g_welford, g_adv_stats);
}

void ppo_gae_device(NeuralNetwork* V, TrajectoryBuffer* b, float gamma, float lambda) {
    gae_device(V, b, gamma, lambda, NULL, b->reward_p);
}

long ppo_gae_state(double* welford, float* v, float* v_next, long n) {
    phip_sync();
    if (n > g_gae_n) n = g_gae_n;
    if (welford) {
        double w[6] = {0, 0, 0, 0, 0, 0};
        if (g_welford) phip_d2h(w, g_welford, 3 * sizeof(double));
        if (phip_comm_world() > 1 && g_welford_all)
            phip_d2h(w + 3, g_welford_all + 3 * (size_t)phip_comm_rank(), 3 * sizeof(double));
        else
            memcpy(w + 3, w, 3 * sizeof(double));
        memcpy(welford, w, sizeof(w));
    }
    if (v && n > 0) phip_d2h(v, g_v, sizeof(float) * (size_t)n);
    if (v_next && n > 0) phip_d2h(v_next, g_vn, sizeof(float) * (size_t)n);
    return g_gae_n;
}

/* device buffer (after buffer_to_device); `horizon` is unused: the scan is exact (D7) */
void compute_gae_cuda(NeuralNetwork* V, TrajectoryBuffer* buffer, float gamma, float lambda, int horizon) {
    (void)horizon;
    ppo_gae_device(V, buffer, gamma, lambda);
}

/* host buffer: staged through the device mirror */
void compute_gae(NeuralNetwork* V, TrajectoryBuffer* buffer, float gamma, float lambda) {
    const int was_device = buffer->on_device;
    if (!was_device) buffer_to_device(buffer);
    ppo_gae_device(V, buffer, gamma, lambda);
    if (!was_device) buffer_to_host(buffer);
}

/* ------------------------------------------------------------------ */
/* clipped surrogate (ppo.cu:82-169)                                   */
/* ------------------------------------------------------------------ */
float policy_loss_and_grad_cuda(float* grad_logprob, float* grad_entropy, float* adv, float* logprobs,
                                float* old_logprobs, float entropy, float ent_coeff, float epsilon, int m) {
    float* d = (float*)stage(ST_H, 16);
    phip_h2d(d + 1, &entropy, sizeof(float));
    phip_policy_loss(adv, logprobs, old_logprobs, grad_logprob, m, epsilon, ent_coeff, d + 1, d, NULL);
    float loss = 0.f;
    phip_d2h(&loss, d, sizeof(float));
    *grad_entropy = -ent_coeff;
    return loss;
}

float policy_loss_and_grad(float* grad_logprob, float* grad_entropy, float* adv, float* logprobs,
                           float* old_logprobs, float entropy, float ent_coeff, float epsilon, int m) {
    float* da = stage_up(ST_A, adv, (size_t)m);
    float* dl = stage_up(ST_B, logprobs, (size_t)m);
    float* dol = stage_up(ST_C, old_logprobs, (size_t)m);
    float* dg = (float*)stage(ST_D, sizeof(float) * (size_t)(m > 0 ? m : 1));
    float loss = policy_loss_and_grad_cuda(dg, grad_entropy, da, dl, dol, entropy, ent_coeff, epsilon, m);
    phip_d2h(grad_logprob, dg, sizeof(float) * (size_t)m);
    return loss;
}

/* ------------------------------------------------------------------ */
/* the update                                                          */
/* ------------------------------------------------------------------ */
static const int* next_perm(PPO* ppo, PPODev* d, int shuffle_mode, uint64_t* key) {
    if (shuffle_mode == PPO_SHUFFLE_DEVICE) {
        *key = d->key++;
        return NULL;
    }
    shuffle_buffer_cuda(ppo->buffer);                   /* reference: host rand() swap shuffle */
    *key = 0;
    return ppo->buffer->random_idx;
}

/* ------------------------------------------------------------------ */
/* small networks: every minibatch step of a phase in one workgroup    */
/* (csrc/tiny.hip); same arithmetic, rand() order and Adam step counts  */
/* ------------------------------------------------------------------ */
/* max_w: widest layer the kernel takes (128 for the single-workgroup kernel; the multi-workgroup
 * cluster kernel checks its own shapes) */
static int tiny_net(NeuralNetwork* nn, Adam* adam, PhipTinyNet* t, int max_w) {
    const int L = nn->num_layers - 1;
    if (nn->dtype != 0 || L < 1 || L > 8 || !adam_owns(adam, nn->d_params, nn->d_grads)) return -1;
    if (nn_has_tanh(nn)) return -1;      /* the single-workgroup and cluster kernels know relu[i] ∈ {0, 1} only */
    for (int i = 0; i < L; i++)
        if (nn->layers[i].input_size > max_w || nn->layers[i].output_size > max_w) return -1;
    long nw = 0;
    for (int i = 0; i < L; i++) nw += (long)nn->layers[i].input_size * nn->layers[i].output_size;
    if (max_w <= 128 && nw > nn->tiny_wt_cap) {
        phip_free(nn->d_tiny_wt);
        nn->d_tiny_wt = (float*)phip_malloc(sizeof(float) * (size_t)nw);
        nn->tiny_wt_cap = nw;
    }
    memset(t, 0, sizeof(*t));
    t->L = L;
    for (int i = 0; i <= L; i++) t->sizes[i] = nn->layers[i].input_size;
    for (int i = 0; i < L; i++) {
        t->relu[i] = nn_is_relu(nn, i);
        t->woff[i] = nn->param_offset[i];
        t->boff[i] = nn->bias_offset[i];
    }
    if (t->sizes[L] > 32) return -1;
    t->params = nn->d_params;
    t->grads = nn->d_grads;
    t->wt = (float*)nn->d_tiny_wt;
    t->wt_cap = nn->tiny_wt_cap;
    t->m = adam->m;
    t->v = adam->v;
    t->span = adam->span;
    return 0;
}

/* Adam step of a network's flat span; in bf16 mode the same pass refreshes the bf16 parameter
 * shadow when the span starts at the network's parameters, else a separate conversion does.
 * zero_grads: the same pass clears the gradients it read (the next backward skips its memset);
 * rate: by value, or in a device word (the adaptive schedule); coef: NULL, or the step's device clip
 * coefficient; skip: NULL, or the device stop word of target-KL early stopping */
static int adam_update_net(Adam* adam, PhipAdamRate rate, NeuralNetwork* nn, int zero_grads, const float* coef,
                           const unsigned* skip) {
    const int own = adam_owns(adam, nn->d_params, nn->d_grads);
    const int fused = nn->dtype == 1 && own;
    const int r = adam_update_dev(adam, rate, fused ? nn->d_w16 : NULL, nn->num_params, zero_grads && own, coef, skip);
    /* a skipped step left the parameters, hence their shadow, as they were: the refresh rewrites the same bits */
    if (!(r & 1) && nn->dtype == 1) nn_sync_w16(nn);
    return (r & 2) != 0;                 /* the network's gradients are zero again */
}

/* the step-table form of adam_update_net / the entropy Adam (graph replay): flat span, gradients
 * cleared, step sizes from the table; which = 0 advances the step counter (the network's Adam,
 * the step's last kernel), 1 reads the entropy entry */
static void adam_net_tab(Adam* adam, NeuralNetwork* nn, PPODev* d, int ph, int which) {
    const int fused = nn && nn->dtype == 1;
    const PhipAdamSpan s = {adam->weights[0], adam->grad_weights[0], adam->m, adam->v, adam->span, 0.f, 0.f,
                            adam->grad_scale, 1};
    phip_adam_flat_tab(&s, d->tab[ph], d->ctr + ph, (unsigned*)(d->ctr + 2 + ph), which, adam->beta1, adam->beta2,
                       fused ? nn->d_w16 : NULL, fused ? nn->num_params : 0);
    nn_note_device_update(adam->weights[0]);
}

static float* tiny_steps(PPODev* d, int slot, Adam* adam, float lr, int n) {
    float* h = (float*)xmalloc(sizeof(float) * 2 * (size_t)n);
    for (int i = 0; i < n; i++) adam_next_step(adam, lr, &h[2 * i], &h[2 * i + 1]);
    if (n > d->tiny_cap[slot]) {
        phip_free(d->tiny_steps[slot]);
        d->tiny_steps[slot] = (float*)phip_malloc(sizeof(float) * 2 * (size_t)n);
        d->tiny_cap[slot] = n;
    }
    phip_h2d(d->tiny_steps[slot], h, sizeof(float) * 2 * (size_t)n);
    free(h);
    return d->tiny_steps[slot];
}

/* every epoch's minibatch order for one phase (slot 0 value, 1 policy), drawn in the reference's
 * order (one shuffle per epoch): device-shuffle keys into keys[], or host rand() permutations
 * copied into HBM, epoch e at the returned pointer + e·limit */
static const int* phase_perms(PPO* ppo, PPODev* d, int shuffle_mode, int n_epochs, int limit, int slot,
                              uint64_t* keys) {
    if (shuffle_mode == PPO_SHUFFLE_DEVICE) {
        for (int e = 0; e < n_epochs; e++) keys[e] = d->key++;
        return NULL;
    }
    const long need = (long)n_epochs * limit;
    if (need > d->perm_cap[slot]) {
        phip_free(d->perm[slot]);
        d->perm[slot] = (int*)phip_malloc(sizeof(int) * (size_t)need);
        d->perm_cap[slot] = need;
    }
    for (int e = 0; e < n_epochs; e++) {
        shuffle_buffer_cuda(ppo->buffer);
        phip_d2d(d->perm[slot] + (long)e * limit, ppo->buffer->random_idx, sizeof(int) * (size_t)limit);
        keys[e] = 0;
    }
    return d->perm[slot];
}

static const int* tiny_perms(PPO* ppo, PPODev* d, int shuffle_mode, int n_epochs, int limit, PhipTinyPhase* ph) {
    uint64_t keys[16];
    const int* perms = phase_perms(ppo, d, shuffle_mode, n_epochs, limit, ph->policy, keys);
    if (shuffle_mode == PPO_SHUFFLE_DEVICE)
        for (int e = 0; e < n_epochs; e++)
            for (int r = 0; r < 4; r++) ph->feistel_k[4 * e + r] = (uint32_t)splitmix64(keys[e] + (uint64_t)r);
    return perms;
}

/* state: the rows the phases read — the buffer's, or their normalised shadow */
static int ppo_update_tiny(PPO* ppo, PPODev* d, const float* state, int B, int n_epochs_policy, int n_epochs_value,
                           int shuffle_mode) {
    TrajectoryBuffer* buf = ppo->buffer;
    const int limit = buf->full ? buf->capacity : buf->idx;
    const int num_batches = buf->capacity / B;
    if (getenv("PPO_NO_TINY") || phip_comm_world() > 1 || n_epochs_value > 16 || n_epochs_policy > 16) return -1;
    /* the single-workgroup and cluster kernels run their Adam steps inside the launch and do not clip:
     * with gradient clipping on, the update takes the multi-launch loop */
    if (d->max_grad_norm > 0.f) return -1;
    /* … and they neither measure the KL nor read a stop word: target-KL early stopping takes that loop too */
    if (kl_target(d) > 0.f) return -1;
    /* … and their value heads are plain MSE: value-loss clipping takes that loop as well */
    if (d->value_clip > 0.f) return -1;
    /* … and they gather their own advantages: per-minibatch advantage normalisation takes that loop too */
    if (d->adv_norm_mode != PPO_ADV_NORM_GLOBAL) return -1;
    /* … and their policy heads are Gaussian: a categorical policy takes that loop too */
    if (cat_on(d)) return -1;
    /* … as does the state-dependent-σ Gaussian, whose head reads half of μ's outputs as log σ */
    if (sd_on(d)) return -1;
    PhipTinyNet nv, np;
    /* one workgroup per phase for networks ≤ 128 wide; otherwise the cluster kernel (S → 256 → 256 → O
     * at B = 64, cluster.hip) when it takes the shape */
    int cluster = 0;
    if (tiny_net(ppo->V, ppo->adam_V, &nv, 128) || tiny_net(ppo->policy->mu, ppo->adam_policy, &np, 128)) {
        if (tiny_net(ppo->V, ppo->adam_V, &nv, 1 << 20) || tiny_net(ppo->policy->mu, ppo->adam_policy, &np, 1 << 20))
            return -1;
        cluster = 1;
    }
    int (*phase_fn)(const PhipTinyNet*, const PhipTinyPhase*) = cluster ? phip_cluster_update : phip_tiny_update;
    if (!adam_owns(ppo->adam_entropy, NULL, ppo->policy->d_log_std_grad)) return -1;
    GaussianPolicy* pol = ppo->policy;
    np.log_std = pol->d_log_std;
    np.log_std_grad = pol->d_log_std_grad;
    np.m_ls = ppo->adam_entropy->m;
    np.v_ls = ppo->adam_entropy->v;
    PhipTinyPhase ph;
    memset(&ph, 0, sizeof(ph));
    ph.state = state; ph.action = buf->action_p; ph.logprob = buf->logprob_p;
    ph.adv = buf->advantage_p; ph.adv_target = buf->adv_target_p;
    ph.limit = limit; ph.B = B; ph.num_batches = num_batches;
    ph.b1 = 0.9f; ph.b2 = 0.999f; ph.eps = ppo->epsilon; ph.ent_coeff = ppo->ent_coeff;
    ph.stats = d->stats;
    /* fit check before any state (rand() stream, Adam steps, keys) is consumed: a dry phase */
    {
        PhipTinyNet probe = nv;
        PhipTinyPhase pp = ph;
        pp.n_epochs = 0;
        if (phase_fn(&probe, &pp) != 0) return -1;
        probe = np;
        pp.policy = 1;
        if (phase_fn(&probe, &pp) != 0) return -1;
    }
    /* both phases' permutations and Adam step tables first, in the reference's order (value
     * epochs' shuffles, then the policy's); then the two single-workgroup phases run concurrently
     * (value on libppo's stream, policy on the side stream: they share only read-only buffer
     * arrays), each on its own CU.  PPO_SERIAL=1 runs them one after the other. */
    PhipTinyPhase pv = ph, pp = ph;
    /* step caps (ppo_set_step_limit): the first max steps of each phase, as in the multi-launch loop */
    long cap_v = (long)n_epochs_value * num_batches, cap_p = (long)n_epochs_policy * num_batches;
    if (d->max_v >= 0 && cap_v > d->max_v) cap_v = d->max_v;
    if (d->max_p >= 0 && cap_p > d->max_p) cap_p = d->max_p;
    const int run_v = cap_v > 0, run_p = cap_p > 0;
    if (run_v) {
        pv.policy = 0;
        pv.n_epochs = n_epochs_value;
        pv.max_steps = cap_v;
        pv.perms = tiny_perms(ppo, d, shuffle_mode, n_epochs_value, limit, &pv);
        pv.steps = tiny_steps(d, 0, ppo->adam_V, d->lr_use[1], (int)cap_v);
    } else if (n_epochs_value > 0) {
        for (int j = 0; j < n_epochs_value; j++) { uint64_t key; next_perm(ppo, d, shuffle_mode, &key); }
    }
    if (run_p) {
        pp.policy = 1;
        pp.n_epochs = n_epochs_policy;
        pp.max_steps = cap_p;
        pp.perms = tiny_perms(ppo, d, shuffle_mode, n_epochs_policy, limit, &pp);
        /* per step the entropy Adam steps before the policy Adam (ppo.cu:440-442); their step
         * counters are independent, so the two sequences can be generated one after the other */
        pp.steps_ls = tiny_steps(d, 1, ppo->adam_entropy, d->lr_use[0], (int)cap_p);
        pp.steps = tiny_steps(d, 2, ppo->adam_policy, d->lr_use[0], (int)cap_p);
    } else if (n_epochs_policy > 0) {
        for (int j = 0; j < n_epochs_policy; j++) { uint64_t key; next_perm(ppo, d, shuffle_mode, &key); }
    }
    const char* serial_env = getenv("PPO_SERIAL");
    const int concurrent = run_v && run_p && !(serial_env && *serial_env && *serial_env != '0');
    if (concurrent) phip_side_fork();
    if (run_v) {
        if (phase_fn(&nv, &pv) != 0) die("ppo_update: single-launch value phase failed to launch");
        d->n_v += cap_v;
    }
    if (run_p) {
        if (concurrent) phip_side_use(1);
        if (phase_fn(&np, &pp) != 0) die("ppo_update: single-launch policy phase failed to launch");
        if (concurrent) phip_side_use(0);
        d->n_p += cap_p;
    }
    if (concurrent) phip_side_join();
    if (cluster) {
        /* a barrier timeout leaves the phase's parameters and Adam state half-written (the workgroups
         * leave without their write-back): detect it before this update returns, so no caller reads,
         * checkpoints or continues from that state */
        phip_sync();
        if (phip_cluster_error())
            die("ppo_update: a multi-workgroup phase (cluster.hip) timed out at a grid barrier; "
                "the update's parameters and Adam state are incomplete");
        phip_cluster_report();
    }
    return 0;
}

/* ------------------------------------------------------------------ */
/* one value / policy minibatch step (ppo.cu:395-443 bodies)           */
/* ------------------------------------------------------------------ */
/* gradient clipping (off: NULL, nothing launched): the global L2 norm of the loop's summed gradient
 * — the Adam's flat span plus `side` (the policy's log σ gradient) — and the clip coefficient, on the
 * device (clip.hip), after the all-reduce has joined and before the step's Adam, which reads the
 * coefficient through the returned pointer.  Under data parallelism the buffer holds the sum over ranks
 * and every rank computes the same bits from it, so the replicas stay identical. */
static const float* clip_coef(PPODev* d, int ph, Adam* adam, const float* side, int n_side) {
    if (!(d->max_grad_norm > 0.f)) return NULL;
    if (!adam->flat) die("ppo_update: gradient clipping needs flat Adam spans");
    phip_grad_norm(adam->grad_weights[0], adam->span, side, n_side, adam->grad_scale, d->max_grad_norm, d->clip[ph]);
    return &d->clip[ph]->coef;
}

typedef struct {
    PPO* ppo;
    PPODev* d;
    int B, S, A, limit, num_batches, comm, fuse_v, fuse_p, wide_p, fold_v;
    const int *perms_v, *perms_p;
    const uint64_t *keys_v, *keys_p;
    long nv, np;
    void *gv, *gp;                /* captured graphs of K steps each (value, policy) */
    void *gv1, *gp1;              /* … and of one step (the remainder) */
    int K;                        /* requested steps per graph (PPO_GRAPH_STEPS, default 16) */
    long Kv, Kp;                  /* steps per graph as captured */
    int phg;                      /* the phases' inputs were gathered up front (PPODev ph_*) */
    const float* state;           /* layer 0's rows: buf->state_p, or its normalised shadow (obs_prepare) */
} StepCtx;

/* value step iv (tab: the step-table form captured into a graph: gather and Adam read their
 * per-step arguments from d->tab[0] at the device step counter); returns whether its Adam cleared
 * the gradients */
static int value_step(StepCtx* c, long iv, int v_zero, int tab) {
    PPO* ppo = c->ppo;
    PPODev* d = c->d;
    TrajectoryBuffer* buf = ppo->buffer;
    NeuralNetwork* V = ppo->V;
    const int B = c->B;
    const int* rows = d->rows;
    const float* tgt = d->tgt;
    if (tab) {
        phip_gather_rows_tab(d->tab[0], d->ctr + 0, c->perms_v, c->limit, B, c->A, buf->action_p, buf->logprob_p,
                             buf->advantage_p, buf->adv_target_p, NULL, NULL, NULL, d->tgt, d->rows);
    } else if (c->phg) {
        rows = d->ph_rows[0] + iv * B;
        tgt = d->ph_tgt + iv * B;
    } else {
        const int j = (int)(iv / c->num_batches), k = (int)(iv % c->num_batches);
        const int* perm = c->perms_v ? c->perms_v + (long)j * c->limit : NULL;
        /* gather fused into layer 0: the kernel emits row indices (+ targets); the layer-0 GEMM
         * reads the buffer rows through them and leaves the gathered copy for its grad_W */
        phip_gather_rows(perm, c->keys_v[j], k * B, c->limit, B, c->S, c->A, c->state, buf->action_p,
                         buf->logprob_p, buf->advantage_p, buf->adv_target_p, NULL, NULL, NULL, NULL, d->tgt, d->rows);
    }
    /* value-loss clipping (off: NULL, every head runs its arithmetic and launches as before): slot i's old
     * value is v_old[rows[i]], read inside whichever form of the head the step takes — no launch of its own.
     * The default old values are g_v, the V(state) of every buffer row that this update's own GAE left behind:
     * a global that any later compute_gae_cuda call overwrites, but inside ppo_update the GAE has just run and
     * nothing rewrites it before the update returns, so it is valid for every value step.  The head is
     * element-wise: no collective is added, and the order of collectives does not depend on the setting. */
    PhipVClip vclip = {d->v_old_user ? d->v_old_user : g_v, rows, d->value_clip, d->vclip_counts};
    const PhipVClip* vc = !tab && d->value_clip > 0.f ? &vclip : NULL;
    /* with a communicator: the gradients all-reduced after the backward (comm.hip: one all-reduce in
     * this stream by default; PPO_COMM_ASYNC=1 per-layer buckets on the comm stream), joined before Adam */
    if (c->fold_v && !tab) {   /* output layer + MSE folded into the last hidden layer (nn_value_fold_step) */
        nn_value_fold_step(V, c->state, rows, d->states, B, v_zero, c->comm ? 0 : -1, tgt, d->stats + 0, vc);
    } else if (c->fuse_v) {    /* output layer + MSE + output-layer backward in one pass (out_head.hip) */
        nn_out_head_step(V, 0, c->state, rows, d->states, B, v_zero, c->comm ? 0 : -1, tgt, NULL, NULL,
                         NULL, NULL, 0.f, 0.f, NULL, d->stats + 0, vc);
    } else {
        nn_forward_dev_rows(V, c->state, rows, d->states, B);
        if (vc) phip_mse_vclip(V->d_output, tgt, B, d->gv, d->stats + 0, vc);      /* the same kernel and grid */
        else phip_mse(V->d_output, tgt, B, d->gv, NULL, d->stats + 0);
        nn_backward_dev_z(V, d->gv, B, 0, v_zero, c->comm ? 0 : -1);
    }
    phip_allreduce_join();
    if (tab) {
        adam_net_tab(ppo->adam_V, V, d, 0, 0);
        return 1;
    }
    /* the value rate: by value (the schedule's, d->lr_use), or — the adaptive schedule with coupling — the word the
     * coupling launch wrote ahead of the loops */
    const PhipAdamRate rate = {d->lr_use[1], lr_adaptive(d) && d->lr_couple ? &d->kl->lr_v : NULL};
    return adam_update_net(ppo->adam_V, rate, V, iv + 1 < c->nv, clip_coef(d, 0, ppo->adam_V, NULL, 0), NULL);
}

static void policy_step(StepCtx* c, long ip, int* p_zero, int* ls_zero, int tab) {
    PPO* ppo = c->ppo;
    PPODev* d = c->d;
    TrajectoryBuffer* buf = ppo->buffer;
    GaussianPolicy* pol = ppo->policy;
    NeuralNetwork* mu = pol->mu;
    const int B = c->B, A = c->A;
    const int* rows = d->rows_p;
    const float *act = d->actions, *olp = d->old_lp, *adv = d->adv;
    if (tab) {
        phip_gather_rows_tab(d->tab[1], d->ctr + 1, c->perms_p, c->limit, B, A, buf->action_p, buf->logprob_p,
                             buf->advantage_p, buf->adv_target_p, d->actions, d->old_lp, d->adv, NULL, d->rows_p);
    } else if (c->phg) {
        rows = d->ph_rows[1] + ip * B;
        act = d->ph_act + ip * B * A;
        olp = d->ph_olp + ip * B;
        adv = d->ph_adv + ip * B;
    } else {
        const int j = (int)(ip / c->num_batches), k = (int)(ip % c->num_batches);
        const int* perm = c->perms_p ? c->perms_p + (long)j * c->limit : NULL;
        phip_gather_rows(perm, c->keys_p[j], k * B, c->limit, B, c->S, A, c->state, buf->action_p,
                         buf->logprob_p, buf->advantage_p, buf->adv_target_p, NULL, d->actions, d->old_lp, d->adv,
                         NULL, d->rows_p);
    }
    /* μ grads + (top bucket) the log σ gradient behind them */
    const int cat = !tab && cat_on(d);
    const int sd = !tab && sd_on(d);
    /* the KL monitor under masking: the masked joint lp, the categorical policy as nvec = {A} */
    const int kl_mask = cat && mask_on(d);
    const int kl_dist = kl_mask ? 2 : cat || sd ? d->action_dist : 0;
    const int* kl_off = kl_mask ? disc_off(d) : md_off(d);
    const int kl_D = kl_mask ? disc_D(d) : d->md_D;
    const uint32_t* kl_m = kl_mask ? d->mask : NULL;
    if (cat) {             /* a discrete policy: the plain branch with its own head */
        /* log σ is unused: the head writes no gradient to it, and the entropy Adam below steps on the zeros
         * kept here, which leaves log σ bit-identical */
        /* ppo_set_action_dist and ppo_set_compute_dtype decline the pair; nn_set_compute_dtype on μ itself does not
         * know the PPO, so the combination is caught where it would run: the head reads fp32 logits */
        if (mu->dtype != 0)
            die(md_on(d) ? "ppo_update: the multi-discrete policy needs fp32 compute mode (μ is in bf16 mode)"
                         : "ppo_update: the categorical policy needs fp32 compute mode (μ is in bf16 mode)");
        if (!*ls_zero) phip_memset(pol->d_log_std_grad, 0, sizeof(float) * (size_t)A);
        *ls_zero = 1;
        phip_memset(d->cat_ent, 0, sizeof(float));
        d->cat_rows = B;
        nn_forward_dev_rows(mu, c->state, rows, d->states_p, B);
        const int masked = mask_on(d);
        if (!md_on(d) && !masked)     /* the categorical policy's register-resident head (categorical.hip) */
            phip_cat_head(mu->d_output, act, adv, olp, B, A, ppo->epsilon, ppo->ent_coeff, d->gmu, NULL, NULL,
                          d->stats + 1, d->cat_ent);
        else               /* the tile head; under masking the stored masks, read in place through the row indices */
            phip_disc_head(mu->d_output, act, adv, olp, masked ? d->mask : NULL, masked ? rows : NULL, B, A,
                           disc_off(d), disc_D(d), disc_max_n(d, A), ppo->epsilon, ppo->ent_coeff, d->gmu, NULL, NULL,
                           d->stats + 1, d->cat_ent);
        nn_backward_dev_z(mu, d->gmu, B, 0, *p_zero, c->comm ? align4(A) : -1);
    } else if (sd) {       /* the state-dependent-σ Gaussian: the plain branch with its own head (gauss_sd.hip) */
        /* log σ is unused, as under a discrete policy: the head writes no gradient to it and the entropy Adam below
         * steps on the zeros kept here, which leaves log σ bit-identical */
        if (mu->dtype != 0)
            die("ppo_update: the state-dependent-σ Gaussian policy needs fp32 compute mode (μ is in bf16 mode)");
        if (!*ls_zero) phip_memset(pol->d_log_std_grad, 0, sizeof(float) * (size_t)A);
        *ls_zero = 1;
        phip_memset(d->sd_rec, 0, offsetof(PhipSdRec, ticket));
        d->sd_rows = B;
        nn_forward_dev_rows(mu, c->state, rows, d->states_p, B);
        phip_sd_head(mu->d_output, act, adv, olp, B, A, d->sd_ls[0], d->sd_ls[1], ppo->epsilon, ppo->ent_coeff, d->gmu,
                     NULL, NULL, d->sd_rec, d->stats + 1);
        nn_backward_dev_z(mu, d->gmu, B, 0, *p_zero, c->comm ? align4(A) : -1);
    } else if (c->fuse_p) {       /* output layer + clipped surrogate + output-layer backward (out_head.hip) */
        if (!*ls_zero) phip_memset(pol->d_log_std_grad, 0, sizeof(float) * (size_t)A);
        nn_out_head_step(mu, 1, c->state, rows, d->states_p, B, *p_zero, c->comm ? align4(A) : -1, NULL,
                         pol->d_log_std, act, adv, olp, ppo->epsilon, ppo->ent_coeff,
                         pol->d_log_std_grad, d->stats + 1, NULL);
    } else if (c->wide_p) { /* A = 17: policy head + output-layer backward in one pass (out_head.hip) */
        if (!*ls_zero) phip_memset(pol->d_log_std_grad, 0, sizeof(float) * (size_t)A);
        nn_policy_wide_step(mu, c->state, rows, d->states_p, B, *p_zero, c->comm ? align4(A) : -1,
                            pol->d_log_std, act, adv, olp, ppo->epsilon, ppo->ent_coeff,
                            pol->d_log_std_grad, d->stats + 1);
    } else {
        nn_forward_dev_rows(mu, c->state, rows, d->states_p, B);
        phip_policy_head(mu->d_output, pol->d_log_std, act, adv, olp, B, A, ppo->epsilon,
                         ppo->ent_coeff, d->gmu, pol->d_log_std_grad, d->stats + 1, *ls_zero);
        nn_backward_dev_z(mu, d->gmu, B, 0, *p_zero, c->comm ? align4(A) : -1);
    }
    /* target-KL early stopping (off: nothing launched): the step's KL and clip fraction from the μ the
     * forward just left, on the device (kl.hip), before the step's Adam, which reads the stop word through
     * `skip`.  Without a communicator one launch sums and decides.  With one, the sum launch writes this
     * rank's two sums, one all-reduce of those four floats follows the step's gradient all-reduce on the
     * same stream and communicator, and a one-workgroup launch decides from the global sums after the join:
     * every rank decides from the same bits.  The extra collective is a function of the setting only, so
     * the fixed order of collectives (comm.hip) holds as long as every rank holds the same target_kl. */
    const float target_kl = kl_target(d);
    const int kl_on = !tab && target_kl > 0.f;
    const long kl_rows = (long)B * phip_comm_world();
    /* the closed-form estimator: the same launch reads the behaviour distribution the update stored at its head, in
     * place through this step's row indices (they exist in every form of the step); its sum rides in sums[2] */
    const int kl_x = kl_on && kl_exact(d);
    const PhipKlExact kl_ex = {d->kl_old, d->kl_old_ls, rows, cat ? disc_off(d) : NULL, cat ? disc_D(d) : 0,
                               cat && disc_max_n(d, A) > 32, NULL};
    if (kl_on && c->comm) {
        phip_policy_kl(mu->d_output, pol->d_log_std, act, olp, B, A, kl_dist, ppo->epsilon, target_kl, kl_rows,
                       0, d->kl, kl_off, kl_D, kl_m, kl_m ? rows : NULL, kl_x ? &kl_ex : NULL, d->sd_ls);
        phip_allreduce_sum_f32_async(d->kl->sums, 4);
    }
    phip_allreduce_join();
    /* ppo.cu:440-442 order; the entropy Adam clears the log σ gradient it read (the next policy head
     * accumulates into zeros) */
    if (tab) {
        adam_net_tab(ppo->adam_entropy, NULL, d, 1, 1);
        adam_net_tab(ppo->adam_policy, mu, d, 1, 0);
        *ls_zero = *p_zero = 1;
        return;
    }
    /* both Adams in one launch where they qualify (flat spans, the network's 16-B aligned) */
    Adam* ap = ppo->adam_policy;
    /* μ's gradient span and the log σ gradient clip as one group: one coefficient for both Adams */
    const float* coef = clip_coef(d, 1, ap, pol->d_log_std_grad, A);
    const unsigned* skip = NULL;
    if (kl_on) {
        if (!ap->flat || !ppo->adam_entropy->flat)
            die(d->target_kl > 0.f ? "ppo_update: target-KL early stopping needs flat Adam spans"
                                   : "ppo_update: the adaptive learning-rate schedule needs flat Adam spans");
        if (c->comm) phip_kl_decide(d->kl, target_kl, kl_rows, kl_x);
        else
            phip_policy_kl(mu->d_output, pol->d_log_std, act, olp, B, A, kl_dist, ppo->epsilon, target_kl, kl_rows,
                           1, d->kl, kl_off, kl_D, kl_m, kl_m ? rows : NULL, kl_x ? &kl_ex : NULL, d->sd_ls);
        skip = &d->kl->stopped;
    }
    /* the last step of a policy epoch keeps its gradients while the feature is on: the host looks at the
     * record behind it and may end the loop there, and a caller may read the last issued step's gradients
     * (the next step, if one follows, clears them itself) */
    const int clear = ip + 1 < c->np && !(kl_on && (ip + 1) % c->num_batches == 0);
    const int own = adam_owns(ap, mu->d_params, mu->d_grads);
    const int fused = mu->dtype == 1 && own;
    const int ls_own = adam_owns(ppo->adam_entropy, NULL, pol->d_log_std_grad);
    /* the policy rate, shared by both Adams as ever: by value, or — the adaptive schedule — the record's word, which
     * this step's decision has just written */
    const PhipAdamRate rate = {d->lr_use[0], lr_adaptive(d) ? &d->kl->lr : NULL};
    const int r = adam_update_pair_dev(ap, rate, fused ? mu->d_w16 : NULL, mu->num_params, clear && own,
                                       ppo->adam_entropy, rate, clear && ls_own, coef, skip);
    if (r >= 0) {
        if (!(r & 1) && mu->dtype == 1) nn_sync_w16(mu);
        *ls_zero = ls_own && (r & 4);
        *p_zero = (r & 2) != 0;
        return;
    }
    *ls_zero = ls_own && (adam_update_dev(ppo->adam_entropy, rate, NULL, 0, clear, coef, skip) & 2);
    *p_zero = adam_update_net(ppo->adam_policy, rate, mu, clear, coef, skip);
}

/* the closed-form estimator's behaviour distribution, at the head of an update (stream-ordered on libppo's stream,
 * behind the observation shadow and ahead of the loops' fork): policy parameters do not change between the rollout
 * and the update, so μ forwarded over state[0, limit) — the array the policy loop reads — IS what the rollout acted
 * with, however the buffer was filled.  Forwarded in chunks of at most KL_OLD_CHUNK contiguous rows, so that μ's
 * activation workspaces grow to max(B, min(limit, KL_OLD_CHUNK)) rows and never to the buffer's; 16384 rows keep the
 * GEMMs at full-size tiles (64 chunks per 2^20 rows).  A chunk's forward may pick another GEMM configuration than a
 * minibatch's, so the first policy step's exact KL is tiny but need not be 0. */
#define KL_OLD_CHUNK 16384
static void kl_old_prepare(PPO* ppo, PPODev* d, const float* state, int limit) {
    TrajectoryBuffer* buf = ppo->buffer;
    NeuralNetwork* mu = ppo->policy->mu;
    const int S = buf->state_size, A = buf->action_size;
    if (!d->kl_old) {
        d->kl_old = (float*)phip_malloc(sizeof(float) * (size_t)buf->capacity * A);
        d->kl_old_ls = (float*)phip_malloc(sizeof(float) * (size_t)A);
    }
    for (long r0 = 0; r0 < limit; r0 += KL_OLD_CHUNK) {
        const int rows = (int)(limit - r0 < KL_OLD_CHUNK ? limit - r0 : KL_OLD_CHUNK);
        nn_forward_dev(mu, state + r0 * S, rows);
        phip_d2d(d->kl_old + r0 * A, mu->d_output, sizeof(float) * (size_t)rows * A);
    }
    if (!cat_on(d)) phip_d2d(d->kl_old_ls, ppo->policy->d_log_std, sizeof(float) * (size_t)A);
    d->kl_old_rows = limit;
}

/* target-KL early stopping, at a policy-epoch boundary: the host waits for the policy loop's stream only
 * (the bounded wait over every stream while a communicator is up) and reads the record's head */
static int kl_stopped(PPODev* d, int comm, PhipKlRec* head) {
    if (comm) phip_comm_wait("target-KL epoch check");
    else phip_stream_wait();
    phip_d2h(head, d->kl, offsetof(PhipKlRec, ticket));
    return head->stopped != 0;
}

/* graph replay (opt-in, PPO_GRAPH=1; PPO_GRAPH_STEPS = steps per captured graph, default 16) for
 * small minibatches on one GPU when every Adam of the step is a flat, 16-B aligned span that owns its
 * network (the table kernels' form).  Measured at C3, B = 64 (profiles/r03_graph_replay.txt): eager
 * 2062 ms per update, graphs of 1 / 4 / 16 / 64 steps 2375 / 2156 / 2104 / 2091 ms — on this ROCm a
 * graph replays its kernel nodes at the eager launch cost, and the step is GPU-bound (≈ 36 µs for 8–9
 * dependent small kernels), so it stays off by default. */
static int step_graphs_ok(const StepCtx* c) {
    const char* e = getenv("PPO_GRAPH");
    if (!(e && *e && *e != '0') || c->comm || phip_comm_world() > 1 || c->B > 2048 || c->A > 32) return 0;
    if (c->d->max_grad_norm > 0.f) return 0;      /* the table Adam does not read a clip coefficient */
    if (kl_target(c->d) > 0.f) return 0;          /* … nor a stop word, and a captured step has no KL launch */
    if (c->d->value_clip > 0.f) return 0;         /* … and a captured value step's head is the plain MSE */
    if (cat_on(c->d) || sd_on(c->d)) return 0;    /* … and a captured policy step's head is the Gaussian one */
    if (c->d->adv_norm_mode != PPO_ADV_NORM_GLOBAL) return 0;   /* … and a captured policy step gathers for itself */
    PPO* ppo = c->ppo;
    Adam* ads[3] = {ppo->adam_V, ppo->adam_policy, ppo->adam_entropy};
    for (int i = 0; i < 3; i++)
        if (!ads[i]->flat || !adam_span_aligned(ads[i])) return 0;
    /* the table Adam always clears the gradient it read (the captured steps run their backward with
     * the gradients already zero), so every Adam must own its network's gradient span, as `own` in
     * adam_update_net requires on the eager path */
    if (!adam_owns(ppo->adam_V, ppo->V->d_params, ppo->V->d_grads) ||
        !adam_owns(ppo->adam_policy, ppo->policy->mu->d_params, ppo->policy->mu->d_grads) ||
        !adam_owns(ppo->adam_entropy, NULL, ppo->policy->d_log_std_grad))
        return 0;
    /* only the combination tests/test_gpu_update.py replays against eager launches: fp32 networks with
     * the fused output heads (value A = 1, policy A <= 6) */
    if (ppo->V->dtype != 0 || ppo->policy->mu->dtype != 0 || !c->fuse_v || !c->fuse_p || c->fold_v) return 0;
    return 1;
}

/* the step table of phase ph (0 value, 1 policy) for steps 1 … n−2 — epoch order, minibatch offset
 * and the Adam step sizes in the reference's step order (advancing the host Adam step counters as
 * the eager path does) — uploaded, the counter reset, and one step captured as a graph */
static void* capture_graph(StepCtx* c, int ph, int steps) {
    if (phip_graph_begin() != 0) return NULL;
    for (int s = 0; s < steps; s++) {
        if (ph) {
            int pz = 1, lz = 1;
            policy_step(c, 1, &pz, &lz, 1);
        } else {
            (void)value_step(c, 1, 1, 1);
        }
    }
    return phip_graph_end();
}

static void capture_steps(StepCtx* c, int ph) {
    PPO* ppo = c->ppo;
    PPODev* d = c->d;
    const long n = (ph ? c->np : c->nv) - 2;
    if (n <= 0) return;
    if (n > d->h_tab_cap) {
        free(d->h_tab);
        d->h_tab = (PhipStepArgs*)xmalloc(sizeof(PhipStepArgs) * (size_t)n);
        d->h_tab_cap = n;
    }
    if (n > d->tab_cap[ph]) {
        phip_free(d->tab[ph]);
        d->tab[ph] = (PhipStepArgs*)phip_malloc(sizeof(PhipStepArgs) * (size_t)n);
        d->tab_cap[ph] = n;
    }
    if (!d->ctr) d->ctr = (int*)phip_malloc(sizeof(int) * 4);
    const int* perms = ph ? c->perms_p : c->perms_v;
    const uint64_t* keys = ph ? c->keys_p : c->keys_v;
    /* the table advances the host Adam step counters as the eager steps would; kept to roll back if
     * the capture fails (the phase then runs every step eagerly) */
    const int t_v = ppo->adam_V->time_step, t_p = ppo->adam_policy->time_step, t_e = ppo->adam_entropy->time_step;
    for (long t = 0; t < n; t++) {
        const long i = t + 1;
        const int j = (int)(i / c->num_batches), k = (int)(i % c->num_batches);
        PhipStepArgs* e = &d->h_tab[t];
        memset(e, 0, sizeof(*e));
        e->perm_off = perms ? (long)j * c->limit : -1;
        if (!perms) phip_step_feistel(e, keys[j], c->limit);
        e->offset = k * c->B;
        if (ph) {
            /* the rates this update passes by value (d->lr_use: the struct's, or their linear decay), as the eager
             * first and last steps of the phase take them */
            adam_next_step(ppo->adam_entropy, d->lr_use[0], &e->step_ls, &e->bc2_ls);     /* ppo.cu:440-442 */
            adam_next_step(ppo->adam_policy, d->lr_use[0], &e->step, &e->bc2);
        } else {
            adam_next_step(ppo->adam_V, d->lr_use[1], &e->step, &e->bc2);
        }
    }
    phip_h2d(d->tab[ph], d->h_tab, sizeof(PhipStepArgs) * (size_t)n);
    phip_memset(d->ctr + ph, 0, sizeof(int));
    phip_memset(d->ctr + 2 + ph, 0, sizeof(int));
    const int K = (int)(n < c->K ? n : c->K);
    void* gk = capture_graph(c, ph, K);
    void* g1 = gk && K > 1 ? capture_graph(c, ph, 1) : NULL;
    if (!gk || (K > 1 && !g1)) {
        /* an opt-in speed feature must not end a training run: warn, drop the graphs, replay nothing */
        fprintf(stderr, "libppo: warning: graph capture of the %s steps failed (%s); running them eagerly\n",
                ph ? "policy" : "value", phip_graph_error());
        phip_graph_destroy(gk);
        phip_graph_destroy(g1);
        ppo->adam_V->time_step = t_v;
        ppo->adam_policy->time_step = t_p;
        ppo->adam_entropy->time_step = t_e;
        return;
    }
    if (ph) { c->gp = gk; c->gp1 = g1; c->Kp = K; } else { c->gv = gk; c->gv1 = g1; c->Kv = K; }
}

static void ppo_update_body(PPO* ppo, float gamma, int batch_size, int n_epochs_policy, int n_epochs_value,
                            int shuffle_mode, unsigned long long seed);

/* the phases' minibatch inputs, gathered before the loops: the rows of epoch j's steps are one gather
 * of num_batches·B consecutive list positions (step k's slot i is position k·B + i, modulo the buffer
 * length, as the per-step gather takes it — trajectory_buffer.cu get_batch), so ph_rows[p] + iv·B holds
 * exactly the rows step iv would have gathered */
static void phase_gather(StepCtx* c) {
    PPO* ppo = c->ppo;
    PPODev* d = c->d;
    TrajectoryBuffer* buf = ppo->buffer;
    const long B = c->B, A = c->A, per = (long)c->num_batches * B;
    for (int ph = 0; ph < 2; ph++) {
        const long n = ph ? c->np : c->nv;
        if (n <= 0) continue;
        if (n * B > d->ph_cap[ph]) {
            phip_free(d->ph_rows[ph]);
            d->ph_rows[ph] = (int*)phip_malloc(sizeof(int) * (size_t)(n * B));
            if (ph) {
                phip_free(d->ph_act); phip_free(d->ph_olp); phip_free(d->ph_adv);
                d->ph_act = (float*)phip_malloc(sizeof(float) * (size_t)(n * B * A));
                d->ph_olp = (float*)phip_malloc(sizeof(float) * (size_t)(n * B));
                d->ph_adv = (float*)phip_malloc(sizeof(float) * (size_t)(n * B));
            } else {
                phip_free(d->ph_tgt);
                d->ph_tgt = (float*)phip_malloc(sizeof(float) * (size_t)(n * B));
            }
            d->ph_cap[ph] = n * B;
        }
        const int* perms = ph ? c->perms_p : c->perms_v;
        const uint64_t* keys = ph ? c->keys_p : c->keys_v;
        for (long j = 0; j * c->num_batches < n; j++) {
            const long steps = n - j * c->num_batches < c->num_batches ? n - j * c->num_batches : c->num_batches;
            const long o = j * per;
            if (steps * B >= (1L << 31)) die("ppo_update: a phase epoch exceeds 2^31 rows");
            phip_gather_rows(perms ? perms + j * c->limit : NULL, keys[j], 0, c->limit, (int)(steps * B), c->S, c->A,
                             c->state, buf->action_p, buf->logprob_p, buf->advantage_p, buf->adv_target_p, NULL,
                             ph ? d->ph_act + o * A : NULL, ph ? d->ph_olp + o : NULL, ph ? d->ph_adv + o : NULL,
                             ph ? NULL : d->ph_tgt + o, d->ph_rows[ph] + o);
        }
    }
    c->phg = 1;
}

/* the replica check's parameter spans in HBM: μ, log σ, V */
static void replica_hash(PPO* ppo) {
    GaussianPolicy* pol = ppo->policy;
    /* … and, while observation normalisation is on, the running triple's 1 + 2S doubles as 32-bit words
     * (off: the three spans, the hash as before) */
    PPODev* d = (PPODev*)ppo->dev;
    const int obs = obs_on(d);
    if (obs) obs_ws(ppo, d);      /* on but never folded or set: the zero triple, hashed like a peer's zeros */
    const float* spans[6] = {pol->mu->d_params, pol->d_log_std, ppo->V->d_params, obs ? (const float*)d->obs_run : NULL,
                             NULL};
    long lens[6] = {pol->mu->num_params, pol->action_size, ppo->V->num_params,
                    obs ? 2 * (1 + 2L * ppo->buffer->state_size) : 0, 0};
    int n_spans = obs ? 4 : 3;
    /* … and, while reward normalisation is on, the returns' running triple (3 doubles), likewise */
    if (rew_on(d)) {
        rew_ws(d);
        spans[n_spans] = (const float*)d->rew_run;
        lens[n_spans++] = 6;
    }
    /* … and, while the adaptive learning-rate schedule is on, the record's two rate words (lr, lr_v) */
    if (lr_adaptive(d)) {
        spans[n_spans] = &d->kl->lr;
        lens[n_spans++] = 2;
    }
    phip_param_hash(spans, lens, n_spans);
}

unsigned long long ppo_param_hash(void* vppo) {
    unsigned long long h = 0;
    replica_hash((PPO*)vppo);
    char msg[8];
    (void)phip_comm_check_hash(0, &h, msg, 0);    /* this rank's hash only: no collective */
    return h;
}

int ppo_comm_check_replicas(void* vppo) {
    replica_hash((PPO*)vppo);
    char msg[400];
    if (phip_comm_check_hash(1, NULL, msg, (int)sizeof(msg)) == 0) return 0;
    char buf[480];
    snprintf(buf, sizeof(buf), "replica check: parameters differ across ranks: %s", msg);
    phip_record_error(buf);
    return -1;
}

/* PPO_REPLICA_CHECK=K: the replica check after every K-th update at world > 1 (default 1, 0 = off) */
static int replica_check_due(void) {
    static long n = 0;
    const char* e = getenv("PPO_REPLICA_CHECK");
    const long k = e && *e ? atol(e) : 1;
    if (k <= 0) return 0;
    return ++n % k == 0;
}

void ppo_update(void* vppo, float gamma, int batch_size, int n_epochs_policy, int n_epochs_value, int shuffle_mode,
                unsigned long long seed) {
    PPO* ppo = (PPO*)vppo;
    ppo_update_body(ppo, gamma, batch_size, n_epochs_policy, n_epochs_value, shuffle_mode, seed);
    if (ppo->dev && ((PPODev*)ppo->dev)->lr_kind != PPO_LR_CONSTANT) ((PPODev*)ppo->dev)->lr_u += 1;
    ppo->V->dev_version++;               /* HBM parameters moved (also by the single-workgroup path) */
    ppo->policy->mu->dev_version++;
    /* replicated Adam must leave every rank with the same parameters; a rank that drifted
     * would otherwise train on its own weights silently */
    if (phip_comm_world() > 1 && replica_check_due() && ppo_comm_check_replicas(ppo) != 0)
        die(ppo_last_error());
}

static void ppo_update_body(PPO* ppo, float gamma, int batch_size, int n_epochs_policy, int n_epochs_value,
                            int shuffle_mode, unsigned long long seed) {
    TrajectoryBuffer* buf = ppo->buffer;
    if (phip_cluster_error()) die("ppo_update: a multi-workgroup phase (cluster.hip) timed out at a barrier");
    if (!buf->on_device) die("ppo_update: buffer must be device-resident (buffer_to_device / ppo_fill_synthetic)");
    if (batch_size <= 0) die("ppo_update: batch_size must be positive");
    PPODev* d = dev_ws(ppo, batch_size);
    d->gat_np = d->adv_np = 0;            /* what ppo_adv_norm_read / _history may read: this update's, once gathered */
    d->gat_B = 0;
    if (shuffle_mode == PPO_SHUFFLE_DEVICE && (!d->seeded || d->seed != seed)) {
        d->seed = seed;
        d->key = splitmix64(seed);
        d->seeded = 1;
    }
    const int S = buf->state_size, A = buf->action_size, B = batch_size;
    const int limit = buf->full ? buf->capacity : buf->idx;
    const int num_batches = buf->capacity / B;                           /* D13 */
    /* the learning rates this update passes by value: the struct's, or their linear decay at this update's number
     * (the adaptive schedule's policy rate, and its coupled value rate, are device words instead) */
    ppo_dev_lr_now(ppo, d, d->lr_use);
    const int world = phip_comm_world();
    const float gscale = 1.0f / (float)world;
    const int comm = phip_comm_active();
    ppo->adam_V->grad_scale = gscale;
    ppo->adam_policy->grad_scale = gscale;
    ppo->adam_entropy->grad_scale = gscale;
    NeuralNetwork* V = ppo->V;
    GaussianPolicy* pol = ppo->policy;
    NeuralNetwork* mu = pol->mu;

    /* observation normalisation (off: nothing launched, every consumer reads buf->state_p as before): the
     * shadow under the affine pair on entry and the batch triple first; GAE, the phases and both loops then
     * read the shadow.  The caller's buffer is never written. */
    const int obs = obs_on(d);
    const float* state = obs ? obs_prepare(ppo, d, limit) : buf->state_p;
    /* reward normalisation (off: nothing launched, GAE reads buf->reward_p as before): only GAE reads rewards,
     * so the scan, the fold, its collective and the scaled shadow all come here, once per update */
    const float* reward = rew_on(d) ? rew_prepare(ppo, d, limit, gamma) : buf->reward_p;
    gae_device(V, buf, gamma, ppo->lambda, obs ? ppo : NULL, reward);
    /* D19: an empty buffer (idx = 0, not full) has nothing to train on; the reference would divide
     * by zero (rand() % 0 in shuffle_buffer, % limit in get_batch) — here the update ends after GAE.
     * At world > 1 the ranks agree first (min over ranks): one empty shard ends the update on every
     * rank, so no rank waits in a gradient all-reduce the others never issue. */
    if ((world > 1 ? phip_comm_min_i32(limit) : limit) <= 0) return;

    if (ppo_update_tiny(ppo, d, state, B, n_epochs_policy, n_epochs_value, shuffle_mode) == 0) return;

    /* The policy loop reads only the buffer and the advantages — nothing the value loop writes —
     * so on one GPU the two run concurrently: value steps on libppo's stream, policy steps on its
     * side stream (own workspaces), issued interleaved.  Every network sees exactly the reference's
     * sequence of minibatches and Adam steps; epochs' shuffles are drawn up front in the
     * reference's order (value epochs first).  PPO_SERIAL=1 runs them one after the other.  Under
     * data parallelism (world > 1) each loop issues one gradient all-reduce per step in its own
     * stream on its own communicator (comm.hip; PPO_COMM_ASYNC=1: per-layer buckets on one comm
     * stream).  The interleave below is a fixed function of (iv, ip, nv, np), never of timing, so
     * every rank issues the same total order of collectives — half of comm.hip's deadlock argument. */
    long nv = (long)n_epochs_value * num_batches, np = (long)n_epochs_policy * num_batches;
    if (d->max_v >= 0 && nv > d->max_v) nv = d->max_v;
    if (d->max_p >= 0 && np > d->max_p) np = d->max_p;
    uint64_t* keys = (uint64_t*)xmalloc(sizeof(uint64_t) * (size_t)(n_epochs_value + n_epochs_policy + 1));
    uint64_t* keys_v = keys;
    uint64_t* keys_p = keys + n_epochs_value;
    const int* perms_v = phase_perms(ppo, d, shuffle_mode, n_epochs_value, limit, 0, keys_v);
    const int* perms_p = phase_perms(ppo, d, shuffle_mode, n_epochs_policy, limit, 1, keys_p);
    const char* serial_env = getenv("PPO_SERIAL");
    const int concurrent = nv > 0 && np > 0 && !(serial_env && *serial_env && *serial_env != '0');
    /* the fused and the wide output-layer kernels embed the Gaussian head: a categorical policy takes neither */
    const int own_head = cat_on(d) || sd_on(d);
    const int fuse_p = !own_head && nn_out_head_ok(mu, 1);
    StepCtx c = {ppo, d, B, S, A, limit, num_batches, comm, nn_out_head_ok(V, 0), fuse_p,
                 !fuse_p && !own_head && nn_policy_wide_ok(mu, B), nn_value_fold_ok(V, B), perms_v, perms_p, keys_v, keys_p, nv, np,
                 NULL, NULL, NULL, NULL, 16, 1, 1, 0, state};
    {
        const char* ge = getenv("PPO_GRAPH_STEPS");
        if (ge && atoi(ge) > 0) c.K = atoi(ge);
    }
    /* graph replay (opt-in): steps 1 … n−2 of a phase replay captured graphs of K steps (the first
     * step runs eagerly — workspaces allocated, gradients cleared — and the last one too, so the
     * caller can read its gradients) */
    const int graphs = step_graphs_ok(&c);
    /* eager steps: every step's gathered inputs up front (one launch per epoch instead of one per
     * step; on libppo's stream before the fork, so both loops see them) */
    if (!graphs) {
        phase_gather(&c);
        d->gat_np = np;
        d->gat_B = B;
        /* per-minibatch advantage normalisation (off: nothing launched, nothing allocated): one launch over the
         * gathered copy of the policy phase's advantages, on libppo's stream ahead of the fork — segment ip is what
         * policy step ip's head reads through its adv pointer, whichever form of the head it is; the buffer's
         * advantage array is never written.  Target-KL early stopping may leave steps unissued: their segments are
         * normalised and never read.  Per rank and element-wise across segments: no collective. */
        if (d->adv_norm_mode == PPO_ADV_NORM_MINIBATCH && np > 0) {
            if (np > d->adv_cap) {
                phip_free(d->adv_stats);
                d->adv_stats = (float*)phip_malloc(sizeof(float) * 2 * (size_t)np);
                d->adv_cap = np;
            }
            phip_adv_normalize(d->ph_adv, d->ph_adv, np, B, d->adv_stats);
            d->adv_np = np;
        }
    }
    /* target-KL early stopping: the stop word, the stop step and the step counter start afresh with every
     * update (stream-ordered, ahead of the fork: the policy loop's stream sees them) */
    const int kl_on = kl_target(d) > 0.f && np > 0;
    if (kl_on) {
        phip_memset(&d->kl->stopped, 0, 2 * sizeof(unsigned));          /* stopped, step */
        phip_memset(&d->kl->stop_step, 0xFF, sizeof(int));              /* −1 */
        /* the closed-form estimator (off: nothing launched, nothing allocated): the behaviour distribution */
        if (kl_exact(d)) kl_old_prepare(ppo, d, state, limit);
    }
    /* the adaptive schedule's value-rate coupling: one one-thread launch, likewise ahead of the fork, fixes the
     * value Adam's word for the whole update from the policy rate as the last update left it — the value loop
     * never reads a word the policy loop writes */
    if (lr_adaptive(d) && d->lr_couple)
        phip_lr_couple(d->kl, ppo->lr_V, clampf(ppo->lr_policy, d->lr_p[1], d->lr_p[2]));
    long kl_issued = 0, kl_applied = 0;
    if (concurrent) phip_side_fork();
    long iv = 0, ip = 0;
    /* gradients cleared by the previous Adam step (not after a loop's last step: a caller may read
     * the last minibatch's gradients after the update) */
    int v_zero = 0, p_zero = 0, ls_zero = 0;
    while (iv < nv || ip < np) {
        /* serial: every value step first (the reference's order); concurrent: issue in proportion */
        const int take_v = iv < nv && (ip >= np || !concurrent || iv * np <= ip * nv);
        if (take_v) {
            long done = 1;
            if (c.gv && iv >= 1 && iv + 1 < nv) {
                if (nv - 1 - iv >= c.Kv) { phip_graph_launch(c.gv); done = c.Kv; }
                else phip_graph_launch(c.gv1 ? c.gv1 : c.gv);
                d->n_graph += done;
            } else {
                v_zero = value_step(&c, iv, v_zero, 0);
                if (iv == 0 && graphs && nv >= 3) capture_steps(&c, 0);
            }
            d->n_v += done;
            iv += done;
        } else {
            long done = 1;
            if (concurrent) phip_side_use(1);
            if (c.gp && ip >= 1 && ip + 1 < np) {
                if (np - 1 - ip >= c.Kp) { phip_graph_launch(c.gp); done = c.Kp; }
                else phip_graph_launch(c.gp1 ? c.gp1 : c.gp);
                d->n_graph += done;
            } else {
                policy_step(&c, ip, &p_zero, &ls_zero, 0);
                if (ip == 0 && graphs && np >= 3) capture_steps(&c, 1);
                /* target-KL early stopping: behind the last step of each policy epoch (and of the loop) the
                 * host waits for the policy stream and reads the record; once the device has stopped, every
                 * further policy step would be a no-op there, so none is issued — purely a saving: ending
                 * the issue at any later boundary leaves identical parameters.  The decision is the same
                 * bits on every rank, so all ranks end their policy loops at the same step. */
                if (kl_on && ((ip + 1) % num_batches == 0 || ip + 1 == np)) {
                    PhipKlRec head;
                    const int stop = kl_stopped(d, comm, &head);
                    if (stop || ip + 1 == np) {
                        kl_issued = ip + 1;
                        kl_applied = stop ? head.stop_step : ip + 1;
                        np = ip + 1;
                    }
                }
            }
            if (concurrent) phip_side_use(0);
            d->n_p += done;
            ip += done;
        }
    }
    phip_graph_destroy(c.gv);
    phip_graph_destroy(c.gp);
    phip_graph_destroy(c.gv1);
    phip_graph_destroy(c.gp1);
    if (concurrent) phip_side_join();
    /* the host step counters advanced per issued policy step; the steps the device skipped took no Adam
     * step, so bias corrections and checkpoints continue as in a run that broke out of the loop */
    if (kl_on && kl_issued > kl_applied) {
        ppo->adam_policy->time_step -= (int)(kl_issued - kl_applied);
        ppo->adam_entropy->time_step -= (int)(kl_issued - kl_applied);
    }
    free(keys);
}

void ppo_set_step_limit(void* vppo, long max_value_steps, long max_policy_steps) {
    PPODev* d = dev_ws((PPO*)vppo, 1);
    d->max_v = max_value_steps;
    d->max_p = max_policy_steps;
}

void ppo_reset_stats(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    PPODev* d = dev_ws(ppo, 1);
    phip_memset(d->stats, 0, 4 * sizeof(float));
    /* norm, coef and the clipped-step counter (the 16 bytes ahead of the ticket) */
    for (int i = 0; i < 2; i++) phip_memset(d->clip[i], 0, offsetof(PhipClipRec, ticket));
    phip_memset(d->kl, 0, offsetof(PhipKlRec, ticket));      /* the head: KL, clip fraction, stop state, applied */
    phip_memset(&d->kl->lr_raised, 0, 2 * sizeof(unsigned)); /* the adaptive schedule's raises and lowerings */
    if (d->kl_est == PPO_KL_EXACT) phip_memset(&d->kl->kl_other, 0, sizeof(float));
    phip_memset(d->vclip_counts, 0, 2 * sizeof(unsigned long long));
    d->n_v = d->n_p = d->n_graph = 0;
}

void ppo_read_stats(void* vppo, double* out, int n) {
    PPO* ppo = (PPO*)vppo;
    PPODev* d = dev_ws(ppo, 1);
    float s[4] = {0, 0, 0, 0}, a[2] = {0, 0};
    phip_d2h(s, d->stats, sizeof(s));
    if (g_adv_stats) phip_d2h(a, g_adv_stats, sizeof(a));
    double v[36] = {s[0], (double)d->n_v, s[1], (double)d->n_p, compute_entropy_cuda(ppo->policy), a[0], a[1],
                    (double)g_gae_own_rows, (double)d->n_graph, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n > 9 && d->max_grad_norm > 0.f) {      /* gradient clipping: zeros while it is off */
        for (int i = 0; i < 2; i++) {
            PhipClipRec r;
            phip_d2h(&r, d->clip[i], offsetof(PhipClipRec, partial));
            v[9 + i] = r.norm;
            v[11 + i] = (double)r.clipped;
        }
    }
    if (n > 13 && kl_target(d) > 0.f) {         /* target-KL early stopping (or the adaptive rate's monitor): zeros while off */
        PhipKlRec r;
        phip_d2h(&r, d->kl, offsetof(PhipKlRec, ticket));
        v[13] = r.kl;
        v[14] = r.clip_frac;
        v[15] = (double)r.applied;
        v[16] = r.stopped ? (double)r.stop_step : -1.0;
    }
    if (n > 17 && d->value_clip > 0.f) {        /* value-loss clipping: zeros while it is off */
        unsigned long long cnt[2];
        phip_d2h(cnt, d->vclip_counts, sizeof(cnt));
        v[17] = (double)cnt[0];
        v[18] = (double)cnt[1];
    }
    if (n > 19 && obs_on(d) && d->obs_run) {    /* observation normalisation: zeros while it is off */
        unsigned long long cnt[2];
        phip_d2h(&v[19], d->obs_run, sizeof(double));
        phip_d2h(cnt, d->obs_counts, sizeof(cnt));
        v[20] = (double)cnt[0];
        v[21] = (double)cnt[1];
    }
    if (n > 22 && rew_on(d) && d->rew_run) {    /* reward normalisation: zeros while it is off */
        unsigned long long cnt[2];
        phip_d2h(&v[22], d->rew_run, sizeof(double));
        phip_d2h(cnt, d->rew_counts, sizeof(cnt));
        v[23] = (double)cnt[0];
        v[24] = (double)cnt[1];
    }
    if (cat_on(d)) {         /* categorical / multi-discrete: the mean (joint) row entropy of the last policy step */
        float h = 0.f;
        phip_d2h(&h, d->cat_ent, sizeof(float));
        v[4] = d->cat_rows > 0 ? (double)h / d->cat_rows : 0.0;
    }
    if (n > 25) {            /* the learning rates in use, and the adaptive schedule's raises and lowerings */
        double lr[2];
        ppo_get_lr(ppo, lr);
        v[25] = lr[0];
        v[26] = lr[1];
        if (lr_adaptive(d)) {
            unsigned cnt[2];
            phip_d2h(cnt, &d->kl->lr_raised, sizeof(cnt));
            v[27] = (double)cnt[0];
            v[28] = (double)cnt[1];
        }
    }
    if (n > 29 && d->adv_norm_mode != PPO_ADV_NORM_GLOBAL) {    /* advantage normalisation: zeros while it is off */
        v[29] = (double)d->adv_norm_mode;
        if (d->adv_np > 0) {
            float* h = (float*)xmalloc(sizeof(float) * 2 * (size_t)d->adv_np);
            phip_d2h(h, d->adv_stats, sizeof(float) * 2 * (size_t)d->adv_np);
            float lo = h[1], hi = h[1];
            for (long i = 1; i < d->adv_np; i++) {
                const float sd = h[2 * i + 1];
                /* a NaN segment shows in both: the comparisons below are false for NaN, so it is carried by hand */
                lo = isnan(lo) || isnan(sd) ? NAN : sd < lo ? sd : lo;
                hi = isnan(hi) || isnan(sd) ? NAN : sd > hi ? sd : hi;
            }
            free(h);
            v[30] = lo;
            v[31] = hi;
        }
    }
    if (n > 32) {            /* the KL monitor's estimator, and the other estimator's value of the last decided step */
        v[32] = (double)d->kl_est;
        if (kl_exact(d)) {
            float o = 0.f;
            phip_d2h(&o, &d->kl->kl_other, sizeof(float));
            v[33] = o;
        }
    }
    if (sd_on(d) && d->sd_rec) {   /* the state-dependent-σ Gaussian: the last policy step's mean row entropy and its
                                    * clamped log-σ elements and elements (this rank's rows); zeros while it is off */
        PhipSdRec r;
        phip_d2h(&r, d->sd_rec, offsetof(PhipSdRec, ticket));
        v[4] = d->sd_rows > 0 ? r.ent_sum / d->sd_rows : 0.0;
        v[34] = (double)r.counts[0];
        v[35] = (double)r.counts[1];
    }
    for (int i = 0; i < n && i < 36; i++) out[i] = v[i];
}

/* ppo_ext.h: running return-based reward normalisation */
int ppo_set_reward_norm(void* vppo, float clip) {
    if (isnan(clip)) return -1;
    PPODev* d = dev_ws((PPO*)vppo, 1);
    d->rew_clip = clip > 0.f ? clip : 0.f;                   /* +inf stays: scale, never clamp */
    return 0;
}

float ppo_get_reward_norm(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    return ppo->dev ? ((PPODev*)ppo->dev)->rew_clip : 0.f;
}

int ppo_reward_norm_freeze(void* vppo, int frozen) {
    PPODev* d = dev_ws((PPO*)vppo, 1);
    const int was = d->rew_frozen;
    d->rew_frozen = frozen != 0;
    return was;
}

void ppo_reward_norm_get_state(void* vppo, double* out3) {
    PPODev* d = dev_ws((PPO*)vppo, 1);
    phip_sync();
    if (d->rew_run) phip_d2h(out3, d->rew_run, 3 * sizeof(double));
    else memset(out3, 0, 3 * sizeof(double));
}

int ppo_reward_norm_set_state(void* vppo, const double* in3) {
    PPODev* d = dev_ws((PPO*)vppo, 1);
    if (!in3 || !(in3[0] >= 0.0) || isinf(in3[0]) || !isfinite(in3[1]) || !(in3[2] >= 0.0) || isinf(in3[2])) return -1;
    rew_ws(d);
    phip_sync();                                             /* nothing queued still reads the old scale */
    phip_h2d(d->rew_run, in3, 3 * sizeof(double));
    phip_ret_fold(NULL, 0, d->rew_run, d->rew_scale, NULL);
    phip_sync();
    return 0;
}

float ppo_reward_norm_scale(void* vppo) {
    PPODev* d = dev_ws((PPO*)vppo, 1);
    float s = 1.f;
    rew_ws(d);
    phip_sync();
    phip_d2h(&s, d->rew_scale, sizeof(float));
    return s;
}

int ppo_reward_returns_device(const float* d_reward, const unsigned char* d_term, const unsigned char* d_trunc, long n,
                              float gamma, int seg_len, const double* d_carry_in, const unsigned char* d_cont,
                              double* d_returns, double* d_carry_out, double* out3) {
    static double* triple = NULL;                 /* one per process, never freed (as ppo_obs_stats_device's) */
    if (!out3 || n < 0 || seg_len < 0 || isnan(gamma) || (n > 0 && (!d_reward || !d_term || !d_trunc))) return -1;
    if (seg_len > 0 && (n % seg_len != 0 || (n > 0 && (!d_carry_in || (d_carry_out && !d_cont))))) return -1;
    if (!triple) triple = (double*)phip_malloc(3 * sizeof(double));
    phip_ret_scan(d_reward, d_term, d_trunc, n, gamma, n > 0 ? seg_len : 0, d_carry_in, d_cont, d_returns,
                  seg_len > 0 ? d_carry_out : NULL, triple, NULL, NULL, NULL);
    phip_sync();
    phip_d2h(out3, triple, 3 * sizeof(double));
    return 0;
}

/* ppo_ext.h: episode statistics */
/* the eight reported values of one aggregate {n, mean, M2, min, max, Σlen, mean disc} */
static void ep_report(const double* a, double* v) {
    memset(v, 0, 8 * sizeof(double));
    if (!(a[0] > 0.0)) return;
    v[0] = a[0];
    v[1] = a[1];
    v[2] = sqrt(a[2] / a[0]);
    v[3] = a[3];
    v[4] = a[4];
    v[5] = a[5] / a[0];
    v[6] = a[6];
    v[7] = a[2];
}

int ppo_episode_stats(void* vppo, double* out, int n) {
    if (!vppo || !out || n <= 0) return 0;
    PPODev* d = dev_ws((PPO*)vppo, 1);
    double agg[16], v[PPO_EP_NSTAT];
    memset(agg, 0, sizeof(agg));
    phip_sync();
    if (d->ep_agg) phip_d2h(agg, d->ep_agg, sizeof(agg));
    ep_report(agg, v);
    ep_report(agg + 8, v + 8);
    if (n > PPO_EP_NSTAT) n = PPO_EP_NSTAT;
    memcpy(out, v, sizeof(double) * (size_t)n);
    return n;
}

void ppo_episode_reset_stats(void* vppo) {
    PPODev* d = dev_ws((PPO*)vppo, 1);
    if (d->ep_agg) phip_memset(d->ep_agg, 0, 8 * sizeof(double));
}

float ppo_episode_gamma(void* vppo, float gamma) {
    PPODev* d = dev_ws((PPO*)vppo, 1);
    const float was = d->ep_gamma;
    if (gamma >= 0.f && gamma <= 1.f) d->ep_gamma = gamma;       /* NaN fails both comparisons */
    return was;
}

int ppo_episode_scan_device(const float* d_reward, const unsigned char* d_term, const unsigned char* d_trunc,
                            const unsigned char* d_cont, int E, int T, float gamma, double* d_state, double* d_row_ret,
                            double* d_row_disc, double* out) {
    static double* agg = NULL;                    /* one per process, never freed (as ppo_reward_returns_device's) */
    if (!d_reward || !d_term || !d_trunc || !out || E <= 0 || T <= 0) return -1;
    if (!agg) agg = (double*)phip_malloc(8 * sizeof(double));
    phip_episode_scan(d_reward, d_term, d_trunc, d_cont, E, T, gamma, d_state, d_state, d_row_ret, d_row_disc, agg,
                      NULL);
    phip_sync();
    phip_d2h(out, agg, PPO_EP_NBATCH * sizeof(double));
    return 0;
}

/* ppo_eval_device's scratch for E environments and N = E·T rows (grow-only per part) */
static void eval_ws(PPODev* d, int E, long N, int S, int A) {
    if (E > d->ev_E) {
        phip_free(d->ev_env); phip_free(d->ev_obs); phip_free(d->ev_obsn); phip_free(d->ev_act);
        phip_free(d->ev_lp); phip_free(d->ev_rows); phip_free(d->ev_cont);
        d->ev_env = (float*)phip_malloc(sizeof(float) * (size_t)E * PHIP_ENV_STATE(S));
        d->ev_obs = (float*)phip_malloc(sizeof(float) * (size_t)E * S);
        d->ev_obsn = (float*)phip_malloc(sizeof(float) * (size_t)E * S);
        d->ev_act = (float*)phip_malloc(sizeof(float) * (size_t)E * A);
        d->ev_lp = (float*)phip_malloc(sizeof(float) * (size_t)E);
        d->ev_rows = (int*)phip_malloc(sizeof(int) * (size_t)E);
        d->ev_cont = (unsigned char*)phip_malloc((size_t)E);
        phip_rollout_rows(d->ev_rows, E, 1);                     /* rows[e] = e */
        d->ev_E = E;
    }
    if (N > d->ev_N) {
        phip_free(d->ev_reward); phip_free(d->ev_term); phip_free(d->ev_trunc);
        d->ev_reward = (float*)phip_malloc(sizeof(float) * (size_t)N);
        d->ev_term = (unsigned char*)phip_malloc((size_t)N);
        d->ev_trunc = (unsigned char*)phip_malloc((size_t)N);
        d->ev_N = N;
    }
    if (!d->ev_agg) d->ev_agg = (double*)phip_malloc(8 * sizeof(double));
}

int ppo_eval_device(void* vppo, int n_envs, int horizon, int env_kind, unsigned long long seed, int deterministic,
                    float gamma, double* out, int n) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo || !out || n < 9 || n_envs <= 0 || horizon <= 0 || isnan(gamma)) return -1;
    if (env_kind < 0 || env_kind > 2) return -1;
    const int E = n_envs, T = horizon;
    const int S = ppo->buffer->state_size, A = ppo->buffer->action_size;
    /* the action columns the environment reads, from the PPODev if there is one: a declined call creates nothing */
    const int Au = sd_on((const PPODev*)ppo->dev) ? A / 2 : A;
    if (env_kind == 0 && (S != 3 || Au != 1)) return -1;
    PPODev* d = dev_ws(ppo, 1);
    const int cat = cat_on(d), sd = sd_on(d);
    if (env_kind == 2 && (S != 4 || A != 2 || !cat)) return -1;
    eval_ws(d, E, (long)E * T, S, A);
    /* the first reset and the key of every later draw, as ppo_rollout_device derives them; the step counter is
     * local: the training rollout's position in the streams does not move */
    phip_env_reset(env_kind, d->ev_env, d->ev_obs, E, 1, S, splitmix64(seed));
    phip_env_first_obs(env_kind, d->ev_env, d->ev_obs, E, 1, S);
    const uint64_t key = splitmix64(seed ^ 0x524F4C4CULL);
    GaussianPolicy* pol = ppo->policy;
    const int norm = obs_on(d);
    if (norm) obs_ws(ppo, d);
    for (int t = 0; t < T; t++) {
        /* normalised under the pair as it stands, uncounted, nothing folded */
        if (norm)
            phip_obs_normalize_rows(d->ev_obs, NULL, d->ev_obsn, NULL, E, S, d->obs_m, d->obs_m + S, d->obs_clip,
                                    d->obs_run);
        /* through the row list, as the rollout forwards: the same kernels over the same E rows */
        nn_forward_dev_rows(pol->mu, norm ? d->ev_obsn : d->ev_obs, d->ev_rows, NULL, E);
        const uint64_t step = (uint64_t)t;
        if (cat && deterministic) phip_disc_argmax(pol->mu->d_output, NULL, disc_off(d), d->ev_act, E, A, disc_D(d));
        else if (cat)
            phip_disc_sample_rows(pol->mu->d_output, NULL, d->ev_rows, disc_off(d), d->ev_act, d->ev_lp, NULL, E, A,
                                  disc_D(d), key, step);
        else if (sd && deterministic) phip_sd_mean(pol->mu->d_output, d->ev_act, E, A);
        else if (sd)
            phip_sd_sample_rows(pol->mu->d_output, d->ev_rows, d->ev_act, d->ev_lp, E, A, d->sd_ls[0], d->sd_ls[1], key,
                                step);
        else if (deterministic) phip_mean_action(pol->mu->d_output, d->ev_act, (long)E * A);
        else phip_sample_rows(pol->mu->d_output, pol->d_log_std, d->ev_rows, d->ev_act, d->ev_lp, E, A, key, step);
        phip_env_step_eval(env_kind, d->ev_env, d->ev_obs, d->ev_act, d->ev_reward, d->ev_term, d->ev_trunc,
                           d->ev_cont, E, T, t, step, S, A, key, cat, md_off(d), d->md_D, Au);
    }
    phip_episode_scan(d->ev_reward, d->ev_term, d->ev_trunc, d->ev_cont, E, T, gamma, NULL, NULL, NULL, NULL,
                      d->ev_agg, NULL);
    double agg[8];
    phip_sync();
    phip_d2h(agg, d->ev_agg, sizeof(agg));
    ep_report(agg, out);
    out[8] = agg[7];
    return 9;
}

/* ppo_ext.h: running observation normalisation */
int ppo_set_obs_norm(void* vppo, float clip) {
    if (isnan(clip)) return -1;
    PPODev* d = dev_ws((PPO*)vppo, 1);
    d->obs_clip = clip > 0.f ? clip : 0.f;                   /* +inf stays: normalise, never clamp */
    return 0;
}

float ppo_get_obs_norm(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    return ppo->dev ? ((PPODev*)ppo->dev)->obs_clip : 0.f;
}

int ppo_obs_norm_freeze(void* vppo, int frozen) {
    PPODev* d = dev_ws((PPO*)vppo, 1);
    const int was = d->obs_frozen;
    d->obs_frozen = frozen != 0;
    return was;
}

int ppo_obs_norm_fold_buffer(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    PPODev* d = dev_ws(ppo, 1);
    TrajectoryBuffer* buf = ppo->buffer;
    if (!obs_on(d) || d->obs_frozen) return -1;
    if (!buf->on_device) die("ppo_obs_norm_fold_buffer: buffer must be device-resident");
    obs_ws(ppo, d);
    phip_obs_stats(buf->state_p, buf->full ? buf->capacity : buf->idx, buf->state_size, d->obs_batch);
    obs_fold_batch(ppo, d);
    return 0;
}

int ppo_obs_norm_get_state(void* vppo, double* out, long n) {
    PPO* ppo = (PPO*)vppo;
    PPODev* d = dev_ws(ppo, 1);
    const long len = 1 + 2L * ppo->buffer->state_size;
    if (!out || n < len) return -1;
    phip_sync();
    if (d->obs_run) phip_d2h(out, d->obs_run, sizeof(double) * (size_t)len);
    else memset(out, 0, sizeof(double) * (size_t)len);
    return (int)len;
}

int ppo_obs_norm_set_state(void* vppo, const double* in, long n) {
    PPO* ppo = (PPO*)vppo;
    PPODev* d = dev_ws(ppo, 1);
    const int S = ppo->buffer->state_size;
    if (!in || n != 1 + 2L * S || !(in[0] >= 0.0) || isinf(in[0])) return -1;
    for (int j = 0; j < S; j++)
        if (!isfinite(in[1 + j]) || !(in[1 + S + j] >= 0.0) || isinf(in[1 + S + j])) return -1;
    obs_ws(ppo, d);
    phip_sync();                                             /* nothing queued still reads the old pair */
    phip_h2d(d->obs_run, in, sizeof(double) * (size_t)n);
    phip_obs_affine(d->obs_run, S, d->obs_m, d->obs_m + S);
    phip_sync();
    return 0;
}

int ppo_obs_norm_affine(void* vppo, float* mean, float* rstd, int S) {
    PPO* ppo = (PPO*)vppo;
    PPODev* d = dev_ws(ppo, 1);
    if (S != ppo->buffer->state_size) return -1;
    obs_ws(ppo, d);
    phip_sync();
    if (mean) phip_d2h(mean, d->obs_m, sizeof(float) * (size_t)S);
    if (rstd) phip_d2h(rstd, d->obs_m + S, sizeof(float) * (size_t)S);
    return 0;
}

int ppo_obs_normalize_device(void* vppo, const float* d_in, float* d_out, long m) {
    PPO* ppo = (PPO*)vppo;
    PPODev* d = dev_ws(ppo, 1);
    const int S = ppo->buffer->state_size;
    if (!obs_on(d) || !d_in || !d_out || m < 0) return -1;
    obs_ws(ppo, d);
    /* uncounted: ppo_read_stats out[20] / out[21] keep describing the last update */
    phip_obs_normalize(d_in, d_out, m, S, d->obs_m, d->obs_m + S, d->obs_clip, d->obs_run, NULL);
    phip_sync();
    return 0;
}

int ppo_obs_stats_device(const float* d_x, long n, int S, double* out) {
    /* one grow-only scratch per process, never freed (as g_v / g_welford above): libppo's entry points are
     * called from one host thread and launch on libppo's stream, and this one synchronises before it returns */
    static double* triple = NULL;
    static int cap_S = 0;
    if (!out || n < 0 || S <= 0 || (!d_x && n > 0)) return -1;
    if (S > cap_S) {
        phip_free(triple);
        triple = (double*)phip_malloc(sizeof(double) * (size_t)(1 + 2L * S));
        cap_S = S;
    }
    phip_obs_stats(d_x, n, S, triple);
    phip_sync();
    phip_d2h(out, triple, sizeof(double) * (size_t)(1 + 2L * S));
    return 0;
}

/* ppo_ext.h: PPO2 value-loss clipping */
int ppo_set_value_clip(void* vppo, float eps_v) {
    if (isnan(eps_v)) return -1;
    PPODev* d = dev_ws((PPO*)vppo, 1);
    d->value_clip = (eps_v > 0.f && !isinf(eps_v)) ? eps_v : 0.f;
    return 0;
}

float ppo_get_value_clip(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    return ppo->dev ? ((PPODev*)ppo->dev)->value_clip : 0.f;
}

int ppo_value_clip_old_values(void* vppo, const float* d_v_old, long n) {
    PPO* ppo = (PPO*)vppo;
    if (d_v_old && n < (long)ppo->buffer->capacity) return -1;     /* indexed by buffer row: every row must exist */
    dev_ws(ppo, 1)->v_old_user = d_v_old;
    return 0;
}

int ppo_value_clip_head_device(const float* d_y, const float* d_v_old, const int* d_rows, const float* d_tgt, int m,
                               float eps_v, float* d_g, double* out3) {
    static float* loss = NULL;                    /* [0] the loss, then the two counters (8-B aligned) */
    if (!d_y || !d_v_old || !d_tgt || !d_g || !out3 || m <= 0 || !(eps_v > 0.f)) return -1;
    if (!loss) loss = (float*)phip_malloc(2 * sizeof(float) + 2 * sizeof(unsigned long long));
    unsigned long long* cnt = (unsigned long long*)(loss + 2);
    phip_memset(loss, 0, 2 * sizeof(float) + 2 * sizeof(unsigned long long));
    const PhipVClip vc = {d_v_old, d_rows, eps_v, cnt};
    phip_mse_vclip(d_y, d_tgt, m, d_g, loss, &vc);
    float l = 0.f;
    unsigned long long c[2] = {0, 0};
    phip_d2h(&l, loss, sizeof(float));
    phip_d2h(c, cnt, sizeof(c));
    out3[0] = (double)l;
    out3[1] = (double)c[0];
    out3[2] = (double)c[1];
    return 0;
}

/* ppo_ext.h: per-minibatch advantage normalisation */
int ppo_set_adv_norm(void* vppo, int mode) {
    if (!vppo || (mode != PPO_ADV_NORM_GLOBAL && mode != PPO_ADV_NORM_MINIBATCH)) return -1;
    dev_ws((PPO*)vppo, 1)->adv_norm_mode = mode;
    return 0;
}

int ppo_get_adv_norm(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    return ppo && ppo->dev ? ((PPODev*)ppo->dev)->adv_norm_mode : PPO_ADV_NORM_GLOBAL;
}

int ppo_adv_normalize_device(const float* d_in, float* d_out, long n_seg, int B, float* d_stats) {
    if (!d_in || !d_out || n_seg <= 0 || n_seg > 0x7fffffffL || B <= 0) return -1;
    phip_adv_normalize(d_in, d_out, n_seg, B, d_stats);
    phip_sync();
    return 0;
}

int ppo_adv_norm_history(void* vppo, float* out, int n) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo || !ppo->dev) return 0;
    PPODev* d = (PPODev*)ppo->dev;
    phip_sync();
    if (d->adv_norm_mode == PPO_ADV_NORM_GLOBAL || d->adv_np <= 0) return 0;
    const long have = d->adv_np < (long)n ? d->adv_np : (long)n;
    if (out && have > 0) phip_d2h(out, d->adv_stats, sizeof(float) * 2 * (size_t)have);
    return (int)d->adv_np;
}

int ppo_adv_norm_read(void* vppo, long step, int* rows, float* adv, int cap) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo || !ppo->dev) return -1;
    PPODev* d = (PPODev*)ppo->dev;
    if (step < 0 || step >= d->gat_np || cap < d->gat_B) return -1;
    const size_t B = (size_t)d->gat_B;
    phip_sync();
    if (rows) phip_d2h(rows, d->ph_rows[1] + (size_t)step * B, sizeof(int) * B);
    if (adv) phip_d2h(adv, d->ph_adv + (size_t)step * B, sizeof(float) * B);
    return d->gat_B;
}

/* ppo_ext.h: target-KL early stopping */
int ppo_set_target_kl(void* vppo, float target_kl) {
    if (isnan(target_kl)) return -1;
    PPODev* d = dev_ws((PPO*)vppo, 1);
    d->target_kl = target_kl > 0.f ? target_kl : 0.f;        /* +inf stays: measure, never stop */
    return 0;
}

float ppo_get_target_kl(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    return ppo->dev ? ((PPODev*)ppo->dev)->target_kl : 0.f;
}

/* ppo_ext.h: the KL monitor's estimator */
int ppo_set_kl_estimator(void* vppo, int estimator) {
    if (!vppo || (estimator != PPO_KL_K3 && estimator != PPO_KL_EXACT)) return -1;
    dev_ws((PPO*)vppo, 1)->kl_est = estimator;
    return 0;
}

int ppo_get_kl_estimator(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    return ppo && ppo->dev ? ((PPODev*)ppo->dev)->kl_est : PPO_KL_K3;
}

const float* ppo_kl_old_dist(void* vppo, const float** d_log_std_old) {
    PPO* ppo = (PPO*)vppo;
    const PPODev* d = ppo ? (const PPODev*)ppo->dev : NULL;
    const int have = d && d->kl_old && d->kl_old_rows > 0;
    if (d_log_std_old) *d_log_std_old = have ? d->kl_old_ls : NULL;
    return have ? d->kl_old : NULL;
}

/* ppo_ext.h: learning-rate schedules */
int ppo_set_lr_schedule(void* vppo, int kind, float p0, float p1, float p2) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo || isnan(p0) || isnan(p1) || isnan(p2)) return -1;
    if (kind == PPO_LR_LINEAR) {
        if (!(p0 >= 1.f) || isinf(p0) || !(p1 >= 0.f && p1 <= 1.f)) return -1;
    } else if (kind == PPO_LR_ADAPTIVE) {
        if (!(p0 > 0.f) || isinf(p0) || !(p1 > 0.f) || isinf(p1) || !(p2 >= p1) || isinf(p2)) return -1;
    } else if (kind != PPO_LR_CONSTANT) {
        return -1;
    }
    PPODev* d = dev_ws(ppo, 1);
    const int on = kind == PPO_LR_ADAPTIVE;
    /* the record's share: the rate, the coupled value rate (the base until the first coupling launch), the rule's
     * parameters (lr_kl = 0 turns the rule off inside decide()) and the counters — stream-ordered, like every write
     * to the record */
    const float words[5] = {on ? clampf(ppo->lr_policy, p1, p2) : 0.f, on ? ppo->lr_V : 0.f, on ? p0 : 0.f,
                            on ? p1 : 0.f, on ? p2 : 0.f};
    phip_sync();
    phip_h2d(&d->kl->lr, words, sizeof(words));
    phip_memset(&d->kl->lr_raised, 0, 2 * sizeof(unsigned));
    d->lr_kind = kind;
    d->lr_p[0] = kind == PPO_LR_CONSTANT ? 0.f : p0;
    d->lr_p[1] = kind == PPO_LR_CONSTANT ? 0.f : p1;
    d->lr_p[2] = kind == PPO_LR_ADAPTIVE ? p2 : 0.f;
    d->lr_u = 0;
    return 0;
}

int ppo_get_lr_schedule(void* vppo, float* out4) {
    PPO* ppo = (PPO*)vppo;
    const PPODev* d = ppo ? (const PPODev*)ppo->dev : NULL;
    if (out4) {
        for (int i = 0; i < 3; i++) out4[i] = d ? d->lr_p[i] : 0.f;
        out4[3] = d ? (float)d->lr_couple : 0.f;
    }
    return d ? d->lr_kind : PPO_LR_CONSTANT;
}

int ppo_lr_couple_value(void* vppo, int on) {
    if (!vppo) return -1;
    PPODev* d = dev_ws((PPO*)vppo, 1);
    const int was = d->lr_couple;
    d->lr_couple = on != 0;
    return was;
}

int ppo_get_lr(void* vppo, double* out2) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo || !out2) return -1;
    PPODev* d = dev_ws(ppo, 1);
    float now[2];
    ppo_dev_lr_now(ppo, d, now);
    if (lr_adaptive(d)) {
        float w[2];
        phip_sync();
        phip_d2h(w, &d->kl->lr, sizeof(w));
        now[0] = w[0];
        if (d->lr_couple) now[1] = w[1];
    }
    out2[0] = now[0];
    out2[1] = now[1];
    return 0;
}

int ppo_lr_history(void* vppo, float* out, int n) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo || !ppo->dev) return 0;
    PPODev* d = (PPODev*)ppo->dev;
    if (!lr_adaptive(d)) return 0;
    unsigned steps = 0;
    phip_sync();
    phip_d2h(&steps, &d->kl->step, sizeof(unsigned));
    const int have = (int)(steps < (unsigned)PHIP_KL_HIST ? steps : (unsigned)PHIP_KL_HIST);
    if (out && n > 0 && have > 0) phip_d2h(out, d->kl->lr_hist, sizeof(float) * (size_t)(n < have ? n : have));
    return (int)steps;
}

int ppo_kl_history(void* vppo, double* out, int n) {
    return ppo_kl_history_est(vppo, ppo_get_kl_estimator(vppo), out, n);
}

int ppo_kl_history_est(void* vppo, int estimator, double* out, int n) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo) return 0;
    PPODev* d = dev_ws(ppo, 1);
    phip_sync();
    if (!(kl_target(d) > 0.f)) return 0;
    /* the deciding estimator's values are in hist; under the closed-form one k3's are kept beside them */
    const float* src = estimator == d->kl_est ? d->kl->hist
                       : estimator == PPO_KL_K3 && d->kl_est == PPO_KL_EXACT ? d->kl->hist_other : NULL;
    if (!src) return 0;
    unsigned steps = 0;
    phip_d2h(&steps, &d->kl->step, sizeof(unsigned));
    long have = steps < (unsigned)PHIP_KL_HIST ? (long)steps : PHIP_KL_HIST;
    if (have > n) have = n;
    if (out && have > 0) {
        float* h = (float*)xmalloc(sizeof(float) * (size_t)have);
        phip_d2h(h, src, sizeof(float) * (size_t)have);
        for (long i = 0; i < have; i++) out[i] = (double)h[i];
        free(h);
    }
    return (int)steps;
}

int ppo_policy_kl_device(const float* d_mu, const float* d_log_std, const float* d_action, const float* d_old_lp,
                         int m, int A, float eps, double* out2) {
    static PhipKlRec* rec = NULL;
    if (!d_mu || !d_log_std || !d_action || !d_old_lp || !out2 || m <= 0 || A <= 0) return -1;
    if (!rec) rec = (PhipKlRec*)phip_malloc(sizeof(PhipKlRec));
    phip_memset(rec, 0, offsetof(PhipKlRec, ticket));
    phip_policy_kl(d_mu, d_log_std, d_action, d_old_lp, m, A, 0, eps, INFINITY, m, 1, rec, NULL, 0, NULL, NULL, NULL,
                   NULL);
    float sums[4];
    phip_d2h(sums, rec->sums, sizeof(sums));
    out2[0] = (double)sums[0] / m;
    out2[1] = (double)sums[1] / m;
    return 0;
}

/* ppo_ext.h: one form of the policy head on caller-supplied device arrays */
int ppo_policy_head_device(int form, int m, int A, int n, int relu_in, float eps, float ent_coeff,
                           const float* d_log_std, const float* d_action, const float* d_adv, const float* d_old_lp,
                           float* d_mu, const float* d_x, const float* d_W, const float* d_b, float* d_lp,
                           float* d_grad_mu, float* d_gx, float* d_gW, float* d_grad_log_std, double* loss) {
    static float* word = NULL;                    /* [0] the loss, [1] form 0's entropy */
    static float* glp = NULL;                     /* form 0: ∂L/∂lp [glp_cap] */
    static long glp_cap = 0;
    if (form < 0 || form > 4 || m <= 0 || A <= 0 || isnan(eps) || !d_log_std || !d_action || !d_adv || !d_old_lp ||
        !d_mu || !d_grad_log_std || !loss)
        return -1;
    const int net = form >= 2;                    /* the forms that carry the output layer */
    if (net) {
        if (n <= 0 || !d_x || !d_W || !d_gx || !d_gW || (form != 3 && !d_b)) return -1;
        if ((((uintptr_t)d_x | (uintptr_t)d_gx | (uintptr_t)d_W | (uintptr_t)d_gW) & 15u) != 0) return -1;
    } else if (!d_grad_mu || (form == 0 && !d_lp)) {
        return -1;
    }
    /* the shape, by the kernels' own predicates */
    if (form == 0 && A > 16384) return 1;         /* log_prob_bwd_kernel: A column sums in 64 KiB of LDS */
    if (form == 1 && A > 4096) return 1;          /* phip_policy_head's own limit */
    if (form == 2 && !phip_out_head_supported(1, n, A)) return 1;
    if (form == 3 && !phip_out_bwd_wide_ok(m, n, A, 1)) return 1;
    if (!word) word = (float*)phip_malloc(4 * sizeof(float));
    float* gb = net ? d_gW + (long)A * n : NULL;
    phip_memset(word, 0, 4 * sizeof(float));
    phip_memset(d_grad_log_std, 0, sizeof(float) * (size_t)A);
    if (net) phip_memset(d_gW, 0, sizeof(float) * ((size_t)A * n + A));
    switch (form) {
        case 0:
            if (glp_cap < m) {
                if (glp) phip_free(glp);
                glp = (float*)phip_malloc(sizeof(float) * (size_t)m);
                glp_cap = m;
            }
            phip_log_prob(d_mu, d_log_std, d_action, d_lp, m, A);
            phip_entropy(d_log_std, A, word + 1);
            phip_policy_loss(d_adv, d_lp, d_old_lp, glp, m, eps, ent_coeff, word + 1, NULL, word);
            phip_log_prob_bwd(d_mu, d_log_std, d_action, glp, d_grad_mu, d_grad_log_std, m, A);
            break;
        case 1:
            phip_policy_head(d_mu, d_log_std, d_action, d_adv, d_old_lp, m, A, eps, ent_coeff, d_grad_mu,
                             d_grad_log_std, word, 1);
            break;
        case 2:
            phip_out_head(1, 0, d_x, relu_in, d_W, d_b, m, n, A, NULL, d_log_std, d_action, d_adv, d_old_lp, eps,
                          ent_coeff, d_mu, d_gx, d_gW, gb, d_grad_log_std, word, NULL);
            break;
        case 3:
            if (!phip_policy_head_bwd_wide(d_mu, d_log_std, d_action, d_adv, d_old_lp, eps, ent_coeff, d_grad_log_std,
                                           word, d_x, d_W, relu_in, d_gW, gb, d_gx, m, n, A))
                return 1;
            break;
        default:
            if (!phip_policy_out_fused(d_x, d_W, d_b, d_mu, d_log_std, d_action, d_adv, d_old_lp, eps, ent_coeff,
                                       d_grad_log_std, word, relu_in, d_gW, gb, d_gx, m, n, A))
                return 1;
            break;
    }
    phip_sync();
    float l = 0.f;
    phip_d2h(&l, word, sizeof(float));
    *loss = (double)l;
    return 0;
}

/* the mask store: on — capacity × W words (allocated once: neither capacity nor A changes), every bit set; off —
 * freed once nothing in flight reads it */
static void mask_store(PPO* ppo, PPODev* d, int on) {
    const int A = ppo->buffer->action_size;
    phip_sync();
    if (!on) {
        phip_free(d->mask);
        d->mask = NULL;
        d->mask_on = 0;
        return;
    }
    const size_t bytes = sizeof(uint32_t) * (size_t)ppo->buffer->capacity * (size_t)mask_words(A);
    if (!d->mask) d->mask = (uint32_t*)phip_malloc(bytes);
    phip_memset(d->mask, 0xFF, bytes);
    d->mask_on = 1;
}

/* ppo_ext.h: the action distribution */
int ppo_set_action_dist(void* vppo, int dist) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo || (dist != 0 && dist != 1)) return -1;
    if (dist == 1) {
        const int A = ppo->buffer->action_size;
        if (A < 2 || A > PHIP_CAT_MAX_A) return -1;
        if (ppo->V->dtype == 1 || ppo->policy->mu->dtype == 1) return -1;       /* bf16 compute mode */
    }
    PPODev* d = dev_ws(ppo, 1);
    if (dist == 1 && !d->cat_off) {                  /* the categorical policy as nvec = {A}: A never changes */
        const int off[2] = {0, ppo->buffer->action_size};
        d->cat_off = (int*)phip_malloc(sizeof(off));
        phip_h2d(d->cat_off, off, sizeof(off));
    }
    d->action_dist = dist;
    /* masking belongs to a discrete policy: off with it; under another one the columns mean something else: full
     * masks again */
    if (d->mask_on) mask_store(ppo, d, dist != 0);
    return 0;
}

int ppo_get_action_dist(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    return ppo && ppo->dev ? ((PPODev*)ppo->dev)->action_dist : 0;
}

/* nvec → the D + 1 offsets in off (host) and the widest component; −1 unless 1 <= D <= PPO_MD_MAX_D, every n_d >= 2,
 * Σ n_d == A and 2 <= A <= PHIP_CAT_MAX_A */
static int md_offsets(const int* nvec, int D, int A, int* off) {
    if (!nvec || D < 1 || D > PHIP_MD_MAX_D || A < 2 || A > PHIP_CAT_MAX_A) return -1;
    int max_n = 0;
    off[0] = 0;
    for (int i = 0; i < D; i++) {
        if (nvec[i] < 2 || nvec[i] > A) return -1;
        off[i + 1] = off[i] + nvec[i];
        if (off[i + 1] > A) return -1;
        if (nvec[i] > max_n) max_n = nvec[i];
    }
    return off[D] == A ? max_n : -1;
}

/* ppo_ext.h: the multi-discrete policy */
int ppo_set_action_multidiscrete(void* vppo, const int* nvec, int D) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo || !nvec) return -1;
    int off[PHIP_MD_MAX_D + 1];
    const int max_n = md_offsets(nvec, D, ppo->buffer->action_size, off);
    if (max_n < 0) return -1;
    if (ppo->V->dtype == 1 || ppo->policy->mu->dtype == 1) return -1;           /* bf16 compute mode */
    PPODev* d = dev_ws(ppo, 1);
    if (!d->md_off) d->md_off = (int*)phip_malloc(sizeof(int) * (PHIP_MD_MAX_D + 1));
    phip_sync();                                     /* nothing in flight reads the offsets being replaced */
    phip_h2d(d->md_off, off, sizeof(int) * (size_t)(D + 1));
    memcpy(d->md_nvec, nvec, sizeof(int) * (size_t)D);
    d->md_D = D;
    d->md_max_n = max_n;
    d->action_dist = 2;
    if (d->mask_on) mask_store(ppo, d, 1);           /* the columns mean something else now: full masks again */
    return 0;
}

int ppo_get_action_nvec(void* vppo, int* out, int cap) {
    PPO* ppo = (PPO*)vppo;
    const PPODev* d = ppo ? (const PPODev*)ppo->dev : NULL;
    if (!md_on(d)) return 0;
    for (int i = 0; out && i < d->md_D && i < cap; i++) out[i] = d->md_nvec[i];
    return d->md_D;
}

/* ppo_ext.h: the state-dependent-σ Gaussian */
static int sd_bounds_ok(float lo, float hi) {
    return !isnan(lo) && !isnan(hi) && lo < hi && lo >= -20.f && lo <= 20.f && hi >= -20.f && hi <= 20.f;
}

int ppo_set_action_gaussian_sd(void* vppo, float ls_min, float ls_max) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo || !sd_bounds_ok(ls_min, ls_max) || !phip_sd_shape_ok(ppo->buffer->action_size)) return -1;
    if (ppo->V->dtype == 1 || ppo->policy->mu->dtype == 1) return -1;           /* bf16 compute mode */
    PPODev* d = dev_ws(ppo, 1);
    if (!d->sd_rec) d->sd_rec = (PhipSdRec*)phip_malloc(sizeof(PhipSdRec));
    d->sd_ls[0] = ls_min;
    d->sd_ls[1] = ls_max;
    d->action_dist = 3;
    if (d->mask_on) mask_store(ppo, d, 0);           /* masking belongs to a discrete policy: off with it */
    return 0;
}

int ppo_get_action_gaussian_sd(void* vppo, float* out2) {
    PPO* ppo = (PPO*)vppo;
    const PPODev* d = ppo ? (const PPODev*)ppo->dev : NULL;
    if (!sd_on(d)) return 0;
    if (out2) { out2[0] = d->sd_ls[0]; out2[1] = d->sd_ls[1]; }
    return 1;
}

/* the head, the sampler and the closed-form KL launch on caller-supplied device arrays (test entries: bad arguments
 * return −1 ahead of any device call, so nothing is recorded for ppo_last_error) */
int ppo_gauss_sd_head_device(const float* d_z, const float* d_action, const float* d_adv, const float* d_old_lp,
                             int m, int A, float ls_min, float ls_max, float eps, float ent_coeff, float* d_grad,
                             float* d_lp, float* d_ent, double* loss, long long* clamped2) {
    static PhipSdRec* rec = NULL;
    if (!d_z || !d_action || !d_adv || !d_old_lp || !d_grad || !d_lp || !d_ent || !loss || !clamped2 || m <= 0 ||
        !phip_sd_shape_ok(A) || !sd_bounds_ok(ls_min, ls_max) || isnan(eps))
        return -1;
    if (!rec) rec = (PhipSdRec*)phip_malloc(sizeof(PhipSdRec));
    phip_memset(rec, 0, offsetof(PhipSdRec, ticket));
    phip_sd_head(d_z, d_action, d_adv, d_old_lp, m, A, ls_min, ls_max, eps, ent_coeff, d_grad, d_lp, d_ent, rec, NULL);
    phip_sync();
    PhipSdRec r;
    phip_d2h(&r, rec, offsetof(PhipSdRec, ticket));
    *loss = r.loss;
    clamped2[0] = (long long)r.counts[0];
    clamped2[1] = (long long)r.counts[1];
    return 0;
}

int ppo_gauss_sd_sample_device(const float* d_z, int m, int A, float ls_min, float ls_max, unsigned long long key,
                               unsigned long long offset, float* d_action, float* d_log_prob) {
    if (!d_z || !d_action || !d_log_prob || m <= 0 || !phip_sd_shape_ok(A) || !sd_bounds_ok(ls_min, ls_max)) return -1;
    phip_sd_sample(d_z, NULL, d_action, d_log_prob, m, A, ls_min, ls_max, key, offset);
    phip_sync();
    return 0;
}

int ppo_gauss_sd_kl_exact_device(const float* d_new, const float* d_old, const int* d_rows, int m, int A, float ls_min,
                                 float ls_max, double* d_row_kl, double* out_mean) {
    static PhipKlRec* rec = NULL;
    if (!d_new || !d_old || !out_mean || m <= 0 || !phip_sd_shape_ok(A) || !sd_bounds_ok(ls_min, ls_max)) return -1;
    if (!rec) rec = (PhipKlRec*)phip_malloc(sizeof(PhipKlRec));
    phip_memset(rec, 0, offsetof(PhipKlRec, ticket));
    const PhipKlExact ex = {d_old, NULL, d_rows, NULL, 0, 0, d_row_kl};
    const float sd[2] = {ls_min, ls_max};
    phip_policy_kl(d_new, NULL, NULL, NULL, m, A, 3, 0.f, INFINITY, m, 1, rec, NULL, 0, NULL, NULL, &ex, sd);
    phip_sync();
    float sums[4];
    phip_d2h(sums, rec->sums, sizeof(sums));
    *out_mean = (double)sums[2] / m;
    return 0;
}

/* the discrete head and sampler on caller-supplied device arrays (the test entries below: bad arguments return −1
 * ahead of any device call, so nothing is recorded for ppo_last_error); nvec is a host array, its offsets go to a
 * device array kept here */
static int* md_test_offsets(const int* nvec, int D, int A, int* max_n) {
    static int* d_off = NULL;
    int off[PHIP_MD_MAX_D + 1];
    *max_n = md_offsets(nvec, D, A, off);
    if (*max_n < 0) return NULL;
    if (!d_off) d_off = (int*)phip_malloc(sizeof(int) * (PHIP_MD_MAX_D + 1));
    phip_sync();
    phip_h2d(d_off, off, sizeof(int) * (size_t)(D + 1));
    return d_off;
}

/* d_mask NULL: the unmasked head (d_rows unread) */
static int disc_head_device(const float* d_logits, const float* d_action, const float* d_adv, const float* d_old_lp,
                            const uint32_t* d_mask, const int* d_rows, int m, int A, const int* nvec, int D, float eps,
                            float ent_coeff, float* d_grad, float* d_lp, float* d_ent, double* loss) {
    static float* word = NULL;
    if (!d_logits || !d_action || !d_adv || !d_old_lp || !d_grad || !d_lp || !d_ent || !loss || m <= 0 || isnan(eps))
        return -1;
    int max_n;
    const int* d_off = md_test_offsets(nvec, D, A, &max_n);
    if (!d_off) return -1;
    if (!word) word = (float*)phip_malloc(4 * sizeof(float));
    phip_memset(word, 0, 4 * sizeof(float));
    phip_disc_head(d_logits, d_action, d_adv, d_old_lp, d_mask, d_rows, m, A, d_off, D, max_n, eps, ent_coeff, d_grad,
                   d_lp, d_ent, word, NULL);
    phip_sync();
    float l = 0.f;
    phip_d2h(&l, word, sizeof(float));
    *loss = (double)l;
    return 0;
}

/* d_mask NULL: the unmasked sampler */
static int disc_sample_device(const float* d_logits, const uint32_t* d_mask, int m, int A, const int* nvec, int D,
                              unsigned long long key, unsigned long long offset, float* d_action, float* d_log_prob) {
    if (!d_logits || !d_action || !d_log_prob || m <= 0) return -1;
    int max_n;
    const int* d_off = md_test_offsets(nvec, D, A, &max_n);
    if (!d_off) return -1;
    phip_disc_sample(d_logits, d_mask, NULL, d_off, d_action, d_log_prob, NULL, m, A, D, key, offset);
    phip_sync();
    return 0;
}

int ppo_multidiscrete_head_device(const float* d_logits, const float* d_action, const float* d_adv,
                                  const float* d_old_lp, int m, int A, const int* nvec, int D, float eps,
                                  float ent_coeff, float* d_grad, float* d_lp, float* d_ent, double* loss) {
    return disc_head_device(d_logits, d_action, d_adv, d_old_lp, NULL, NULL, m, A, nvec, D, eps, ent_coeff, d_grad,
                            d_lp, d_ent, loss);
}

int ppo_multidiscrete_sample_device(const float* d_logits, int m, int A, const int* nvec, int D,
                                    unsigned long long key, unsigned long long offset, float* d_action,
                                    float* d_log_prob) {
    return disc_sample_device(d_logits, NULL, m, A, nvec, D, key, offset, d_action, d_log_prob);
}

/* ppo_ext.h: invalid-action masking */
int ppo_set_action_mask(void* vppo, int on) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo) return -1;
    PPODev* d = dev_ws(ppo, 1);
    if (!cat_on(d)) return -1;                       /* a Gaussian policy has no columns to mask */
    if ((on != 0) != (d->mask_on != 0)) mask_store(ppo, d, on != 0);
    return 0;
}

int ppo_get_action_mask(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    return ppo && mask_on((const PPODev*)ppo->dev);
}

int ppo_action_mask_words(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    return ppo ? mask_words(ppo->buffer->action_size) : 0;
}

uint32_t* ppo_action_mask_buffer(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    return ppo && mask_on((const PPODev*)ppo->dev) ? ((PPODev*)ppo->dev)->mask : NULL;
}

/* the masked head, sampler and greedy action on caller-supplied device arrays (test entries; the categorical policy
 * is nvec = {A}) */
int ppo_masked_head_device(const float* d_logits, const float* d_action, const float* d_adv, const float* d_old_lp,
                           const uint32_t* d_mask, const int* d_rows, int m, int A, const int* nvec, int D, float eps,
                           float ent_coeff, float* d_grad, float* d_lp, float* d_ent, double* loss) {
    if (!d_mask) return -1;
    return disc_head_device(d_logits, d_action, d_adv, d_old_lp, d_mask, d_rows, m, A, nvec, D, eps, ent_coeff, d_grad,
                            d_lp, d_ent, loss);
}

int ppo_masked_sample_device(const float* d_logits, const uint32_t* d_mask, int m, int A, const int* nvec, int D,
                             unsigned long long key, unsigned long long offset, float* d_action, float* d_log_prob) {
    if (!d_mask) return -1;
    return disc_sample_device(d_logits, d_mask, m, A, nvec, D, key, offset, d_action, d_log_prob);
}

int ppo_masked_argmax_device(const float* d_logits, const uint32_t* d_mask, int m, int A, const int* nvec, int D,
                             float* d_action) {
    if (!d_logits || !d_mask || !d_action || m <= 0) return -1;
    int max_n;
    const int* d_off = md_test_offsets(nvec, D, A, &max_n);
    if (!d_off) return -1;
    phip_disc_argmax(d_logits, d_mask, d_off, d_action, m, A, D);
    phip_sync();
    return 0;
}

/* ppo_ext.h: the closed-form KL launch of the update on caller-supplied device arrays (a test entry) */
int ppo_policy_kl_exact_device(int dist, const float* d_new, const float* d_log_std_new, const float* d_old,
                               const float* d_log_std_old, const int* d_rows, const float* d_action,
                               const uint32_t* d_mask, int m, int A, const int* nvec, int D, double* d_row_kl,
                               double* out_mean) {
    static PhipKlRec* rec = NULL;
    if (!d_new || !d_old || !out_mean || m <= 0 || A <= 0 || dist < 0 || dist > 2) return -1;
    if (dist == 0 && (!d_log_std_new || !d_log_std_old || d_mask)) return -1;
    if (d_mask && !d_action) return -1;
    const int* d_off = NULL;
    int max_n = 0;
    if (dist != 0) {
        const int one[1] = {A};
        if (dist == 2 && (!nvec || D < 1)) return -1;
        d_off = md_test_offsets(dist == 1 ? one : nvec, dist == 1 ? 1 : D, A, &max_n);
        if (!d_off) return -1;
    }
    const int Dc = dist == 1 ? 1 : dist == 2 ? D : 0;
    if (!rec) rec = (PhipKlRec*)phip_malloc(sizeof(PhipKlRec));
    phip_memset(rec, 0, offsetof(PhipKlRec, ticket));
    const PhipKlExact ex = {d_old, d_log_std_old, d_rows, d_off, Dc, max_n > 32, d_row_kl};
    /* a mask takes the multi-discrete form of the launch, the categorical policy as nvec = {A} */
    phip_policy_kl(d_new, d_log_std_new, d_action, NULL, m, A, dist == 0 ? 0 : 2, 0.f, INFINITY, m, 1, rec, d_off, Dc,
                   d_mask, d_mask ? d_rows : NULL, &ex, NULL);
    phip_sync();
    float sums[4];
    phip_d2h(sums, rec->sums, sizeof(sums));
    *out_mean = (double)sums[2] / m;
    return 0;
}

/* the categorical head and sampler on caller-supplied device arrays (test entries); the sampler is nvec = {A} */
int ppo_categorical_head_device(const float* d_logits, const float* d_action, const float* d_adv,
                                const float* d_old_lp, int m, int A, float eps, float ent_coeff, float* d_grad,
                                float* d_lp, float* d_ent, double* loss) {
    static float* word = NULL;
    if (!d_logits || !d_action || !d_adv || !d_old_lp || !d_grad || !d_lp || !d_ent || !loss || m <= 0 || A < 2 ||
        A > PHIP_CAT_MAX_A || isnan(eps))
        return -1;
    if (!word) word = (float*)phip_malloc(4 * sizeof(float));
    phip_memset(word, 0, 4 * sizeof(float));
    phip_cat_head(d_logits, d_action, d_adv, d_old_lp, m, A, eps, ent_coeff, d_grad, d_lp, d_ent, word, NULL);
    phip_sync();
    float l = 0.f;
    phip_d2h(&l, word, sizeof(float));
    *loss = (double)l;
    return 0;
}

int ppo_categorical_sample_device(const float* d_logits, int m, int A, unsigned long long key,
                                  unsigned long long offset, float* d_action, float* d_log_prob) {
    return disc_sample_device(d_logits, NULL, m, A, &A, 1, key, offset, d_action, d_log_prob);
}

/* ppo_ext.h: global gradient-norm clipping */
int ppo_set_max_grad_norm(void* vppo, float max_norm) {
    if (isnan(max_norm)) return -1;
    PPODev* d = dev_ws((PPO*)vppo, 1);
    d->max_grad_norm = (max_norm > 0.f && !isinf(max_norm)) ? max_norm : 0.f;
    return 0;
}

float ppo_get_max_grad_norm(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    return ppo->dev ? ((PPODev*)ppo->dev)->max_grad_norm : 0.f;
}

double ppo_grad_norm_device(const float* d_a, long na, const float* d_b, long nb) {
    static PhipClipRec* rec = NULL;
    if (!rec) rec = (PhipClipRec*)phip_malloc(sizeof(PhipClipRec));
    if (na < 0) na = 0;
    if (nb < 0) nb = 0;
    phip_memset(rec, 0, offsetof(PhipClipRec, partial));
    phip_grad_norm(d_a, na, d_b, nb, 1.0f, INFINITY, rec);
    double norm = 0.0;
    phip_d2h(&norm, &rec->norm, sizeof(double));
    return norm;
}

/* ppo.cu:451-558 */
void train_ppo_epoch(PPO* ppo, Env* env, int steps_per_epoch, int batch_size, int n_epochs_policy,
                     int n_epochs_value) {
    /* the host rollout samples from μ(raw state): it has no handle to the normaliser */
    if (sd_on((PPODev*)ppo->dev))
        die("train_ppo_epoch: the state-dependent-σ Gaussian policy (ppo_set_action_gaussian_sd) is not supported by "
            "the host rollout; use ppo_rollout_device + ppo_update");
    if (cat_on((PPODev*)ppo->dev))
        die("train_ppo_epoch: a discrete policy (ppo_set_action_dist, ppo_set_action_multidiscrete) is not supported "
            "by the host rollout; use ppo_rollout_device + ppo_update");
    if (obs_on((PPODev*)ppo->dev))
        die("train_ppo_epoch: observation normalisation (ppo_set_obs_norm) is not supported by the host rollout; "
            "use ppo_rollout_device + ppo_update");
    /* the host rollout resets the environment at each call: its buffer is scanned with no carry (reward
     * normalisation), and a device rollout after it starts from a zero carry */
    if (ppo->dev) ((PPODev*)ppo->dev)->ro_laid = ((PPODev*)ppo->dev)->rew_scanned = 0;
    if (ppo->dev && ((PPODev*)ppo->dev)->ext_open) ((PPODev*)ppo->dev)->ext_open = ((PPODev*)ppo->dev)->ext_done = 0;
    for (int i = 0; i < steps_per_epoch / ppo->buffer->capacity; i++) {
        collect_trajectories(ppo->buffer, env, ppo->policy, ppo->buffer->capacity);
        buffer_to_device(ppo->buffer);
        ppo_update(ppo, env->gamma, batch_size, n_epochs_policy, n_epochs_value, PPO_SHUFFLE_HOST_RAND, 0);
        buffer_to_host(ppo->buffer);
        policy_to_host(ppo->policy);
        nn_write_weights_to_host(ppo->V);
    }
}

/* ppo.cu:560-583: rollout `steps` and print the mean discounted return J and return R */
void eval_ppo(PPO* ppo, Env* env, int steps) {
    if (sd_on((PPODev*)ppo->dev))
        die("eval_ppo: the state-dependent-σ Gaussian policy (ppo_set_action_gaussian_sd) is not supported by the host "
            "rollout; use ppo_eval_device");
    if (cat_on((PPODev*)ppo->dev))
        die("eval_ppo: a discrete policy (ppo_set_action_dist, ppo_set_action_multidiscrete) is not supported by the "
            "host rollout; use ppo_eval_device");
    if (obs_on((PPODev*)ppo->dev))
        die("eval_ppo: observation normalisation (ppo_set_obs_norm) is not supported by the host rollout");
    reset_buffer(ppo->buffer);
    collect_trajectories(ppo->buffer, env, ppo->policy, steps);
    TrajectoryBuffer* b = ppo->buffer;
    float rewards = *b->reward(b, steps - 1);
    float episode_J = *b->reward(b, steps - 1);
    int n_episodes = 1;
    float sum_J = 0;
    for (int i = steps - 2; i >= 0; i--) {
        rewards += *b->reward(b, i);
        episode_J = *b->reward(b, i) + env->gamma * episode_J;
        if (*b->terminated(b, i) || *b->truncated(b, i)) {
            n_episodes++;
            sum_J += episode_J;
            episode_J = 0;
        }
    }
    printf("J: %f R: %f Episodes: %d\n", sum_J / n_episodes, rewards / n_episodes, n_episodes);
    reset_buffer(ppo->buffer);
}

/* ------------------------------------------------------------------ */
/* batched sampling / synthetic rollouts (ppo_ext.h)                   */
/* ------------------------------------------------------------------ */
void ppo_sample_action_device(void* vpolicy, float* d_state, float* d_action, float* d_log_prob, int m,
                              unsigned long long seed, unsigned long long offset) {
    GaussianPolicy* p = (GaussianPolicy*)vpolicy;
    nn_forward_dev(p->mu, d_state, m);
    phip_sample(p->mu->d_output, p->d_log_std, d_action, d_log_prob, m, p->action_size, seed, offset);
}

/* The pieces ppo_rollout_device and the open rollout (ppo_rollout_begin … _end) share, so that the two cannot
 * drift.  The row map rows[t·E + e] = e·T + t for E × T (called before ro_E changes): */
static void ro_rows_ws(PPODev* d, int E, int T) {
    if (d->ro_E == E && d->ro_T == T && d->ro_rows) return;
    phip_free(d->ro_rows);
    d->ro_rows = (int*)phip_malloc(sizeof(int) * (size_t)E * (size_t)T);
    phip_rollout_rows(d->ro_rows, E, T);
    d->ro_T = T;
}

void ppo_dev_ro_rows(PPODev* d, int E, int T) { ro_rows_ws(d, E, T); }

/* fresh episodes in E environments of `kind`: nothing continues, nothing is carried (phip_malloc zeroes) */
static void ro_fresh(PPODev* d, int E, int kind, int S) {
    phip_free(d->ro_cont); phip_free(d->rew_carry_in); phip_free(d->rew_carry_out);
    d->ro_cont = (unsigned char*)phip_malloc((size_t)E);
    d->rew_carry_in = (double*)phip_malloc(sizeof(double) * (size_t)E);
    d->rew_carry_out = (double*)phip_malloc(sizeof(double) * (size_t)E);
    d->rew_scanned = 0;
    /* episode statistics: the episodes in progress are dropped with the environments, the window stays */
    phip_free(d->ep_state);
    d->ep_state = (double*)phip_malloc(4 * sizeof(double) * (size_t)E);
    d->ep_fresh = 1;
    d->ro_E = E;
    d->ro_kind = kind;
    d->ro_S = S;
}

/* the returns' carry (reward normalisation; kept with the feature off too, so that it may be turned on
 * between a rollout and its update): what an update's scan of the rollout just before this one left
 * becomes this one's carry_in; with no such scan every return restarts from 0 */
static void ro_carry_swap(PPODev* d, int E) {
    if (d->rew_scanned) {
        double* t = d->rew_carry_in;
        d->rew_carry_in = d->rew_carry_out;
        d->rew_carry_out = t;
    } else {
        phip_memset(d->rew_carry_in, 0, sizeof(double) * (size_t)E);
    }
    d->rew_scanned = 0;
}

/* behind the last step of a rollout of E × T rows: the buffer becomes rollout-laid and ready for ppo_update */
static void ro_finish(PPO* ppo, PPODev* d, int E, int T) {
    TrajectoryBuffer* b = ppo->buffer;
    const long N = (long)E * T;
    /* episode statistics: one scan of the rows just laid (two launches, no host read) — the batch becomes the
     * last rollout's aggregate and is folded into the window */
    if (!d->ep_agg) d->ep_agg = (double*)phip_malloc(16 * sizeof(double));
    phip_episode_scan(b->d_reward_p, (const uint8_t*)b->d_terminated_p, (const uint8_t*)b->d_truncated_p, d->ro_cont,
                      E, T, d->ep_gamma, d->ep_fresh ? NULL : d->ep_state, d->ep_state, NULL, NULL, d->ep_agg + 8,
                      d->ep_agg);
    d->ep_fresh = 0;
    phip_memset(b->d_advantage_p, 0, sizeof(float) * (size_t)N);
    phip_memset(b->d_adv_target_p, 0, sizeof(float) * (size_t)N);
    b->idx = (int)(N % b->capacity);
    b->full = N == b->capacity;
    buffer_point_device(b);
    d->ro_laid = 1;
}

void ppo_rollout_device(void* vppo, int n_envs, int horizon, int env_kind, unsigned long long seed) {
    PPO* ppo = (PPO*)vppo;
    TrajectoryBuffer* b = ppo->buffer;
    const int E = n_envs, T = horizon;
    const long N = (long)E * T;
    if (E <= 0 || T <= 0 || N > b->capacity) die("ppo_rollout_device: n_envs*horizon must be in [1, capacity]");
    if (env_kind < 0 || env_kind > 2)
        die("ppo_rollout_device: env_kind must be 0 (Pendulum-v1), 1 (synthetic) or 2 (CartPole-v1)");
    const int S = b->state_size, A = b->action_size;
    PPODev* d = dev_ws(ppo, 1);
    const int cat = cat_on(d), sd = sd_on(d);
    const int Au = sd ? A / 2 : A;                   /* the action columns the environment reads */
    if (env_kind == 0 && (S != 3 || Au != 1))
        die("ppo_rollout_device: Pendulum-v1 needs state_size 3, action_size 1 (2 under the state-dependent-σ Gaussian)");
    if (env_kind == 2 && (S != 4 || A != 2 || !cat))
        die("ppo_rollout_device: CartPole-v1 needs state_size 4, action_size 2 and the categorical policy "
            "(ppo_set_action_dist, or ppo_set_action_multidiscrete with nvec = {2})");
    d->ext_open = d->ext_done = 0;                               /* an open rollout is simply closed */
    ro_rows_ws(d, E, T);
    if (d->ro_E != E || d->ro_kind != env_kind || d->ro_S != S || !d->env_state) {
        phip_free(d->env_state);
        d->env_state = (float*)phip_malloc(sizeof(float) * (size_t)E * PHIP_ENV_STATE(S));
        phip_env_reset(env_kind, d->env_state, b->d_state_p, E, T, S, splitmix64(seed));
        ro_fresh(d, E, env_kind, S);
    }
    ro_carry_swap(d, E);
    const uint64_t key = splitmix64(seed ^ 0x524F4C4CULL);
    GaussianPolicy* pol = ppo->policy;
    mask_fill_full(d, N, A);                         /* the built-in environments have no illegal actions */
    phip_env_first_obs(env_kind, d->env_state, b->d_state_p, E, T, S);
    /* observation normalisation: each step's E rows are normalised through the row map into the shadow (the
     * same rows there) and μ is forwarded from it; the buffer keeps the raw observations */
    float* shadow = obs_on(d) ? obs_shadow(ppo, d) : NULL;
    for (int t = 0; t < T; t++) {
        const int* rows = d->ro_rows + (long)t * E;
        if (shadow)
            phip_obs_normalize_rows(b->d_state_p, rows, shadow, rows, E, S, d->obs_m, d->obs_m + S, d->obs_clip,
                                    d->obs_run);
        nn_forward_dev_rows(pol->mu, shadow ? shadow : b->d_state_p, rows, NULL, E);
        /* one position in the Philox streams per step of every call: the policy noise and the environment's
         * draws never repeat under a constant seed */
        const uint64_t step = d->ro_step++;
        if (cat)
            phip_disc_sample_rows(pol->mu->d_output, NULL, rows, disc_off(d), b->d_action_p, b->d_logprob_p, NULL, E, A,
                                  disc_D(d), key, step);
        else if (sd)
            phip_sd_sample_rows(pol->mu->d_output, rows, b->d_action_p, b->d_logprob_p, E, A, d->sd_ls[0], d->sd_ls[1],
                                key, step);
        else phip_sample_rows(pol->mu->d_output, pol->d_log_std, rows, b->d_action_p, b->d_logprob_p, E, A, key, step);
        phip_env_step(env_kind, d->env_state, b->d_state_p, b->d_action_p, b->d_next_state_p, b->d_reward_p,
                      (uint8_t*)b->d_terminated_p, (uint8_t*)b->d_truncated_p, d->ro_cont, E, T, t, step, S, A, key,
                      cat, md_off(d), d->md_D, Au);
    }
    ro_finish(ppo, d, E, T);
}

void ppo_fill_synthetic(void* vppo, int n_envs, int horizon, unsigned long long seed, float p_terminate) {
    PPO* ppo = (PPO*)vppo;
    TrajectoryBuffer* b = ppo->buffer;
    const long N = (long)n_envs * horizon;
    if (N <= 0 || N > b->capacity) die("ppo_fill_synthetic: n_envs*horizon must be in [1, capacity]");
    const int S = b->state_size, A = b->action_size;
    const uint64_t s0 = splitmix64(seed);
    phip_fill_uniform(b->d_state_p, N * S, s0 ^ 0x1, -1.f, 1.f);
    phip_fill_rollout_flags((uint8_t*)b->d_terminated_p, (uint8_t*)b->d_truncated_p, n_envs, horizon, p_terminate,
                            s0 ^ 0x2);
    phip_link_next_state(b->d_next_state_p, b->d_state_p, (const uint8_t*)b->d_terminated_p, n_envs, horizon, S,
                         s0 ^ 0x3);
    phip_fill_normal(b->d_reward_p, N, s0 ^ 0x4, 0.1f);
    /* observation normalisation: the actions are sampled from μ(norm(state)) */
    float* obs = b->d_state_p;
    if (ppo->dev && obs_on((PPODev*)ppo->dev)) {
        PPODev* d = (PPODev*)ppo->dev;
        obs = obs_shadow(ppo, d);
        phip_obs_normalize(b->d_state_p, obs, N, S, d->obs_m, d->obs_m + S, d->obs_clip, d->obs_run, NULL);
    }
    if (cat_on((PPODev*)ppo->dev)) {     /* discrete: one uniform per (row, component) from the "action noise" key */
        nn_forward_dev(ppo->policy->mu, obs, (int)N);
        PPODev* d = (PPODev*)ppo->dev;
        mask_fill_full(d, N, A);                     /* sampled unmasked: the rows carry full masks */
        phip_disc_sample(ppo->policy->mu->d_output, NULL, NULL, disc_off(d), b->d_action_p, b->d_logprob_p, NULL, (int)N,
                         A, disc_D(d), s0 ^ 0x5, 0);
    } else if (sd_on((PPODev*)ppo->dev)) {           /* the "action noise" key, counter i·Aa + j */
        PPODev* d = (PPODev*)ppo->dev;
        nn_forward_dev(ppo->policy->mu, obs, (int)N);
        phip_sd_sample(ppo->policy->mu->d_output, NULL, b->d_action_p, b->d_logprob_p, (int)N, A, d->sd_ls[0],
                       d->sd_ls[1], s0 ^ 0x5, 0);
    } else {
        ppo_sample_action_device(ppo->policy, obs, b->d_action_p, b->d_logprob_p, (int)N, s0 ^ 0x5, 0);
    }
    phip_memset(b->d_advantage_p, 0, sizeof(float) * (size_t)N);
    phip_memset(b->d_adv_target_p, 0, sizeof(float) * (size_t)N);
    b->idx = (int)(N % b->capacity);
    b->full = N == b->capacity;
    buffer_point_device(b);
    /* not laid by a device rollout: scanned as one stream, and the next rollout starts from a zero carry */
    if (ppo->dev) ((PPODev*)ppo->dev)->ro_laid = ((PPODev*)ppo->dev)->rew_scanned = 0;
    /* an open rollout is simply closed: its rows are gone, so nothing continues from it */
    if (ppo->dev && ((PPODev*)ppo->dev)->ext_open) ((PPODev*)ppo->dev)->ext_open = ((PPODev*)ppo->dev)->ext_done = 0;
}

/* ------------------------------------------------------------------ */
/* the open rollout: the caller steps the environment (ppo_ext.h)      */
/* ------------------------------------------------------------------ */
int ppo_rollout_begin(void* vppo, int n_envs, int horizon, const float* d_obs0, unsigned long long seed) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo || n_envs <= 0 || horizon <= 0) return -1;
    TrajectoryBuffer* b = ppo->buffer;
    const int E = n_envs, T = horizon, S = b->state_size;
    if ((long)E * T > b->capacity) return -1;
    PPODev* d = dev_ws(ppo, 1);
    if (!d_obs0 && !(d->ext_done && !d->ext_open && d->ro_kind == PHIP_ENV_EXTERNAL && d->ro_E == E && d->ro_S == S))
        return -1;
    ro_rows_ws(d, E, T);
    if (d_obs0) {
        if ((long)E * S > d->ext_obs_cap) {
            phip_free(d->ext_obs);
            d->ext_obs = (float*)phip_malloc(sizeof(float) * (size_t)E * S);
            d->ext_obs_cap = (long)E * S;
        }
        phip_d2d(d->ext_obs, d_obs0, sizeof(float) * (size_t)E * S);
        ro_fresh(d, E, PHIP_ENV_EXTERNAL, S);
    }
    ro_carry_swap(d, E);
    /* rows e·T ← the current observations: the synthetic environment's state is its observation, [E, S] */
    phip_env_first_obs(1, d->ext_obs, b->d_state_p, E, T, S);
    d->ext_key = splitmix64(seed ^ 0x524F4C4CULL);
    d->ext_open = 1;
    d->ext_done = d->ext_acted = d->ext_t = 0;
    return 0;
}

/* one act of the open rollout; d_mask [E, W] (NULL: unmasked — the step's rows get full masks while masking is on) */
static long long rollout_act(PPO* ppo, const uint32_t* d_mask, float* d_action) {
    PPODev* d = ppo ? (PPODev*)ppo->dev : NULL;
    if (!d || !d_action || !d->ext_open || d->ext_acted || d->ext_t >= d->ro_T) return -1;
    TrajectoryBuffer* b = ppo->buffer;
    GaussianPolicy* pol = ppo->policy;
    const int E = d->ro_E, S = b->state_size, A = b->action_size;
    const int* rows = d->ro_rows + (long)d->ext_t * E;
    /* as ppo_rollout_device's step: normalise into the shadow, forward μ over the step's rows, sample into them */
    float* shadow = obs_on(d) ? obs_shadow(ppo, d) : NULL;
    if (shadow)
        phip_obs_normalize_rows(b->d_state_p, rows, shadow, rows, E, S, d->obs_m, d->obs_m + S, d->obs_clip,
                                d->obs_run);
    nn_forward_dev_rows(pol->mu, shadow ? shadow : b->d_state_p, rows, NULL, E);
    const uint64_t step = d->ro_step++;
    if (cat_on(d))         /* under the caller's masks, which go to the step's rows of the store in the same launch */
        phip_disc_sample_rows(pol->mu->d_output, d_mask, rows, disc_off(d), b->d_action_p, b->d_logprob_p,
                              d_mask ? d->mask : NULL, E, A, disc_D(d), d->ext_key, step);
    else if (sd_on(d))
        phip_sd_sample_rows(pol->mu->d_output, rows, b->d_action_p, b->d_logprob_p, E, A, d->sd_ls[0], d->sd_ls[1],
                            d->ext_key, step);
    else phip_sample_rows(pol->mu->d_output, pol->d_log_std, rows, b->d_action_p, b->d_logprob_p, E, A, d->ext_key, step);
    if (!d_mask && mask_on(d)) phip_mask_fill_rows(d->mask, rows, E, A);
    phip_action_rows_out(b->d_action_p, rows, d_action, E, A);
    d->ext_acted = 1;
    return (long long)step;
}

long long ppo_rollout_act(void* vppo, float* d_action) { return rollout_act((PPO*)vppo, NULL, d_action); }

long long ppo_rollout_act_masked(void* vppo, const uint32_t* d_mask, float* d_action) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo || !d_mask || !mask_on((const PPODev*)ppo->dev)) return -1;
    return rollout_act(ppo, d_mask, d_action);
}

int ppo_rollout_store(void* vppo, const float* d_reward, const float* d_next_obs, const unsigned char* d_term,
                      const unsigned char* d_trunc, const float* d_obs_after) {
    PPO* ppo = (PPO*)vppo;
    PPODev* d = ppo ? (PPODev*)ppo->dev : NULL;
    if (!d || !d_reward || !d_next_obs || !d_term || !d_trunc || !d->ext_open || !d->ext_acted) return -1;
    TrajectoryBuffer* b = ppo->buffer;
    phip_ext_store(d_next_obs, d_obs_after, d_reward, d_term, d_trunc, b->d_state_p, b->d_next_state_p, b->d_reward_p,
                   (uint8_t*)b->d_terminated_p, (uint8_t*)b->d_truncated_p, d->ro_cont, d->ext_obs, d->ro_E, d->ro_T,
                   d->ext_t, b->state_size);
    d->ext_acted = 0;
    d->ext_t++;
    return 0;
}

int ppo_rollout_end(void* vppo) {
    PPO* ppo = (PPO*)vppo;
    PPODev* d = ppo ? (PPODev*)ppo->dev : NULL;
    if (!d || !d->ext_open || d->ext_acted || d->ext_t != d->ro_T) return -1;
    ro_finish(ppo, d, d->ro_E, d->ro_T);
    d->ext_open = 0;
    d->ext_done = 1;
    return 0;
}

/* ppo_act_device's scratch for m rows (grow-only) */
static void act_ws(PPODev* d, int m, int S) {
    if (m <= d->act_m) return;
    phip_free(d->act_obsn); phip_free(d->act_lp); phip_free(d->act_rows);
    d->act_obsn = (float*)phip_malloc(sizeof(float) * (size_t)m * S);
    d->act_lp = (float*)phip_malloc(sizeof(float) * (size_t)m);
    d->act_rows = (int*)phip_malloc(sizeof(int) * (size_t)m);
    phip_rollout_rows(d->act_rows, m, 1);                        /* rows[i] = i */
    d->act_m = m;
}

/* d_mask [m, W] (NULL: unmasked) */
static int act_device(PPO* ppo, const float* d_obs, const uint32_t* d_mask, int m, int deterministic,
                      unsigned long long seed, unsigned long long step, float* d_action, float* d_log_prob) {
    if (!ppo || !d_obs || !d_action || m <= 0) return -1;
    const int S = ppo->buffer->state_size, A = ppo->buffer->action_size;
    PPODev* d = dev_ws(ppo, 1);
    GaussianPolicy* pol = ppo->policy;
    const int cat = cat_on(d), norm = obs_on(d);
    act_ws(d, m, S);
    /* normalised under the pair as it stands, uncounted, nothing folded (as ppo_eval_device) */
    if (norm) {
        obs_ws(ppo, d);
        phip_obs_normalize_rows(d_obs, NULL, d->act_obsn, NULL, m, S, d->obs_m, d->obs_m + S, d->obs_clip, d->obs_run);
    }
    /* through the row list, as the rollout forwards: the same kernels over the same rows */
    nn_forward_dev_rows(pol->mu, norm ? d->act_obsn : d_obs, d->act_rows, NULL, m);
    const uint64_t key = splitmix64(seed ^ 0x524F4C4CULL);
    float* lp = d_log_prob ? d_log_prob : d->act_lp;
    if (cat && deterministic) phip_disc_argmax(pol->mu->d_output, d_mask, disc_off(d), d_action, m, A, disc_D(d));
    else if (cat)
        phip_disc_sample_rows(pol->mu->d_output, d_mask, d->act_rows, disc_off(d), d_action, lp, NULL, m, A, disc_D(d),
                              key, step);
    else if (sd_on(d) && deterministic) phip_sd_mean(pol->mu->d_output, d_action, m, A);
    else if (sd_on(d))
        phip_sd_sample_rows(pol->mu->d_output, d->act_rows, d_action, lp, m, A, d->sd_ls[0], d->sd_ls[1], key, step);
    else if (deterministic) phip_mean_action(pol->mu->d_output, d_action, (long)m * A);
    else phip_sample_rows(pol->mu->d_output, pol->d_log_std, d->act_rows, d_action, lp, m, A, key, step);
    return 0;
}

int ppo_act_device(void* vppo, const float* d_obs, int m, int deterministic, unsigned long long seed,
                   unsigned long long step, float* d_action, float* d_log_prob) {
    return act_device((PPO*)vppo, d_obs, NULL, m, deterministic, seed, step, d_action, d_log_prob);
}

int ppo_act_device_masked(void* vppo, const float* d_obs, const uint32_t* d_mask, int m, int deterministic,
                          unsigned long long seed, unsigned long long step, float* d_action, float* d_log_prob) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo || !d_mask || !mask_on((const PPODev*)ppo->dev)) return -1;
    return act_device(ppo, d_obs, d_mask, m, deterministic, seed, step, d_action, d_log_prob);
}

/* ------------------------------------------------------------------ */
/* the built-in environments on dense arrays (ppo_ext.h)               */
/* ------------------------------------------------------------------ */
int ppo_env_state_floats(int env_kind, int S) {
    if (env_kind == 0) return S == 3 ? 3 : -1;
    if (env_kind == 1) return S > 0 ? S : -1;
    if (env_kind == 2) return S == 4 ? 5 : -1;
    return -1;
}

int ppo_env_reset_device(int env_kind, float* d_env_state, float* d_obs, int E, int S, unsigned long long seed) {
    if (ppo_env_state_floats(env_kind, S) < 0 || !d_env_state || !d_obs || E <= 0) return -1;
    phip_env_reset(env_kind, d_env_state, d_obs, E, 1, S, splitmix64(seed));
    phip_env_first_obs(env_kind, d_env_state, d_obs, E, 1, S);   /* T = 1: row e of the dense array */
    return 0;
}

int ppo_env_step_device(int env_kind, float* d_env_state, const float* d_action, float* d_next_obs, float* d_obs_after,
                        float* d_reward, unsigned char* d_term, unsigned char* d_trunc, int E, int S, int A,
                        int categorical, unsigned long long seed, unsigned long long step) {
    if (ppo_env_state_floats(env_kind, S) < 0 || E <= 0 || A <= 0) return -1;
    if (!d_env_state || !d_action || !d_next_obs || !d_obs_after || !d_reward || !d_term || !d_trunc) return -1;
    if (env_kind == 0 && A != 1) return -1;
    if (env_kind == 2 && (A != 2 || !categorical)) return -1;
    if (env_kind == 1 && categorical && A < 2) return -1;
    phip_env_step_dense(env_kind, d_env_state, d_action, d_next_obs, d_obs_after, d_reward, d_term, d_trunc, E,
                        (uint64_t)step, S, A, splitmix64(seed ^ 0x524F4C4CULL), categorical != 0);
    return 0;
}

/* ------------------------------------------------------------------ */
/* checkpoint (ppo.cu:585-648 byte layout)                             */
/* ------------------------------------------------------------------ */
/* the byte stream itself, into an open file: save_ppo's body, and the legacy section of a training-state
 * checkpoint (checkpoint.c) */
void save_ppo_file(PPO* ppo, FILE* f) {
    policy_to_host(ppo->policy);
    nn_write_weights_to_host(ppo->V);
    fwrite(&ppo->lambda, sizeof(float), 1, f);
    fwrite(&ppo->epsilon, sizeof(float), 1, f);
    fwrite(&ppo->ent_coeff, sizeof(float), 1, f);
    fwrite(&ppo->lr_policy, sizeof(float), 1, f);
    fwrite(&ppo->lr_V, sizeof(float), 1, f);
    fwrite(&ppo->buffer->state_size, sizeof(int), 1, f);
    fwrite(&ppo->buffer->action_size, sizeof(int), 1, f);
    fwrite(&ppo->buffer->capacity, sizeof(int), 1, f);
    save_policy(ppo->policy, f);
    save_neural_network(ppo->V, f);
    save_adam(ppo->adam_policy, f, true);
    save_adam(ppo->adam_V, f, true);
    save_adam(ppo->adam_entropy, f, true);
}

void save_ppo(PPO* ppo, const char* filename) {
    FILE* f = fopen(filename, "wb");
    if (!f) die("save_ppo: cannot open file");
    save_ppo_file(ppo, f);
    fclose(f);
}

PPO* load_ppo_file(FILE* f, bool use_cuda) {
    PPO* ppo = (PPO*)xcalloc(1, sizeof(PPO));
    ppo->use_cuda = use_cuda;
    int S, A, cap;
    if (fread(&ppo->lambda, sizeof(float), 1, f) != 1 || fread(&ppo->epsilon, sizeof(float), 1, f) != 1 ||
        fread(&ppo->ent_coeff, sizeof(float), 1, f) != 1 || fread(&ppo->lr_policy, sizeof(float), 1, f) != 1 ||
        fread(&ppo->lr_V, sizeof(float), 1, f) != 1 || fread(&S, sizeof(int), 1, f) != 1 ||
        fread(&A, sizeof(int), 1, f) != 1 || fread(&cap, sizeof(int), 1, f) != 1)
        die("load_ppo: unexpected end of file");
    if (S <= 0 || A <= 0 || cap < 0) die("load_ppo: bad header");
    ppo->buffer = create_trajectory_buffer(cap, S, A);
    ppo->policy = load_policy(f, S, A);
    ppo->V = load_neural_network(f);
    if (ppo->policy->mu->layers[0].input_size != S || ppo->policy->mu->output_size != A ||
        ppo->V->layers[0].input_size != S || ppo->V->output_size != 1)
        die("load_ppo: network shapes do not match the header");
    /* optimiser state always lives in HBM (use_cuda is kept for the ABI; both values run the HIP
     * path), so the moments are loaded as device Adams whatever use_cuda says */
    ppo->adam_policy = load_adam_from_nn(f, ppo->policy->mu, true);
    ppo->adam_V = load_adam_from_nn(f, ppo->V, true);
    ppo->adam_entropy = load_adam_ex(f, &ppo->policy->d_log_std, &ppo->policy->d_log_std_grad, &A, 1, true);
    return ppo;
}

PPO* load_ppo(const char* filename, bool use_cuda) {
    FILE* f = fopen(filename, "rb");
    if (!f) die("load_ppo: cannot open file");
    PPO* ppo = load_ppo_file(f, use_cuda);
    fclose(f);
    return ppo;
}

/* ppo_ext.h: compute precision of both networks (bf16 MFMA for config C5) */
int ppo_set_compute_dtype(void* vppo, int dtype) {
    PPO* ppo = (PPO*)vppo;
    if (!ppo) return -1;
    /* bf16 mode knows ReLU and identity: a tanh layer in either network declines it, both left as they were */
    if (dtype == 1 && (nn_has_tanh(ppo->V) || nn_has_tanh(ppo->policy->mu))) return -1;
    /* … and the categorical head reads fp32 logits: bf16 mode is declined while it is on */
    if (dtype == 1 && (cat_on((PPODev*)ppo->dev) || sd_on((PPODev*)ppo->dev))) return -1;
    if (nn_set_compute_dtype(ppo->V, dtype) != 0) return -1;
    return nn_set_compute_dtype(ppo->policy->mu, dtype);
}
