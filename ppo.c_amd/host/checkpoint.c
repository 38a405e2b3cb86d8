/*
 * checkpoint.c — full training-state checkpoints (ppo_ext.h ppo_save_state / ppo_load_state / ppo_state_hash /
 * ppo_state_image; DESIGN.md §4 "Training-state checkpoints").
 *
 * This file captures a PPO into an image (D2H copies between updates, no kernel) and builds a PPO from one.
 * Indexing and validating an image is checkpoint_index.c — libc alone, no HIP call, no die(), compiled on its own
 * for the CPU tests — and ppo_load_state runs it over the whole file first and touches the device only afterwards,
 * so a damaged file is declined before anything is allocated.
 *
 * The image is little-endian and a pure function of the state: every gap is written as zero.
 */
#include "checkpoint.h"
#include "ppo_dev.h"

#include <math.h>

/* a growable byte string; every put is little-endian (arrays are copied as the host holds them: libppo's hosts
 * are little-endian) */
typedef struct {
    uint8_t* p;
    size_t n, cap;
} Bytes;

static uint8_t* bytes_grow(Bytes* b, size_t more) {
    if (b->n + more > b->cap) {
        size_t cap = b->cap ? b->cap : 256;
        while (cap < b->n + more) cap *= 2;
        uint8_t* p = (uint8_t*)realloc(b->p, cap);
        if (!p) die("checkpoint: out of memory");
        b->p = p;
        b->cap = cap;
    }
    uint8_t* at = b->p + b->n;
    memset(at, 0, more);
    b->n += more;
    return at;
}

static void put_mem(Bytes* b, const void* src, size_t n) {
    if (n) memcpy(bytes_grow(b, n), src, n);
}
static void put_u32(Bytes* b, uint32_t v) {
    uint8_t* p = bytes_grow(b, 4);
    for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}
static void put_u64(Bytes* b, uint64_t v) {
    put_u32(b, (uint32_t)v);
    put_u32(b, (uint32_t)(v >> 32));
}
static void put_f32(Bytes* b, float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    put_u32(b, u);
}
static void put_pad(Bytes* b, size_t to) {
    if (b->n % to) bytes_grow(b, to - b->n % to);
}
/* n bytes of device memory (NULL: zeros) */
static void put_dev(Bytes* b, const void* d_src, size_t n) {
    if (!n) return;
    uint8_t* at = bytes_grow(b, n);
    if (d_src) phip_d2h(at, d_src, n);
}
/* n bytes from wherever the trajectory buffer currently points */
static void put_rows(Bytes* b, const TrajectoryBuffer* tb, const void* src, size_t n) {
    if (tb->on_device) put_dev(b, src, n);
    else put_mem(b, src, n);
}

static void put_section(Bytes* img, uint32_t tag, const Bytes* payload) {
    put_u32(img, tag);
    put_u32(img, 0);
    put_u64(img, (uint64_t)payload->n);
    put_u64(img, ckpt_fnv1a64(payload->p, payload->n));
    put_mem(img, payload->p, payload->n);
    if (payload->n % 8) bytes_grow(img, 8 - payload->n % 8);     /* the payload padded to 8 bytes, with zeros */
}

static int buffer_limit(const TrajectoryBuffer* b) { return b->full ? b->capacity : b->idx; }

/* the image of `ppo` under the caller's flags, or −1 (nothing allocated) for a NULL ppo or an open rollout */
static int build_image(PPO* ppo, int flags, Bytes* img) {
    memset(img, 0, sizeof(*img));
    if (!ppo) return -1;
    PPODev* d = ppo_dev(ppo);
    if (d->ext_open) return -1;                     /* partly laid rows are not a state worth keeping */
    phip_sync();
    const TrajectoryBuffer* tb = ppo->buffer;
    const size_t S = (size_t)tb->state_size, A = (size_t)tb->action_size;
    const int with_buffer = (flags & PPO_CKPT_BUFFER) != 0;
    const int with_rollout = d->ro_cont != NULL && d->ro_E > 0;
    /* a schedule other than the constant one: with it off the image is what it always was, byte for byte */
    const int with_lr = d->lr_kind != PPO_LR_CONSTANT;
    /* … and an advantage-normalisation mode other than the global one, likewise */
    const int with_adv = d->adv_norm_mode != PPO_ADV_NORM_GLOBAL;
    /* … and a KL estimator other than k3, likewise */
    const int with_klest = d->kl_est != PPO_KL_K3;
    /* … and the state-dependent-σ Gaussian, likewise: its section exists only while the distribution is 3 */
    const int with_sd = d->action_dist == 3;
    Bytes s;

    put_mem(img, CKPT_MAGIC, 8);
    put_u32(img, CKPT_VERSION);
    put_u32(img, (with_buffer ? CKPT_F_BUFFER : 0u) | (with_rollout ? CKPT_F_ROLLOUT : 0u) |
                     (with_lr ? CKPT_F_LRSCHED : 0u) | (with_adv ? CKPT_F_ADVNORM : 0u) |
                     (with_klest ? CKPT_F_KLEST : 0u) | (with_sd ? CKPT_F_GAUSS_SD : 0u));
    put_u32(img, 4u + (uint32_t)with_rollout + (uint32_t)with_buffer + (uint32_t)with_lr + (uint32_t)with_adv +
                     (uint32_t)with_klest + (uint32_t)with_sd);

    /* Legacy: save_ppo's byte stream */
    {
        char* mem = NULL;
        size_t n = 0;
        FILE* f = open_memstream(&mem, &n);
        if (!f) die("checkpoint: open_memstream failed");
        save_ppo_file(ppo, f);
        if (fclose(f) != 0) die("checkpoint: writing the legacy section failed");
        const Bytes legacy = {(uint8_t*)mem, n, n};
        put_section(img, CKPT_TAG_LEGACY, &legacy);
        free(mem);
    }

    /* Settings */
    memset(&s, 0, sizeof(s));
    put_f32(&s, d->max_grad_norm);
    put_f32(&s, d->target_kl);
    put_f32(&s, d->value_clip);
    put_f32(&s, d->obs_clip);
    put_u32(&s, (uint32_t)(d->obs_frozen != 0));
    put_f32(&s, d->rew_clip);
    put_u32(&s, (uint32_t)(d->rew_frozen != 0));
    put_f32(&s, d->ep_gamma);
    put_u32(&s, (uint32_t)d->action_dist);
    const int D = d->action_dist == 2 ? d->md_D : 0;
    put_u32(&s, (uint32_t)D);
    for (int i = 0; i < D; i++) put_u32(&s, (uint32_t)d->md_nvec[i]);
    put_u32(&s, (uint32_t)(ppo_get_action_mask(ppo) != 0));
    put_u32(&s, (uint32_t)(ppo->V->dtype != 0));
    put_u32(&s, (uint32_t)(ppo->policy->mu->dtype != 0));
    put_section(img, CKPT_TAG_SETTINGS, &s);
    free(s.p);

    /* Normalisers */
    memset(&s, 0, sizeof(s));
    if (d->obs_run) put_dev(&s, d->obs_run, sizeof(double) * (1 + 2 * S));
    put_dev(&s, d->rew_run, 3 * sizeof(double));
    put_section(img, CKPT_TAG_NORMALISERS, &s);
    free(s.p);

    /* Shuffle */
    memset(&s, 0, sizeof(s));
    put_u64(&s, d->key);
    put_u64(&s, d->seed);
    put_u32(&s, (uint32_t)(d->seeded != 0));
    put_section(img, CKPT_TAG_SHUFFLE, &s);
    free(s.p);

    if (with_rollout) {
        const size_t E = (size_t)d->ro_E;
        const int external = d->ro_kind == PHIP_ENV_EXTERNAL;
        const int ext_done = external && d->ext_done && d->ext_obs;
        memset(&s, 0, sizeof(s));
        put_u32(&s, (uint32_t)d->ro_E);
        put_u32(&s, (uint32_t)d->ro_T);
        put_u32(&s, (uint32_t)d->ro_kind);
        put_u32(&s, (uint32_t)d->ro_S);
        put_u64(&s, d->ro_step);
        put_u32(&s, (uint32_t)(with_buffer && d->ro_laid));      /* without the rows nothing is laid */
        put_u32(&s, (uint32_t)(d->rew_scanned != 0));
        if (!external) put_dev(&s, d->env_state, sizeof(float) * E * (size_t)PHIP_ENV_STATE(d->ro_S));
        put_pad(&s, 8);
        put_dev(&s, d->ro_cont, E);
        put_pad(&s, 8);
        put_dev(&s, d->rew_carry_in, sizeof(double) * E);
        put_dev(&s, d->rew_carry_out, sizeof(double) * E);
        put_u32(&s, (uint32_t)(d->ep_fresh != 0));
        put_u32(&s, (uint32_t)ext_done);
        put_dev(&s, d->ep_state, 4 * sizeof(double) * E);
        put_dev(&s, d->ep_agg, 16 * sizeof(double));
        put_u64(&s, ext_done ? d->ext_key : 0);
        if (ext_done) put_dev(&s, d->ext_obs, sizeof(float) * E * S);
        put_section(img, CKPT_TAG_ROLLOUT, &s);
        free(s.p);
    }

    if (with_buffer) {
        const size_t n = (size_t)buffer_limit(tb);
        const size_t W = ppo_get_action_mask(ppo) ? (size_t)ppo_action_mask_words(ppo) : 0;
        memset(&s, 0, sizeof(s));
        put_u32(&s, (uint32_t)tb->idx);
        put_u32(&s, (uint32_t)(tb->full != 0));
        put_u32(&s, (uint32_t)n);
        put_u32(&s, (uint32_t)W);
        put_rows(&s, tb, tb->state_p, sizeof(float) * n * S);
        put_rows(&s, tb, tb->action_p, sizeof(float) * n * A);
        put_rows(&s, tb, tb->logprob_p, sizeof(float) * n);
        put_rows(&s, tb, tb->reward_p, sizeof(float) * n);
        put_rows(&s, tb, tb->next_state_p, sizeof(float) * n * S);
        put_rows(&s, tb, tb->terminated_p, n);
        put_rows(&s, tb, tb->truncated_p, n);
        put_pad(&s, 4);
        if (W) put_dev(&s, d->mask, sizeof(uint32_t) * n * W);
        put_section(img, CKPT_TAG_BUFFER, &s);
        free(s.p);
    }

    if (with_lr) {
        const int adaptive = d->lr_kind == PPO_LR_ADAPTIVE;
        memset(&s, 0, sizeof(s));
        put_u32(&s, (uint32_t)d->lr_kind);
        for (int i = 0; i < 3; i++) put_f32(&s, d->lr_p[i]);
        put_u32(&s, (uint32_t)(d->lr_couple != 0));
        put_u32(&s, 0);
        put_u64(&s, d->lr_u);
        put_dev(&s, adaptive ? &d->kl->lr : NULL, 2 * sizeof(float));               /* lr, lr_v */
        put_dev(&s, adaptive ? &d->kl->lr_raised : NULL, 2 * sizeof(unsigned));     /* raised, lowered */
        put_section(img, CKPT_TAG_LRSCHED, &s);
        free(s.p);
    }

    if (with_adv) {
        memset(&s, 0, sizeof(s));
        put_u32(&s, (uint32_t)d->adv_norm_mode);
        put_u32(&s, 0);
        put_section(img, CKPT_TAG_ADVNORM, &s);
        free(s.p);
    }

    if (with_klest) {
        memset(&s, 0, sizeof(s));
        put_u32(&s, (uint32_t)d->kl_est);
        put_u32(&s, 0);
        put_section(img, CKPT_TAG_KLEST, &s);
        free(s.p);
    }

    if (with_sd) {
        memset(&s, 0, sizeof(s));
        put_u32(&s, 1);
        put_u32(&s, 0);
        put_f32(&s, d->sd_ls[0]);
        put_f32(&s, d->sd_ls[1]);
        put_section(img, CKPT_TAG_GAUSS_SD, &s);
        free(s.p);
    }
    return 0;
}

int ppo_state_image(void* vppo, int flags, void* out, long cap) {
    Bytes img;
    if (build_image((PPO*)vppo, flags, &img) != 0) return -1;
    const long n = (long)img.n;
    int r = (int)n;
    if (out) {
        if (cap < n) r = -1;
        else memcpy(out, img.p, img.n);
    }
    free(img.p);
    return r;
}

unsigned long long ppo_state_hash(void* vppo, int flags) {
    Bytes img;
    if (build_image((PPO*)vppo, flags, &img) != 0) return 0;
    const uint64_t h = ckpt_fnv1a64(img.p, img.n);
    free(img.p);
    return h;
}

int ppo_save_state(void* vppo, const char* path, int flags) {
    if (!vppo || !path) return -1;
    if (ppo_dev((PPO*)vppo)->ext_open) return -1;                /* declined before any file is created */
    const size_t plen = strlen(path);
    char* tmp = (char*)xmalloc(plen + 5);
    memcpy(tmp, path, plen);
    memcpy(tmp + plen, ".tmp", 5);
    /* the path is tried first: nothing is captured for a file that cannot be written */
    FILE* f = fopen(tmp, "wb");
    if (!f) {
        free(tmp);
        return -1;
    }
    Bytes img;
    int ok = build_image((PPO*)vppo, flags, &img) == 0;
    if (ok) ok = fwrite(img.p, 1, img.n, f) == img.n;
    if (fclose(f) != 0) ok = 0;
    if (ok) ok = rename(tmp, path) == 0;
    if (!ok) remove(tmp);
    free(img.p);
    free(tmp);
    return ok ? 0 : -1;
}

/* ---- load ---- */
static float get_f32(const uint8_t* p) {
    const uint32_t u = ckpt_rd32(p);
    float v;
    memcpy(&v, &u, 4);
    return v;
}

static void* set_err(char* err, int err_cap, const char* msg) {
    if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "ppo_load_state: %s", msg);
    return NULL;
}

/* device memory of n bytes holding src */
static void* dev_from(const uint8_t* src, size_t n) {
    void* p = phip_malloc(n ? n : 1);
    if (n) phip_h2d(p, src, n);
    return p;
}

/* the sections behind Legacy onto a PPO built from it; NULL, or what was declined */
static const char* apply_sections(PPO* ppo, const uint8_t* img, const CkptIndex* ix) {
    PPODev* d = ppo_dev(ppo);
    TrajectoryBuffer* tb = ppo->buffer;
    const size_t S = (size_t)ix->S, A = (size_t)ix->A;

    /* Settings, through the setters, in an order they accept: the distribution before the mask, the dtype last */
    const uint8_t* st = img + ix->sec[CKPT_TAG_SETTINGS].off;
    const uint8_t* tail = st + 40 + 4 * (size_t)ix->md_D;
    if (ppo_set_max_grad_norm(ppo, get_f32(st)) != 0 || ppo_set_target_kl(ppo, get_f32(st + 4)) != 0 ||
        ppo_set_value_clip(ppo, get_f32(st + 8)) != 0 || ppo_set_obs_norm(ppo, get_f32(st + 12)) != 0 ||
        ppo_set_reward_norm(ppo, get_f32(st + 20)) != 0)
        return "a setting the setter declines (NaN)";
    ppo_obs_norm_freeze(ppo, (int)ckpt_rd32(st + 16));
    ppo_reward_norm_freeze(ppo, (int)ckpt_rd32(st + 24));
    const float ep_gamma = get_f32(st + 28);
    if (!(ep_gamma >= 0.f && ep_gamma <= 1.f)) return "an episode discount outside [0, 1]";
    ppo_episode_gamma(ppo, ep_gamma);
    if (ix->action_dist == 2) {
        int nvec[CKPT_MD_MAX_D];
        for (int i = 0; i < ix->md_D; i++) nvec[i] = (int)ckpt_rd32(st + 40 + 4 * (size_t)i);
        if (ppo_set_action_multidiscrete(ppo, nvec, ix->md_D) != 0) return "an nvec ppo_set_action_multidiscrete declines";
    } else if (ix->action_dist == 3) {
        if (ppo_set_action_gaussian_sd(ppo, ix->sd_ls[0], ix->sd_ls[1]) != 0)
            return "bounds or an action size ppo_set_action_gaussian_sd declines";
    } else if (ppo_set_action_dist(ppo, ix->action_dist) != 0) {
        return "an action distribution ppo_set_action_dist declines";
    }
    if (ix->mask_on && ppo_set_action_mask(ppo, 1) != 0) return "a mask ppo_set_action_mask declines";
    const int dt_v = (int)ckpt_rd32(tail + 4), dt_mu = (int)ckpt_rd32(tail + 8);
    if ((dt_v != ppo->V->dtype && nn_set_compute_dtype(ppo->V, dt_v) != 0) ||
        (dt_mu != ppo->policy->mu->dtype && nn_set_compute_dtype(ppo->policy->mu, dt_mu) != 0))
        return "a compute dtype the networks decline";

    /* Normalisers: the triples, the fp32 pair and scale refreshed as _set_state does */
    const uint8_t* nm = img + ix->sec[CKPT_TAG_NORMALISERS].off;
    if (ix->has_obs) {
        const long n = 1 + 2 * (long)S;
        double* t = (double*)xmalloc(sizeof(double) * (size_t)n);
        memcpy(t, nm, sizeof(double) * (size_t)n);
        const int r = ppo_obs_norm_set_state(ppo, t, n);
        free(t);
        if (r != 0) return "an observation triple ppo_obs_norm_set_state declines";
        nm += sizeof(double) * (size_t)n;
    }
    double rew[3];
    memcpy(rew, nm, sizeof(rew));
    if (ppo_reward_norm_set_state(ppo, rew) != 0) return "a reward triple ppo_reward_norm_set_state declines";

    /* Shuffle */
    const uint8_t* sh = img + ix->sec[CKPT_TAG_SHUFFLE].off;
    d->key = ckpt_rd64(sh);
    d->seed = ckpt_rd64(sh + 8);
    d->seeded = (int)ckpt_rd32(sh + 16);

    if (ix->sec[CKPT_TAG_ROLLOUT].present) {
        const uint8_t* ro = img + ix->sec[CKPT_TAG_ROLLOUT].off;
        const int E = (int)ckpt_rd32(ro), T = (int)ckpt_rd32(ro + 4), kind = (int)ckpt_rd32(ro + 8);
        const size_t nE = (size_t)E;
        ppo_dev_ro_rows(d, E, T);
        d->ro_E = E;
        d->ro_kind = kind;
        d->ro_S = (int)S;
        d->ro_step = ckpt_rd64(ro + 16);
        d->ro_laid = (int)ckpt_rd32(ro + 24);
        d->rew_scanned = (int)ckpt_rd32(ro + 28);
        const uint8_t* p = ro + CKPT_ROLLOUT_FIXED;
        const size_t env = sizeof(float) * nE * (size_t)PHIP_ENV_STATE((int)S);
        if (kind != PHIP_ENV_EXTERNAL) {
            d->env_state = (float*)dev_from(p, env);
            p += (env + 7) & ~(size_t)7;
        }
        d->ro_cont = (unsigned char*)dev_from(p, nE);
        p += (nE + 7) & ~(size_t)7;
        d->rew_carry_in = (double*)dev_from(p, sizeof(double) * nE);
        p += sizeof(double) * nE;
        d->rew_carry_out = (double*)dev_from(p, sizeof(double) * nE);
        p += sizeof(double) * nE;
        d->ep_fresh = (int)ckpt_rd32(p);
        d->ext_done = (int)ckpt_rd32(p + 4);
        p += 8;
        d->ep_state = (double*)dev_from(p, 4 * sizeof(double) * nE);
        p += 4 * sizeof(double) * nE;
        d->ep_agg = (double*)dev_from(p, 16 * sizeof(double));
        p += 16 * sizeof(double);
        d->ext_key = ckpt_rd64(p);
        p += 8;
        if (d->ext_done) {
            d->ext_obs = (float*)dev_from(p, sizeof(float) * nE * S);
            d->ext_obs_cap = (long)(nE * S);
        }
    }

    if (ix->sec[CKPT_TAG_BUFFER].present) {
        const uint8_t* bf = img + ix->sec[CKPT_TAG_BUFFER].off;
        const size_t n = (size_t)ckpt_rd32(bf + 8), W = (size_t)ckpt_rd32(bf + 12);
        const uint8_t* p = bf + CKPT_BUFFER_FIXED;
        tb->idx = (int)ckpt_rd32(bf);
        tb->full = ckpt_rd32(bf + 4) != 0;
        if (n) {
            phip_h2d(tb->d_state_p, p, sizeof(float) * n * S);
            p += sizeof(float) * n * S;
            phip_h2d(tb->d_action_p, p, sizeof(float) * n * A);
            p += sizeof(float) * n * A;
            phip_h2d(tb->d_logprob_p, p, sizeof(float) * n);
            p += sizeof(float) * n;
            phip_h2d(tb->d_reward_p, p, sizeof(float) * n);
            p += sizeof(float) * n;
            phip_h2d(tb->d_next_state_p, p, sizeof(float) * n * S);
            p += sizeof(float) * n * S;
            phip_h2d(tb->d_terminated_p, p, n);
            p += n;
            phip_h2d(tb->d_truncated_p, p, n);
            p += n;
            p += (4 - (2 * n) % 4) % 4;
            if (W) phip_h2d(ppo_action_mask_buffer(ppo), p, sizeof(uint32_t) * n * W);
        }
        buffer_point_device(tb);
    }

    /* the learning-rate schedule through its setter, then the state the setter restarted */
    if (ix->sec[CKPT_TAG_LRSCHED].present) {
        const uint8_t* lr = img + ix->sec[CKPT_TAG_LRSCHED].off;
        const int kind = (int)ckpt_rd32(lr);
        if (ppo_set_lr_schedule(ppo, kind, get_f32(lr + 4), get_f32(lr + 8), get_f32(lr + 12)) != 0)
            return "a learning-rate schedule ppo_set_lr_schedule declines";
        ppo_lr_couple_value(ppo, (int)ckpt_rd32(lr + 16));
        d->lr_u = ckpt_rd64(lr + 24);
        if (kind == PPO_LR_ADAPTIVE) {
            phip_h2d(&d->kl->lr, lr + 32, 2 * sizeof(float));
            phip_h2d(&d->kl->lr_raised, lr + 40, 2 * sizeof(unsigned));
        }
    }

    /* the advantage-normalisation mode through its setter */
    if (ix->sec[CKPT_TAG_ADVNORM].present &&
        ppo_set_adv_norm(ppo, (int)ckpt_rd32(img + ix->sec[CKPT_TAG_ADVNORM].off)) != 0)
        return "an advantage-normalisation mode ppo_set_adv_norm declines";
    /* the KL monitor's estimator through its setter */
    if (ix->sec[CKPT_TAG_KLEST].present &&
        ppo_set_kl_estimator(ppo, (int)ckpt_rd32(img + ix->sec[CKPT_TAG_KLEST].off)) != 0)
        return "a KL estimator ppo_set_kl_estimator declines";
    phip_sync();
    return NULL;
}

void* ppo_load_state(const char* path, char* err, int err_cap) {
    if (err && err_cap > 0) err[0] = 0;
    if (!path) return set_err(err, err_cap, "NULL path");
    FILE* f = fopen(path, "rb");
    if (!f) return set_err(err, err_cap, "cannot open the file");
    uint8_t* img = NULL;
    long len = -1;
    if (fseek(f, 0, SEEK_END) == 0) len = ftell(f);
    if (len >= 0 && fseek(f, 0, SEEK_SET) == 0) {
        img = (uint8_t*)malloc(len > 0 ? (size_t)len : 1);
        if (img && fread(img, 1, (size_t)len, f) != (size_t)len) {
            free(img);
            img = NULL;
        }
    }
    fclose(f);
    if (!img) return set_err(err, err_cap, "cannot read the file");
    /* validate first, allocate after: nothing below the index touches the device */
    CkptIndex ix;
    if (ckpt_index(img, (size_t)len, &ix) != 0) {
        free(img);
        return set_err(err, err_cap, ix.err);
    }
    FILE* lf = fmemopen(img + ix.sec[CKPT_TAG_LEGACY].off, (size_t)ix.sec[CKPT_TAG_LEGACY].len, "rb");
    if (!lf) {
        free(img);
        return set_err(err, err_cap, "cannot open the legacy section");
    }
    PPO* ppo = load_ppo_file(lf, true);
    fclose(lf);
    const char* what = apply_sections(ppo, img, &ix);
    free(img);
    if (what) {
        free_ppo(ppo);
        return set_err(err, err_cap, what);
    }
    return ppo;
}
