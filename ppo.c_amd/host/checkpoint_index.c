/*
 * checkpoint_index.c — the container of a training-state checkpoint (DESIGN.md §4 "Training-state checkpoints"):
 * indexing and validating an image in memory.  libc alone — no HIP call, no die(), nothing of libppo — so this file
 * compiles on its own for the CPU (tests/test_checkpoint_cpu.py runs it under sanitizers); checkpoint.c holds the
 * half that captures a PPO into an image and builds one from it, and calls ckpt_index before it touches the device.
 */
#include "checkpoint.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

/* ------------------------------------------------------------------ */
/* part 1: the container — index and validate                          */
/* ------------------------------------------------------------------ */
uint32_t ckpt_rd32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

uint64_t ckpt_rd64(const uint8_t* p) { return (uint64_t)ckpt_rd32(p) | ((uint64_t)ckpt_rd32(p + 4) << 32); }

uint64_t ckpt_fnv1a64(const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    uint64_t h = 0xcbf29ce484222325ULL;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ULL;
    return h;
}

static uint64_t pad8(uint64_t n) { return (n + 7) & ~(uint64_t)7; }

static int fail(CkptIndex* ix, const char* msg) {
    snprintf(ix->err, sizeof(ix->err), "%s", msg);
    return -1;
}

static int fail_tag(CkptIndex* ix, const char* what, uint32_t tag) {
    snprintf(ix->err, sizeof(ix->err), "section %u: %s", (unsigned)tag, what);
    return -1;
}

static int is01(uint32_t v) { return v <= 1u; }

static float rd_f32(const uint8_t* p) {
    const uint32_t u = ckpt_rd32(p);
    float v;
    memcpy(&v, &u, 4);
    return v;
}

/* every known section's length and fields against the shapes of the legacy header (all sizes in uint64: S and A
 * are bounded below so that no product can wrap) */
static int check_sections(const uint8_t* img, CkptIndex* ix) {
    const CkptSection* s = ix->sec;
    for (int t = CKPT_TAG_LEGACY; t <= CKPT_TAG_SHUFFLE; t++)
        if (!s[t].present) return fail_tag(ix, "a required section is missing", (uint32_t)t);
    if (((ix->flags & CKPT_F_BUFFER) != 0) != (s[CKPT_TAG_BUFFER].present != 0))
        return fail(ix, "the header's buffer flag and the Buffer section disagree");
    if (((ix->flags & CKPT_F_ROLLOUT) != 0) != (s[CKPT_TAG_ROLLOUT].present != 0))
        return fail(ix, "the header's rollout flag and the Rollout section disagree");
    if (((ix->flags & CKPT_F_LRSCHED) != 0) != (s[CKPT_TAG_LRSCHED].present != 0))
        return fail(ix, "the header's schedule flag and the learning-rate schedule section disagree");
    if (((ix->flags & CKPT_F_KLEST) != 0) != (s[CKPT_TAG_KLEST].present != 0))
        return fail(ix, "header flags and the KL-estimator section disagree");
    if (((ix->flags & CKPT_F_ADVNORM) != 0) != (s[CKPT_TAG_ADVNORM].present != 0))
        return fail(ix, "the header's advantage-normalisation flag and its section disagree");
    if (((ix->flags & CKPT_F_GAUSS_SD) != 0) != (s[CKPT_TAG_GAUSS_SD].present != 0))
        return fail(ix, "the header's state-dependent-sigma flag and its section disagree");

    /* Legacy: five floats, then state size, action size, capacity */
    if (s[CKPT_TAG_LEGACY].len < 32) return fail_tag(ix, "shorter than the legacy header", CKPT_TAG_LEGACY);
    const uint8_t* lg = img + s[CKPT_TAG_LEGACY].off;
    const uint32_t S = ckpt_rd32(lg + 20), A = ckpt_rd32(lg + 24), cap = ckpt_rd32(lg + 28);
    if (S == 0 || S > (1u << 24) || A == 0 || A > (1u << 24) || cap > 0x7fffffffu)
        return fail_tag(ix, "bad shapes in the legacy header", CKPT_TAG_LEGACY);
    ix->S = (int)S;
    ix->A = (int)A;
    ix->cap = (int)cap;

    /* Settings: 10 words, nvec[D], 3 words */
    if (s[CKPT_TAG_SETTINGS].len < CKPT_SETTINGS_FIXED) return fail_tag(ix, "too short", CKPT_TAG_SETTINGS);
    const uint8_t* st = img + s[CKPT_TAG_SETTINGS].off;
    const uint32_t dist = ckpt_rd32(st + 32), D = ckpt_rd32(st + 36);
    if (dist > 3u || D > (uint32_t)CKPT_MD_MAX_D || (D != 0) != (dist == 2u))
        return fail_tag(ix, "bad action distribution or component count", CKPT_TAG_SETTINGS);
    if (s[CKPT_TAG_SETTINGS].len != CKPT_SETTINGS_FIXED + 4ull * D)
        return fail_tag(ix, "length contradicts its component count", CKPT_TAG_SETTINGS);
    const uint8_t* tail = st + 40 + 4u * D;
    const uint32_t mask_on = ckpt_rd32(tail);
    if (!is01(ckpt_rd32(st + 16)) || !is01(ckpt_rd32(st + 24)) || !is01(mask_on) || (mask_on && (dist == 0 || dist == 3)) ||
        !is01(ckpt_rd32(tail + 4)) || !is01(ckpt_rd32(tail + 8)))
        return fail_tag(ix, "a flag or dtype out of range", CKPT_TAG_SETTINGS);
    ix->action_dist = (int)dist;
    ix->md_D = (int)D;
    ix->mask_on = (int)mask_on;

    /* Normalisers: [the observation triple, 1 + 2S doubles] the reward triple, 3 doubles */
    const uint64_t nlen = s[CKPT_TAG_NORMALISERS].len;
    if (nlen == 24) ix->has_obs = 0;
    else if (nlen == 24 + 8ull * (1 + 2ull * S)) ix->has_obs = 1;
    else return fail_tag(ix, "length contradicts the state size (the observation triple is 1 + 2S doubles)",
                         CKPT_TAG_NORMALISERS);

    /* Shuffle: key, seed, seeded */
    if (s[CKPT_TAG_SHUFFLE].len != 20) return fail_tag(ix, "bad length", CKPT_TAG_SHUFFLE);
    if (!is01(ckpt_rd32(img + s[CKPT_TAG_SHUFFLE].off + 16))) return fail_tag(ix, "bad flag", CKPT_TAG_SHUFFLE);

    if (s[CKPT_TAG_ROLLOUT].present) {
        if (s[CKPT_TAG_ROLLOUT].len < CKPT_ROLLOUT_FIXED) return fail_tag(ix, "too short", CKPT_TAG_ROLLOUT);
        const uint8_t* ro = img + s[CKPT_TAG_ROLLOUT].off;
        const uint64_t E = ckpt_rd32(ro), T = ckpt_rd32(ro + 4);
        const uint32_t kind = ckpt_rd32(ro + 8), roS = ckpt_rd32(ro + 12), laid = ckpt_rd32(ro + 24);
        if (E == 0 || E > 0x7fffffffu || T == 0 || T > 0x7fffffffu || E * T > cap || kind > (uint32_t)CKPT_ENV_EXTERNAL ||
            roS != S || !is01(laid) || !is01(ckpt_rd32(ro + 28)))
            return fail_tag(ix, "shapes contradict the legacy header", CKPT_TAG_ROLLOUT);
        if (laid && !(ix->flags & CKPT_F_BUFFER)) return fail_tag(ix, "rollout-laid without the buffer", CKPT_TAG_ROLLOUT);
        const uint64_t env = kind == (uint32_t)CKPT_ENV_EXTERNAL ? 0 : 4ull * E * (S > 5 ? S : 5);
        /* fixed words, env_state, cont, both carries, {ep_fresh, ext_done}, ep_state, ep_agg, ext_key */
        const uint64_t base = CKPT_ROLLOUT_FIXED + pad8(env) + pad8(E) + 16ull * E + 8 + 32ull * E + 128 + 8;
        if (s[CKPT_TAG_ROLLOUT].len < base) return fail_tag(ix, "length contradicts its shapes", CKPT_TAG_ROLLOUT);
        const uint8_t* fl = ro + CKPT_ROLLOUT_FIXED + pad8(env) + pad8(E) + 16ull * E;
        const uint32_t ext_done = ckpt_rd32(fl + 4);
        if (!is01(ckpt_rd32(fl)) || !is01(ext_done) || (ext_done && kind != (uint32_t)CKPT_ENV_EXTERNAL))
            return fail_tag(ix, "a flag out of range", CKPT_TAG_ROLLOUT);
        if (s[CKPT_TAG_ROLLOUT].len != base + (ext_done ? 4ull * E * S : 0))
            return fail_tag(ix, "length contradicts its shapes", CKPT_TAG_ROLLOUT);
    }

    if (s[CKPT_TAG_BUFFER].present) {
        if (s[CKPT_TAG_BUFFER].len < CKPT_BUFFER_FIXED) return fail_tag(ix, "too short", CKPT_TAG_BUFFER);
        const uint8_t* bf = img + s[CKPT_TAG_BUFFER].off;
        const uint32_t idx = ckpt_rd32(bf), full = ckpt_rd32(bf + 4), W = ckpt_rd32(bf + 12);
        const uint64_t limit = ckpt_rd32(bf + 8);
        if (!is01(full) || idx > cap || limit != (full ? cap : idx))
            return fail_tag(ix, "idx / full / limit contradict the capacity", CKPT_TAG_BUFFER);
        if (W != (mask_on ? (A + 31) / 32 : 0u)) return fail_tag(ix, "mask words contradict the settings", CKPT_TAG_BUFFER);
        const uint64_t want = CKPT_BUFFER_FIXED + 4ull * limit * (2ull * S + A + 2) + ((2 * limit + 3) & ~3ull) +
                              4ull * limit * W;
        if (s[CKPT_TAG_BUFFER].len != want) return fail_tag(ix, "length contradicts its shapes", CKPT_TAG_BUFFER);
    }

    /* the learning-rate schedule: a kind other than constant, its parameters inside the setter's ranges, rates the
     * rule could have left (inside [lr_min, lr_max]; zeros for the linear kind, which keeps none) */
    if (s[CKPT_TAG_LRSCHED].present) {
        if (s[CKPT_TAG_LRSCHED].len != CKPT_LRSCHED_BYTES) return fail_tag(ix, "bad length", CKPT_TAG_LRSCHED);
        const uint8_t* lr = img + s[CKPT_TAG_LRSCHED].off;
        const uint32_t kind = ckpt_rd32(lr);
        const float p0 = rd_f32(lr + 4), p1 = rd_f32(lr + 8), p2 = rd_f32(lr + 12);
        const float w = rd_f32(lr + 32), wv = rd_f32(lr + 36);
        if (!is01(ckpt_rd32(lr + 16)) || ckpt_rd32(lr + 20) != 0)
            return fail_tag(ix, "a flag out of range", CKPT_TAG_LRSCHED);
        if (kind == (uint32_t)CKPT_LR_LINEAR) {
            if (!(p0 >= 1.f) || isinf(p0) || !(p1 >= 0.f && p1 <= 1.f) || p2 != 0.f)
                return fail_tag(ix, "parameters outside the linear schedule's ranges", CKPT_TAG_LRSCHED);
            if (ckpt_rd64(lr + 32) != 0 || ckpt_rd64(lr + 40) != 0)
                return fail_tag(ix, "rate words or counters with the linear schedule", CKPT_TAG_LRSCHED);
        } else if (kind == (uint32_t)CKPT_LR_ADAPTIVE) {
            if (!(p0 > 0.f) || isinf(p0) || !(p1 > 0.f) || !(p2 >= p1) || isinf(p2))
                return fail_tag(ix, "parameters outside the adaptive schedule's ranges", CKPT_TAG_LRSCHED);
            if (!(w >= p1 && w <= p2) || !(wv >= 0.f) || isinf(wv))
                return fail_tag(ix, "a rate outside [lr_min, lr_max]", CKPT_TAG_LRSCHED);
        } else {
            return fail_tag(ix, "unknown schedule kind", CKPT_TAG_LRSCHED);
        }
    }

    /* advantage normalisation: a mode other than the global one (the writer leaves the section out for that) that
     * this version knows, and a zero word */
    if (s[CKPT_TAG_ADVNORM].present) {
        if (s[CKPT_TAG_ADVNORM].len != CKPT_ADVNORM_BYTES) return fail_tag(ix, "bad length", CKPT_TAG_ADVNORM);
        const uint8_t* an = img + s[CKPT_TAG_ADVNORM].off;
        if (ckpt_rd32(an) > CKPT_ADVNORM_MAX_MODE) return fail_tag(ix, "unknown advantage-normalisation mode", CKPT_TAG_ADVNORM);
        if (ckpt_rd32(an + 4) != 0) return fail_tag(ix, "reserved word not zero", CKPT_TAG_ADVNORM);
    }

    /* the KL monitor's estimator: one other than k3 (the writer leaves the section out for that) that this version
     * knows, and a zero word */
    if (s[CKPT_TAG_KLEST].present) {
        if (s[CKPT_TAG_KLEST].len != CKPT_KLEST_BYTES) return fail_tag(ix, "bad length", CKPT_TAG_KLEST);
        const uint8_t* ke = img + s[CKPT_TAG_KLEST].off;
        if (ckpt_rd32(ke) > CKPT_KLEST_MAX) return fail_tag(ix, "unknown KL estimator", CKPT_TAG_KLEST);
        if (ckpt_rd32(ke + 4) != 0) return fail_tag(ix, "reserved word not zero", CKPT_TAG_KLEST);
    }

    /* the state-dependent-σ Gaussian: present exactly while the action distribution is 3, an even A with A / 2 <= 32,
     * bounds the setter accepts */
    if ((s[CKPT_TAG_GAUSS_SD].present != 0) != (dist == 3u))
        return fail(ix, "the action distribution and the state-dependent-sigma section disagree");
    if (s[CKPT_TAG_GAUSS_SD].present) {
        if (s[CKPT_TAG_GAUSS_SD].len != CKPT_GAUSS_SD_BYTES) return fail_tag(ix, "bad length", CKPT_TAG_GAUSS_SD);
        const uint8_t* sd = img + s[CKPT_TAG_GAUSS_SD].off;
        const float lo = rd_f32(sd + 8), hi = rd_f32(sd + 12);
        if (ckpt_rd32(sd) != 1 || ckpt_rd32(sd + 4) != 0) return fail_tag(ix, "a word out of range", CKPT_TAG_GAUSS_SD);
        if ((A & 1u) || A / 2 > CKPT_GAUSS_SD_MAX_AA)
            return fail_tag(ix, "the action size is odd or wider than 64", CKPT_TAG_GAUSS_SD);
        if (!(lo < hi) || !(lo >= -20.f) || !(hi <= 20.f)) return fail_tag(ix, "bounds outside [-20, 20]", CKPT_TAG_GAUSS_SD);
        ix->sd_ls[0] = lo;
        ix->sd_ls[1] = hi;
    }
    return 0;
}

int ckpt_index(const void* buf, size_t len, CkptIndex* ix) {
    const uint8_t* img = (const uint8_t*)buf;
    memset(ix, 0, sizeof(*ix));
    if (!img || len < CKPT_HEADER_BYTES) return fail(ix, "shorter than the header");
    if (memcmp(img, CKPT_MAGIC, 8) != 0) return fail(ix, "bad magic: not a training-state checkpoint");
    ix->version = ckpt_rd32(img + 8);
    ix->flags = ckpt_rd32(img + 12);
    ix->count = ckpt_rd32(img + 16);
    if (ix->version != CKPT_VERSION) return fail(ix, "unsupported version (this reader knows version 1)");
    if (ix->flags & ~(uint32_t)(CKPT_F_BUFFER | CKPT_F_ROLLOUT | CKPT_F_LRSCHED | CKPT_F_ADVNORM | CKPT_F_KLEST | CKPT_F_GAUSS_SD)) return fail(ix, "unknown header flags");
    if (ix->count > (len - CKPT_HEADER_BYTES) / CKPT_SECTION_BYTES)
        return fail(ix, "more sections than the file could hold");
    size_t pos = CKPT_HEADER_BYTES;
    for (uint32_t i = 0; i < ix->count; i++) {
        if (len - pos < CKPT_SECTION_BYTES) return fail(ix, "truncated inside a section header");
        const uint32_t tag = ckpt_rd32(img + pos);
        const uint64_t bytes = ckpt_rd64(img + pos + 8), sum = ckpt_rd64(img + pos + 16);
        if (ckpt_rd32(img + pos + 4) != 0) return fail_tag(ix, "reserved word not zero", tag);
        pos += CKPT_SECTION_BYTES;
        const size_t room = len - pos;
        if (bytes > room || pad8(bytes) > room) return fail_tag(ix, "payload runs past the end of the file", tag);
        if (ckpt_fnv1a64(img + pos, (size_t)bytes) != sum) return fail_tag(ix, "checksum mismatch", tag);
        for (uint64_t k = bytes; k < pad8(bytes); k++)
            if (img[pos + k] != 0) return fail_tag(ix, "padding not zero", tag);
        if (tag >= CKPT_TAG_LEGACY && tag < CKPT_NTAG) {       /* unknown tags are skipped */
            if (ix->sec[tag].present) return fail_tag(ix, "appears twice", tag);
            ix->sec[tag].present = 1;
            ix->sec[tag].off = pos;
            ix->sec[tag].len = bytes;
        }
        pos += (size_t)pad8(bytes);
    }
    if (pos != len) return fail(ix, "bytes beyond the last section");
    return check_sections(img, ix);
}
