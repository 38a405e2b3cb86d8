/*
 * checkpoint.h — the container of a training-state checkpoint (DESIGN.md §4 "Training-state checkpoints"):
 * its constants and the indexer / validator of an image in memory.  Nothing here needs HIP or libppo:
 * checkpoint_index.c implements it with libc alone and compiles on its own for the CPU.
 */
#ifndef PPO_HOST_CHECKPOINT_H
#define PPO_HOST_CHECKPOINT_H

#include <stddef.h>
#include <stdint.h>

#define CKPT_MAGIC "PPOSTATE"
#define CKPT_VERSION 1u
#define CKPT_HEADER_BYTES 20u          /* magic[8], u32 version, u32 flags, u32 section count */
#define CKPT_SECTION_BYTES 24u         /* u32 tag, u32 reserved (0), u64 payload bytes, u64 FNV-1a-64 of the payload */

/* section tags; 0 and everything above CKPT_TAG_GAUSS_SD is unknown to this version and skipped */
enum { CKPT_TAG_LEGACY = 1, CKPT_TAG_SETTINGS = 2, CKPT_TAG_NORMALISERS = 3, CKPT_TAG_SHUFFLE = 4,
       CKPT_TAG_ROLLOUT = 5, CKPT_TAG_BUFFER = 6, CKPT_TAG_LRSCHED = 7, CKPT_TAG_ADVNORM = 8, CKPT_TAG_KLEST = 9,
       CKPT_TAG_GAUSS_SD = 10, CKPT_NTAG = 11 };
/* header flags: bit 0 is the caller's PPO_CKPT_BUFFER (a Buffer section follows); bit 1 is set by the writer
 * when a Rollout section follows, bit 2 when a learning-rate schedule section follows (written only while a
 * schedule other than the constant one is set), bit 3 when an advantage-normalisation section follows (written
 * only while the mode is not the global one), bit 4 when a KL-estimator section follows (written only while the
 * estimator is not k3), bit 5 when a state-dependent-σ Gaussian section follows (written only while the action
 * distribution is 3) — every optional section is announced in the header, so a damaged
 * tag cannot make one vanish unnoticed */
enum { CKPT_F_BUFFER = 1, CKPT_F_ROLLOUT = 2, CKPT_F_LRSCHED = 4, CKPT_F_ADVNORM = 8, CKPT_F_KLEST = 16, CKPT_F_GAUSS_SD = 32 };

#define CKPT_SETTINGS_FIXED 52u        /* bytes of the Settings payload around nvec[D] */
#define CKPT_ROLLOUT_FIXED 32u         /* bytes of the Rollout payload ahead of env_state */
#define CKPT_BUFFER_FIXED 16u          /* idx, full, limit, mask words */
#define CKPT_LRSCHED_BYTES 48u         /* u32 kind, f32 p0 p1 p2, u32 couple, u32 0, u64 u, f32 lr lr_v, u32 raised lowered */
#define CKPT_ADVNORM_BYTES 8u          /* u32 mode, u32 0 */
#define CKPT_ADVNORM_MAX_MODE 1u       /* ppo_ext.h PPO_ADV_NORM_MINIBATCH */
#define CKPT_KLEST_BYTES 8u            /* u32 estimator, u32 0 */
#define CKPT_KLEST_MAX 1u              /* ppo_ext.h PPO_KL_EXACT */
#define CKPT_GAUSS_SD_BYTES 16u        /* u32 1, u32 0, f32 ls_min, f32 ls_max */
#define CKPT_GAUSS_SD_MAX_AA 32u       /* ppo_ext.h: A even, A / 2 <= 32 */
#define CKPT_LR_LINEAR 1               /* ppo_ext.h PPO_LR_LINEAR / PPO_LR_ADAPTIVE */
#define CKPT_LR_ADAPTIVE 2
#define CKPT_ENV_EXTERNAL 3            /* ro_kind of the open rollout (ppo_hip.h PHIP_ENV_EXTERNAL) */
#define CKPT_MD_MAX_D 256              /* ppo_ext.h PPO_MD_MAX_D */

typedef struct {
    int present;
    uint64_t off, len;                 /* the payload inside the image */
} CkptSection;

typedef struct {
    uint32_t version, flags, count;
    CkptSection sec[CKPT_NTAG];        /* by tag */
    int S, A, cap;                     /* the shapes in the legacy header */
    int action_dist, md_D, mask_on;    /* from Settings */
    int has_obs;                       /* Normalisers holds the observation triple */
    float sd_ls[2];                    /* from the state-dependent-σ Gaussian section (action_dist == 3) */
    char err[160];
} CkptIndex;

/* indexes and validates an image: magic, version, bounds, checksums, zero padding, the required sections and
 * every section's length against the shapes in the legacy header.  Returns 0, or −1 with one line in ix->err. */
int ckpt_index(const void* buf, size_t len, CkptIndex* ix);
uint64_t ckpt_fnv1a64(const void* p, size_t n);
uint32_t ckpt_rd32(const uint8_t* p);
uint64_t ckpt_rd64(const uint8_t* p);

#endif
