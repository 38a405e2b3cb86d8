/*
 * adam.c — Adam objects (reference /root/reference/src/adam.cu).
 *
 * Device Adams detect when their tensors form one contiguous span and then
 * update the whole span with a single vectorised kernel; m and v are flat HBM
 * buffers covering that span.  A caller's tensor list (create_adam_cuda,
 * load_adam) is flat only when its tensors abut: floats between two tensors are
 * the caller's, and the span kernel would read them as gradients and write them
 * as parameters.  The network constructors own their buffers' ≤3 floats of
 * zero-gradient alignment padding between tensors and keep the padded span.
 */
#include "internal.h"

#include <math.h>

#define NN_PAD_GAP 3          /* neural_network.c aligns every tensor of a network's buffer to 4 floats */

static Adam* adam_alloc(float** weights, float** grads, int* length, int num_layers, int size, float beta1,
                        float beta2) {
    Adam* a = (Adam*)xcalloc(1, sizeof(Adam));
    a->weights = (float**)xmalloc(sizeof(float*) * (size_t)num_layers);
    a->grad_weights = (float**)xmalloc(sizeof(float*) * (size_t)num_layers);
    a->lengths = (int*)xmalloc(sizeof(int) * (size_t)num_layers);
    memcpy(a->weights, weights, sizeof(float*) * (size_t)num_layers);
    memcpy(a->grad_weights, grads, sizeof(float*) * (size_t)num_layers);
    memcpy(a->lengths, length, sizeof(int) * (size_t)num_layers);
    a->size = size;
    a->beta1 = beta1;
    a->beta2 = beta2;
    a->time_step = 0;
    a->num_layers = num_layers;
    a->grad_scale = 1.0f;
    return a;
}

/* contiguous with gaps of at most max_gap floats, identical param→grad offset for every tensor.
 * max_gap: 0 for a caller's list, 3 for a network's own buffers (the caller vouches that the
 * gap floats are padding it owns, with zero gradients) */
static long flat_span(float** w, float** g, const int* len, int n, int max_gap) {
    if (n <= 0) return -1;
    const ptrdiff_t dg = g[0] - w[0];
    for (int i = 0; i < n; i++) {
        if (g[i] - w[i] != dg) return -1;
        if (i + 1 < n) {
            const ptrdiff_t gap = w[i + 1] - (w[i] + len[i]);
            if (gap < 0 || gap > max_gap) return -1;
        }
    }
    return (long)((w[n - 1] + len[n - 1]) - w[0]);
}

/* ---------------- host-pointer Adam (adam.cu:6-74) ---------------- */
Adam* create_adam(float** weights, float** grad_weights, int* length, int num_layers, int size, float beta1,
                  float beta2) {
    Adam* a = adam_alloc(weights, grad_weights, length, num_layers, size, beta1, beta2);
    a->m = (float*)xcalloc((size_t)size, sizeof(float));
    a->v = (float*)xcalloc((size_t)size, sizeof(float));
    a->on_device = 0;
    a->span = size;
    return a;
}

Adam* create_adam_from_nn(NeuralNetwork* nn, float beta1, float beta2) {
    const int L = nn->num_layers - 1;
    float** w = (float**)xmalloc(sizeof(float*) * (size_t)(2 * L));
    float** g = (float**)xmalloc(sizeof(float*) * (size_t)(2 * L));
    int* len = (int*)xmalloc(sizeof(int) * (size_t)(2 * L));
    int size = 0;
    for (int i = 0; i < L; i++) {
        Layer* ly = &nn->layers[i];
        w[2 * i] = ly->weights;      g[2 * i] = ly->grad_weights;      len[2 * i] = ly->input_size * ly->output_size;
        w[2 * i + 1] = ly->biases;   g[2 * i + 1] = ly->grad_biases;   len[2 * i + 1] = ly->output_size;
        size += len[2 * i] + len[2 * i + 1];
    }
    Adam* a = create_adam(w, g, len, 2 * L, size, beta1, beta2);
    free(w); free(g); free(len);
    return a;
}

void free_adam(Adam* adam) {
    if (!adam) return;
    if (adam->on_device) { free_adam_cuda(adam); return; }
    free(adam->weights);
    free(adam->grad_weights);
    free(adam->lengths);
    free(adam->m);
    free(adam->v);
    free(adam);
}

static void bias_corrections(Adam* a, float* bc1, float* bc2) {
    a->time_step += 1;
    *bc1 = 1 - powf(a->beta1, a->time_step);     /* adam.cu:56-57 */
    *bc2 = 1 - powf(a->beta2, a->time_step);
}

/* the next step's bias-corrected step size and second-moment correction, as adam_update_cuda
 * computes them (advances time_step) — for kernels that run many Adam steps in one launch */
void adam_next_step(Adam* a, float lr, float* step, float* bc2) {
    float bc1;
    bias_corrections(a, &bc1, bc2);
    *step = lr / bc1;
}

/* host tensors: staged into HBM, updated by the multi-tensor kernel, copied back */
void adam_update(Adam* adam, float lr) {
    if (adam->on_device) { adam_update_cuda(adam, lr); return; }
    float bc1, bc2;
    bias_corrections(adam, &bc1, &bc2);
    const int n = adam->num_layers;
    long total = 0;
    for (int i = 0; i < n; i++) total += adam->lengths[i];
    float* dp = (float*)stage(ST_A, sizeof(float) * (size_t)total);
    float* dg = (float*)stage(ST_B, sizeof(float) * (size_t)total);
    float* dm = stage_up(ST_C, adam->m, (size_t)total);
    float* dv = stage_up(ST_D, adam->v, (size_t)total);
    long off = 0;
    for (int i = 0; i < n; i++) {
        phip_h2d(dp + off, adam->weights[i], sizeof(float) * (size_t)adam->lengths[i]);
        phip_h2d(dg + off, adam->grad_weights[i], sizeof(float) * (size_t)adam->lengths[i]);
        off += adam->lengths[i];
    }
    const PhipAdamSpan s = {dp, dg, dm, dv, total, bc1, bc2, adam->grad_scale, 0};
    phip_adam_flat(&s, (PhipAdamRate){lr, NULL}, adam->beta1, adam->beta2, NULL, 0, NULL, NULL);
    off = 0;
    for (int i = 0; i < n; i++) {
        phip_d2h(adam->weights[i], dp + off, sizeof(float) * (size_t)adam->lengths[i]);
        off += adam->lengths[i];
    }
    phip_d2h(adam->m, dm, sizeof(float) * (size_t)total);
    phip_d2h(adam->v, dv, sizeof(float) * (size_t)total);
}

/* ---------------- device Adam (adam.cu:76-169) ---------------- */
static Adam* adam_create_device(float** weights, float** grad_weights, int* length, int num_layers, int size,
                                float beta1, float beta2, int max_gap) {
    Adam* a = adam_alloc(weights, grad_weights, length, num_layers, size, beta1, beta2);
    a->on_device = 1;
    const long span = flat_span(weights, grad_weights, length, num_layers, max_gap);
    a->flat = span >= 0;
    a->span = a->flat ? span : size;
    a->m = (float*)phip_malloc(sizeof(float) * (size_t)align4(a->span));
    a->v = (float*)phip_malloc(sizeof(float) * (size_t)align4(a->span));
    return a;
}

Adam* create_adam_cuda(float** weights, float** grad_weights, int* length, int num_layers, int size, float beta1,
                       float beta2) {
    return adam_create_device(weights, grad_weights, length, num_layers, size, beta1, beta2, 0);
}

Adam* create_adam_from_nn_cuda(NeuralNetwork* nn, float beta1, float beta2) {
    const int L = nn->num_layers - 1;
    float** w = (float**)xmalloc(sizeof(float*) * (size_t)(2 * L));
    float** g = (float**)xmalloc(sizeof(float*) * (size_t)(2 * L));
    int* len = (int*)xmalloc(sizeof(int) * (size_t)(2 * L));
    int size = 0;
    for (int i = 0; i < L; i++) {
        Layer* ly = &nn->layers[i];
        w[2 * i] = ly->d_weights;    g[2 * i] = ly->d_grad_weights;    len[2 * i] = ly->input_size * ly->output_size;
        w[2 * i + 1] = ly->d_biases; g[2 * i + 1] = ly->d_grad_biases; len[2 * i + 1] = ly->output_size;
        size += len[2 * i] + len[2 * i + 1];
    }
    Adam* a = adam_create_device(w, g, len, 2 * L, size, beta1, beta2, NN_PAD_GAP);
    free(w); free(g); free(len);
    return a;
}

void free_adam_cuda(Adam* adam) {
    if (!adam) return;
    phip_free(adam->m);
    phip_free(adam->v);
    free(adam->weights);
    free(adam->grad_weights);
    free(adam->lengths);
    free(adam);
}

void adam_update_cuda(Adam* adam, float lr) { adam_update_dev(adam, (PhipAdamRate){lr, NULL}, NULL, 0, 0, NULL, NULL); }

/* the Adam's flat span with this step's bias corrections, as the launchers take it */
static PhipAdamSpan flat_span_of(const Adam* a, float bc1, float bc2, int zero_g) {
    return (PhipAdamSpan){a->weights[0], a->grad_weights[0], a->m, a->v, a->span, bc1, bc2, a->grad_scale, zero_g};
}

/* w16 != NULL: also refresh the bf16 shadow of the first n16 parameters (flat spans only).
 * zero_g: clear the gradient span once read (flat spans only).  Returns bit 0: shadow refreshed,
 * bit 1: gradients cleared.  coef != NULL (flat spans only): the step's device clip coefficient
 * (PhipClipRec.coef), multiplied into the gradient scale by the kernel.  skip != NULL (flat spans only): the
 * device stop word of target-KL early stopping (PhipKlRec.stopped): while it is set the kernel takes no step
 * and only clears the gradient where zero_g asks.  The host step counter advances either way; ppo_update
 * sets it back by the steps the device skipped.  rate.d_lr != NULL: the rate comes from that device word (the
 * KL-adaptive schedule's, or a coupled value rate), read by the kernels' device-word instantiations. */
int adam_update_dev(Adam* adam, PhipAdamRate rate, unsigned short* w16, long n16, int zero_g, const float* coef,
                    const unsigned* skip) {
    if (coef && !adam->flat) die("adam_update_dev: gradient clipping needs a flat Adam span");
    if (skip && !adam->flat) die("adam_update_dev: target-KL early stopping needs a flat Adam span");
    float bc1, bc2;
    bias_corrections(adam, &bc1, &bc2);
    nn_note_device_update(adam->weights[0]);          /* the network's host mirrors are now stale */
    if (!adam->flat) {
        phip_adam_multi(adam->weights, adam->grad_weights, adam->lengths, adam->num_layers, adam->m, adam->v, rate,
                        adam->beta1, adam->beta2, bc1, bc2, adam->grad_scale);
        return 0;
    }
    /* the clearing pass is the vectorised kernel's: 16-B aligned spans only */
    if (!adam_span_aligned(adam)) zero_g = 0;
    const PhipAdamSpan s = flat_span_of(adam, bc1, bc2, zero_g);
    phip_adam_flat(&s, rate, adam->beta1, adam->beta2, w16, w16 ? n16 : 0, coef, skip);
    return (w16 != NULL) | (zero_g ? 2 : 0);
}

/* ppo_ext.h (a test entry): one adam_update_cuda step with the rate through a device word */
int ppo_adam_update_lr_device(void* vadam, const float* d_lr) {
    Adam* adam = (Adam*)vadam;
    if (!adam || !adam->on_device || !d_lr) return -1;
    adam_update_dev(adam, (PhipAdamRate){0.f, d_lr}, NULL, 0, 0, NULL, NULL);
    return 0;
}

/* a network's flat Adam (16-B aligned span) and a small flat side Adam (the entropy Adam's log σ) in
 * one launch; the side's step runs first in the step counters (ppo.cu:440-442 order; the spans are
 * independent).  Returns bit 0: shadow refreshed, bit 1: network gradients cleared, bit 2: side
 * gradients cleared; −1 (nothing done) when the pair does not qualify.  coef as in adam_update_dev: one
 * coefficient for both spans; skip likewise: one stop word for both.  The two rates come both by value or both
 * from device words. */
int adam_update_pair_dev(Adam* adam, PhipAdamRate rate, unsigned short* w16, long n16, int zero_g, Adam* side,
                         PhipAdamRate side_rate, int zero_side, const float* coef, const unsigned* skip) {
    if (!rate.d_lr != !side_rate.d_lr) die("adam_update_pair_dev: one rate by value, the other in a device word");
    if (!adam->flat || !side->flat || !adam_span_aligned(adam) || side->span > 256 || side->span < 1 ||
        adam->span < 1 || adam->beta1 != side->beta1 || adam->beta2 != side->beta2 || ((uintptr_t)w16 & 7u))
        return -1;
    float bc1s, bc2s, bc1, bc2;
    bias_corrections(side, &bc1s, &bc2s);
    bias_corrections(adam, &bc1, &bc2);
    nn_note_device_update(adam->weights[0]);
    nn_note_device_update(side->weights[0]);
    const PhipAdamSpan s = flat_span_of(adam, bc1, bc2, zero_g), s2 = flat_span_of(side, bc1s, bc2s, zero_side);
    phip_adam_flat_pair(&s, rate, &s2, side_rate, adam->beta1, adam->beta2, w16, w16 ? n16 : 0, coef, skip);
    return (w16 != NULL) | (zero_g ? 2 : 0) | (zero_side ? 4 : 0);
}

/* ---------------- checkpoint (adam.cu:172-264 byte layout) ---------------- */
/* m / v are written packed by tensor (reference order), whatever the padding in HBM. */
static void moments_to_host(Adam* a, float* m, float* v) {
    if (!a->on_device) {
        memcpy(m, a->m, sizeof(float) * (size_t)a->size);
        memcpy(v, a->v, sizeof(float) * (size_t)a->size);
        return;
    }
    long src = 0, dst = 0;
    for (int i = 0; i < a->num_layers; i++) {
        if (a->flat) src = (long)(a->weights[i] - a->weights[0]);
        phip_d2h(m + dst, a->m + src, sizeof(float) * (size_t)a->lengths[i]);
        phip_d2h(v + dst, a->v + src, sizeof(float) * (size_t)a->lengths[i]);
        dst += a->lengths[i];
        if (!a->flat) src += a->lengths[i];
    }
}

void save_adam(Adam* adam, FILE* file, bool cuda) {
    (void)cuda;
    fwrite(&adam->size, sizeof(int), 1, file);
    fwrite(&adam->time_step, sizeof(int), 1, file);
    fwrite(&adam->beta1, sizeof(float), 1, file);
    fwrite(&adam->beta2, sizeof(float), 1, file);
    fwrite(&adam->num_layers, sizeof(int), 1, file);
    float* m = (float*)xmalloc(sizeof(float) * (size_t)adam->size);
    float* v = (float*)xmalloc(sizeof(float) * (size_t)adam->size);
    moments_to_host(adam, m, v);
    fwrite(m, sizeof(float), (size_t)adam->size, file);
    fwrite(v, sizeof(float), (size_t)adam->size, file);
    free(m);
    free(v);
}

/* n_expected: tensors the caller's arrays hold (−1: unknown, the reference signature) — a checkpoint
 * whose tensor count or size disagrees is rejected before anything is allocated or copied.
 * max_gap: as in flat_span (0 for a caller's list, NN_PAD_GAP for a network's own buffers) */
static Adam* load_adam_gap(FILE* file, float** weights, float** grad_weights, int* length, int n_expected, bool cuda,
                           int max_gap) {
    int size, t, n;
    float b1, b2;
    if (fread(&size, sizeof(int), 1, file) != 1 || fread(&t, sizeof(int), 1, file) != 1 ||
        fread(&b1, sizeof(float), 1, file) != 1 || fread(&b2, sizeof(float), 1, file) != 1 ||
        fread(&n, sizeof(int), 1, file) != 1)
        die("checkpoint: unexpected end of file");
    if (n <= 0 || (n_expected >= 0 && n != n_expected))
        die("checkpoint: Adam tensor count does not match the network");
    long total = 0;
    for (int i = 0; i < n; i++) {
        if (length[i] < 0) die("checkpoint: negative Adam tensor length");
        total += length[i];
    }
    if (size < 0 || (long)size != total) die("checkpoint: Adam size does not match the tensor lengths");
    float* m = (float*)xmalloc(sizeof(float) * (size_t)size);
    float* v = (float*)xmalloc(sizeof(float) * (size_t)size);
    if (fread(m, sizeof(float), (size_t)size, file) != (size_t)size ||
        fread(v, sizeof(float), (size_t)size, file) != (size_t)size)
        die("checkpoint: unexpected end of file");
    Adam* a;
    if (cuda) {
        a = adam_create_device(weights, grad_weights, length, n, size, b1, b2, max_gap);
        long src = 0, dst = 0;
        for (int i = 0; i < n; i++) {
            if (a->flat) dst = (long)(a->weights[i] - a->weights[0]);
            phip_h2d(a->m + dst, m + src, sizeof(float) * (size_t)length[i]);
            phip_h2d(a->v + dst, v + src, sizeof(float) * (size_t)length[i]);
            src += length[i];
            if (!a->flat) dst += length[i];
        }
        free(m);
        free(v);
    } else {
        a = adam_alloc(weights, grad_weights, length, n, size, b1, b2);
        a->m = m;
        a->v = v;
        a->span = size;
    }
    a->time_step = t;
    return a;
}

Adam* load_adam_ex(FILE* file, float** weights, float** grad_weights, int* length, int n_expected, bool cuda) {
    return load_adam_gap(file, weights, grad_weights, length, n_expected, cuda, 0);
}

Adam* load_adam(FILE* file, float** weights, float** grad_weights, int* length, bool cuda) {
    return load_adam_ex(file, weights, grad_weights, length, -1, cuda);
}

Adam* load_adam_from_nn(FILE* file, NeuralNetwork* nn, bool cuda) {
    const int L = nn->num_layers - 1;
    float** w = (float**)xmalloc(sizeof(float*) * (size_t)(2 * L));
    float** g = (float**)xmalloc(sizeof(float*) * (size_t)(2 * L));
    int* len = (int*)xmalloc(sizeof(int) * (size_t)(2 * L));
    for (int i = 0; i < L; i++) {
        Layer* ly = &nn->layers[i];
        w[2 * i] = cuda ? ly->d_weights : ly->weights;
        w[2 * i + 1] = cuda ? ly->d_biases : ly->biases;
        g[2 * i] = cuda ? ly->d_grad_weights : ly->grad_weights;
        g[2 * i + 1] = cuda ? ly->d_grad_biases : ly->grad_biases;
        len[2 * i] = ly->input_size * ly->output_size;
        len[2 * i + 1] = ly->output_size;
    }
    Adam* a = load_adam_gap(file, w, g, len, 2 * L, cuda, NN_PAD_GAP);
    free(w); free(g); free(len);
    return a;
}
