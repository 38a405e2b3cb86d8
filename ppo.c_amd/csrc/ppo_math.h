// ppo_math.h — the per-row arithmetic of the PPO update, written once for every kernel that evaluates it:
// the multi-launch heads (kernels.hip, out_head.hip), the single-workgroup and cluster phases (tiny.hip,
// cluster.hip, cluster_deep.hip), sampling and rollouts (sample.hip, rollout.hip), the KL monitor (kl.hip)
// and Adam (adam.hip).  Every path gives the same bits because every path calls these.
//
// All arithmetic is in the order written here, with the reference's C promotions (its double temporaries);
// the kernels are built with -ffp-contract=off.  tests/policy_head_ref.py and oracle/ref_cpu.c restate it
// independently.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace ppo {

// ---- Gaussian log-prob of one row (policy.cu:67-74): lp = start(A), then lp = sub(lp, term(log σ_j, z_j))
// for j ascending, z_j = (a_j − μ_j) / exp(log σ_j).  A kernel that fuses or splits the loop calls the atoms.
// sub takes the fp32 lp widened at the call (exact): (float)((double)lp − term), one rounding.
__device__ __forceinline__ float log_prob_start(int A) { return (float)(-0.5 * A * (double)logf((float)(2 * M_PI))); }
__device__ __forceinline__ double log_prob_term(float ls, float z) { return (double)ls + 0.5 * (double)(z * z); }
__device__ __forceinline__ float log_prob_sub(double lp, double term) { return (float)(lp - term); }

__device__ __forceinline__ float log_prob_row(const float* mu, const float* log_std, const float* a, int A) {
    float lp = log_prob_start(A);
    for (int j = 0; j < A; ++j) {
        const float z = (a[j] - mu[j]) / expf(log_std[j]);
        lp = log_prob_sub(lp, log_prob_term(log_std[j], z));
    }
    return lp;
}
// es[j] = expf(log_std[j]) computed once by the caller (the same value the per-element expf gives)
__device__ __forceinline__ float log_prob_row_es(const float* mu, const float* log_std, const float* es,
                                                 const float* a, int A) {
    float lp = log_prob_start(A);
    for (int j = 0; j < A; ++j) {
        const float z = (a[j] - mu[j]) / es[j];
        lp = log_prob_sub(lp, log_prob_term(log_std[j], z));
    }
    return lp;
}

// ---- clipped surrogate of one row of a minibatch of m rows (ppo.cu:82-107); *grad = ∂loss/∂lp
__device__ __forceinline__ float surrogate(float adv, float lp, float old_lp, float eps, int m, float* grad) {
    const float ratio = (float)exp((double)(lp - old_lp));
    const int adv_pos = adv > 0;
    const int ratio_pos = ratio > 1 + eps;
    const int ratio_neg = ratio < 1 - eps;
    *grad = -(adv_pos * !ratio_pos + !adv_pos * !ratio_neg) * adv * ratio / m;
    return adv * (adv_pos * (ratio_pos * (1 + eps) + !ratio_pos * ratio) +
                  !adv_pos * (ratio_neg * (1 - eps) + !ratio_neg * ratio));
}

// ---- Categorical policy over A choices (ppo_set_action_dist; no counterpart in the reference): the atoms of
// one row, z its A logits and a the chosen index, all fp32:
//     M   = max_k z_k
//     e_k = expf(z_k − M)                                   cat_exp
//     s   = Σ_k e_k        t = Σ_k e_k·(z_k − M)            k ascending inside each part the kernel sums: one lane
//                                                           sums its own k, parts combine by the kernel's fixed tree
//     ls  = logf(s)
//     lp  = (z_a − M) − ls                                  cat_log_prob
//     p_k = e_k / s
//     H   = ls − t / s                                      cat_entropy
//     g   = ∂loss/∂lp from surrogate(adv, lp, old_lp, eps, m, &g)
//     ∂loss/∂z_k = g·([k == a] − p_k) + (ent_coeff / m)·p_k·(((z_k − M) − ls) + H)          cat_grad
//     loss = −Σ_rows surrogate / m − ent_coeff·(Σ_rows H) / m
// The signs are the Gaussian head's: loss = −mean surrogate − ent_coeff·entropy, once; the second gradient term
// is ∂(−ent_coeff·H/m)/∂z_k = (ent_coeff/m)·p_k·(log p_k + H).  tests/categorical_ref.py restates it.
__device__ __forceinline__ float cat_exp(float z, float M) { return expf(z - M); }
__device__ __forceinline__ float cat_log_prob(float za, float M, float ls) { return (za - M) - ls; }
__device__ __forceinline__ float cat_entropy(float ls, float t, float s) { return ls - t / s; }
// cm = ent_coeff / m, formed once per launch by the caller
__device__ __forceinline__ float cat_grad(float g, bool chosen, float z, float M, float s, float ls, float H,
                                          float cm) {
    const float p = cat_exp(z, M) / s;
    return g * ((chosen ? 1.f : 0.f) - p) + cm * p * (((z - M) - ls) + H);
}
// one thread walks z[0 … n) in index order under a mask (the sampler, the KL monitor, evaluation, a one-lane
// component of the head): M, s and — when t is not NULL — t over the columns mk allows.  M starts from the first
// allowed logit and then takes fmaxf; s and t add k ascending.  NoMask allows every column (and is its own
// per-component view, see "Action masking" below): M = z[0], then fmaxf for k = 1 …, the unmasked sequence.
struct NoMask {
    __device__ __forceinline__ bool allowed(int) const { return true; }
    __device__ __forceinline__ NoMask component(int, int, int) const { return *this; }
};
template <class Mask = NoMask>
__device__ __forceinline__ float cat_row_max(const float* z, int n, const Mask& mk = Mask()) {
    bool first = true;
    float M = 0.f;
    for (int k = 0; k < n; ++k) {
        if (!mk.allowed(k)) continue;
        M = first ? z[k] : fmaxf(M, z[k]);
        first = false;
    }
    return M;
}
template <class Mask = NoMask>
__device__ __forceinline__ float cat_row_sum(const float* z, int n, float M, float* t, const Mask& mk = Mask()) {
    float s = 0.f, tt = 0.f;
    for (int k = 0; k < n; ++k) {
        if (!mk.allowed(k)) continue;
        const float e = cat_exp(z[k], M);
        s += e;
        tt += e * (z[k] - M);
    }
    if (t) *t = tt;
    return s;
}
// the stored action row: column 0 holds the index as an exact float; anything outside [0, A) is clamped
__device__ __forceinline__ int cat_index(float a0, int A) {
    const int a = (int)a0;
    return a < 0 ? 0 : (a >= A ? A - 1 : a);
}
__device__ __forceinline__ float cat_log_prob_row(const float* z, int A, int a) {
    const float M = cat_row_max(z, A);
    return cat_log_prob(z[a], M, logf(cat_row_sum(z, A, M, nullptr)));
}

// ---- Multi-discrete policy (ppo_set_action_multidiscrete; no counterpart in the reference): the A logits of a
// row are D softmaxes side by side.  nvec = (n_0 … n_{D−1}), every n_d >= 2, Σ n_d = A; component d owns the logits
// [o_d, o_d + n_d), o_d = Σ_{j<d} n_j (the offsets array off[0 … D], off[D] = A).  The stored action row holds the
// chosen indices a_d ∈ [0, n_d) as exact floats in columns 0 … D−1 (columns D … A−1 are +0); reads clamp with
// cat_index(·, n_d).  Per row, all fp32, every component through the cat_* atoms above:
//     per component d:  M_d, e_k, s_d, t_d, ls_d = logf(s_d), lp_d = cat_log_prob(z_{o_d + a_d}, M_d, ls_d),
//                       H_d = cat_entropy(ls_d, t_d, s_d)
//     lp = ((lp_0 + lp_1) + lp_2) + …        H = ((H_0 + H_1) + H_2) + …              d ascending
//     g  = ∂loss/∂lp from surrogate(adv, lp, old_lp, eps, m, &g)                      one ratio per row, the joint lp
//     ∂loss/∂z_k, k in component d = cat_grad(g, k == o_d + a_d, z_k, M_d, s_d, ls_d, H_d, ent_coeff / m)
//     loss = −Σ_rows surrogate / m − ent_coeff·(Σ_rows H) / m
// The entropy term of a logit's gradient takes its own component's H_d: ∂H/∂z_k = ∂H_d/∂z_k.  A component with
// n_d <= 32 is summed k ascending by one lane (md_component); a wider one may combine lane partials by the kernel's
// fixed tree.  D = 1 is the categorical policy bit for bit.  tests/multidiscrete_ref.py restates it.
struct MdComp { float M, s, ls, lp, H; };
// one thread walks component z[0 … n) in index order under its effective mask mk; a the chosen index inside it
template <class Mask>
__device__ __forceinline__ MdComp md_component(const float* z, int n, int a, const Mask& mk) {
    MdComp c;
    c.M = cat_row_max(z, n, mk);
    float t;
    c.s = cat_row_sum(z, n, c.M, &t, mk);
    c.ls = logf(c.s);
    c.lp = cat_log_prob(z[a], c.M, c.ls);
    c.H = cat_entropy(c.ls, t, c.s);
    return c;
}
// the joint log-prob of one row by one thread (the KL monitor): md_component's lp per segment, d ascending; rm the
// row's mask (NoMask, or MaskRow over its W words)
template <class RowMask>
__device__ __forceinline__ float md_log_prob_row(const float* z, const int* off, int D, const float* action,
                                                 const RowMask& rm) {
    float lp = 0.f;
    for (int d = 0; d < D; ++d) {
        const int o = off[d], n = off[d + 1] - o;
        const int a = cat_index(action[d], n);
        const float l = md_component(z + o, n, a, rm.component(o, n, a)).lp;
        lp = d == 0 ? l : lp + l;
    }
    return lp;
}

// ---- Action masking (ppo_set_action_mask; no counterpart in the reference; csrc/discrete.hip): a row of A logits
// carries W = (A + 31) / 32 words, bit k & 31 of word k >> 5 set = column k allowed, k counted across the
// components; bits at k >= A are ignored.  The EFFECTIVE mask of component d, columns [o_d, o_d + n_d):
//     1. its stored bits;
//     2. none of them set: every column of the component is allowed (nothing is NaN, nothing aborts);
//     3. where a chosen action exists (the head, the KL monitor): the chosen column is allowed too.
// Per component, fp32, k ascending over the ALLOWED columns only, the atoms above:
//     M_d = max z_k,  e_k = cat_exp(z_k, M_d),  s_d = Σ e_k,  t_d = Σ e_k·(z_k − M_d),
//     ls_d = logf(s_d),  lp_d = cat_log_prob(z_{o_d + a_d}, M_d, ls_d),  H_d = cat_entropy(ls_d, t_d, s_d)
// A masked column enters no max and no sum, its gradient element is +0 and its logit is never read into arithmetic
// (a NaN, an infinity or 1e30 there changes no output bit).  Joint lp and H, the surrogate, cat_grad on the allowed
// columns and the loss are the multi-discrete policy's.  There is one definition: cat_row_max, cat_row_sum,
// md_component and md_log_prob_row above take the mask as a type, MaskComp here or NoMask; with every bit set
// MaskComp skips nothing, which is NoMask's sequence and its bits.  The sampler inverts the CDF over the allowed
// columns (the fallback is the last allowed one); the greedy action is the lowest allowed index holding the allowed
// maximum.  tests/masked_ref.py restates it.
__device__ __forceinline__ bool mask_bit(const uint32_t* w, int k) { return (w[k >> 5] >> (k & 31)) & 1u; }
// any stored bit of columns [o, o + n)
__device__ __forceinline__ bool mask_any(const uint32_t* w, int o, int n) {
    const int last = o + n - 1;
    for (int j = o >> 5; j <= last >> 5; ++j) {
        uint32_t v = w[j];
        if (j == o >> 5) v &= ~0u << (o & 31);
        if (j == last >> 5) v &= ~0u >> (31 - (last & 31));
        if (v) return true;
    }
    return false;
}
// the effective mask of one component, fixed once per (row, component); a the chosen index inside it (−1: none).
// n <= 32: the three rules folded into one word, bit k = column o + k; wider: rule 2 in `full`, rule 3 in `a`, the
// stored bits read in place
struct MaskComp {
    const uint32_t* w;
    int o, a;
    uint32_t win;
    bool narrow, full;
    __device__ __forceinline__ bool allowed(int k) const {
        return narrow ? (win >> k) & 1u : (full || k == a || mask_bit(w, o + k));
    }
};
__device__ __forceinline__ MaskComp mask_component(const uint32_t* w, int o, int n, int a) {
    MaskComp mc;
    mc.w = w; mc.o = o; mc.a = a;
    mc.narrow = n <= 32;
    mc.win = 0u;
    mc.full = false;
    if (mc.narrow) {
        const int j = o >> 5, sh = o & 31;
        uint32_t v = w[j] >> sh;
        if (sh && ((o + n - 1) >> 5) > j) v |= w[j + 1] << (32 - sh);
        const uint32_t all = ~0u >> (32 - n);
        v &= all;
        if (!v) v = all;
        if (a >= 0) v |= 1u << a;
        mc.win = v;
    } else {
        mc.full = !mask_any(w, o, n);
    }
    return mc;
}
// a row's W words as the source of its components' effective masks (NoMask is the unmasked counterpart)
struct MaskRow {
    const uint32_t* w;
    __device__ __forceinline__ MaskComp component(int o, int n, int a) const { return mask_component(w, o, n, a); }
};
// the row mask of a kernel instantiated with or without masking; w is unread when MASKED is false
template <bool MASKED>
__device__ __forceinline__ auto mask_row(const uint32_t* w) {
    if constexpr (MASKED) return MaskRow{w};
    else return NoMask{};
}

// ---- Closed-form KL(old ‖ new) of one row (ppo_set_kl_estimator, PPO_KL_EXACT; the KL monitor, kl.hip; no
// counterpart in the reference): fp32 inputs, every operation in double, j / k / d ascending.
// Diagonal Gaussian, old (μo, lso) and new (μn, lsn) with ls = log σ, per column j:
//     d      = lso_j − lsn_j
//     term_j = (0.5·expm1(2d) − d) + 0.5·(μo_j − μn_j)²·exp(−2·lsn_j)          kl_gauss_term
//     KL     = Σ_j term_j
// the textbook log(σn/σo) + (σo² + Δμ²)/(2σn²) − ½ with σo²/(2σn²) − ½ written as ½·expm1(2d), which does not cancel
// near d = 0; identical inputs give exactly 0.  rsl_rl adds 1e-5 inside its log (log(σn/σo + 1e-5)); this does not.
// Categorical / multi-discrete / masked, per component over its EFFECTIVE allowed columns only ("Action masking"
// above: the stored bits; none set → all; the chosen column OR-ed in), zo the old logits and zn the new:
//     e_k  = exp(z_k − M),  M = max_k z_k (fp32, exact)                       kl_cat_exp
//     lo_k = (zo_k − Mo) − log Σ_k exp(zo_k − Mo),  ln_k likewise from zn    kl_cat_logp
//     s    = Σ_k exp(lo_k)·(lo_k − ln_k)                                      kl_cat_term
//     KL_d = s < 0 ? 0 : s   (a NaN stays NaN)                                kl_cat_clamp
//     KL   = Σ_d KL_d
// A masked column is read in neither zo nor zn.  One thread walks a component k ascending (kl_cat_component); a
// kernel that spreads a wide component over a wave sums each lane's k ascending and combines the lanes by its fixed
// tree, through the same atoms.  tests/kl_exact_ref.py restates it.
__device__ __forceinline__ double kl_gauss_term(float mo, float lso, float mn, float lsn) {
    const double d = (double)lso - (double)lsn;
    const double dm = (double)mo - (double)mn;
    return (0.5 * expm1(2.0 * d) - d) + 0.5 * (dm * dm) * exp(-2.0 * (double)lsn);
}
__device__ __forceinline__ double kl_gauss_row(const float* mo, const float* lso, const float* mn, const float* lsn,
                                               int A) {
    double kl = 0.0;
    for (int j = 0; j < A; ++j) kl += kl_gauss_term(mo[j], lso[j], mn[j], lsn[j]);
    return kl;
}
__device__ __forceinline__ double kl_cat_exp(float z, float M) { return exp((double)z - (double)M); }
__device__ __forceinline__ double kl_cat_logp(float z, float M, double ls) { return ((double)z - (double)M) - ls; }
__device__ __forceinline__ double kl_cat_term(double lo, double ln) { return exp(lo) * (lo - ln); }
__device__ __forceinline__ double kl_cat_clamp(double s) { return s < 0.0 ? 0.0 : s; }
// one thread, one component zo / zn[0 … n) under its effective mask mk
template <class Mask>
__device__ __forceinline__ double kl_cat_component(const float* zo, const float* zn, int n, const Mask& mk) {
    const float Mo = cat_row_max(zo, n, mk), Mn = cat_row_max(zn, n, mk);
    double so = 0.0, sn = 0.0;
    for (int k = 0; k < n; ++k) {
        if (!mk.allowed(k)) continue;
        so += kl_cat_exp(zo[k], Mo);
        sn += kl_cat_exp(zn[k], Mn);
    }
    const double lso = log(so), lsn = log(sn);
    double s = 0.0;
    for (int k = 0; k < n; ++k) {
        if (!mk.allowed(k)) continue;
        s += kl_cat_term(kl_cat_logp(zo[k], Mo, lso), kl_cat_logp(zn[k], Mn, lsn));
    }
    return kl_cat_clamp(s);
}
// one thread, one row of D components; action (NULL without a mask) holds the chosen indices for rule 3
template <class RowMask>
__device__ __forceinline__ double kl_cat_row(const float* zo, const float* zn, const int* off, int D,
                                             const float* action, const RowMask& rm) {
    double kl = 0.0;
    for (int d = 0; d < D; ++d) {
        const int o = off[d], n = off[d + 1] - o;
        const int a = action ? cat_index(action[d], n) : -1;
        kl += kl_cat_component(zo + o, zn + o, n, rm.component(o, n, a));
    }
    return kl;
}

// ---- Gaussian entropy (policy.cu:171-193): this constant, then += log σ_j for j ascending, at the call site
// (the sum inside a helper compiled to other code than the kernels' own loops)
__device__ __forceinline__ float entropy_start(int A) { return (float)(A * 0.5 * (1 + log(2 * M_PI))); }

// ---- State-dependent-σ Gaussian (ppo_set_action_gaussian_sd; csrc/gauss_sd.hip; no counterpart in the reference):
// a row of μ's A outputs z is Aa = A / 2 means followed by Aa raw log σ, clamped to [ls_min, ls_max] on read.  Per
// row, fp32, j ascending, through the Gaussian atoms above:
//     ls_j = t < ls_min ? ls_min : (t > ls_max ? ls_max : t),   t = z_{Aa+j}          sd_clamp   (NaN propagates)
//     in_j = !(t < ls_min) && !(t > ls_max)                                            sd_inside  (NaN counts as inside)
//     lp   = log_prob_start(Aa), then lp = log_prob_sub(lp, log_prob_term(ls_j, (a_j − μ_j) / expf(ls_j)))   sd_lp_step
//     H    = entropy_start(Aa), then += ls_j                                           sd_row
//     g    = ∂loss/∂lp from surrogate(adv, lp, old_lp, eps, m, &g)
//     ∂loss/∂z_j      = (a_j − μ_j)·expf(−2·ls_j)·g                                    sd_grad_mu (the Gaussian head's)
//     ∂loss/∂z_{Aa+j} = in_j ? (−1 + (a_j − μ_j)²·expf(−2·ls_j))·g − ent_coeff/m : +0  sd_grad_ls
//     loss = −Σ_rows surrogate / m − ent_coeff·(Σ_rows H) / m
// A row whose ls equals a fixed log σ vector gets log_prob_row's and the Gaussian head's bits.  The closed-form
// KL(old ‖ new) is kl_gauss_term over the clamped halves of both rows (sd_kl_row).  tests/gauss_sd_ref.py restates it.
__device__ __forceinline__ float sd_clamp(float t, float lo, float hi) { return t < lo ? lo : (t > hi ? hi : t); }
__device__ __forceinline__ bool sd_inside(float t, float lo, float hi) { return !(t < lo) && !(t > hi); }
__device__ __forceinline__ float sd_lp_step(float lp, float a, float mu, float ls) {
    const float z = (a - mu) / expf(ls);
    return log_prob_sub(lp, log_prob_term(ls, z));
}
struct SdRow { float lp, H; int clamped; };
// one thread walks one row: z its A = 2·Aa outputs, a its Aa actions
__device__ __forceinline__ SdRow sd_row(const float* z, const float* a, int Aa, float lo, float hi) {
    SdRow r;
    r.lp = log_prob_start(Aa);
    r.H = entropy_start(Aa);
    r.clamped = 0;
    for (int j = 0; j < Aa; ++j) {
        const float t = z[Aa + j], ls = sd_clamp(t, lo, hi);
        r.lp = sd_lp_step(r.lp, a[j], z[j], ls);
        r.H += ls;
        r.clamped += !sd_inside(t, lo, hi);
    }
    return r;
}
__device__ __forceinline__ float sd_grad_mu(float a, float mu, float ls, float g) {
    const float d = a - mu;
    return d * expf(-2 * ls) * g;
}
// t the raw log σ; cm = ent_coeff / m, formed once per launch by the caller
__device__ __forceinline__ float sd_grad_ls(float a, float mu, float t, float lo, float hi, float g, float cm) {
    if (!sd_inside(t, lo, hi)) return 0.f;
    const float d = a - mu;
    return (-1 + d * d * expf(-2 * t)) * g - cm;
}
__device__ __forceinline__ double sd_kl_row(const float* zo, const float* zn, int Aa, float lo, float hi) {
    double kl = 0.0;
    for (int j = 0; j < Aa; ++j)
        kl += kl_gauss_term(zo[j], sd_clamp(zo[Aa + j], lo, hi), zn[j], sd_clamp(zn[Aa + j], lo, hi));
    return kl;
}

// ---- Adam on one element (adam.cu:53-74): step = lr/bc1, ε added in double
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float step, float b1, float b2,
                                          float bc2) {
    m = b1 * m + (1 - b1) * g;
    v = b2 * v + (1 - b2) * (g * g);
    const float denom = (float)((double)sqrtf(v / bc2) + 1e-8);
    p -= step * m / denom;
}

}  // namespace ppo
