/*
 * advnorm.h — per-minibatch advantage normalisation: the one definition (ppo_ext.h ppo_set_adv_norm quotes it,
 * advnorm.hip computes it, tests/advnorm_ref.py restates it in numpy).
 *
 * A segment is B consecutive floats x_0 … x_{B−1}: the advantages of one policy minibatch, as GAE's global
 * normalisation left them.  It is rewritten as
 *
 *     p_t  = Σ_{i ≡ t (mod 256), i ascending} (double)x_i          t = 0 … 255   (from +0.0; empty lanes stay +0.0)
 *     S    = pairwise tree over p (stride 1, 2, 4 … 128: p_t += p_{t+stride} for t a multiple of 2·stride), S = p_0
 *     mean = S / B                                                  (double)
 *     q_t, Q likewise over d_i·d_i,  d_i = (double)x_i − mean       (product rounded, then added: no FMA)
 *     sd   = (float)sqrt(Q / max(B − 1, 1))                         (the unbiased std of torch.Tensor.std)
 *     m    = (float)mean
 *     y_i  = (float)((double)(x_i − m) / ((double)sd + 1e-8))       (the form of gae.hip's normalize_kernel:
 *                                                                    x_i − m is an fp32 difference)
 *
 * and (m, sd) is the segment's statistics pair.  Every operation is IEEE round-to-nearest; the result is a function
 * of (B, data) alone.  A NaN propagates within its own segment only (mean, sd and every y_i of it are NaN); a
 * constant segment gives y = 0 (the lane sums of a constant are exact, so mean is the constant); B == 1 gives y = 0.
 *
 * Against Stable-Baselines3 (normalize_advantage) and CleanRL (norm_adv), which compute
 * (a − a.mean()) / (a.std() + 1e-8) on the raw advantages a of the minibatch: x is a global affine image of a
 * (x = (a − μ)/(σ_pop + 1e-8), GAE's normalisation over the whole buffer), and the map above is invariant under such
 * a map, so y equals their result up to rounding and the two 1e-8 terms — not bit for bit.
 */
#ifndef PPO_ADVNORM_H
#define PPO_ADVNORM_H

#define ADVNORM_LANES 256           /* lane partials = threads of the segment's workgroup = doubles of LDS */
#define ADVNORM_REG 16              /* elements a thread keeps in registers across the three passes */

#endif
