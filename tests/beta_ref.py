"""The Beta policy (csrc/ppo_math.h beta_*, csrc/beta.hip) in float64, on numpy and torch's lgamma / digamma / polygamma.
Bounds: the device evaluates in double and stores in fp32, so each stored quantity gets 2⁻²³·Σ|terms| of its own sum (the
cast's 2⁻²⁴ plus the double arithmetic's error, which is relative to the terms): lp and H over their terms; the gradient
|g|·Σ|terms of ∂lp/∂α| + (ent_coeff/m)·Σ|terms of ∂H/∂α|, times sigmoid(z), g the fp32 surrogate's on the lp the device
returned; the loss Σ|sur_i|·(lp's bound_i + 3·2⁻²⁴)/m plus 2⁻⁴⁰ relative.  A clamped logit's bound is 0: +0."""
import numpy as np
import torch

from policy_head_ref import F32, F64, U

EPS, ENT = 0.2, 0.01
Z_MAX = 20.0            # the tests' clamp: softplus(−20) = 2e−9 is below fp32 resolution, so α = β = 1 to fp32 there
X_LO, X_HI = F32(2.0 ** -24), F32(1 - 2.0 ** -24)
lgamma = lambda x: torch.lgamma(torch.as_tensor(np.asarray(x, F64))).numpy()            # noqa: E731
digamma = lambda x: torch.digamma(torch.as_tensor(np.asarray(x, F64))).numpy()          # noqa: E731
trigamma = lambda x: torch.polygamma(1, torch.as_tensor(np.asarray(x, F64))).numpy()    # noqa: E731


def shapes(z, zmax):
    """α, β [m, Aa], ∂α/∂z, ∂β/∂z (0 on a clamped logit) and `inside` [m, A]; NaN propagates and counts as inside"""
    z = np.asarray(z, F64)
    Aa = z.shape[1] // 2
    with np.errstate(invalid="ignore"):
        low, high = z < -zmax, z > zmax
    zc, inside = np.where(low, -zmax, np.where(high, zmax, z)), ~low & ~high
    s = 1 + np.maximum(zc, 0) + np.log1p(np.exp(-np.abs(zc)))
    ds = np.where(inside, 1 / (1 + np.exp(-zc)), 0.0)
    return s[:, :Aa], s[:, Aa:], ds[:, :Aa], ds[:, Aa:], inside


def surrogate_f32(adv, lp, old, eps, m):
    """ppo_math.h surrogate in its own arithmetic (fp32, the ratio through a double exp): g = ∂loss/∂lp and `clipped`"""
    adv, eps = np.asarray(adv, F32), F32(eps)
    with np.errstate(all="ignore"):
        ratio = np.exp((np.asarray(lp, F32) - np.asarray(old, F32)).astype(F64)).astype(F32)
        on = np.where(adv > 0, ~(ratio > F32(1) + eps), ~(ratio < F32(1) - eps))
        return -(on.astype(F32)) * adv * ratio / F32(m), ~on


def head_f64(z, action, adv, old_lp, eps, ent_coeff, zmax, lp_for_g=None):
    """float64 from the fp32 inputs as given: per row lp, H, sur, g; grad [m, A] = ∂loss/∂z; the loss; the counters; the
    module docstring's bounds under b_*"""
    m, A = np.asarray(z).shape
    x = np.asarray(action, F64)[:, :A // 2]
    a, b, da, db, inside = shapes(z, zmax)
    cat, cm = (lambda p, q: np.concatenate([p * da, q * db], axis=1)), ent_coeff / m
    with np.errstate(all="ignore"):
        lx, l1x, s = np.log(x), np.log(1 - x), a + b - 2
        ga, gb, gab, pa, pb, pab = lgamma(a), lgamma(b), lgamma(a + b), digamma(a), digamma(b), digamma(a + b)
        ta, tb, tab = trigamma(a), trigamma(b), trigamma(a + b)
        lp_t = [(a - 1) * lx, (b - 1) * l1x, gab, -ga, -gb]
        H_t = [ga, gb, -gab, -(a - 1) * pa, -(b - 1) * pb, s * pab]
        lp, H = sum(lp_t).sum(axis=1), sum(H_t).sum(axis=1)
        g, clipped = surrogate_f32(adv, lp if lp_for_g is None else lp_for_g, old_lp, eps, m)
        g = g.astype(F64)[:, None]
        grad = np.where(inside, g * cat(lx + pab - pa, l1x + pab - pb) - cm * cat(s * tab - (a - 1) * ta,
                                                                                  s * tab - (b - 1) * tb), 0.0)
        r = np.exp(lp - np.asarray(old_lp, F64))
        sur = np.asarray(adv, F64) * np.where(np.asarray(adv) > 0, np.minimum(r, 1 + eps), np.maximum(r, 1 - eps))
        b_lp = 2 * U * sum(np.abs(t) for t in lp_t).sum(axis=1)
        mag_lp = cat(np.abs(lx) + np.abs(pab) + np.abs(pa), np.abs(l1x) + np.abs(pab) + np.abs(pb))
        mag_H = cat(np.abs(s * tab) + np.abs((a - 1) * ta), np.abs(s * tab) + np.abs((b - 1) * tb))
    return dict(lp=lp, H=H, sur=sur, ratio=r, clipped=clipped, g=g[:, 0], grad=grad, inside=inside,
                loss=-sur.sum() / m - ent_coeff * H.sum() / m, clamped=int((~inside).sum()), elems=m * A, b_lp=b_lp,
                b_H=2 * U * sum(np.abs(t) for t in H_t).sum(axis=1),
                b_grad=np.where(inside, 2 * U * (np.abs(g) * mag_lp + cm * mag_H), 0.0),
                b_loss=((np.abs(sur) * (b_lp + 3 * U)).sum() + 2.0 ** -40 * (np.abs(sur).sum() + ent_coeff * np.abs(H).sum())) / m)


def kl_rows_f64(z_old, z_new, zmax):
    """KL(old ‖ new) per row over the clamped rows and its 2⁻²³·Σ|terms| bound; unprimed = old"""
    (a, b), (an, bn) = shapes(z_old, zmax)[:2], shapes(z_new, zmax)[:2]
    t = [lgamma(an), lgamma(bn), -lgamma(an + bn), -lgamma(a), -lgamma(b), lgamma(a + b), (a - an) * digamma(a),
         (b - bn) * digamma(b), (an - a + bn - b) * digamma(a + b)]
    kl = ((t[0] + t[1] + t[2]) + (t[3] + t[4] + t[5])) + t[6] + t[7] + t[8]        # lnB′ − lnB first: identical rows give 0
    return kl.sum(axis=1), 2 * U * sum(np.abs(v) for v in t).sum(axis=1)


def moments(a, b, k):                               # E[x^k] of Beta(a, b) = Π_{i<k} (a + i)/(a + b + i)
    return np.prod([(a + i) / (a + b + i) for i in range(k)], axis=0)


def head_inputs(Aa, m):
    """logits half in ±3, half in ±(z_max + 4), some at −z_max; x from the row's own Beta, some on each storage clamp;
    old_lp = lp − d with |d| in [0.3, 0.5] (clipped under the matching sign of adv) or [0.02, 0.1]: no ratio near 1 ± eps"""
    rng = np.random.default_rng(7300 + 31 * Aa + 7 * m)
    z = np.where(rng.random((m, 2 * Aa)) < 0.5, rng.uniform(-3, 3, (m, 2 * Aa)), rng.uniform(-Z_MAX - 4, Z_MAX + 4, (m, 2 * Aa)))
    z[rng.random(z.shape) < 0.05] = -Z_MAX
    z = z.astype(F32)
    x = np.clip(rng.beta(*shapes(z, Z_MAX)[:2]).astype(F32), X_LO, X_HI)
    x[rng.random(x.shape) < 0.03], x[rng.random(x.shape) < 0.03] = X_LO, X_HI
    act, adv = np.concatenate([x, np.zeros_like(x)], axis=1), rng.normal(size=m).astype(F32)
    d = rng.choice([-1.0, 1.0], m) * np.where(np.arange(m) % 2, rng.uniform(0.3, 0.5, m), rng.uniform(0.02, 0.1, m))
    lp = head_f64(z, act, adv, np.zeros(m), EPS, 0.0, Z_MAX)["lp"]
    return dict(z=z, act=act, adv=adv, old=(lp - d).astype(F32))
