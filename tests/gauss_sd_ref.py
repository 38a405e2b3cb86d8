"""The state-dependent-σ Gaussian policy (ppo_set_action_gaussian_sd; csrc/ppo_math.h sd_*, csrc/gauss_sd.hip): the
definition in float64, an fp32 mirror built from policy_head_ref.policy_head_f32 (imported, not edited), the rounding
bounds the GPU tests hold the kernels to — derived the way policy_head_ref derives its own — and the inputs those tests
run on.  Pinned on the CPU in test_gauss_sd_cpu.py against torch.distributions.Normal."""
import functools
import struct

import numpy as np

import policy_head_ref as ph
from policy_head_ref import F32, F64, U

EPS, ENT = 0.2, 0.01
LS_MIN, LS_MAX = -2.0, 1.0                       # the tests' bounds: narrow, so that all three classes are populated
HEAD_AA = [1, 3, 17, 32]
HEAD_M = [1, 63, 64, 65, 300]


def clamp(t, lo, hi):
    """ls and `inside` of raw log σ t: NaN propagates through the clamp and counts as inside."""
    t = np.asarray(t)
    with np.errstate(invalid="ignore"):
        low, high = t < lo, t > hi
    ls = np.where(low, t.dtype.type(lo), np.where(high, t.dtype.type(hi), t))
    return ls, ~low & ~high


def head_f64(z, action, adv, old_lp, eps, ent_coeff, lo, hi):
    """Everything in float64 from the fp32 inputs as given.  z [m, A] = [mean | raw log σ], action [m, A] (columns
    Aa … unread).  Per row: lp, H, ratio, clipped, dlp, sur; grad [m, A] = ∂loss/∂z (a clamped column: 0); the loss;
    the counters."""
    z, action, adv, old = (np.asarray(v, F64) for v in (z, action, adv, old_lp))
    m, A = z.shape
    Aa = A // 2
    mu, t, a = z[:, :Aa], z[:, Aa:], action[:, :Aa]
    ls, inside = clamp(t, F64(lo), F64(hi))
    with np.errstate(all="ignore"):
        zz = (a - mu) / np.exp(ls)
        lp = -0.5 * Aa * np.log(2 * np.pi) - (ls + 0.5 * zz * zz).sum(axis=1)
        H = Aa * 0.5 * (1 + np.log(2 * np.pi)) + ls.sum(axis=1)
        ratio = np.exp(lp - old)
        pos = adv > 0
        clipped = np.where(pos, ratio > 1 + eps, ratio < 1 - eps)
        dlp = np.where(clipped, 0.0, -adv * ratio / m)
        sur = adv * np.where(clipped, np.where(pos, 1 + eps, 1 - eps), ratio)
        d, e2 = a - mu, np.exp(-2 * ls)
        g_mu = d * e2 * dlp[:, None]
        g_ls = np.where(inside, (-1 + d * d * e2) * dlp[:, None] - ent_coeff / m, 0.0)
    return dict(lp=lp, H=H, ratio=ratio, clipped=clipped, dlp=dlp, sur=sur, grad=np.concatenate([g_mu, g_ls], axis=1),
                inside=inside, ls=ls, loss=-sur.sum() / m - ent_coeff * H.sum() / m,
                clamped=int((~inside).sum()), elems=m * Aa)


def kl_rows_f64(z_old, z_new, lo, hi):
    """KL(old ‖ new) per row over the clamped halves, the Gaussian closed form."""
    zo, zn = np.asarray(z_old, F64), np.asarray(z_new, F64)
    Aa = zo.shape[1] // 2
    lso, lsn = clamp(zo[:, Aa:], F64(lo), F64(hi))[0], clamp(zn[:, Aa:], F64(lo), F64(hi))[0]
    d, dm = lso - lsn, zo[:, :Aa] - zn[:, :Aa]
    return ((0.5 * np.expm1(2 * d) - d) + 0.5 * dm * dm * np.exp(-2 * lsn)).sum(axis=1)


def head_f32(z, action, adv, old_lp, eps, ent_coeff, lo, hi):
    """The fp32 mirror: every row is the Gaussian head's row at width Aa under its own clamped log σ, so it runs
    policy_head_f32 row by row (its log σ is per column) and adds the clamp's zero and the ent_coeff / m term."""
    z, action, adv, old = (np.ascontiguousarray(v, F32) for v in (z, action, adv, old_lp))
    m, A = z.shape
    Aa = A // 2
    ls, inside = clamp(z[:, Aa:], F32(lo), F32(hi))
    lp, sur, grad = np.empty(m, F32), np.empty(m, F32), np.empty((m, A), F32)
    H = np.empty(m, F32)
    cm = F32(ent_coeff) / F32(m)
    h0 = F32(Aa * 0.5 * (1 + np.log(2 * np.pi)))
    for i in range(m):
        r = ph.policy_head_f32(z[i:i + 1, :Aa], ls[i], action[i:i + 1, :Aa], adv[i:i + 1], old[i:i + 1], eps)
        lp[i], sur[i] = r["lp"][0], r["sur"][0]
        # policy_head_f32 divides by m = 1: the device divides by the minibatch's m, in the same place
        dlp = (r["dlp"][0] * F32(1)) / F32(m) if m != 1 else r["dlp"][0]
        d = action[i, :Aa] - z[i, :Aa]
        e2 = ph.expf(F32(-2) * ls[i])
        grad[i, :Aa] = d * e2 * dlp
        grad[i, Aa:] = np.where(inside[i], (F32(-1) + d * d * e2) * dlp - cm, F32(0))
        h = h0
        for j in range(Aa):
            h = F32(h + ls[i, j])
        H[i] = h
    return dict(lp=lp, sur=sur, grad=grad, H=H)


# ---------------------------------------------------------------------------------------------------- bounds
def head_bounds(z, action, adv, old_lp, eps, ent_coeff, lo, hi):
    """Per element, in float64, from the rounding of the listed operations (policy_head_ref's derivation at width Aa
    under the row's own log σ):
      lp    policy_head_ref.lp_bound of the row, plus 2.5·Aa·2⁻²⁴ for the constant −0.5·Aa·logf((float)2π): the
            argument's rounding moves the logarithm by 2⁻²⁴, a 1-ulp logf of 1.84 by 3.7·2⁻²⁴, times 0.5·Aa — a term
            that shows only where a row's z and log σ are both small, as in rows clamped at a small |ls|.
      H     (Aa + 1)·2⁻²⁴·max |partial sum|: the constant's rounding and Aa fp32 additions.
      grad  mean half: |g|·(row_rel_bound + 6·2⁻²⁴) — the ratio's relative error, then a − μ, a 2-ulp expf(−2 ls) and
            two products; log-σ half: the same relative bound on (|−1| + d²e2)·|dlp| (the sum's terms, not their
            difference) plus 2·2⁻²⁴·(|term| + ent_coeff/m) for the subtraction and ent_coeff / m itself.
    A clamped column's bound is 0: the device writes +0."""
    r = head_f64(z, action, adv, old_lp, eps, ent_coeff, lo, hi)
    z64, a64 = np.asarray(z, F64), np.asarray(action, F64)
    m, A = z64.shape
    Aa = A // 2
    ls = r["ls"]
    # lp_bound broadcasts over a per-row log σ [m, Aa] as it does over its per-column one
    lp_b = ph.lp_bound(z64[:, :Aa], ls, a64[:, :Aa]) + 2.5 * Aa * U
    part = Aa * 0.5 * (1 + np.log(2 * np.pi)) + np.cumsum(ls, axis=1)
    H_b = (Aa + 1) * U * np.maximum(np.abs(part).max(axis=1), Aa * 0.5 * (1 + np.log(2 * np.pi)))
    rel = lp_b + 8 * U + 6 * U
    d, e2 = a64[:, :Aa] - z64[:, :Aa], np.exp(-2 * ls)
    dlp = np.abs(r["dlp"])[:, None]
    g_mu = np.abs(r["grad"][:, :Aa]) * rel[:, None]
    mag = (1 + d * d * e2) * dlp
    g_ls = mag * rel[:, None] + 2 * U * (mag + ent_coeff / m)
    g_ls = np.where(r["inside"], g_ls, 0.0)
    return dict(lp=lp_b, H=H_b, grad=np.concatenate([g_mu, g_ls], axis=1), rel=rel)


def loss_bound(ref, b, m, ent_coeff):
    """The device sums the fp32 row surrogates and entropies in double: the bound is the rows' own errors —
    |sur_i|·(rel_i + 2⁻²⁴) and the H bound — divided by m, plus 2⁻⁵⁰ relative for the double sums and 2⁻²⁴ for the
    fp32 ent_coeff widened."""
    sur_err = (np.abs(ref["sur"]) * (b["rel"] + U)).sum() / m
    ent_err = ent_coeff * (b["H"].sum() / m + 2 * U * np.abs(ref["H"]).sum() / m)
    return sur_err + ent_err + 2.0 ** -40 * (np.abs(ref["sur"]).sum() / m + ent_coeff * np.abs(ref["H"]).sum() / m)


def near_clip(ratio, eps=EPS):
    return (np.abs(ratio - (1 + eps)) < 1e-4) | (np.abs(ratio - (1 - eps)) < 1e-4)


# ---------------------------------------------------------------------------------------------------- inputs
ROWS = 300


def classes(ref, adv):
    """the fractions of the eight classes the issue's input condition names"""
    pos, cl = np.asarray(adv) > 0, ref["clipped"]
    neg = np.asarray(adv) < 0
    return dict(pos_unclipped=(pos & ~cl).mean(), pos_clipped=(pos & cl).mean(), neg_unclipped=(neg & ~cl).mean(),
                neg_clipped=(neg & cl).mean())


def ls_classes(z, lo, hi):
    Aa = z.shape[1] // 2
    t = np.asarray(z)[:, Aa:]
    return dict(low=(t < lo).mean(), high=(t > hi).mean(), inside=((t >= lo) & (t <= hi)).mean())


@functools.lru_cache(maxsize=None)
def head_inputs(Aa, m=ROWS, seed=0):
    """z = [μ ~ N(0, 1) | raw log σ ~ U(lo − 1.2, hi + 1.2)], action = μ + σ·N(0, 1) (zeros after it), old_lp = lp − x
    with x laid out so that each of the four (sign of adv, clipped) classes holds a quarter of the rows whatever m is:
    row i takes sign pattern i mod 4, |x| ∈ [0.3, 0.5] (clipped: ratio beyond 1 ± 0.2) or [0.02, 0.1] (unclipped).
    No row is within 1e-4 of the clip boundary (asserted).  For m = 1 the class condition cannot hold and is not
    asserted.  Read-only arrays."""
    rng = np.random.default_rng(9100 + 31 * Aa + 7 * m + seed)
    A = 2 * Aa
    mu = rng.normal(size=(m, Aa)).astype(F32)
    raw = rng.uniform(LS_MIN - 1.2, LS_MAX + 1.2, (m, Aa)).astype(F32)
    z = np.concatenate([mu, raw], axis=1)
    ls = clamp(raw, F32(LS_MIN), F32(LS_MAX))[0]
    act = np.zeros((m, A), F32)
    act[:, :Aa] = mu + rng.normal(size=(m, Aa)).astype(F32) * np.exp(ls)
    lp = head_f64(z, act, np.zeros(m), np.zeros(m), EPS, 0.0, LS_MIN, LS_MAX)["lp"]
    k = (np.arange(m) + seed) % 4                   # 0: pos unclipped, 1: pos clipped, 2: neg unclipped, 3: neg clipped
    adv = np.abs(rng.normal(size=m)).astype(F32) + F32(0.05)
    adv[k >= 2] *= F32(-1)
    big = rng.uniform(0.3, 0.5, m)
    small = rng.uniform(0.02, 0.1, m) * rng.choice([-1.0, 1.0], m)
    # lp − old = x: ratio = e^x; positive advantage clips above (x > 0), negative below (x < 0)
    x = np.where(k == 1, big, np.where(k == 3, -big, small))
    old = (lp - x).astype(F32)
    out = dict(z=z, act=act, adv=adv, old=old)
    for v in out.values():
        v.setflags(write=False)
    return out


def check_input_condition(i, what=""):
    """the issue's condition on a head case, on the model: >= 10 % of the rows in each (sign, clipped) class and
    >= 10 % of the log-σ elements in each clamp class"""
    ref = head_f64(i["z"], i["act"], i["adv"], i["old"], EPS, ENT, LS_MIN, LS_MAX)
    assert not near_clip(ref["ratio"]).any(), what
    for name, frac in {**classes(ref, i["adv"]), **ls_classes(i["z"], LS_MIN, LS_MAX)}.items():
        assert frac >= 0.10, f"{what}: class {name} holds {frac:.3f} of the case"
    return ref


def smallest_covering(Aa, m):
    """inputs of m rows for width Aa that meet the condition; small m draws seeds until the classes are populated
    (m = 1 cannot: returned as drawn)"""
    if m < 40:
        return head_inputs(Aa, m)
    for seed in range(64):
        i = head_inputs(Aa, m, seed)
        try:
            check_input_condition(i)
            return i
        except AssertionError:
            continue
    raise AssertionError(f"no seed meets the input condition at Aa {Aa}, m {m}")


# ---------------------------------------------------------------------------------------------------- checkpoint
TAG_GAUSS_SD, F_GAUSS_SD, GAUSS_SD_BYTES = 10, 32, 16


def pack_section(ls_min, ls_max):
    """the optional section's payload: u32 1, u32 0, f32 ls_min, f32 ls_max"""
    return struct.pack("<IIff", 1, 0, ls_min, ls_max)
