"""The squashed (tanh) Gaussian policy (ppo_set_action_squashed_gaussian; csrc/ppo_math.h sq_*, csrc/squash.hip) in
float64: head, sampler and both KL estimators.  Everything Gaussian is gauss_sd_ref's and the normals are rng_ref's;
only the new terms are restated.  The inputs are gauss_sd_ref's head inputs moved over (squashed).

Bounds, derived as gauss_sd_ref.head_bounds derives its own, nothing fitted to a run.  U = 2⁻²⁴ is one fp32 rounding, a
k-ulp function counts 2k·U relative: gauss_sd_ref's expf 2 ulp, and the OpenCL limits log1pf 2 ulp, tanhf 5 ulp.
  ldj(x)  t = expf(−|2x|): 4U·t; l = log1pf(t): the argument's error (slope <= 1) + 4U·l; s = max + l, ln2 − x (and
          the constant's own rounding), their difference: one U each on its result; the factor 2 is exact.
  ε       test_gpu_rng.py's rule: four times what numpy's fp32 Box–Muller misses the float64 one by, at least 4 ulp of
          the largest draw.   q = expf(ls)·ε: ε's error·e^ls + 5U·|q|.   u′ = μ + q: q's error + U·|u′|.
  ldj(u′) its own error + |ldj′| = 2|tanh u′| <= 2 times u′'s.   tanhf(u′): 10U·|th| + (1 − th²)·u′'s error.
  lp      gauss_sd_ref's lp bound at u + Σ_j ldj's + Aa fp32 additions of J + the final subtraction.
  H       gauss_sd_ref's H bound + Σ_j ldj(u′)'s + Aa additions + the final addition.
  grad    mean half: gauss_sd_ref's bound under lp's new error + cm·2·th's error + 3U on the term + U on the sum;
          log-σ half: likewise, the term T = cm·(1 − 2·th·q): cm·2·(th's error·|q| + |th|·q's error) + 4U·cm·(1 + 2|th·q|).
A clamped column's bound is 0."""
import numpy as np

import gauss_sd_ref as sd
import rng_ref
from gauss_sd_ref import F32, F64, U

U64 = np.uint64


def ldj(x):
    return 2 * ((np.log(2.0) - x) - np.logaddexp(0.0, -2 * x))


def ldj_bound(x):
    t, a = np.exp(-np.abs(2 * x)), np.abs(np.log(2.0) - x)
    s = np.maximum(-2 * x, 0) + np.log1p(t)
    return 2 * (4 * U * t + 4 * U * np.log1p(t) + U * s + U * (a + 0.7) + U * np.abs(ldj(x)) / 2)


def normals(m, Aa, key, offset):
    """rng_ref's normals at counter i·Aa + j and the device's tolerance on one of them (the rule above)"""
    cnt = np.arange(m, dtype=U64)[:, None] * U64(Aa) + np.arange(Aa, dtype=U64)[None, :]
    n, n32 = (rng_ref.normal_at(cnt, U64(offset), U64(key), t) for t in (F64, F32))
    return n, max(4.0 * float(np.abs(n32.astype(F64) - n).max()), 4.0 * float(np.spacing(F32(np.abs(n).max()))))


def squashed(i):
    """gauss_sd_ref's inputs moved over: the action half into the u columns, a = tanh(u), old shifted by −J — the
    ratios stay the ones gauss_sd_ref.check_input_condition accepts (up to old's fp32 rounding)"""
    u = i["act"][:, :i["z"].shape[1] // 2]
    act = np.concatenate([np.tanh(u.astype(F64)).astype(F32), u], axis=1)
    old = (i["old"].astype(F64) - ldj(u.astype(F64)).sum(axis=1)).astype(F32)
    return dict(z=i["z"], act=act, adv=i["adv"], old=old)


def head_f64(z, act, adv, old, eps, ent, lo, hi, key, offset):
    """the definition and its bounds b_*; the Gaussian terms: gauss_sd_ref at u, old + J for old (the same ratio), ent 0"""
    m, A = z.shape
    Aa, cm = A // 2, ent / m
    u, mu = np.asarray(act, F64)[:, Aa:], np.asarray(z, F64)[:, :Aa]
    J = ldj(u).sum(axis=1)
    args = (z, u, adv, np.asarray(old, F64) + J, eps, 0.0, lo, hi)
    r, b = sd.head_f64(*args), sd.head_bounds(*args)
    e, e_tol = normals(m, Aa, key, offset)
    q = np.exp(r["ls"]) * e
    up, th = mu + q, np.tanh(mu + q)
    b_q = e_tol * np.exp(r["ls"]) + 5 * U * np.abs(q)
    b_up = b_q + U * np.abs(up)
    b_th = 10 * U * np.abs(th) + (1 - th * th) * b_up
    Jp = ldj(up).sum(axis=1)
    sums = lambda v: Aa * U * np.abs(np.cumsum(v, axis=1)).max(axis=1)                   # noqa: E731
    out = dict(r, lp=r["lp"] - J, H=r["H"] + Jp, e=e, up=up)
    out["b_lp"] = b["lp"] + ldj_bound(u).sum(axis=1) + sums(ldj(u)) + U * np.abs(out["lp"])
    out["b_H"] = b["H"] + (ldj_bound(up) + 2 * b_up).sum(axis=1) + sums(ldj(up)) + U * np.abs(out["H"])
    rel = (out["b_lp"] + 14 * U)[:, None]
    dlp = np.abs(r["dlp"])[:, None]
    d, e2 = u - mu, np.exp(-2 * r["ls"])
    g_mu, t_mu = r["grad"][:, :Aa], cm * 2 * th
    g_ls, t_ls = r["grad"][:, Aa:], np.where(r["inside"], cm * (1 - 2 * th * q), 0.0)
    mag = (1 + d * d * e2) * dlp
    b_mu = np.abs(g_mu) * rel + cm * 2 * b_th + 3 * U * np.abs(t_mu) + U * np.abs(g_mu + t_mu)
    b_ls = (mag * (rel + 2 * U) + cm * 2 * (b_th * np.abs(q) + np.abs(th) * b_q) + 4 * U * cm * (1 + 2 * np.abs(th * q))
            + U * np.abs(g_ls - t_ls))
    out["grad"] = np.concatenate([g_mu + t_mu, g_ls - t_ls], axis=1)
    out["b_grad"] = np.concatenate([b_mu, np.where(r["inside"], b_ls, 0.0)], axis=1)
    out["loss"] = -r["sur"].sum() / m - ent * out["H"].sum() / m
    out["b_loss"] = sd.loss_bound(out, dict(rel=rel[:, 0], H=out["b_H"]), m, ent)
    return out


def sample_f64(z, lo, hi, key, offset):
    """u = μ + normal·e^ls and its bound (test_gpu_gauss_sd.py's: the normal, a 2-ulp expf, the product, the sum)"""
    Aa = z.shape[1] // 2
    n, n_tol = normals(z.shape[0], Aa, key, offset)
    ls = sd.clamp(z[:, Aa:].astype(F64), lo, hi)[0]
    u = z[:, :Aa].astype(F64) + n * np.exp(ls)
    return u, (n_tol + 8 * U * np.abs(n)) * np.exp(ls) + 2 * U * np.abs(u)


def kl_f64(z_new, z_old, act, old_lp, eps, lo, hi):
    """k3 (x carries lp's error Δ: a term moves by (|expm1 x| + Δ)·Δ), the clip fraction, the base Gaussians' row KL"""
    m = z_new.shape[0]
    r = head_f64(z_new, act, np.ones(m), old_lp, eps, 0.0, lo, hi, 0, 0)
    x, dx = r["lp"] - np.asarray(old_lp, F64), r["b_lp"]
    return dict(x=x, k3=(np.expm1(x) - x).mean(), b_k3=((np.abs(np.expm1(x)) + dx) * dx).mean(),
                clip=float((np.abs(np.expm1(x)) > eps).sum()) / m, rows=sd.kl_rows_f64(z_old, z_new, lo, hi))
