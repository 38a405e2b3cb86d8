"""float64 numpy model of the closed-form KL(old ‖ new) of the KL monitor (ppo_ext.h ppo_set_kl_estimator,
PPO_KL_EXACT; csrc/ppo_math.h kl_gauss_row / kl_cat_row) — an independent restatement: fp32 inputs widened to
float64, every operation in float64, j / k / d ascending.

Every function returns (kl, mag) per row: the row's KL and Σ|term| of the row, the scale the kernel tests compare
against (for a discrete row the terms are exp(lo_k)·(lo_k − ln_k), before the clamp at 0).
"""
import numpy as np

F64 = np.float64


def gaussian(mu_old, ls_old, mu_new, ls_new):
    """mu_* [m, A], ls_* [A] → (kl [m], mag [m])"""
    mo, mn = np.asarray(mu_old, F64), np.asarray(mu_new, F64)
    lo, ln = np.asarray(ls_old, F64), np.asarray(ls_new, F64)
    m, A = mo.shape
    kl, mag = np.zeros(m), np.zeros(m)
    for j in range(A):
        d = lo[j] - ln[j]
        dm = mo[:, j] - mn[:, j]
        term = (0.5 * np.expm1(2.0 * d) - d) + 0.5 * (dm * dm) * np.exp(-2.0 * ln[j])
        kl = kl + term
        mag = mag + np.abs(term)
    return kl, mag


def effective_mask(bits, n, chosen):
    """the three rules of ppo_set_action_mask for one component: bits [n] bool (None: unmasked) → [n] bool"""
    if bits is None:
        return np.ones(n, bool)
    eff = np.array(bits, bool)
    if not eff.any():
        eff[:] = True
    if chosen is not None:
        eff[min(max(int(chosen), 0), n - 1)] = True
    return eff


def component(zo, zn, allowed):
    """one component of one row: zo, zn [n], allowed [n] bool → (KL_d, Σ|term|).  Only the allowed columns are read."""
    idx = np.flatnonzero(allowed)
    a, b = np.asarray(zo)[idx].astype(F64), np.asarray(zn)[idx].astype(F64)
    Mo, Mn = a.max(), b.max()
    so = sn = 0.0
    for k in range(idx.size):
        so += np.exp(a[k] - Mo)
        sn += np.exp(b[k] - Mn)
    lso, lsn = np.log(so), np.log(sn)
    s = mag = 0.0
    for k in range(idx.size):
        lo, ln = (a[k] - Mo) - lso, (b[k] - Mn) - lsn
        t = np.exp(lo) * (lo - ln)
        s += t
        mag += abs(t)
    return (0.0 if s < 0 else s), mag


def unpack_mask(words, A):
    """[m, W] uint32 → [m, A] bool: bit k & 31 of word k >> 5 = column k allowed"""
    w = np.asarray(words, np.uint32)
    k = np.arange(A)
    return ((w[:, k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(bool)


def pack_mask(allowed):
    """[m, A] bool → [m, W] uint32"""
    allowed = np.asarray(allowed, bool)
    m, A = allowed.shape
    out = np.zeros((m, (A + 31) // 32), np.uint32)
    for k in range(A):
        out[:, k >> 5] |= allowed[:, k].astype(np.uint32) << np.uint32(k & 31)
    return out


def discrete(z_old, z_new, nvec, mask=None, action=None):
    """z_* [m, A] logits, nvec the component widths (Σ = A; the categorical policy: [A]); mask [m, A] bool or None;
    action [m, ≥D] the chosen indices (needed under a mask: rule 3) → (kl [m], mag [m])"""
    zo, zn = np.asarray(z_old), np.asarray(z_new)
    m, A = zo.shape
    assert sum(nvec) == A
    kl, mag = np.zeros(m), np.zeros(m)
    for i in range(m):
        o = 0
        for d, n in enumerate(nvec):
            bits = None if mask is None else mask[i, o:o + n]
            chosen = None if mask is None or action is None else action[i, d]
            eff = effective_mask(bits, n, chosen)
            k, g = component(zo[i, o:o + n], zn[i, o:o + n], eff)
            kl[i] += k
            mag[i] += g
            o += n
    return kl, mag
