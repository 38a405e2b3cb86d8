"""Running observation normalisation (ppo_ext.h ppo_set_obs_norm): a numpy reference.

A triple is a float64 array {n, mean[S], M2[S]} of 1 + 2S entries, the layout ppo_obs_norm_get_state and
ppo_obs_stats_device use.  stats64 is exact (two passes of math.fsum), chan is Chan et al.'s pairwise combine as
csrc/obsnorm.hip applies it, and normalize_f32 mirrors the device expression operation for operation in np.float32,
so it is bit-comparable with the kernels (built with -ffp-contract=off)."""
import math

import numpy as np

F32 = np.float32


def stats64(x):
    """The exact triple of the rows x [n, S]: mean by fsum, M2 = fsum((x − mean)²), per column."""
    x = np.asarray(x, np.float64)
    n, S = x.shape
    out = np.zeros(1 + 2 * S)
    out[0] = n
    if n == 0:
        return out
    for j in range(S):
        col = x[:, j]
        mean = math.fsum(col.tolist()) / n
        out[1 + j] = mean
        out[1 + S + j] = math.fsum(((col - mean) ** 2).tolist())
    return out


def chan(a, b):
    """a ⊕ b for two triples; an empty side leaves the other as it is."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    S = (a.size - 1) // 2
    na, nb = a[0], b[0]
    if not nb > 0:
        return a.copy()
    if not na > 0:
        return b.copy()
    n = na + nb
    delta = b[1:1 + S] - a[1:1 + S]
    out = np.empty_like(a)
    out[0] = n
    out[1:1 + S] = a[1:1 + S] + delta * (nb / n)
    out[1 + S:] = (a[1 + S:] + b[1 + S:]) + delta * delta * (na * (nb / n))
    return out


def affine(triple):
    """The fp32 pair (m, r) of a triple: m = fp32(mean), r = fp32(1/sqrt(M2/n + 1e-8)); n = 0: (0, 1)."""
    t = np.asarray(triple, np.float64)
    S = (t.size - 1) // 2
    if not t[0] > 0:
        return np.zeros(S, F32), np.ones(S, F32)
    return t[1:1 + S].astype(F32), (1.0 / np.sqrt(t[1 + S:] / t[0] + 1e-8)).astype(F32)


def normalize_f32(x, m, r, c):
    """(y, clamped mask) of t = (x − m)·r, y = t < −c ? −c : (t > c ? c : t), every operation in np.float32;
    an element is clamped when y != t and t is not NaN."""
    x, m, r = np.ascontiguousarray(x, F32), np.asarray(m, F32), np.asarray(r, F32)
    c = F32(c)
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((x - m).astype(F32) * r).astype(F32)
        y = np.where(t < -c, -c, np.where(t > c, c, t)).astype(F32)
        clamped = (y != t) & ~np.isnan(t)
    return y, clamped
