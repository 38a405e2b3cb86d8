"""Running return-based reward normalisation (ppo_ext.h ppo_set_reward_norm): a numpy reference.

returns64 is the sequential float64 evaluation of the recurrence of ppo_ext.h,
    k_i = !(term_i or trunc_i)   (k_{-1} = 0),      R_i = r_i + g·(k_{i-1}·R_{i-1} + c_i),
with g = float64(float32(gamma)) and c_i = carry_in[e] at row e·seg_len (seg_len = 0: no carry).  The triple and
the scale are obsnorm_ref's stats64 / chan / affine with S = 1, the scaling is its normalize_f32 with m = 0
((x − 0)·s is x·s exactly, so it stays bit-comparable with the kernel)."""
import numpy as np

from obsnorm_ref import F32, affine, chan, normalize_f32, stats64


def returns64(r, term, trunc, g, seg_len=0, carry_in=None, cont=None):
    """(R [n] float64, carry_out [n / seg_len] float64 or None): carry_out[e] = cont[e] ? R[e·T + T − 1] : 0."""
    r = np.asarray(r, F32).astype(np.float64)
    end = np.asarray(term, bool) | np.asarray(trunc, bool)
    n = r.size
    g = float(np.float64(F32(g)))
    assert seg_len == 0 or n % seg_len == 0
    R = np.empty(n)
    prev, keep = 0.0, 0.0
    for i in range(n):
        c = float(carry_in[i // seg_len]) if seg_len and i % seg_len == 0 else 0.0
        prev = float(r[i]) + g * (keep * prev + c)
        R[i] = prev
        keep = 0.0 if end[i] else 1.0
    carry_out = None
    if seg_len and cont is not None:
        carry_out = np.where(np.asarray(cont, bool), R[seg_len - 1::seg_len], 0.0)
    return R, carry_out


def bound(r, term, trunc, g, seg_len=0, carry_in=None):
    """The per-row accuracy bound 4(L_i + 2)·2^-53·G_i between two float64 evaluations of the recurrence in any
    composition order: L_i is the distance of row i from the start of its chain, a carried start counting as one
    more, and G_i the same recurrence over |r| and |carry|.  Each evaluation is within 2(L_i + 2)·2^-53·G_i of
    the exact value: every term passes through at most L_i + 1 multiplications and additions."""
    r = np.abs(np.asarray(r, F32).astype(np.float64))
    end = np.asarray(term, bool) | np.asarray(trunc, bool)
    n = r.size
    g = float(np.float64(F32(g)))
    L, G = np.empty(n), np.empty(n)
    l, gsum, keep = 0.0, 0.0, 0.0
    for i in range(n):
        c = abs(float(carry_in[i // seg_len])) if seg_len and i % seg_len == 0 else 0.0
        l = keep * (l + 1.0)
        if c != 0.0:
            l += 1.0
        gsum = float(r[i]) + g * (keep * gsum + c)
        L[i], G[i] = l, gsum
        keep = 0.0 if end[i] else 1.0
    return 4.0 * (L + 2.0) * 2.0 ** -53 * G


def triple64(R):
    """The exact triple {n, mean, M2} of the returns R (stats64 with S = 1)."""
    return stats64(np.asarray(R, np.float64).reshape(-1, 1))


def scale_of(triple):
    """The fp32 scale s = fp32(1/sqrt(M2/n + 1e-8)) of a triple; n = 0: 1."""
    return affine(triple)[1][0]


def scale_f32(r, s, c):
    """(y, clamped mask) of t = r·s, y = clamp(t, ±c) in np.float32 (normalize_f32 with m = 0)."""
    r = np.ascontiguousarray(r, F32)
    y, cl = normalize_f32(r.reshape(-1, 1), np.zeros(1, F32), np.full(1, s, F32), c)
    return y.reshape(r.shape), cl.reshape(r.shape)


__all__ = ["F32", "returns64", "bound", "triple64", "scale_of", "scale_f32", "chan", "stats64", "affine", "normalize_f32"]
