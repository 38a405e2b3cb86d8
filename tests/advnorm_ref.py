"""Per-minibatch advantage normalisation in numpy: the definition of ppo.c_amd/csrc/advnorm.h restated operation by
operation (ppo_ext.h ppo_set_adv_norm quotes it), so that the device kernel can be held against it bit for bit.

A segment x_0 … x_{B−1} of float32 becomes

    p_t  = Σ_{i ≡ t (mod 256), i ascending} (double)x_i          t = 0 … 255
    S    = pairwise tree over p (stride 1, 2, 4 … 128: p_t += p_{t+stride} for t a multiple of 2·stride)
    mean = S / B                                                  (double)
    q_t, Q likewise over d_i·d_i,  d_i = (double)x_i − mean       (product rounded, then added)
    sd   = (float)sqrt(Q / max(B − 1, 1))
    m    = (float)mean
    y_i  = (float)((double)(x_i − m) / ((double)sd + 1e-8))       (x_i − m an fp32 difference)

numpy's float64 / float32 add, subtract, multiply, divide and sqrt are IEEE round-to-nearest, one rounding each, and
nothing here is written so that numpy could fuse a product into a sum.
"""
import numpy as np

F32, F64 = np.float32, np.float64
LANES = 256


def _lane_tree(v):
    """Σ v by advnorm.h's order: v float64 [B] → lane partials (element i to lane i % 256, ascending), then the tree"""
    B = v.shape[0]
    rounds = -(-B // LANES)
    padded = np.zeros(rounds * LANES, F64)
    padded[:B] = v
    padded = padded.reshape(rounds, LANES)
    # a lane with fewer elements than `rounds` must not add the padding's +0.0 (it would turn a −0.0 partial into
    # +0.0, which the kernel's guarded add does not): add row k only where it holds an element
    p = np.zeros(LANES, F64)
    for k in range(rounds):
        n = min(LANES, B - k * LANES)
        p[:n] = p[:n] + padded[k, :n]
    stride = 1
    while stride < LANES:
        idx = np.arange(0, LANES, 2 * stride)
        p[idx] = p[idx] + p[idx + stride]
        stride *= 2
    return p[0]


def normalize_segment(x):
    """x float32 [B] → (y float32 [B], m float32, sd float32)"""
    x = np.ascontiguousarray(x, F32)
    B = x.shape[0]
    assert B >= 1
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xd = x.astype(F64)
        mean = _lane_tree(xd) / F64(B)
        d = xd - mean
        Q = _lane_tree(d * d)
        sd = F32(np.sqrt(Q / F64(max(B - 1, 1))))
        m = F32(mean)
        den = F64(sd) + F64(1e-8)
        y = ((x - m).astype(F64) / den).astype(F32)
    return y, m, sd


def normalize(x, B):
    """x float32 [n_seg·B] (or [n_seg, B]) → (y like x, stats float32 [n_seg, 2] = (m, sd))"""
    x = np.ascontiguousarray(x, F32)
    segs = x.reshape(-1, B)
    y = np.empty_like(segs)
    stats = np.empty((segs.shape[0], 2), F32)
    for s in range(segs.shape[0]):
        y[s], stats[s, 0], stats[s, 1] = normalize_segment(segs[s])
    return y.reshape(x.shape), stats
