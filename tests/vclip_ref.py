"""PPO2 value-loss clipping (ppo_ext.h ppo_set_value_clip): the definition in float64, and an fp32 model that
mirrors csrc/vclip.h value_head_row operation for operation (np.float32 arrays only, so it is bit-comparable
with the kernels, which are built with -ffp-contract=off).  Pinned against torch in test_vclip_cpu.py."""
import numpy as np

F32 = np.float32


def vclip_f64(y, t, v_old, eps_v):
    """(loss, g [m], clipped mask [m]) of mean(max((y − t)², (v_old + clamp(y − v_old, ±eps_v) − t)²)) with the
    sub-gradient of ppo_ext.h: an inside row and a row whose unclipped term is >= the clipped one take
    2(y − t)/m, the others 0."""
    y, t, v_old = (np.asarray(a, np.float64) for a in (y, t, v_old))
    m = y.size
    d = y - v_old
    inside = ~(np.abs(d) > eps_v)
    lu = (t - y) ** 2
    lc = (t - (v_old + np.copysign(eps_v, d))) ** 2
    clipped = ~inside & ~(lu >= lc)
    loss = np.where(clipped, lc, lu).sum() / m
    g = np.where(clipped, 0.0, 2 * (y - t) / m)
    return loss, g, clipped


def vclip_f32(y, t, v_old, eps_v):
    """The kernel's arithmetic: (per-row loss terms l [m] fp32, g [m] fp32, clipped mask [m]); the head's loss is
    Σ l / m (the sum's order is the kernel's own: compare it with float(l.astype(np.float64).sum()) / m)."""
    y, t, v_old = (np.ascontiguousarray(a, F32) for a in (y, t, v_old))
    eps = F32(eps_v)
    mf = F32(y.size)
    with np.errstate(invalid="ignore", over="ignore"):
        du = t - y
        lu = du * du
        gu = F32(2) * (y - t) / mf
        d = y - v_old
        outside = np.abs(d) > eps                   # NaN: inside
        yc = v_old + np.copysign(eps, d)
        dc = t - yc
        lc = dc * dc
        clipped = outside & ~(lu >= lc)
    l = np.where(clipped, lc, lu).astype(F32)
    g = np.where(clipped, F32(0), gu).astype(F32)
    return l, g, clipped
