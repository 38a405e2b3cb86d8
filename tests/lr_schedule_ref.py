"""The learning-rate schedules of ppo_set_lr_schedule as a numpy model (include/ppo_ext.h states them).

Everything the device does in fp32 is done here in np.float32 operations, one IEEE operation per line of the rule —
no float64 shortcut: lr / 1.5f and lr · 1.5f are each one correctly rounded fp32 operation, as on the device.  Only the
linear formula is in double, rounded to fp32 once, as the host does it.
"""
import numpy as np

F32 = np.float32
CONSTANT, LINEAR, ADAPTIVE = 0, 1, 2
UP = F32(1.5)


def clamp(x, lo, hi):
    return np.minimum(F32(hi), np.maximum(F32(lo), F32(x)))


def adapt_step(lr, kl, desired_kl, lr_min, lr_max):
    """one decided policy step: (new lr, raised, lowered)"""
    lr, kl, want = F32(lr), F32(kl), F32(desired_kl)
    if kl > F32(2.0) * want:
        return np.maximum(F32(lr_min), lr / UP), 0, 1
    if kl < F32(0.5) * want and kl > F32(0.0):
        return np.minimum(F32(lr_max), lr * UP), 1, 0
    return lr, 0, 0                         # the dead band, kl == 0, a NaN kl


def replay(lr0, kls, desired_kl, lr_min, lr_max, stop_step=-1):
    """The rule over one update's KL history from the rate lr0: the rate each step's Adam used (lr_hist), the final
    rate and the two counters.  stop_step >= 0: target-KL early stopping tripped at that step — the step itself
    still adapts (the rule runs before the stop test), every later one leaves the rate alone."""
    lr, hist, raised, lowered = F32(lr0), [], 0, 0
    for k, kl in enumerate(kls):
        if stop_step < 0 or k <= stop_step:
            lr, r, l = adapt_step(lr, kl, desired_kl, lr_min, lr_max)
            raised += r
            lowered += l
        hist.append(lr)
    return np.array(hist, F32), F32(lr), raised, lowered


def initial_lr(lr_policy, lr_min, lr_max):
    return clamp(lr_policy, lr_min, lr_max)


def coupled_value_lr(lr_V, lr, lr_policy, lr_min, lr_max):
    """lr_v = lr_V · (lr / clamp(lr_policy, lr_min, lr_max)): one fp32 division, one fp32 product"""
    ratio = F32(lr) / clamp(lr_policy, lr_min, lr_max)
    assert ratio.dtype == F32
    return F32(lr_V) * ratio


def linear_lr(base, u, N, f):
    """(float)((double)base · (1 − (1 − f)·(min(u, N)/N))): double, the quotient first (u >= N then gives base · f
    exactly), rounded once; base, N and f are the fp32 values the setter received"""
    base, N, f = float(F32(base)), float(F32(N)), float(F32(f))
    return F32(base * (1.0 - (1.0 - f) * (min(float(u), N) / N)))


def steps_to_floor(lr0, lr_min):
    """lowerings from lr0 until the rate sits at lr_min, by running the fp32 rule (kl above the band every step)"""
    lr, n = F32(lr0), 0
    while lr != F32(lr_min):
        lr = adapt_step(lr, 1.0, 1e-3, lr_min, 1.0)[0]
        n += 1
        assert n < 1000
    return n
