"""float64 numpy reference of the update's policy-drift statistics (csrc/kl.hip), pinned against torch in
test_kl_cpu.py."""
import numpy as np


def approx_kl(lp, old_lp):
    """mean(expm1(x) − x), x = lp − old_lp: Schulman's k3 estimator, as Stable-Baselines3 computes it."""
    x = np.asarray(lp, np.float64) - np.asarray(old_lp, np.float64)
    return float(np.mean(np.expm1(x) - x))


def clip_fraction(lp, old_lp, eps):
    """mean(|exp(x) − 1| > eps)."""
    x = np.asarray(lp, np.float64) - np.asarray(old_lp, np.float64)
    return float(np.mean(np.abs(np.exp(x) - 1.0) > eps))
