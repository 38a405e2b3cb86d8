"""The numpy KL / clip-fraction helpers the GPU target-KL tests use as their reference equal torch's
expressions (Stable-Baselines3: approx_kl = mean((exp(x) − 1) − x), clip_fraction = mean(|ratio − 1| > ε))."""
import numpy as np
import pytest
import torch

from kl_ref import approx_kl, clip_fraction


@pytest.mark.parametrize("scale", [1e-4, 0.05, 0.5])
def test_numpy_kl_matches_torch(scale):
    rng = np.random.default_rng(9)
    old = rng.normal(scale=3.0, size=4097)
    lp = old + rng.normal(scale=scale, size=old.size)
    x = torch.tensor(lp, dtype=torch.float64) - torch.tensor(old, dtype=torch.float64)
    want = float((torch.exp(x) - 1 - x).mean())
    got = approx_kl(lp, old)
    # torch's (exp(x) − 1) − x cancels where expm1 does not: each term is within 2.2e-16 absolute of the
    # exact one, so the means agree to a few 1e-16 whatever the scale
    assert got > 0 and abs(got - want) <= 1e-15 + 1e-12 * want
    for eps in (0.05, 0.2):
        want_f = float(((torch.exp(x) - 1).abs() > eps).to(torch.float64).mean())
        assert clip_fraction(lp, old, eps) == want_f


def test_kl_zero_and_float32_inputs():
    lp = np.linspace(-5, 5, 33, dtype=np.float32)
    assert approx_kl(lp, lp) == 0.0 and clip_fraction(lp, lp, 0.2) == 0.0
    # float32 inputs are widened before the subtraction
    old = (lp + np.float32(0.1)).astype(np.float32)
    x = lp.astype(np.float64) - old.astype(np.float64)
    assert approx_kl(lp, old) == float(np.mean(np.expm1(x) - x))
