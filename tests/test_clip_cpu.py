"""The numpy clip helper the GPU clipping tests use as their reference equals torch's clip_grad_norm_."""
import numpy as np
import pytest
import torch

from clip_ref import clip_grad_norm

SHAPES = [(7, 5), (11,), (3, 2, 2)]


def _case(kind):
    rng = np.random.default_rng(5)
    if kind == "above":          # norm ≈ sqrt(50)·3 ≫ max_norm
        return [rng.normal(scale=3.0, size=s) for s in SHAPES], 0.5
    if kind == "below":          # norm ≈ 0.07 < max_norm: coef clamps to 1
        return [rng.normal(scale=0.01, size=s) for s in SHAPES], 0.5
    return [np.zeros(s) for s in SHAPES], 0.5


@pytest.mark.parametrize("kind", ["above", "below", "zero"])
def test_numpy_clip_matches_torch(kind):
    grads, max_norm = _case(kind)
    params = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = torch.tensor(g, dtype=torch.float64)
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    norm, coef, clipped = clip_grad_norm(grads, max_norm)
    assert abs(norm - total) <= 1e-6 * total
    if kind == "above":
        assert coef < 0.1
        # the 1e-6 in the denominator is part of the formula: without it the coefficient differs visibly
        assert abs(coef - max_norm / (total + 1e-6)) <= 1e-15
    else:
        assert coef == 1.0
    for p, c in zip(params, clipped):
        np.testing.assert_allclose(p.grad.numpy(), c, rtol=1e-6, atol=0)
