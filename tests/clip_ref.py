"""The float64 reference of global gradient-norm clipping (torch.nn.utils.clip_grad_norm_'s formula)."""
import numpy as np


def clip_grad_norm(grads, max_norm, grad_scale=1.0):
    """norm = grad_scale·sqrt(Σ g²) over every array of `grads` jointly (float64);
    coef = min(1, max_norm / (norm + 1e-6)).  Returns (norm, coef, [grad_scale·coef·g] as float64)."""
    total = sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads)
    norm = float(grad_scale) * float(np.sqrt(total))
    coef = min(1.0, float(max_norm) / (norm + 1e-6))
    return norm, coef, [np.asarray(g, np.float64) * (float(grad_scale) * coef) for g in grads]
