"""layernorm_ref.py on the CPU (numpy only): its backward against a central finite difference of its forward, and its
two fp32 bounds against the float32 restatement of the stated arithmetic in two sum orders."""
import numpy as np
import pytest

import layernorm_ref as R

F64 = np.float64
EPS = 1e-5


@pytest.mark.parametrize("act", ["none", "relu", "tanh", "elu"])
def test_backward_is_the_derivative_of_forward(act):
    rng = np.random.default_rng(7)
    z, g = rng.normal(size=(3, 11)), rng.uniform(-1, 1, (3, 11))
    h = R.forward(z, EPS, act)[0]
    dz = R.backward(g, z, h, EPS, act)[0]
    fd, step = np.empty_like(z), 1e-6
    for i, j in np.ndindex(*z.shape):
        e = np.zeros_like(z)
        e[i, j] = step
        fd[i, j] = ((R.forward(z + e, EPS, act)[0] - R.forward(z - e, EPS, act)[0]) * g).sum() / (2 * step)
    assert np.abs(dz - fd).max() <= 1e-8 * max(1.0, np.abs(dz).max())


@pytest.mark.parametrize("pairwise", [False, True])
@pytest.mark.parametrize("l", [3, 72, 1030])
def test_bounds_hold_for_the_fp32_restatement(l, pairwise):
    z, g = R.crafted(9, l, l)
    for act in ("relu", "tanh"):
        h, mean, r, dz = R.f32_model(z, g, EPS, act, pairwise)
        h_ref, mean_ref, r_ref, _ = R.forward(z, EPS, act)
        tf, tm, tr = R.tol_fwd(z, EPS)
        assert (np.abs(h - h_ref) <= tf).all() and (np.abs(mean - mean_ref) <= tm).all()
        assert (np.abs(r - r_ref) <= tr).all()
        assert (np.abs(dz - R.backward(g, z, h, EPS, act)[0]) <= R.tol_bwd(g, z, h, EPS, act)).all()
    # the bounds are sharp where it matters: an unbiased variance or another eps is far outside tol_fwd
    if l == 72:
        zz = z.astype(F64)
        d = zz - zz.mean(axis=1, keepdims=True)
        for var, e in (((d * d).sum(axis=1) / (l - 1), EPS), ((d * d).mean(axis=1), 1e-6)):
            wrong = d / np.sqrt(var + e)[:, None]
            assert (np.abs(wrong - R.forward(z, EPS, "none")[0]) / R.tol_fwd(z, EPS)[0]).max() > 100
