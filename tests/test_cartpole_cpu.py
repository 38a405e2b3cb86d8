"""One CartPole-v1 step: the float64 model against gymnasium's published equations at a hand-checked point, and the
fp32 mirror of csrc/rollout.hip cartpole_advance inside the bound the GPU test uses (tests/categorical_ref.py)."""
import numpy as np

import categorical_ref as cr
from categorical_ref import F32, F64


def states(n, seed=3):
    rng = np.random.default_rng(seed)
    s = np.stack([rng.uniform(-2.4, 2.4, n), rng.uniform(-3, 3, n), rng.uniform(-0.21, 0.21, n),
                  rng.uniform(-3.5, 3.5, n)], axis=1).astype(F32)
    s[0] = 0                                               # the upright rest state
    return s, rng.integers(0, 2, n)


def test_model_at_rest():
    """From rest a push right gives temp = 10/1.1, θ̈ = −temp/(0.5·(4/3 − 0.1/1.1)), ẍ = temp − 0.05·θ̈/1.1, and only
    the velocities move in the first Euler step."""
    nxt, term = cr.cartpole_f64(np.zeros((2, 4)), np.array([1, 0]))
    temp = 10 / 1.1
    thacc = -temp / (0.5 * (4 / 3 - 0.1 / 1.1))
    xacc = temp - 0.05 * thacc / 1.1
    np.testing.assert_allclose(nxt[0], [0, 0.02 * xacc, 0, 0.02 * thacc], rtol=1e-15)
    np.testing.assert_allclose(nxt[1], -nxt[0], rtol=1e-15)              # the mirror image under a push left
    assert not term.any()
    assert abs(nxt[0, 1] - 0.1951219512195122) < 1e-15                   # gymnasium's first step from rest


def test_termination_thresholds():
    s = np.array([[2.39, 1.0, 0, 0], [2.37, 1.0, 0, 0], [0, 0, 0.2094, 0.5], [0, 0, 0.19, 0.5], [-2.39, -1.0, 0, 0]])
    _, term = cr.cartpole_f64(s, np.zeros(5, int))
    np.testing.assert_array_equal(term, [True, False, True, False, True])


def test_mirror_within_bounds():
    s, a = states(20000)
    want, term64 = cr.cartpole_f64(s, a)
    got, term32 = cr.cartpole_f32(s, a)
    b = cr.cartpole_bounds(s, a)
    err = np.abs(got.astype(F64) - want)
    ratio = float((err / b).max())
    print(f"mirror next_state error / bound {ratio:.3f}; bound at most {b.max():.3g}")
    assert (err <= b).all(), ratio
    assert b.max() < 2e-5                                   # a rounding bound: ≈ 30 operations on values below 200
    # flags agree wherever the next |x| / |θ| is further than the bound from its threshold; under 1 % are not
    near = ((np.abs(np.abs(want[:, 0]) - cr.X_LIMIT) <= b[:, 0] + cr.LIMIT_SLACK[0])
            | (np.abs(np.abs(want[:, 2]) - cr.TH_LIMIT) <= b[:, 2] + cr.LIMIT_SLACK[1]))
    assert near.mean() < 0.01
    np.testing.assert_array_equal(term32[~near], term64[~near])
    assert term64.any() and not term64.all()
