"""The float64 tanh-network model of tanh_ref.py, pinned on the CPU (no GPU, no libppo):

  * its backward against a central finite difference of its own forward, for a pure tanh network, a mixed
    relu / tanh one and a tanh output layer;
  * the fp32 statement of tanh′ the kernels use, gx = acc − (acc·h)·h, against the float64 acc·(1 − h²) at
    h = 0, ±1, within an ulp of ±1, NaN, and over random operands.

The bound of the fp32 statement, derived: with u = 2⁻²⁴, t1 = fl(acc·h) = acc·h·(1 + d1), t2 = fl(t1·h) =
acc·h²·(1 + d1)(1 + d2), gx = fl(acc − t2) = (acc − t2)(1 + d3), |d_i| ≤ u.  So
|gx − acc(1 − h²)| ≤ |acc|·h²·(2u + u²) + u·|acc − t2| ≤ |acc|·(3u + 2u²) for |h| ≤ 1 — an error relative to the
PRODUCT acc, not to the result (near h = ±1 the result is ~2u·|acc| and carries no correct digit; the GEMM bound
the GPU tests use, helpers.gemm_tol of the product, is relative to max|acc| and 3u sits far inside it)."""
import numpy as np
import pytest

import tanh_ref as T

F32, F64 = np.float32, np.float64
U = 2.0 ** -24


def _loss(sizes, acts, params, x, w):
    """A scalar of the output with a fixed random weighting, float64."""
    hs, _ = T.forward(sizes, acts, params, x)
    return float((hs[-1] * w).sum())


@pytest.mark.parametrize("acts", [["tanh", "tanh", "none"], ["relu", "tanh", "none"], ["tanh", "relu", "tanh"]])
def test_backward_matches_central_difference(acts):
    sizes, m = [5, 7, 6, 3], 9
    rng = np.random.default_rng(11)
    params = rng.uniform(-0.8, 0.8, T.num_params(sizes))
    x = rng.uniform(-1, 1, (m, sizes[0]))
    w = rng.normal(size=(m, sizes[-1]))
    hs, zs = T.forward(sizes, acts, params, x)
    # keep every ReLU pre-activation away from its kink, where a finite difference is meaningless
    for z, a in zip(zs, acts):
        if a == "relu":
            assert np.abs(z).min() > 1e-4
    g, gx0 = T.backward(sizes, acts, params, hs, w)
    eps = 1e-6
    num = np.empty_like(params)
    for i in range(params.size):
        p = params.copy()
        p[i] += eps
        up = _loss(sizes, acts, p, x, w)
        p[i] -= 2 * eps
        num[i] = (up - _loss(sizes, acts, p, x, w)) / (2 * eps)
    # central difference: truncation O(eps²·f‴) ≈ 1e-12, rounding O(2⁻⁵³·|f|/eps) ≈ 1e-9 for |f| ~ 10
    np.testing.assert_allclose(g, num, rtol=1e-6, atol=2e-8)
    numx = np.empty_like(x)
    for idx in np.ndindex(*x.shape):
        xp = x.copy()
        xp[idx] += eps
        up = _loss(sizes, acts, params, xp, w)
        xp[idx] -= 2 * eps
        numx[idx] = (up - _loss(sizes, acts, params, xp, w)) / (2 * eps)
    np.testing.assert_allclose(gx0, numx, rtol=1e-6, atol=2e-8)


def test_tanh_bwd_fp32_special_values():
    one = F32(1.0)
    below, above = np.nextafter(one, F32(0)), np.nextafter(one, F32(2))
    acc = np.array([0.0, 1.0, -3.25, 1e-30, 6.5e4, -1e-3], F32)
    for h in (F32(0), one, -one):
        got = T.tanh_bwd_f32(acc, np.full_like(acc, h))
        want = acc if h == 0 else np.zeros_like(acc)
        np.testing.assert_array_equal(got, want)               # h = 0: acc exactly; h = ±1: exactly 0
        assert got.dtype == F32
    for h in (below, -below, above, -above):                   # within an ulp of ±1
        hv = np.full_like(acc, h)
        got = T.tanh_bwd_f32(acc, hv).astype(F64)
        ref = T.tanh_bwd_f64(acc, hv)
        assert np.isfinite(got).all()
        assert (np.abs(got - ref) <= np.abs(acc.astype(F64)) * (3 * U + 2 * U * U) * float(h) ** 2 + 1e-45).all()
    # NaN propagates from either operand, whatever the other holds
    nan = F32(np.nan)
    assert np.isnan(T.tanh_bwd_f32(acc, np.full_like(acc, nan))).all()
    assert np.isnan(T.tanh_bwd_f32(np.full_like(acc, nan), np.array([0, 1, -1, 0.5, below, above], F32))).all()
    assert np.isnan(T.tanh_bwd_f64(acc, np.full_like(acc, nan))).all()


def test_tanh_bwd_fp32_random_within_bound():
    rng = np.random.default_rng(5)
    acc = (rng.normal(size=200000) * np.exp(rng.uniform(-20, 20, 200000))).astype(F32)
    h = np.tanh(rng.normal(scale=3.0, size=200000)).astype(F32)       # many values rounding to ±1
    assert (np.abs(h) == 1).any() and (np.abs(h) < 1).any()
    got = T.tanh_bwd_f32(acc, h).astype(F64)
    ref = T.tanh_bwd_f64(acc, h)
    assert (np.abs(got - ref) <= np.abs(acc.astype(F64)) * (3 * U + 2 * U * U)).all()
    assert (got[np.abs(h) == 1] == 0).all()


def test_activation_of_the_model():
    z = np.array([-2.0, -0.0, 0.0, 0.5, 30.0])
    np.testing.assert_array_equal(T.act_f(z, "none"), z)
    np.testing.assert_array_equal(T.act_f(z, "relu"), [0, 0, 0, 0.5, 30.0])
    np.testing.assert_allclose(T.act_f(z, "tanh"), np.tanh(z), rtol=0, atol=0)
    h = np.tanh(z)
    np.testing.assert_allclose(T.act_bwd(np.ones(5), h, "tanh"), 1 / np.cosh(z) ** 2, rtol=1e-12, atol=1e-16)
