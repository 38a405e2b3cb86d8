"""tests/vclip_ref.py pinned on the CPU: the float64 definition against torch autograd, the fp32 kernel model
against the float64 definition, and the stated edge cases of ppo_ext.h ppo_set_value_clip."""
import numpy as np
import torch

from vclip_ref import F32, vclip_f32, vclip_f64

EPS = 0.2


def _inputs(seed, m):
    """y, t, v_old in float64 with no row within 1e-3 of either decision boundary (|d| = eps, lu = lc)."""
    rng = np.random.default_rng(seed)
    y, t, v_old = rng.normal(size=m), rng.normal(size=m), rng.normal(size=m)
    d = y - v_old
    lu = (t - y) ** 2
    lc = (t - (v_old + np.copysign(EPS, d))) ** 2
    keep = (np.abs(np.abs(d) - EPS) > 1e-3) & (np.abs(lu - lc) > 1e-3)
    return y[keep], t[keep], v_old[keep]


def test_f64_against_torch_autograd():
    y, t, v_old = _inputs(3, 4000)
    d = y - v_old
    lu, lc = (t - y) ** 2, (t - (v_old + np.copysign(EPS, d))) ** 2
    assert (np.abs(np.abs(d) - EPS) > 1e-3).all() and (np.abs(lu - lc) > 1e-3).all() and y.size > 3000
    ty = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    tt, tv = torch.tensor(t), torch.tensor(v_old)
    loss_t = torch.max((ty - tt) ** 2, (tv + torch.clamp(ty - tv, -EPS, EPS) - tt) ** 2).mean()
    loss_t.backward()
    loss, g, clipped = vclip_f64(y, t, v_old, EPS)
    assert 0.1 < clipped.mean() < 0.9                    # both branches are exercised
    np.testing.assert_allclose(loss, loss_t.item(), rtol=1e-13)
    np.testing.assert_allclose(g, ty.grad.numpy(), rtol=1e-13, atol=0)
    assert (g[clipped] == 0).all() and (g[~clipped] != 0).all()


def test_f32_model_against_f64():
    y, t, v_old = _inputs(5, 4000)
    y32, t32, v32 = y.astype(F32), t.astype(F32), v_old.astype(F32)
    l, g, clipped = vclip_f32(y32, t32, v32, EPS)
    assert l.dtype == F32 and g.dtype == F32
    loss, g64, c64 = vclip_f64(y32, t32, v32, float(F32(EPS)))
    np.testing.assert_array_equal(clipped, c64)          # 1e-3 from the boundaries: no fp32 decision can differ
    np.testing.assert_allclose(l.astype(np.float64).sum() / y.size, loss, rtol=1e-6)
    np.testing.assert_allclose(g, g64, rtol=4 * 2.0 ** -24, atol=0)      # a subtraction, a product, a division


def test_edge_cases():
    e = F32(0.25)
    # |d| == eps_v is inside: the unclipped term and gradient, although the clipped term would be larger
    y, v_old, t = np.array([1.25, -1.25], F32), np.array([1.0, -1.0], F32), np.array([1.25, -1.25], F32)
    t = t + np.array([0.5, -0.5], F32)                   # beyond y: lu = 0.25, lc (were it outside) = 0.25 too
    l, g, c = vclip_f32(y, t, v_old, e)
    assert not c.any() and (g == F32(2) * (y - t) / F32(2)).all() and (l == (t - y) * (t - y)).all()
    # lu == lc outside the range is unclipped (ties go to the unclipped term): t midway between y and yc
    y, v_old = np.array([2.0], F32), np.array([1.0], F32)             # yc = 1.25
    t = np.array([1.625], F32)                                         # lu = lc = 0.375²
    l, g, c = vclip_f32(y, t, v_old, e)
    assert not c.any() and g[0] == F32(2) * (y[0] - t[0]) / F32(1) and l[0] == F32(0.375) * F32(0.375)
    # … and the clipped term just larger is clipped, gradient zero
    l, g, c = vclip_f32(y, np.array([1.75], F32), v_old, e)          # lu = 0.0625 < lc = 0.25
    assert c.all() and g[0] == 0 and l[0] == F32(0.25)
    # NaN y: inside, a NaN gradient and loss term, exactly as with clipping off
    l, g, c = vclip_f32(np.array([np.nan, 0.5], F32), np.array([0.0, 1.0], F32), np.array([0.0, 0.0], F32), e)
    assert np.isnan(g[0]) and np.isnan(l[0]) and not c[0] and c[1] and g[1] == 0
    # eps_v huge: the plain MSE gradient bit for bit
    rng = np.random.default_rng(11)
    y, t, v_old = (rng.normal(size=1000).astype(F32) for _ in range(3))
    for big in (F32(3e38), F32(np.inf)):
        l, g, c = vclip_f32(y, t, v_old, big)
        assert not c.any()
        np.testing.assert_array_equal(g, F32(2) * (y - t) / F32(1000))
        np.testing.assert_array_equal(l, (t - y) * (t - y))
