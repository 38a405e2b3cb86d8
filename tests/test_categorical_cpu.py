"""The categorical head's float64 model against finite differences, and the fp32 mirror inside every bound the GPU
tests use (tests/categorical_ref.py): a bound the mirror leaves on the CPU would not be valid on the device."""
import numpy as np
import pytest

import categorical_ref as cr
from categorical_ref import ENT, EPS, F32, F64, U

SIZES_A = [2, 3, 17, 32, 33, 64, 65, 257]


@pytest.mark.parametrize("A", [2, 3, 6, 17])
def test_model_gradient_is_the_loss_derivative(A):
    """∂loss/∂z of head_f64 — both terms, the entropy one included — against central differences of its own loss
    in float64 (h = 1e-6: truncation ~1e-12·|f‴|, rounding ~1e-16/1e-6)."""
    rng = np.random.default_rng(A)
    m = 9
    z = rng.normal(size=(m, A))
    act = np.zeros((m, A))
    act[:, 0] = rng.integers(0, A, m)
    adv = rng.normal(size=m)
    lp = cr.head_f64(z, act, adv, np.zeros(m), EPS, 0.0)["lp"]
    old = lp - rng.uniform(-0.15, 0.15, m)                  # unclipped: the loss is differentiable there
    old[0], old[1] = lp[0] - 0.5, lp[1] + 0.5               # … and two rows on the clip sides
    adv[0], adv[1] = abs(adv[0]) + 0.1, -abs(adv[1]) - 0.1  # ratio > 1 + eps with adv > 0; < 1 − eps with adv < 0
    for ent in (0.0, 0.3):
        ref = cr.head_f64(z, act, adv, old, EPS, ent)
        assert ref["clipped"][0] and ref["clipped"][1] and not ref["clipped"][2:].any()
        num = np.zeros_like(z)
        h = 1e-6
        for i in range(m):
            for k in range(A):
                zp, zm = z.copy(), z.copy()
                zp[i, k] += h
                zm[i, k] -= h
                num[i, k] = (cr.loss_of(zp, act, adv, old, EPS, ent) - cr.loss_of(zm, act, adv, old, EPS, ent)) / (2 * h)
        np.testing.assert_allclose(ref["grad"], num, rtol=0, atol=2e-8, err_msg=f"ent {ent}")
        assert np.abs(ref["grad"].sum(axis=1)).max() < 1e-15    # softmax gradients sum to zero over a row


def test_model_entropy_and_probabilities():
    z = np.array([[0.0, 0.0, 0.0, 0.0], [30.0, -30.0, 0.0, 1.0]])
    act = np.zeros((2, 4))
    ref = cr.head_f64(z, act, np.zeros(2), np.zeros(2), EPS, 0.0)
    assert abs(ref["H"][0] - np.log(4)) < 1e-15 and abs(ref["lp"][0] + np.log(4)) < 1e-15
    np.testing.assert_allclose(ref["p"].sum(axis=1), 1.0, atol=1e-15)
    p = ref["p"][1]
    assert abs(ref["H"][1] + (p * np.log(p)).sum()) < 1e-12


@pytest.mark.parametrize("A", [513, 1024, 1025, 2048, 2049, 4096])
def test_mirror_within_bounds_wide(A):
    """The 5-row inputs of the GPU test's wide shapes: the mirror inside the same bounds."""
    i = cr.head_inputs(A, 5)
    ref = cr.head_f64(i["z"], i["act"], i["adv"], i["old"], EPS, ENT)
    got = cr.head_f32(i["z"], i["act"], i["adv"], i["old"], EPS, ENT)
    b = cr.head_bounds(i["z"], i["act"], i["adv"], i["old"], EPS, ENT)
    np.testing.assert_array_equal(got["clipped"], ref["clipped"])
    for name in ("lp", "H", "grad"):
        assert (np.abs(got[name].astype(F64) - ref[name]) <= b[name]).all(), name


@pytest.mark.parametrize("A", SIZES_A)
def test_mirror_within_bounds(A):
    """lp, H and every gradient element of the fp32 mirror within head_bounds of the float64 model, with no row of
    the inputs in the clip guard band and none whose branch differs (so the GPU test's 1 % allowance is unused by
    the mirror); the largest error/bound ratio is printed."""
    i = cr.head_inputs(A)
    m = i["z"].shape[0]
    ref = cr.head_f64(i["z"], i["act"], i["adv"], i["old"], EPS, ENT)
    got = cr.head_f32(i["z"], i["act"], i["adv"], i["old"], EPS, ENT)
    b = cr.head_bounds(i["z"], i["act"], i["adv"], i["old"], EPS, ENT)
    assert not cr.near_clip(ref["ratio"]).any()
    np.testing.assert_array_equal(got["clipped"], ref["clipped"])
    assert ref["clipped"][i["adv"] > 0].any() and ref["clipped"][i["adv"] < 0].any() and (~ref["clipped"]).sum() > m // 4
    for name in ("lp", "H", "grad"):
        err = np.abs(got[name].astype(F64) - ref[name])
        ratio = float((err / b[name]).max())
        print(f"A {A}: mirror {name} error / bound {ratio:.3f}")
        assert (err <= b[name]).all(), (name, ratio)
    # the bounds are rounding bounds, not slack: a few hundred half-ulps of the values they bound at most
    assert (b["lp"] <= 4 * (A + 200) * U * (1 + np.abs(ref["lp"]))).all()
    sur = got["sur"].astype(F64)
    loss32 = -(sur.sum()) / m - ENT * got["H"].astype(F64).sum() / m
    assert abs(loss32 - ref["loss"]) <= cr.loss_bound(ref, b, m, ENT)
    # the underflow row and the flat row are what they claim to be
    e0 = np.exp(i["z"][0].astype(F64) - i["z"][0].max())
    assert A < 3 or e0.min() < 2.0 ** -80
    assert abs(ref["H"][1] - np.log(A)) < 1e-12


@pytest.mark.parametrize("A", [2, 6, 65])
def test_sampler_mirror(A):
    """The seed of the GPU sampler test: rows whose threshold lies within the bound of a cumulative boundary stay
    under the 1 % cap for the mirror itself; the mirror's index is the definition's (float64 inverse CDF) on every
    other row; columns and clamp."""
    z = cr.sample_inputs(A)
    m = z.shape[0]
    u = cr.sample_u(m, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET)
    assert u.dtype == F32 and (u > 0).all() and (u <= 1).all()
    a, lp, margin = cr.sample_f32(z, u)
    s_rel = (A + 70) * U                                   # ≥ head_bounds' s_rel for |z − M| ≤ 60 (asserted below)
    b = cr.head_bounds(z, np.zeros((m, A)), np.zeros(m), np.zeros(m), EPS, 0.0)      # every row
    assert (b["s_rel"] <= s_rel).all()
    near = margin <= 2 * s_rel + 2 * U
    print(f"A {A}: {int(near.sum())} of {m} rows within the bound of a boundary")
    assert near.mean() < 0.01
    z64 = z.astype(F64)
    e = np.exp(z64 - z64.max(axis=1, keepdims=True))
    c = np.cumsum(e, axis=1)
    want = (u.astype(F64)[:, None] * c[:, -1:] <= c).argmax(axis=1)
    np.testing.assert_array_equal(a[~near], want[~near])
    assert a.min() >= 0 and a.max() <= A - 1
    ref_lp = np.log(e[np.arange(m), a] / c[:, -1])
    assert np.abs(lp - ref_lp).max() <= (A + 200) * U * (1 + np.abs(ref_lp).max())


def test_sampler_frequencies_mirror():
    A = 6
    z = cr.sample_inputs(A, shared_row=True)
    m = z.shape[0]
    a, _, _ = cr.sample_f32(z, cr.sample_u(m, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET))
    p = cr.head_f64(z[:1], np.zeros((1, A)), np.zeros(1), np.zeros(1), EPS, 0.0)["p"][0]
    freq = np.bincount(a, minlength=A) / m
    assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / m)).all(), (freq, p)
