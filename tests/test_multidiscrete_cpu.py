"""The multi-discrete head's float64 model against finite differences and against the categorical model at D = 1,
the fp32 mirror inside every bound the GPU tests use (tests/multidiscrete_ref.py): a bound the mirror leaves on the
CPU would not be valid on the device — and the bounds tell the H-for-H_d mistake apart."""
import os
import re

import numpy as np
import pytest

import categorical_ref as cr
import multidiscrete_ref as md
from categorical_ref import ENT, EPS, F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(nv, 257) for nv in md.HEAD_NVEC] + [(nv, 5) for nv in md.HEAD_NVEC_WIDE]
ids = lambda c: f"{c[0][0]}x{len(c[0])}-A{sum(c[0])}"        # noqa: E731


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_mirror_inside_bounds(case):
    nvec, m = case
    i = md.head_inputs(nvec, m)
    args = (i["z"], i["act"], i["adv"], i["old"], EPS, ENT, nvec)
    ref, got, b = md.head_f64(*args), md.head_f32(*args), md.head_bounds(*args)
    assert not cr.near_clip(ref["ratio"]).any()
    np.testing.assert_array_equal(got["clipped"][i["adv"] != 0], ref["clipped"][i["adv"] != 0])
    for name in ("lp", "H", "grad"):
        err = np.abs(got[name].astype(F64) - ref[name])
        assert (err <= b[name]).all(), (name, float((err / b[name]).max()))
        assert np.isfinite(b[name]).all() and (b[name] < 1e-2 * (1 + np.abs(ref[name]))).all(), name   # and says something
    loss = float((-got["sur"].astype(F64) / m).sum() - ENT * got["H"].astype(F64).sum() / m)
    assert abs(loss - ref["loss"]) <= md.loss_bound(ref, b, m, ENT)
    # both clip sides and the unclipped side occur in the full sets
    if m >= 64:
        assert ref["clipped"].any() and (~ref["clipped"]).any()


@pytest.mark.parametrize("case", [c for c in CASES if len(c[0]) >= 2], ids=ids)
def test_row_entropy_mistake_leaves_the_bound(case):
    """Row 0 holds a flat and a peaked component: the model that takes the row's H in a logit's entropy term is
    outside the gradient bound there, so a kernel with that mistake fails test_gpu_multidiscrete's head test."""
    nvec, m = case
    i = md.head_inputs(nvec, m)
    args = (i["z"], i["act"], i["adv"], i["old"], EPS, ENT, nvec)
    r = md.mixed_row(nvec)
    ref, wrong, b = md.head_f64(*args), md.head_f64(*args, row_H=True), md.head_bounds(*args)
    assert ref["H_d"][r, 0] > 0.69 and ref["H_d"][r, 1] < 1e-6
    excess = np.abs(wrong["grad"][r] - ref["grad"][r]) / b["grad"][r]
    assert excess.max() > 100, excess.max()


@pytest.mark.parametrize("nvec", [[2, 2], [3, 5, 2], [7] * 3, [33, 2]])
def test_gradient_is_the_derivative(nvec):
    i = md.rows_of(md.head_inputs(nvec), 9)
    z = i["z"].astype(F64)
    args = (i["act"], i["adv"], i["old"], EPS, ENT, nvec)
    grad = md.head_f64(z, *args)["grad"]
    h = 1e-6
    num = np.empty_like(grad)
    for r in range(z.shape[0]):
        for k in range(z.shape[1]):
            zp, zm = z.copy(), z.copy()
            zp[r, k] += h
            zm[r, k] -= h
            num[r, k] = (md.loss_of(zp, *args) - md.loss_of(zm, *args)) / (2 * h)
    np.testing.assert_allclose(grad, num, rtol=1e-6, atol=1e-9 * np.abs(grad).max())


@pytest.mark.parametrize("A", [2, 3, 17, 32, 33, 257])
def test_one_component_is_categorical(A):
    i = cr.head_inputs(A)
    args = (i["z"], i["act"], i["adv"], i["old"], EPS, ENT)
    ref, got = cr.head_f64(*args), md.head_f64(*args, [A])
    for name in ("lp", "H", "grad", "ratio", "dlp", "loss_terms"):
        np.testing.assert_array_equal(got[name], ref[name], err_msg=name)
    assert got["loss"] == ref["loss"]
    m32, c32 = md.head_f32(*args, [A]), cr.head_f32(*args)
    for name in ("lp", "H", "grad"):
        assert m32[name].tobytes() == c32[name].tobytes(), name
    b, cb = md.head_bounds(*args, [A]), cr.head_bounds(*args)
    for name in ("lp", "H", "grad"):
        np.testing.assert_array_equal(b[name], cb[name])


def test_sampler_mirror():
    """D = 1 is categorical_ref's sampler; at D = 9 the words .x … .w of three counters, the near-boundary count
    per component the GPU test caps at 1 %, and the joint log-prob inside the lp bound."""
    z = cr.sample_inputs(6)
    m = z.shape[0]
    u = md.sample_u(m, 1, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET)
    assert u[:, 0].tobytes() == cr.sample_u(m, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET).tobytes()
    a, lp, margin = md.sample_f32(z, u, [6])
    a1, lp1, margin1 = cr.sample_f32(z, u[:, 0])
    assert (a[:, 0] == a1).all() and lp.tobytes() == lp1.tobytes() and (margin[:, 0] == margin1).all()

    nvec = md.SAMPLE_NVEC
    z = md.sample_inputs(nvec)
    u = md.sample_u(m, len(nvec), cr.SAMPLE_KEY, cr.SAMPLE_OFFSET)
    assert u.min() > 0 and u.max() <= 1
    # every component its own uniform: distinct columns, each U(0, 1]
    assert len({u[:, d].tobytes() for d in range(len(nvec))}) == len(nvec)
    assert np.abs(u.mean(axis=0) - 0.5).max() < 5 * np.sqrt(1 / 12 / m)
    a, lp, margin = md.sample_f32(z, u, nvec)
    assert (md.near_boundary(margin, nvec).mean(axis=0) < 0.01).all()
    act = md.action_rows(a, sum(nvec))
    zero = np.zeros(m)
    ref = md.head_f64(z, act, zero, zero, EPS, 0.0, nvec)
    b = md.head_bounds(z, act, zero, zero, EPS, 0.0, nvec)
    assert (np.abs(lp.astype(F64) - ref["lp"]) <= b["lp"]).all()


def test_public_names():
    """The four new entries are declared in ppo_ext.h and have ctypes signatures."""
    import ppo_ffi

    text = open(os.path.join(ROOT, "include", "ppo_ext.h")).read()
    assert re.search(r"#define\s+PPO_MD_MAX_D\s+256\b", text)
    for name in ("ppo_set_action_multidiscrete", "ppo_get_action_nvec", "ppo_multidiscrete_head_device",
                 "ppo_multidiscrete_sample_device"):
        assert re.search(r"\bint\s+" + name + r"\(", text), name
        assert name in ppo_ffi._SIGS, name
    assert len(ppo_ffi._SIGS["ppo_multidiscrete_head_device"][1]) == 14
    assert len(ppo_ffi._SIGS["ppo_multidiscrete_sample_device"][1]) == 9
