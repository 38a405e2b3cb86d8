"""Invalid-action masking on the CPU (tests/masked_ref.py): the fp32 mirror inside every bound the GPU tests use,
the float64 gradient against finite differences (and exactly 0 on masked logits), a full mask against
multidiscrete_ref exactly, the outputs independent of what masked columns hold, the bounds telling the
zero-p-after-an-unmasked-softmax mistake apart, and the input sets free of near-clip rows."""
import os
import re

import numpy as np
import pytest

import categorical_ref as cr
import masked_ref as mk
import multidiscrete_ref as md
from categorical_ref import ENT, EPS, F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(nv, 257) for nv in mk.HEAD_NVEC] + [(nv, 5) for nv in mk.HEAD_NVEC_WIDE]
ids = lambda c: f"{c[0][0]}x{len(c[0])}-A{sum(c[0])}"        # noqa: E731


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_mirror_inside_bounds(case):
    nvec, m = case
    i = mk.head_inputs(nvec, m)
    args = mk.head_args(i, nvec)
    ref, got, b = mk.head_f64(*args), mk.head_f32(*args), mk.head_bounds(*args)
    skip = cr.near_clip(ref["ratio"])
    assert skip.mean() <= 0.01 and not skip.any()          # the cap on skipped rows, and these inputs skip none
    np.testing.assert_array_equal(got["clipped"][i["adv"] != 0], ref["clipped"][i["adv"] != 0])
    for name in ("lp", "H", "grad"):
        assert np.isfinite(ref[name]).all() and np.isfinite(got[name]).all(), name
        err = np.abs(got[name].astype(F64) - ref[name])
        assert (err <= b[name]).all(), (name, float((err / np.maximum(b[name], 1e-300)).max()))
        assert np.isfinite(b[name]).all() and (b[name] < 1e-2 * (1 + np.abs(ref[name]))).all(), name
    # masked gradient elements: +0 in the mirror, 0 in the model, a zero bound
    masked = ~ref["eff"]
    assert masked.any() or m < 4
    assert not got["grad"][masked].any() and not np.signbit(got["grad"][masked]).any()
    assert not ref["grad"][masked].any() and not b["grad"][masked].any()
    loss = float((-got["sur"].astype(F64) / m).sum() - ENT * got["H"].astype(F64).sum() / m)
    assert abs(loss - ref["loss"]) <= mk.loss_bound(ref, b, m, ENT)
    if m >= 64:
        assert ref["clipped"].any() and (~ref["clipped"]).any()


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_pinned_rows(case):
    """The generator's edge rows are what they say."""
    nvec, m = case
    i = mk.head_inputs(nvec, m)
    A, off = sum(nvec), mk.offsets(nvec)
    a = mk.indices(i["act"], nvec)
    st = i["stored"]
    ref = mk.head_f64(*mk.head_args(i, nvec))
    assert (mk.unpack(i["mask"], A) == st).all() and i["mask"].shape == (m, mk.words(A))
    assert st[np.arange(m)[:, None], off[:-1][None, :] + a][5:].all()          # the chosen bit is on off the pins
    # row 0: one allowed column in component 0 — H_0 = 0, lp_0 = 0, its gradient exactly 0
    assert st[0, off[0]:off[1]].sum() == 1 and ref["H_d"][0, 0] == 0 and ref["lp_d"][0, 0] == 0
    assert not ref["grad"][0, off[0]:off[1]].any()
    f32 = mk.head_f32(*mk.head_args(i, nvec))
    assert not f32["grad"][0, off[0]:off[1]].any()
    # row 1: all-zero stored bits read as full; row 2: the chosen bit is off and OR-ed in; row 3: full
    D = len(nvec)
    assert not st[1, off[D - 1]:off[D]].any() and ref["eff"][1, off[D - 1]:off[D]].all()
    assert not st[2, off[0] + a[2, 0]] and ref["eff"][2, off[0] + a[2, 0]] and st[2, off[0]:off[1]].sum() == 1
    assert st[3].all()
    if mk.straddle_row(A) is not None:
        assert np.flatnonzero(st[4]).tolist() == [31, 32]
        assert i["mask"][4, 0] == 1 << 31 and i["mask"][4, 1] == 1 and not i["mask"][4, 2:].any()
    # the poison: every kind occurs in masked columns, none in allowed ones
    z, eff = i["z"], ref["eff"]
    assert np.isfinite(z[eff]).all() and np.abs(z[eff]).max() <= 30
    if m == 257 and A > 2:
        bad = z[~eff]
        assert np.isnan(bad).any() and (bad == np.inf).any() and (bad == -np.inf).any() and (bad == F32(1e30)).any()
        assert (np.abs(bad[np.isfinite(bad)]) < 40).any()


@pytest.mark.parametrize("nvec", [[2], [3, 5, 2], [7] * 3, [33, 2]])
def test_gradient_is_the_derivative(nvec):
    """Central differences over the allowed logits; exactly 0 on the masked ones."""
    i = mk.rows_of(mk.head_inputs(nvec), 9)
    eff = mk.head_f64(*mk.head_args(i, nvec))["eff"]
    z = np.where(eff, i["z"], 0).astype(F64)
    args = (i["act"], i["adv"], i["old"], EPS, ENT, nvec, i["stored"])
    grad = mk.head_f64(z, *args)["grad"]
    h = 1e-6
    num = np.zeros_like(grad)
    for r, k in zip(*np.nonzero(eff)):
        zp, zm = z.copy(), z.copy()
        zp[r, k] += h
        zm[r, k] -= h
        num[r, k] = (mk.loss_of(zp, *args) - mk.loss_of(zm, *args)) / (2 * h)
    # the difference quotient's own noise: two float64 losses of magnitude |loss|, rounded, over 2h
    noise = 4 * np.finfo(F64).eps * abs(mk.loss_of(z, *args)) / (2 * h)
    np.testing.assert_allclose(grad, num, rtol=1e-6, atol=1e-9 * np.abs(grad).max() + noise)
    assert (~eff).any() and not grad[~eff].any()
    # and the loss does not move with a masked logit at all
    r, k = (int(v[0]) for v in np.nonzero(~eff))
    zp = z.copy()
    zp[r, k] += 1.0
    assert mk.loss_of(zp, *args) == mk.loss_of(z, *args)


@pytest.mark.parametrize("case", [(nv, 257) for nv in md.HEAD_NVEC] + [(nv, 5) for nv in md.HEAD_NVEC_WIDE], ids=ids)
def test_full_mask_is_unmasked(case):
    """Every bit set: the float64 model, the fp32 mirror and the bounds are multidiscrete_ref's, exactly."""
    nvec, m = case
    i = md.head_inputs(nvec, m)
    args = (i["z"], i["act"], i["adv"], i["old"], EPS, ENT, nvec)
    full = np.ones(i["z"].shape, bool)
    ref, got = md.head_f64(*args), mk.head_f64(*args, full)
    for name in ("lp", "H", "lp_d", "H_d", "grad", "ratio", "dlp", "loss_terms", "p"):
        np.testing.assert_array_equal(got[name], ref[name], err_msg=name)
    assert got["loss"] == ref["loss"]
    r32, g32 = md.head_f32(*args), mk.head_f32(*args, full)
    for name in ("lp", "H", "grad"):
        assert g32[name].tobytes() == r32[name].tobytes(), name
    rb, gb = md.head_bounds(*args), mk.head_bounds(*args, full)
    for name in ("lp", "H", "grad", "s_rel", "ratio_rel"):
        np.testing.assert_array_equal(gb[name], rb[name], err_msg=name)
    # all-zero stored bits read the same
    none = mk.head_f32(*args, np.zeros(i["z"].shape, bool))
    for name in ("lp", "H", "grad"):
        assert none[name].tobytes() == r32[name].tobytes(), name


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_masked_columns_are_never_read(case):
    """The poisoned logits, the clean ones and a third filling of the masked columns give identical outputs."""
    nvec, m = case
    i = mk.head_inputs(nvec, m)
    args = mk.head_args(i, nvec)
    eff = mk.head_f64(*args)["eff"]
    other = np.where(eff, i["z"], F32(-7.5))
    for model in (mk.head_f64, mk.head_f32, mk.head_bounds):
        a, b, c = (model(zz, *args[1:]) for zz in (i["z"], i["z_clean"], other))
        for name in ("lp", "H", "grad"):
            assert np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes() == np.asarray(c[name]).tobytes()


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_zero_p_mistake_leaves_the_bound(case):
    """An unmasked softmax whose p is zeroed on the masked columns afterwards (no renormalisation) is far outside
    the gradient bound, so a kernel with that mistake fails test_gpu_masked's head test: on the pinned rows 0 … 2 and
    4 taken together, and on most rows that have a masked column at all.  (One pinned row alone may not show it: where
    multidiscrete_ref's ±30 row leaves the chosen column with p = 1 either way, or its flat row is clipped, the two
    models coincide.)"""
    nvec, m = case
    i = mk.head_inputs(nvec, m)
    args = (i["z_clean"],) + mk.head_args(i, nvec)[1:]
    ref, wrong, b = mk.head_f64(*args), mk.head_f64(*args, zero_p=True), mk.head_bounds(*args)
    ok = ref["eff"]
    excess = np.where(ok, np.abs(wrong["grad"] - ref["grad"]) / np.maximum(b["grad"], 1e-300), 0.0).max(axis=1)
    has_masked = ~ok.all(axis=1)
    pinned = [r for r in (0, 1, 2, 4) if r < m and has_masked[r]]
    assert pinned and excess[pinned].max() > 100, excess[pinned]
    if m == 257:
        assert (excess[has_masked] > 100).mean() > 0.5, (excess[has_masked] > 100).mean()


def test_sampler_mirror():
    """Full masks: multidiscrete_ref's mirror exactly.  Random masks: no masked index is chosen, the near-boundary
    count the GPU test caps at 1 % is below it, the joint log-prob is inside the lp bound, and the greedy action is
    numpy's masked argmax."""
    nvec = mk.SAMPLE_NVEC
    A, D = sum(nvec), len(nvec)
    z = md.sample_inputs(nvec, shared_row=True)
    m = z.shape[0]
    u = mk.sample_u(m, D, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET)
    a0, lp0, mg0 = md.sample_f32(z, u, nvec)
    a1, lp1, mg1 = mk.sample_f32(z, u, nvec, np.ones((m, A), bool))
    assert (a0 == a1).all() and lp0.tobytes() == lp1.tobytes() and (mg0 == mg1).all()
    st = mk.random_masks(nvec, m, 41)
    eff = mk.effective(st, nvec)
    zp = mk.poison(z, eff)
    a, lp, margin = mk.sample_f32(zp, u, nvec, st)
    off = mk.offsets(nvec)
    assert eff[np.arange(m)[:, None], off[:-1][None, :] + a].all()
    assert (mk.near_boundary(margin, nvec).any(axis=1)).mean() < 0.01
    act = md.action_rows(a, A)
    zero = np.zeros(m)
    ref = mk.head_f64(zp, act, zero, zero, EPS, 0.0, nvec, st)
    b = mk.head_bounds(zp, act, zero, zero, EPS, 0.0, nvec, st)
    assert (np.abs(lp.astype(F64) - ref["lp"]) <= b["lp"]).all()
    # every allowed index of every component is drawn somewhere, and the last allowed one is reachable
    assert all(len(np.unique(a[:, d])) == nvec[d] for d in range(D))
    g = mk.argmax(zp, nvec, st)
    assert eff[np.arange(m)[:, None], off[:-1][None, :] + g].all()
    ties = np.zeros((3, 5), F32)
    assert mk.argmax(ties, [5], np.array([[0, 1, 1, 0, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 1]], bool)).ravel().tolist() \
        == [1, 0, 4]


def test_pack_unpack():
    rng = np.random.default_rng(5)
    for A in (2, 31, 32, 33, 64, 65, 119, 4096):
        st = rng.random((7, A)) < 0.5
        w = mk.pack(st)
        assert w.dtype == np.uint32 and w.shape == (7, (A + 31) // 32)
        assert (mk.unpack(w, A) == st).all()
        k = int(rng.integers(0, A))
        assert bool((w[3, k >> 5] >> np.uint32(k & 31)) & 1) == bool(st[3, k])
        if A % 32:                                             # bits at k >= A are ignored
            w2 = w.copy()
            w2[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(A % 32)
            assert (mk.unpack(w2, A) == st).all()


def test_public_names():
    """The new entries are declared in ppo_ext.h and have ctypes signatures; the sentence that said masking was not
    provided is gone."""
    import ppo_ffi

    text = open(os.path.join(ROOT, "include", "ppo_ext.h")).read()
    assert "masking is\n * not provided" not in text and "masking is not provided" not in text
    for name, n_args in (("ppo_set_action_mask", 2), ("ppo_get_action_mask", 1), ("ppo_action_mask_words", 1),
                         ("ppo_action_mask_buffer", 1), ("ppo_rollout_act_masked", 3), ("ppo_act_device_masked", 9),
                         ("ppo_masked_head_device", 16), ("ppo_masked_sample_device", 10),
                         ("ppo_masked_argmax_device", 7)):
        assert re.search(r"\b" + name + r"\(", text), name
        assert name in ppo_ffi._SIGS and len(ppo_ffi._SIGS[name][1]) == n_args, name
