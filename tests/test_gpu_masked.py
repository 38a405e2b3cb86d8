"""Invalid-action masking on the device (ppo_set_action_mask; csrc/discrete.hip) against tests/masked_ref.py: the head
row by row, a full mask against the unmasked heads bit for bit, the sampler and the greedy action, the KL monitor, one
policy step of an update, the open rollout and the argument handling.  Every bound comes from masked_ref /
multidiscrete_ref / categorical_ref (derived from the rounding of the listed operations and validated by the fp32
mirror on the CPU in test_masked_cpu.py); nothing is taken from a run of the kernels."""
import ctypes as C

import numpy as np
import pytest

import categorical_ref as cr
import kl_ref
import masked_ref as mk
import multidiscrete_ref as md
import ppo_ffi
import tanh_ref
from categorical_ref import ENT, EPS, F32, F64, U
from helpers import dev, empty, gemm_tol, nn_grads_packed, nn_input_rows, nn_params_packed
from test_gpu_update import adam_first_step, assert_adam_delta

pytestmark = pytest.mark.gpu

U32 = np.uint32
ids = lambda nv: f"{nv[0]}x{len(nv)}-A{sum(nv)}"        # noqa: E731


def no_error(lib):
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


def run_head(lib, i, nvec, ent=ENT, mask=None, rows=None, z=None):
    """the masked head over i's inputs; mask / rows: another store and the row list into it"""
    z = i["z"] if z is None else z
    m, A = z.shape
    mask = i["mask"] if mask is None else mask
    d = dict(z=dev(lib, z), act=dev(lib, i["act"]), adv=dev(lib, i["adv"]), old=dev(lib, i["old"]),
             mask=dev(lib, mask), g=dev(lib, np.full((m, A), np.nan, F32)), lp=empty(lib, m), H=empty(lib, m))
    if rows is not None:
        d["rows"] = dev(lib, np.asarray(rows, np.int32))
    try:
        loss = C.c_double(np.nan)
        rc = lib.ppo_masked_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, d["mask"].ptr,
                                        d["rows"].ptr if rows is not None else None, m, A, ppo_ffi.c_ints(nvec),
                                        len(nvec), EPS, ent, d["g"].ptr, d["lp"].ptr, d["H"].ptr, C.byref(loss))
        assert rc == 0
        return dict(grad=d["g"].to_numpy(F32, m * A).reshape(m, A), lp=d["lp"].to_numpy(F32, m),
                    H=d["H"].to_numpy(F32, m), loss=loss.value)
    finally:
        for a in d.values():
            a.free()


def run_unmasked(lib, i, nvec, cat=False):
    m, A = i["z"].shape
    d = dict(z=dev(lib, i["z"]), act=dev(lib, i["act"]), adv=dev(lib, i["adv"]), old=dev(lib, i["old"]),
             g=empty(lib, m * A), lp=empty(lib, m), H=empty(lib, m))
    try:
        loss = C.c_double(np.nan)
        if cat:
            rc = lib.ppo_categorical_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, m, A, EPS, ENT,
                                                 d["g"].ptr, d["lp"].ptr, d["H"].ptr, C.byref(loss))
        else:
            rc = lib.ppo_multidiscrete_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, m, A,
                                                   ppo_ffi.c_ints(nvec), len(nvec), EPS, ENT, d["g"].ptr, d["lp"].ptr,
                                                   d["H"].ptr, C.byref(loss))
        assert rc == 0
        return dict(grad=d["g"].to_numpy(F32, m * A).reshape(m, A), lp=d["lp"].to_numpy(F32, m),
                    H=d["H"].to_numpy(F32, m))
    finally:
        for a in d.values():
            a.free()


def same(a, b, what):
    for name in ("lp", "H", "grad"):
        assert a[name].tobytes() == b[name].tobytes(), f"{what}: {name}"


def check_head(lib, i, nvec, what):
    m, A = i["z"].shape
    args = mk.head_args(i, nvec)
    ref, b = mk.head_f64(*args), mk.head_bounds(*args)
    got = run_head(lib, i, nvec)
    skip = cr.near_clip(ref["ratio"])
    assert skip.mean() <= 0.01 and not skip.any(), what       # the cap, and these inputs contain none
    live = ~skip & (i["adv"] != 0)
    first = run_head(lib, i, nvec, ent=0.0)["grad"]
    clipped_dev = ~(first != 0).any(axis=1)
    # a row whose every component has a single allowed column has a zero gradient clipped or not: it shows no branch
    shows = live & (np.abs(ref["grad"]).max(axis=1) > 0) & ((ref["p"] > 0) & (ref["p"] < 1)).any(axis=1)
    np.testing.assert_array_equal(clipped_dev[shows], ref["clipped"][shows], err_msg=what)
    for name in ("lp", "H", "grad"):
        assert np.isfinite(got[name]).all(), f"{what}: {name} not finite"
        err = np.abs(got[name].astype(F64) - ref[name])[~skip]
        bound = b[name][~skip]
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{what}: {name} error / bound {ratio:.3f}")
        assert (err <= bound).all(), f"{what}: {name} at {ratio:.3g} of the bound"
    masked = ~ref["eff"]
    assert not got["grad"].view(U32)[masked].any(), f"{what}: a masked gradient element is not +0"
    bound = mk.loss_bound(ref, b, m, ENT)
    print(f"{what}: loss error / bound {abs(got['loss'] - ref['loss']) / bound:.3f}")
    assert abs(got["loss"] - ref["loss"]) <= bound, f"{what}: loss {got['loss']} vs {ref['loss']} ± {bound}"
    # the masks read in place through a row list: a larger store, permuted, gives the bytes of the gathered run
    rng = np.random.default_rng(7 + m)
    cap = m + 37
    rows = rng.permutation(cap)[:m]
    store = rng.integers(0, 2 ** 32, (cap, mk.words(A)), dtype=np.uint64).astype(U32)
    store[rows] = i["mask"]
    again = run_head(lib, i, nvec, mask=store, rows=rows)
    same(got, again, f"{what}: through rows")


# ------------------------------------------------------------------------------------------ 1. head rows
@pytest.mark.parametrize("nvec", mk.HEAD_NVEC, ids=ids)
def test_head_rows(lib, nvec):
    """lp, H and every element of ∂loss/∂logits within head_bounds of the float64 model, the loss within loss_bound,
    masked gradient elements bitwise +0, at m ∈ {1, 63, 64, 257}; the masked columns of the logits hold NaN, ±inf and
    1e30; rows 0 … 4 are masked_ref.make_mask's pinned ones; a run through a permuted row list into a larger store
    gives the same bytes."""
    full = mk.head_inputs(nvec)
    for m in mk.HEAD_M:
        check_head(lib, mk.rows_of(full, m), nvec, f"nvec {ids(nvec)} m {m}")
    no_error(lib)


@pytest.mark.parametrize("nvec", mk.HEAD_NVEC_WIDE, ids=ids)
def test_head_rows_wide(lib, nvec):
    """D at the cap and components up to the head's limit (W = 16 and 128, the R = 1 … 4 tiles), 5 rows."""
    check_head(lib, mk.head_inputs(nvec, 5), nvec, f"nvec {ids(nvec)} m 5")
    no_error(lib)


# ------------------------------------------------------------------------------------------- 2. full mask
@pytest.mark.parametrize("nvec", mk.HEAD_NVEC + mk.HEAD_NVEC_WIDE, ids=ids)
def test_full_mask_is_the_unmasked_head(lib, nvec):
    """Every bit set (and, the same thing, no bit set): lp, H and the gradient are ppo_multidiscrete_head_device's
    bytes at every row count of case 1."""
    wide = nvec in mk.HEAD_NVEC_WIDE
    inp = md.head_inputs(nvec, 5 if wide else 257)
    A = sum(nvec)
    for m in ([5] if wide else mk.HEAD_M):
        i = md.rows_of(inp, m)
        want = run_unmasked(lib, i, nvec)
        ones = np.full((m, mk.words(A)), 0xFFFFFFFF, U32)
        same(run_head(lib, i, nvec, mask=ones), want, f"nvec {ids(nvec)} m {m}: full")
        same(run_head(lib, i, nvec, mask=np.zeros_like(ones)), want, f"nvec {ids(nvec)} m {m}: all-zero")
    no_error(lib)


@pytest.mark.parametrize("A", [2, 17, 32])
def test_full_mask_one_component_is_categorical(lib, A):
    """nvec = {A}, A <= 32, a full mask: also ppo_categorical_head_device's bytes."""
    i = cr.head_inputs(A)
    ones = np.full((i["z"].shape[0], 1), 0xFFFFFFFF, U32)
    got = run_head(lib, i, [A], mask=ones)
    same(got, run_unmasked(lib, i, [A], cat=True), f"A {A}: categorical")
    same(got, run_unmasked(lib, i, [A]), f"A {A}: multi-discrete")
    no_error(lib)


@pytest.mark.parametrize("nvec", [[3, 5, 2], [7] * 17, [65, 3, 64], [4094, 2]], ids=ids)
def test_masked_columns_are_never_read(lib, nvec):
    """A second run with the masked columns' contents replaced gives byte-identical output."""
    i = mk.head_inputs(nvec, 5 if nvec in mk.HEAD_NVEC_WIDE else 257)
    eff = mk.head_f64(*mk.head_args(i, nvec))["eff"]
    got = run_head(lib, i, nvec)
    same(got, run_head(lib, i, nvec, z=i["z_clean"]), "clean logits")
    same(got, run_head(lib, i, nvec, z=np.where(eff, i["z"], F32(-3e38))), "−3e38")
    no_error(lib)


# -------------------------------------------------------------------------------------------- 3. sampler
def run_sampler(lib, z, nvec, mask, key, offset, masked=True):
    m, A = z.shape
    d = dict(z=dev(lib, z), act=dev(lib, np.full((m, A), np.nan, F32)), lp=empty(lib, m), mask=dev(lib, mask))
    try:
        if masked:
            rc = lib.ppo_masked_sample_device(d["z"].ptr, d["mask"].ptr, m, A, ppo_ffi.c_ints(nvec), len(nvec), key,
                                              offset, d["act"].ptr, d["lp"].ptr)
        else:
            rc = lib.ppo_multidiscrete_sample_device(d["z"].ptr, m, A, ppo_ffi.c_ints(nvec), len(nvec), key, offset,
                                                     d["act"].ptr, d["lp"].ptr)
        assert rc == 0
        return d["act"].to_numpy(F32, m * A).reshape(m, A), d["lp"].to_numpy(F32, m)
    finally:
        for a in d.values():
            a.free()


def run_argmax(lib, z, nvec, mask):
    m, A = z.shape
    d = dict(z=dev(lib, z), act=dev(lib, np.full((m, A), np.nan, F32)), mask=dev(lib, mask))
    try:
        assert lib.ppo_masked_argmax_device(d["z"].ptr, d["mask"].ptr, m, A, ppo_ffi.c_ints(nvec), len(nvec),
                                            d["act"].ptr) == 0
        return d["act"].to_numpy(F32, m * A).reshape(m, A)
    finally:
        for a in d.values():
            a.free()


def test_sampler(lib):
    """D = 9, 65 536 rows of one shared logit row under random masks (the masked columns poisoned): no masked index
    is ever chosen; every index equals the mirror's wherever the threshold is further from a cumulative boundary than
    the bound (under 1 % of the rows may be left out; the mirror's own count is below that, checked on the CPU too);
    columns D … A−1 are +0; the joint log-prob is within the lp bound; a full mask gives
    ppo_multidiscrete_sample_device's bytes; the greedy action is numpy's masked argmax."""
    nvec = mk.SAMPLE_NVEC
    A, D = sum(nvec), len(nvec)
    z = md.sample_inputs(nvec, shared_row=True)
    m = z.shape[0]
    st = mk.random_masks(nvec, m, 41)
    eff = mk.effective(st, nvec)
    zp = mk.poison(z, eff)
    act, lp = run_sampler(lib, zp, nvec, mk.pack(st), cr.SAMPLE_KEY, cr.SAMPLE_OFFSET)
    a = act[:, :D].astype(np.int64)
    assert (act[:, :D] == a).all() and a.min() >= 0 and (a.max(axis=0) <= np.asarray(nvec) - 1).all()
    assert not act[:, D:].any() and not np.signbit(act[:, D:]).any()
    off = mk.offsets(nvec)
    assert eff[np.arange(m)[:, None], off[:-1][None, :] + a].all(), "a masked index was chosen"
    a_ref, _, margin = mk.sample_f32(zp, mk.sample_u(m, D, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET), nvec, st)
    near = mk.near_boundary(margin, nvec)
    assert near.any(axis=1).mean() < 0.01
    np.testing.assert_array_equal(a[~near], a_ref[~near])
    zero = np.zeros(m)
    ref = mk.head_f64(zp, act, zero, zero, EPS, 0.0, nvec, st)
    b = mk.head_bounds(zp, act, zero, zero, EPS, 0.0, nvec, st)
    err = np.abs(lp.astype(F64) - ref["lp"])
    print(f"{int((a != a_ref).sum())} indices differ from the mirror ({int(near.sum())} near a boundary); "
          f"lp error / bound {float((err / b['lp']).max()):.3f}")
    assert (err <= b["lp"]).all()
    # a full mask: the unmasked sampler's bytes
    ones = np.full((m, mk.words(A)), 0xFFFFFFFF, U32)
    zz = md.sample_inputs(nvec)
    fa, flp = run_sampler(lib, zz, nvec, ones, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET)
    ua, ulp = run_sampler(lib, zz, nvec, ones, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET, masked=False)
    assert fa.tobytes() == ua.tobytes() and flp.tobytes() == ulp.tobytes()
    # the greedy action: the shared row, and rows with ties
    g = run_argmax(lib, zp, nvec, mk.pack(st))
    np.testing.assert_array_equal(g[:, :D].astype(np.int64), mk.argmax(zp, nvec, st))
    assert not g[:, D:].any()
    ties = np.zeros((3, 5), F32)
    tm = np.array([[0, 1, 1, 0, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 1]], bool)
    assert run_argmax(lib, ties, [5], mk.pack(tm))[:, 0].tolist() == [1, 0, 4]
    no_error(lib)


def cdf_consistent(z, u, nvec, st, a):
    """Every chosen index is a first crossing of its component's masked CDF up to the rounding bound: with c the
    mirror's cumulative sums over the allowed columns, c[a] >= u·s − tol (or a is the last allowed column) and the
    sum before a is < u·s + tol, tol = near_boundary's bound times s.  Holds for every row, however dense the steps."""
    off = mk.offsets(nvec)
    eff = mk.effective(st, nvec)
    z = np.where(eff, np.asarray(z, F32), F32(0))
    rows = np.arange(z.shape[0])
    for d, n in enumerate(nvec):
        seg, ok = np.ascontiguousarray(z[:, off[d]:off[d + 1]]), eff[:, off[d]:off[d + 1]]
        _, _, c, _ = mk.row_stats_f32(seg, ok)
        c = c.astype(F64)
        s = c[:, -1]
        thr, tol = u[:, d].astype(F64) * s, (2 * (n + 70) * U + 2 * U) * s
        ad = a[:, d]
        last = n - 1 - ok[:, ::-1].argmax(axis=1)
        before = np.where(ad > 0, c[rows, np.maximum(ad - 1, 0)], 0.0)
        if not (ok[rows, ad] & ((c[rows, ad] >= thr - tol) | (ad == last)) & (before < thr + tol)).all():
            return False
    return True


def test_sampler_wide(lib):
    """A component across several mask words (nvec = [65, 3, 64], W = 5) and the widest one ([4096], W = 128), row 0
    with columns 31 and 32 alone: no masked index chosen, every index a first crossing of the masked CDF within the
    rounding bound (the steps of a 4096-wide CDF are too dense to compare indices with the mirror's), the masked
    argmax."""
    for nvec, m in (([65, 3, 64], 4096), ([4096], 64)):
        A, D = sum(nvec), len(nvec)
        z = md.sample_inputs(tuple(nvec), m)
        st = mk.random_masks(nvec, m, 43)
        st[0] = False
        st[0, 31:33] = True                                    # row 0: only columns 31 and 32
        eff = mk.effective(st, nvec)
        zp = mk.poison(z, eff)
        act, lp = run_sampler(lib, zp, nvec, mk.pack(st), 5, 9)
        a = act[:, :D].astype(np.int64)
        off = mk.offsets(nvec)
        assert (act[:, :D] == a).all() and a.min() >= 0 and (a.max(axis=0) <= np.asarray(nvec) - 1).all()
        assert eff[np.arange(m)[:, None], off[:-1][None, :] + a].all()
        assert a[0, 0] in (31, 32)
        u = mk.sample_u(m, D, 5, 9)
        assert cdf_consistent(zp, u, nvec, st, a)
        assert not cdf_consistent(zp, u, nvec, st, np.roll(a, 1, axis=0))          # the check tells rows apart
        zero = np.zeros(m)
        ref = mk.head_f64(zp, act, zero, zero, EPS, 0.0, nvec, st)
        b = mk.head_bounds(zp, act, zero, zero, EPS, 0.0, nvec, st)
        assert (np.abs(lp.astype(F64) - ref["lp"]) <= b["lp"]).all()
        g = run_argmax(lib, zp, nvec, mk.pack(st))
        np.testing.assert_array_equal(g[:, :D].astype(np.int64), mk.argmax(zp, nvec, st))
    no_error(lib)


# ----------------------------------------------------------------------------- 4. / 5. one policy step
SIZES, N, B, SEED = [5, 16, 9], 256, 64, 11
ACTS = ["relu", "none"]
POLICIES = [("md-3-4-2", [3, 4, 2], 2), ("cat-9", [9], 1), ("md-5-4", [5, 4], 2)]


def make_ppo(lib, nvec, dist, masked, seed=5):
    C.CDLL("libc.so.6").srand(seed)
    ppo = lib.create_ppo(ppo_ffi.c_strings(ACTS), ppo_ffi.c_ints(SIZES), len(SIZES), N, 3e-4, 3e-4, 0.95, EPS, ENT, 1.0,
                         True)
    if dist == 1:
        assert lib.ppo_set_action_dist(ppo, 1) == 0
    else:
        assert lib.ppo_set_action_multidiscrete(ppo, ppo_ffi.c_ints(nvec), len(nvec)) == 0
    if masked:
        assert lib.ppo_set_action_mask(ppo, 1) == 0 and lib.ppo_get_action_mask(ppo) == 1
        assert lib.ppo_action_mask_words(ppo) == mk.words(SIZES[-1])
    return ppo


def read_store(lib, ppo, n=N):
    W = lib.ppo_action_mask_words(ppo)
    return ppo_ffi.d2h(lib, lib.ppo_action_mask_buffer(ppo), U32, n * W).reshape(n, W)


def update(lib, ppo, stored=None):
    """ppo_fill_synthetic (which lays full masks), then the caller's masks into the store, one policy step"""
    lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 100)
    if stored is not None:
        lib.ppo_synchronize()
        assert (read_store(lib, ppo) == 0xFFFFFFFF).all()
        ppo_ffi.h2d(lib, lib.ppo_action_mask_buffer(ppo), mk.pack(stored))
    lib.ppo_reset_stats(ppo)
    lib.ppo_set_step_limit(ppo, 0, 1)
    lib.ppo_update(ppo, 0.99, B, 1, 0, 1, SEED)
    lib.ppo_synchronize()


def read_buffer(lib, ppo):
    b = ppo.contents.buffer.contents
    S, A = SIZES[0], SIZES[-1]
    return dict(state=ppo_ffi.d2h(lib, b.d_state_p, F32, N * S).reshape(N, S),
                act=ppo_ffi.d2h(lib, b.d_action_p, F32, N * A).reshape(N, A),
                old=ppo_ffi.d2h(lib, b.d_logprob_p, F32, N), adv=ppo_ffi.d2h(lib, b.d_advantage_p, F32, N))


def update_masks(nvec):
    """the store's contents for the update tests: random bits, rows 0 … 7 with an all-zero first component; the
    sampled actions contradict them freely — rule 3 covers it"""
    st = mk.random_masks(nvec, N, 61)
    st[:8, :nvec[0]] = False
    return st


@pytest.mark.parametrize("case", POLICIES, ids=lambda c: c[0])
def test_policy_step(lib, oracle, case):
    """A fresh {5, 16, 9} PPO, buffer 256, batch 64, masks written into ppo_action_mask_buffer, target KL on "measure
    only", ppo_update capped at one policy step with split-K atomics off: μ's gradient is the float64 masked head's
    pushed through the restated backward (gemm_tol at K = B), the parameters Adam's first step of it; the step's KL
    and clip fraction are kl_ref's on the masked log-prob within the bound test_gpu_multidiscrete derives; and with
    the store left full the parameter bytes equal those of a run with masking off."""
    _, nvec, dist = case
    lib.ppo_gemm_tune(-1, 1)
    try:
        one, full, off_ = make_ppo(lib, nvec, dist, 1), make_ppo(lib, nvec, dist, 1), make_ppo(lib, nvec, dist, 0)
        mu = one.contents.policy.contents.mu
        mu0 = nn_params_packed(lib, mu)
        assert lib.ppo_set_target_kl(one, float("inf")) == 0
        stored = update_masks(nvec)
        update(lib, one, stored)
        update(lib, full)
        update(lib, off_)
    finally:
        lib.ppo_gemm_tune(-1, 0)
    assert lib.ppo_action_mask_buffer(off_) is None and lib.ppo_get_action_mask(off_) == 0
    p_full, p_off = (nn_params_packed(lib, p.contents.policy.contents.mu) for p in (full, off_))
    assert p_full.tobytes() == p_off.tobytes() and (p_off != mu0).any()
    assert (read_store(lib, one) == mk.pack(stored)).all()
    buf = read_buffer(lib, one)
    lr = 3e-4
    r1 = oracle.feistel_perm(N, oracle.splitmix64(SEED))[:B]
    np.testing.assert_array_equal(nn_input_rows(lib, mu, B), buf["state"][r1])
    hs, _ = tanh_ref.forward(SIZES, ACTS, mu0, buf["state"][r1])
    z = hs[-1].astype(F32)
    args = (z, buf["act"][r1], buf["adv"][r1], buf["old"][r1], EPS, ENT, nvec, stored[r1])
    head = mk.head_f64(*args)
    assert (~head["eff"]).any() and not stored[r1][np.arange(B), mk.indices(buf["act"][r1], nvec)[:, 0]].all()
    g1 = tanh_ref.backward(SIZES, ACTS, mu0, hs, head["grad"])[0]
    got_g1 = nn_grads_packed(lib, mu)
    print(f"{case[0]}: gradient error / tolerance {np.abs(got_g1 - g1).max() / gemm_tol(g1, B):.3f}")
    assert np.abs(got_g1 - g1).max() <= gemm_tol(g1, B)
    unmasked = md.head_f64(*args[:-1])["grad"]
    assert np.abs(tanh_ref.backward(SIZES, ACTS, mu0, hs, unmasked)[0] - g1).max() > 10 * gemm_tol(g1, B)
    mu1 = nn_params_packed(lib, mu)
    flips = assert_adam_delta(mu1, adam_first_step(mu0, g1, lr), g1, lr, "step 1")
    assert flips <= max(2, mu1.size // 1000)
    # the KL monitor on the masked joint lp
    st = (C.c_double * 17)()
    lib.ppo_read_stats(one, st, 17)
    hist = (C.c_double * 2)()
    assert lib.ppo_kl_history(one, hist, 2) == 1 and hist[0] == st[13]
    want = kl_ref.approx_kl(head["lp"], buf["old"][r1])
    lp_err = (mk.head_bounds(*args)["lp"].max() + 2 * len(nvec) * (gemm_tol(z, SIZES[1]) + U * np.abs(z).max()))
    x = head["lp"] - buf["old"][r1].astype(F64)
    bound = np.abs(np.expm1(x)).max() * lp_err + lp_err ** 2 + U * want + 1e-12
    print(f"{case[0]}: kl device {hist[0]:.6e} model {want:.6e} error / bound {abs(hist[0] - want) / bound:.3f}")
    assert abs(hist[0] - want) <= bound, (hist[0], want, bound)
    assert abs(want - kl_ref.approx_kl(md.head_f64(*args[:-1])["lp"], buf["old"][r1])) > 100 * bound
    # the clip fraction: exact but for the rows whose |ratio − 1| is within the lp error (and fp32's rounding) of ε
    dist_eps = np.abs(np.abs(np.exp(x) - 1.0) - EPS)
    unsure = int((dist_eps <= np.exp(x) * np.expm1(lp_err) + 4 * U).sum())
    frac = kl_ref.clip_fraction(head["lp"], buf["old"][r1], EPS)
    assert abs(st[14] - frac) <= unsure / B + 1e-7, (st[14], frac, unsure)
    no_error(lib)
    for p in (one, full, off_):
        lib.free_ppo(p)


# -------------------------------------------------------------------------------------- 6. open rollout
def table_masks(nvec, E, t):
    """the table-driven environment's masks at counter t: column k of environment e is allowed when
    (k + e + t) % 3 != 0, every (e + t) % 5 == 0 environment leaves its first component all-zero"""
    A = sum(nvec)
    e, k = np.indices((E, A))
    st = (k + e + t) % 3 != 0
    st[(np.arange(E) + t) % 5 == 0, :nvec[0]] = False
    return st


@pytest.mark.parametrize("case", POLICIES[:2], ids=lambda c: c[0])
def test_open_rollout(lib, case):
    """E = 8, T = 5, a table-driven environment whose mask depends on its counter: every stored action is allowed by
    the (effective) mask stored at its row, the stored masks are the ones passed, the stored log-prob is the mirror's
    within the lp bound (the logits restated from the stored observations), ppo_act_device_masked at the same seed
    and step agrees with ppo_rollout_act_masked bit for bit, its deterministic form is the masked argmax, a plain
    ppo_rollout_act lays full masks, and a following ppo_update leaves ppo_last_error empty and the parameters
    finite."""
    _, nvec, dist = case
    E, T, seed = 8, 5, 29
    S, A, D, W = SIZES[0], SIZES[-1], len(nvec), mk.words(SIZES[-1])
    ppo = make_ppo(lib, nvec, dist, 1, seed=9)
    rng = np.random.default_rng(3)
    obs = rng.uniform(-1, 1, (T + 1, E, S)).astype(F32)
    d_obs, d_nxt = dev(lib, obs[0]), empty(lib, E * S)
    d_act, d_act2, d_lp, d_rew = empty(lib, E * A), empty(lib, E * A), empty(lib, E), dev(lib, np.ones(E, F32))
    d_flag, d_mask = dev(lib, np.zeros(E, np.uint8)), empty(lib, E * W, U32)
    assert lib.ppo_rollout_begin(ppo, E, T, d_obs.ptr, seed) == 0
    plain_t = 3                                               # one step acts unmasked: its rows get full masks
    for t in range(T):
        st = table_masks(nvec, E, t)
        ppo_ffi.h2d(lib, d_mask.ptr, mk.pack(st))
        if t == plain_t:
            step = lib.ppo_rollout_act(ppo, d_act.ptr)
        else:
            step = lib.ppo_rollout_act_masked(ppo, d_mask.ptr, d_act.ptr)
        assert step >= 0
        lib.ppo_synchronize()
        act = d_act.to_numpy(F32, E * A).reshape(E, A)
        if t != plain_t:
            ppo_ffi.h2d(lib, d_obs.ptr, obs[t])
            assert lib.ppo_act_device_masked(ppo, d_obs.ptr, d_mask.ptr, E, 0, seed, step, d_act2.ptr, d_lp.ptr) == 0
            lib.ppo_synchronize()
            assert d_act2.to_numpy(F32, E * A).tobytes() == act.tobytes()
            b = ppo.contents.buffer.contents
            lp_buf = ppo_ffi.d2h(lib, b.d_logprob_p, F32, E * T)[np.arange(E) * T + t]
            assert d_lp.to_numpy(F32, E).tobytes() == lp_buf.tobytes()
            assert lib.ppo_act_device_masked(ppo, d_obs.ptr, d_mask.ptr, E, 1, seed, step, d_act2.ptr, None) == 0
            lib.ppo_synchronize()
            greedy = d_act2.to_numpy(F32, E * A).reshape(E, A)
            eff = mk.effective(st, nvec)
            off = mk.offsets(nvec)
            assert eff[np.arange(E)[:, None], off[:-1][None, :] + greedy[:, :D].astype(np.int64)].all()
        ppo_ffi.h2d(lib, d_nxt.ptr, obs[t + 1])
        assert lib.ppo_rollout_store(ppo, d_rew.ptr, d_nxt.ptr, d_flag.ptr, d_flag.ptr, None) == 0
    assert lib.ppo_rollout_end(ppo) == 0
    lib.ppo_synchronize()
    b = ppo.contents.buffer.contents
    n = E * T
    acts = ppo_ffi.d2h(lib, b.d_action_p, F32, n * A).reshape(E, T, A)
    lps = ppo_ffi.d2h(lib, b.d_logprob_p, F32, n).reshape(E, T)
    states = ppo_ffi.d2h(lib, b.d_state_p, F32, n * S).reshape(E, T, S)
    store = read_store(lib, ppo, n).reshape(E, T, W)
    params = nn_params_packed(lib, ppo.contents.policy.contents.mu)
    off = mk.offsets(nvec)
    for t in range(T):
        st = table_masks(nvec, E, t)
        if t == plain_t:
            assert (store[:, t] == 0xFFFFFFFF).all()
            continue
        assert (store[:, t] == mk.pack(st)).all(), f"step {t}: the stored masks are the ones passed"
        assert states[:, t].tobytes() == obs[t].tobytes()
        a = acts[:, t, :D].astype(np.int64)
        eff = mk.effective(mk.unpack(store[:, t], A), nvec)
        assert eff[np.arange(E)[:, None], off[:-1][None, :] + a].all(), f"step {t}: a stored action is masked"
        z = tanh_ref.forward(SIZES, ACTS, params, obs[t])[0][-1]
        dz = gemm_tol(z, SIZES[1]) + U * np.abs(z).max()
        zero = np.zeros(E)
        ref = mk.head_f64(z.astype(F32), acts[:, t], zero, zero, EPS, 0.0, nvec, st)
        lp_b = mk.head_bounds(z.astype(F32), acts[:, t], zero, zero, EPS, 0.0, nvec, st)["lp"] + 2 * D * dz
        assert (np.abs(lps[:, t].astype(F64) - ref["lp"]) <= lp_b).all(), f"step {t}: log-prob"
        # the sampler's mirror under the policy-noise stream, away from the CDF's steps
        import rng_ref as R
        u = mk.sample_u(E, D, R.rollout_key(seed), cr.K_NOISE + int(t))
        a_ref, _, margin = mk.sample_f32(z.astype(F32), u, nvec, st)
        near = margin <= 2 * (np.asarray(nvec, F64)[None, :] + 70) * U + 2 * U + 2 * np.expm1(2 * dz)
        np.testing.assert_array_equal(a[~near], a_ref[~near])
    lib.ppo_set_step_limit(ppo, -1, -1)
    lib.ppo_update(ppo, 0.99, 8, 1, 1, 1, SEED)
    lib.ppo_synchronize()
    no_error(lib)
    assert np.isfinite(nn_params_packed(lib, ppo.contents.policy.contents.mu)).all()
    assert (nn_params_packed(lib, ppo.contents.policy.contents.mu) != params).any()
    for a in (d_obs, d_nxt, d_act, d_act2, d_lp, d_rew, d_flag, d_mask):
        a.free()
    lib.free_ppo(ppo)


# ----------------------------------------------------------------------------------------- 7. arguments
def test_arguments(lib):
    C.CDLL("libc.so.6").srand(1)
    mkp = lambda sizes: lib.create_ppo(ppo_ffi.c_strings(ACTS), ppo_ffi.c_ints(sizes), 3, 64, 3e-4, 3e-4, 0.95, EPS,  # noqa: E731
                                       0.0, 1.0, True)
    p = mkp([4, 16, 40])
    d = empty(lib, 4 * 64)
    # Gaussian: the setter declines, nothing is on
    assert lib.ppo_set_action_mask(p, 1) == -1 and lib.ppo_get_action_mask(p) == 0
    assert lib.ppo_set_action_mask(None, 1) == -1 and lib.ppo_get_action_mask(None) == 0
    assert lib.ppo_action_mask_buffer(p) is None and lib.ppo_action_mask_words(p) == 2
    assert lib.ppo_action_mask_words(None) == 0 and lib.ppo_action_mask_buffer(None) is None
    # discrete, masking off: the masked acts decline
    assert lib.ppo_set_action_dist(p, 1) == 0
    assert lib.ppo_rollout_begin(p, 4, 2, d.ptr, 1) == 0
    assert lib.ppo_rollout_act_masked(p, d.ptr, d.ptr) == -1
    assert lib.ppo_act_device_masked(p, d.ptr, d.ptr, 4, 0, 1, 0, d.ptr, d.ptr) == -1
    # on: a NULL mask declines; the store is all ones; off again frees it
    assert lib.ppo_set_action_mask(p, 1) == 0 and lib.ppo_get_action_mask(p) == 1
    assert lib.ppo_rollout_act_masked(p, None, d.ptr) == -1 and lib.ppo_rollout_act_masked(None, d.ptr, d.ptr) == -1
    assert lib.ppo_act_device_masked(p, d.ptr, None, 4, 0, 1, 0, d.ptr, d.ptr) == -1
    assert lib.ppo_act_device_masked(p, None, d.ptr, 4, 0, 1, 0, d.ptr, d.ptr) == -1
    assert lib.ppo_act_device_masked(p, d.ptr, d.ptr, 0, 0, 1, 0, d.ptr, d.ptr) == -1
    assert (read_store(lib, p, 64) == 0xFFFFFFFF).all()
    # the setters re-initialise the store; dist 0 turns masking off
    ppo_ffi.h2d(lib, lib.ppo_action_mask_buffer(p), np.zeros((64, 2), U32))
    assert lib.ppo_set_action_multidiscrete(p, ppo_ffi.c_ints([33, 7]), 2) == 0 and lib.ppo_get_action_mask(p) == 1
    assert (read_store(lib, p, 64) == 0xFFFFFFFF).all()
    ppo_ffi.h2d(lib, lib.ppo_action_mask_buffer(p), np.zeros((64, 2), U32))
    assert lib.ppo_set_action_dist(p, 1) == 0 and (read_store(lib, p, 64) == 0xFFFFFFFF).all()
    assert lib.ppo_set_action_dist(p, 0) == 0 and lib.ppo_get_action_mask(p) == 0
    assert lib.ppo_action_mask_buffer(p) is None
    assert lib.ppo_set_action_dist(p, 1) == 0 and lib.ppo_get_action_mask(p) == 0       # it stays off
    assert lib.ppo_set_action_mask(p, 1) == 0 and lib.ppo_set_action_mask(p, 0) == 0
    assert lib.ppo_action_mask_buffer(p) is None
    # the test entries
    loss = C.c_double(0)
    ok = ppo_ffi.c_ints([2, 2])
    head = lambda z, m, A, nv, D, eps=EPS, mask=d.ptr, g=d.ptr: lib.ppo_masked_head_device(  # noqa: E731
        z, d.ptr, d.ptr, d.ptr, mask, None, m, A, nv, D, eps, 0.0, g, d.ptr, d.ptr, C.byref(loss))
    assert head(None, 4, 4, ok, 2) == -1 and head(d.ptr, 0, 4, ok, 2) == -1 and head(d.ptr, 4, 4, None, 2) == -1
    assert head(d.ptr, 4, 5, ok, 2) == -1 and head(d.ptr, 4, 4, ok, 0) == -1 and head(d.ptr, 4, 4, ok, 257) == -1
    assert head(d.ptr, 4, 4, ppo_ffi.c_ints([3, 1]), 2) == -1 and head(d.ptr, 4, 4, ok, 2, float("nan")) == -1
    assert head(d.ptr, 4, 4098, ppo_ffi.c_ints([2049, 2049]), 2) == -1
    assert head(d.ptr, 4, 4, ok, 2, mask=None) == -1 and head(d.ptr, 4, 4, ok, 2, g=None) == -1
    samp = lambda z, m, A, nv, D, mask=d.ptr, act=d.ptr: lib.ppo_masked_sample_device(  # noqa: E731
        z, mask, m, A, nv, D, 1, 0, act, d.ptr)
    assert samp(None, 4, 4, ok, 2) == -1 and samp(d.ptr, 0, 4, ok, 2) == -1 and samp(d.ptr, 4, 4, None, 2) == -1
    assert samp(d.ptr, 4, 5, ok, 2) == -1 and samp(d.ptr, 4, 4, ok, 2, act=None) == -1
    assert samp(d.ptr, 4, 4, ok, 2, mask=None) == -1
    amax = lambda z, m, A, nv, D, mask=d.ptr, act=d.ptr: lib.ppo_masked_argmax_device(z, mask, m, A, nv, D, act)  # noqa: E731
    assert amax(None, 4, 4, ok, 2) == -1 and amax(d.ptr, 0, 4, ok, 2) == -1 and amax(d.ptr, 4, 4, None, 2) == -1
    assert amax(d.ptr, 4, 5, ok, 2) == -1 and amax(d.ptr, 4, 4, ok, 2, act=None) == -1
    assert amax(d.ptr, 4, 4, ok, 2, mask=None) == -1
    d.free()
    no_error(lib)
    lib.free_ppo(p)
