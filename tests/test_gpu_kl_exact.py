"""The closed-form KL(old ‖ new) estimator of the KL monitor on the GPU (ppo_ext.h ppo_set_kl_estimator,
PPO_KL_EXACT; csrc/kl.hip, csrc/ppo_math.h; DESIGN.md §4 "Exact-KL estimator") against tests/kl_exact_ref.py.

1. the launch alone (ppo_policy_kl_exact_device), row by row against the float64 model on the same fp32 inputs;
2. determinism, and exactly 0 for identical inputs;  3. the monitor only observes;  4. the store;
5. step values inside an update;  6. the decision and the adaptive rate use it;  7. loopback data parallelism;
8. checkpoints, and the state hash of a PPO that never set the estimator against the parent commit's.

Kernel tolerance (check 1): |row KL − model| <= 1e-12 · Σ|term| of the row — both sides evaluate the same formula
in double on the same fp32 inputs, so they differ by the rounding of at most A <= 4096 terms at a few ulp (2.2e-16)
each and by libm's exp / log / expm1.  The inputs are drawn with O(1) differences between old and new, so the terms
themselves are not cancellation residues.  out_mean: the record keeps the sum as a float: 2·2⁻²³ relative.
"""
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import kl_exact_ref as kx
import lr_schedule_ref as lrs
import ppo_ffi
from helpers import gemm_tol, nn_params_packed

pytestmark = pytest.mark.gpu
F32, F64, U32 = np.float32, np.float64, np.uint32
K3, EXACT = 0, 1
GAMMA, EPS, ENT = 0.99, 0.2, 0.01
ROW_TOL = 1e-12
MEAN_TOL = 2.0 * 2.0 ** -23
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kl_exact_parent_hash.json")
INF = float("inf")


def no_error(lib):
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


def dev(lib, a):
    return ppo_ffi.DeviceArray.from_numpy(lib, np.ascontiguousarray(a))


def run_kernel(lib, dist, new, ls_new, old, ls_old, rows=None, action=None, mask=None, nvec=None, want_rows=True):
    """ppo_policy_kl_exact_device on host arrays → (row_kl [m] float64 | None, mean)"""
    m, A = new.shape
    arrs = [dev(lib, x) if x is not None else None
            for x in (new, ls_new, old, ls_old, None if rows is None else np.asarray(rows, np.int32), action, mask)]
    d_row = ppo_ffi.DeviceArray(lib, 8 * m) if want_rows else None
    ptr = lambda d: d.ptr if d is not None else None  # noqa: E731
    mean = C.c_double(np.nan)
    rc = lib.ppo_policy_kl_exact_device(dist, ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), ptr(arrs[3]), ptr(arrs[4]),
                                        ptr(arrs[5]), ptr(arrs[6]), m, A,
                                        ppo_ffi.c_ints(nvec) if nvec else None, len(nvec) if nvec else 0, ptr(d_row),
                                        C.byref(mean))
    assert rc == 0
    no_error(lib)
    row = d_row.to_numpy(F64, m) if want_rows else None
    for d in arrs + [d_row]:
        if d is not None:
            d.free()
    return row, mean.value


WORST = {"ratio": 0.0}


def check_rows(row, mean, kl_ref, mag_ref, what):
    ratio = np.abs(row - kl_ref) / np.maximum(mag_ref, np.finfo(F64).tiny)
    WORST["ratio"] = max(WORST["ratio"], float(ratio.max()))
    print(f"{what}: worst |row − model| / Σ|term| = {ratio.max():.3g} (worst so far {WORST['ratio']:.3g})")
    assert np.all(np.abs(row - kl_ref) <= ROW_TOL * mag_ref), f"{what}: ratio {ratio.max():.3g}"
    want = kl_ref.sum() / len(kl_ref)
    tol = (MEAN_TOL * kl_ref.sum() + ROW_TOL * mag_ref.sum()) / len(kl_ref)
    assert abs(mean - want) <= tol, f"{what}: mean {mean!r} vs {want!r}"


# ------------------------------------------------------------------------------------ 1. the launch, row by row
def gaussian_inputs(rng, m, A, store):
    old = rng.standard_normal((store, A)).astype(F32)
    new = rng.standard_normal((m, A)).astype(F32)
    return old, rng.uniform(-1, 0.5, A).astype(F32), new, rng.uniform(-1, 0.5, A).astype(F32)


@pytest.mark.parametrize("A", [1, 3, 17, 33])
def test_gaussian_rows(lib, A):
    for m in (1, 63, 257, 600):                       # one, one, two and three workgroups
        rng = np.random.default_rng(100 * A + m)
        old, lo, new, ln = gaussian_inputs(rng, m, A, m)
        kl, mag = kx.gaussian(old, lo, new, ln)
        row, mean = run_kernel(lib, 0, new, ln, old, lo)
        check_rows(row, mean, kl, mag, f"gaussian A={A} m={m}")
        # a permuted row list into a larger store
        store = m + 37
        old, lo, new, ln = gaussian_inputs(rng, m, A, store)
        rows = rng.permutation(store)[:m]
        kl, mag = kx.gaussian(old[rows], lo, new, ln)
        row, mean = run_kernel(lib, 0, new, ln, old, lo, rows=rows)
        check_rows(row, mean, kl, mag, f"gaussian A={A} m={m} permuted rows")


def test_gaussian_grid_stride(lib):
    m = 65536 + 300                                   # more rows than 256 workgroups of 256 threads take at once
    rng = np.random.default_rng(7)
    old, lo, new, ln = gaussian_inputs(rng, m, 1, m)
    kl, mag = kx.gaussian(old, lo, new, ln)
    row, mean = run_kernel(lib, 0, new, ln, old, lo)
    check_rows(row, mean, kl, mag, "gaussian grid stride")


NVECS = [[2], [3, 2, 4], [33], [70, 2], [4096]]


def discrete_inputs(rng, m, nvec, store):
    A = sum(nvec)
    old = (2 * rng.standard_normal((store, A))).astype(F32)
    new = (2 * rng.standard_normal((m, A))).astype(F32)
    action = np.zeros((m, A), F32)
    for d, n in enumerate(nvec):
        action[:, d] = rng.integers(0, n, m)
    return old, new, action


@pytest.fixture(scope="module")
def discrete_refs():
    """inputs and the float64 model of every (nvec, masked) case, computed once"""
    out = {}
    for nvec in NVECS:
        m = 5 if nvec == [4096] else 300
        rng = np.random.default_rng(sum(nvec))
        store = m + 11
        old, new, action = discrete_inputs(rng, m, nvec, store)
        rows = rng.permutation(store)[:m]
        A = sum(nvec)
        mask = rng.random((store, A)) < 0.6
        mask[rows[0], :nvec[0]] = False                               # a component with no bit set
        mask[rows[1], int(action[1, 0])] = False                      # a chosen action outside its mask
        if m > 2:
            mask[rows[2]] = True                                      # a full mask
        out[tuple(nvec), False] = (old, new, action, rows, None, kx.discrete(old[rows], new, nvec))
        out[tuple(nvec), True] = (old, new, action, rows, mask, kx.discrete(old[rows], new, nvec, mask[rows], action))
    return out


@pytest.mark.parametrize("nvec", NVECS, ids=str)
def test_discrete_rows(lib, discrete_refs, nvec):
    dist = 1 if len(nvec) == 1 else 2
    old, new, action, rows, _, (kl, mag) = discrete_refs[tuple(nvec), False]
    row, mean = run_kernel(lib, dist, new, None, old, None, rows=rows, nvec=nvec)
    check_rows(row, mean, kl, mag, f"discrete {nvec}")
    assert np.all(row >= 0)
    if dist == 1:       # the categorical policy is nvec = {A}: the same bits through dist 2
        row2, mean2 = run_kernel(lib, 2, new, None, old, None, rows=rows, nvec=nvec)
        assert row2.tobytes() == row.tobytes() and mean2 == mean


@pytest.mark.parametrize("nvec", NVECS, ids=str)
def test_masked_rows_and_poison(lib, discrete_refs, nvec):
    dist = 1 if len(nvec) == 1 else 2
    old, new, action, rows, mask, (kl, mag) = discrete_refs[tuple(nvec), True]
    words = kx.pack_mask(mask)
    row, mean = run_kernel(lib, dist, new, None, old, None, rows=rows, action=action, mask=words, nvec=nvec)
    check_rows(row, mean, kl, mag, f"masked {nvec}")
    assert np.isfinite(row).all() and np.all(row >= 0)
    # NaN / 1e30 in every masked column of both the old and the new logits: not one output bit moves
    eff = np.zeros((len(rows), sum(nvec)), bool)
    for i, r in enumerate(rows):
        o = 0
        for d, n in enumerate(nvec):
            eff[i, o:o + n] = kx.effective_mask(mask[r, o:o + n], n, action[i, d])
            o += n
    assert (~eff).any()
    p_new, p_old = new.copy(), old.copy()
    p_new[~eff] = np.where(np.arange((~eff).sum()) % 2 == 0, np.nan, F32(1e30)).astype(F32)
    sub = p_old[rows]
    sub[~eff] = np.where(np.arange((~eff).sum()) % 2 == 0, F32(1e30), np.nan).astype(F32)
    p_old[rows] = sub
    row_p, mean_p = run_kernel(lib, dist, p_new, None, p_old, None, rows=rows, action=action, mask=words, nvec=nvec)
    assert row_p.tobytes() == row.tobytes() and mean_p == mean


def test_arguments(lib):
    d = ppo_ffi.DeviceArray(lib, 4096)
    out = C.c_double(-1.0)
    f = lib.ppo_policy_kl_exact_device
    nv = ppo_ffi.c_ints([2, 2])
    p = d.ptr
    assert f(0, None, p, p, p, None, None, None, 4, 4, None, 0, None, C.byref(out)) == -1
    assert f(0, p, None, p, p, None, None, None, 4, 4, None, 0, None, C.byref(out)) == -1
    assert f(0, p, p, p, None, None, None, None, 4, 4, None, 0, None, C.byref(out)) == -1
    assert f(0, p, p, p, p, None, None, p, 4, 4, None, 0, None, C.byref(out)) == -1        # a Gaussian mask
    assert f(0, p, p, p, p, None, None, None, 0, 4, None, 0, None, C.byref(out)) == -1
    assert f(0, p, p, p, p, None, None, None, 4, 0, None, 0, None, C.byref(out)) == -1
    assert f(0, p, p, p, p, None, None, None, 4, 4, None, 0, None, None) == -1
    assert f(3, p, p, p, p, None, None, None, 4, 4, None, 0, None, C.byref(out)) == -1
    assert f(2, p, None, p, None, None, None, None, 4, 4, None, 0, None, C.byref(out)) == -1   # no nvec
    assert f(2, p, None, p, None, None, None, None, 4, 5, nv, 2, None, C.byref(out)) == -1     # Σ nvec != A
    assert f(2, p, None, p, None, None, None, p, 4, 4, nv, 2, None, C.byref(out)) == -1        # a mask, no action
    assert out.value == -1.0
    assert f(2, p, None, p, None, None, None, None, 4, 4, nv, 2, None, C.byref(out)) == 0 and out.value == 0.0
    no_error(lib)
    d.free()


# ------------------------------------------------------------------------------------ 2. determinism
def test_deterministic_and_zero_for_identical_inputs(lib, discrete_refs):
    rng = np.random.default_rng(11)
    old, lo, new, ln = gaussian_inputs(rng, 600, 17, 600)
    a = run_kernel(lib, 0, new, ln, old, lo)
    b = run_kernel(lib, 0, new, ln, old, lo)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[1] > 0
    z = run_kernel(lib, 0, old, lo, old, lo)
    assert not z[0].any() and z[1] == 0.0
    for nvec in NVECS:
        dist = 1 if len(nvec) == 1 else 2
        old, new, action, rows, mask, _ = discrete_refs[tuple(nvec), True]
        words = kx.pack_mask(mask)
        a = run_kernel(lib, dist, new, None, old, None, rows=rows, action=action, mask=words, nvec=nvec)
        b = run_kernel(lib, dist, new, None, old, None, rows=rows, action=action, mask=words, nvec=nvec)
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
        same = old[rows]
        for mk in (None, words):
            z = run_kernel(lib, dist, same, None, old, None, rows=rows, action=action if mk is not None else None,
                           mask=mk, nvec=nvec)
            assert not z[0].any() and z[1] == 0.0, nvec


# ------------------------------------------------------------------------------------ the small nets of 3 … 8
N, B, SEED = 512, 128, 23
NB = N // B


def small(lib, kind="gaussian", est=None, target=None, seed=3):
    """S = 5, two hidden layers of 16, capacity 512, filled by ppo_fill_synthetic; kind picks the policy"""
    A = {"gaussian": 3, "obsnorm": 3, "tanh": 3, "categorical": 4, "masked": 5}[kind]
    acts = ["tanh", "tanh", "none"] if kind == "tanh" else ["relu", "relu", "none"]
    C.CDLL("libc.so.6").srand(seed)
    p = lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints([5, 16, 16, A]), 4, N, 3e-4, 1e-3, 0.95, EPS, ENT, 1.0,
                       True)
    if kind == "categorical":
        assert lib.ppo_set_action_dist(p, 1) == 0
    if kind == "masked":
        assert lib.ppo_set_action_multidiscrete(p, ppo_ffi.c_ints([3, 2]), 2) == 0
        assert lib.ppo_set_action_mask(p, 1) == 0
    if kind == "obsnorm":
        assert lib.ppo_set_obs_norm(p, 5.0) == 0
    lib.ppo_fill_synthetic(p, 4, N // 4, 99, 1.0 / 100)
    if kind == "masked":
        lib.ppo_synchronize()
        mask = np.random.default_rng(5).random((N, A)) < 0.6
        ppo_ffi.h2d(lib, lib.ppo_action_mask_buffer(p), kx.pack_mask(mask))
    if est is not None:
        assert lib.ppo_set_kl_estimator(p, est) == 0 and lib.ppo_get_kl_estimator(p) == est
    if target is not None:
        assert lib.ppo_set_target_kl(p, target) == 0
    lib.ppo_reset_stats(p)
    return p


def update(lib, p, epochs=2):
    lib.ppo_update(p, GAMMA, B, epochs, 1, 1, SEED)
    lib.ppo_synchronize()
    no_error(lib)


def history(lib, p, est=None, n=64):
    h = (C.c_double * n)()
    steps = lib.ppo_kl_history(p, h, n) if est is None else lib.ppo_kl_history_est(p, est, h, n)
    return np.array(h[:min(steps, n)], F64).astype(F32)


def stats(lib, p, n=34):
    st = (C.c_double * n)()
    lib.ppo_read_stats(p, st, n)
    return list(st)


def adam_state(lib, ad):
    a = ad.contents
    return ppo_ffi.d2h(lib, a.m, F32, a.size).tobytes() + ppo_ffi.d2h(lib, a.v, F32, a.size).tobytes() + \
        struct.pack("<i", a.time_step)


def training_state(lib, p):
    c = p.contents
    pol = c.policy.contents
    A = c.buffer.contents.action_size
    return (nn_params_packed(lib, pol.mu).tobytes(), nn_params_packed(lib, c.V).tobytes(),
            ppo_ffi.d2h(lib, pol.d_log_std, F32, A).tobytes(), adam_state(lib, c.adam_policy),
            adam_state(lib, c.adam_entropy), adam_state(lib, c.adam_V))


# ------------------------------------------------------------------------------------ 3. the monitor only observes
@pytest.mark.parametrize("kind", ["gaussian", "categorical", "masked", "obsnorm", "tanh"])
def test_monitor_only_observes(lib, monkeypatch, kind):
    monkeypatch.delenv("PPO_GRAPH", raising=False)
    a, b = small(lib, kind, K3, INF), small(lib, kind, EXACT, INF)
    assert training_state(lib, a) == training_state(lib, b)
    assert lib.ppo_kl_old_dist(b, None) is None
    update(lib, a)
    update(lib, b)
    assert training_state(lib, a) == training_state(lib, b)
    k3 = history(lib, a)
    assert len(k3) == 2 * NB
    assert history(lib, b, K3).tobytes() == k3.tobytes() == history(lib, a, K3).tobytes()
    ex = history(lib, b)
    assert len(ex) == 2 * NB and ex.tobytes() == history(lib, b, EXACT).tobytes()
    assert np.all(ex >= 0) and np.isfinite(ex).all() and ex[-1] > 0 and ex.tobytes() != k3.tobytes()
    assert len(history(lib, a, EXACT)) == 0 and len(history(lib, a, 7)) == 0
    sa, sb = stats(lib, a), stats(lib, b)
    assert sa[32] == K3 and sa[33] == 0 and sa[13] == float(k3[-1])
    assert sb[32] == EXACT and sb[13] == float(ex[-1]) and sb[33] == float(k3[-1])
    assert sa[14:17] == sb[14:17] and stats(lib, b, 32) == sb[:32]
    assert lib.ppo_kl_old_dist(a, None) is None and lib.ppo_kl_old_dist(b, None) is not None
    lib.free_ppo(a)
    lib.free_ppo(b)


def test_off_means_nothing_allocated(lib):
    """EXACT with the monitor off: no store, no history, out[33] = 0; the setter declines what it does not know"""
    p = small(lib, "gaussian", EXACT)
    q = small(lib, "gaussian")
    update(lib, p)
    update(lib, q)
    assert training_state(lib, p) == training_state(lib, q)
    assert lib.ppo_kl_old_dist(p, None) is None and len(history(lib, p)) == 0
    st = stats(lib, p)
    assert st[32] == EXACT and st[33] == 0 and st[13] == 0
    for bad in (-1, 2, 1 << 20):
        assert lib.ppo_set_kl_estimator(p, bad) == -1 and lib.ppo_get_kl_estimator(p) == EXACT
    assert lib.ppo_set_kl_estimator(p, K3) == 0 and lib.ppo_get_kl_estimator(q) == K3
    lib.free_ppo(p)
    lib.free_ppo(q)


# ------------------------------------------------------------------------------------ 4. the store
def test_store_is_the_behaviour_policy(lib):
    p = small(lib, "obsnorm", EXACT, INF)
    assert lib.ppo_obs_norm_fold_buffer(p) == 0           # a pair that is not the identity …
    assert lib.ppo_obs_norm_freeze(p, 1) in (0, 1)       # … and stays: the update and the act normalise alike
    c = p.contents
    buf, pol = c.buffer.contents, c.policy.contents
    ls0 = ppo_ffi.d2h(lib, pol.d_log_std, F32, 3)
    act = ppo_ffi.DeviceArray(lib, 4 * N * 3)
    assert lib.ppo_act_device(p, buf.state_p, N, 1, 0, 0, act.ptr, None) == 0
    mu0 = act.to_numpy(F32, N * 3).reshape(N, 3)
    update(lib, p)
    ls_ptr = C.c_void_p()
    store = lib.ppo_kl_old_dist(p, C.byref(ls_ptr))
    assert store and ls_ptr.value
    got = ppo_ffi.d2h(lib, store, F32, N * 3).reshape(N, 3)
    tol = gemm_tol(mu0, 16)
    print(f"store vs ppo_act_device: max |diff| {np.abs(got - mu0).max():.3g}, bound {tol:.3g}")
    assert np.abs(got - mu0).max() <= tol
    assert ppo_ffi.d2h(lib, ls_ptr, F32, 3).tobytes() == ls0.tobytes()
    assert ppo_ffi.d2h(lib, pol.d_log_std, F32, 3).tobytes() != ls0.tobytes()      # the update moved log σ
    act.free()
    lib.free_ppo(p)


# ------------------------------------------------------------------------------------ 5. step values
def mlp64(params, sizes, x):
    """float64 forward of the ReLU MLP from its packed fp32 parameters"""
    h, off = np.asarray(x, F64), 0
    for i in range(len(sizes) - 1):
        n, l = sizes[i], sizes[i + 1]
        W = params[off:off + n * l].astype(F64).reshape(l, n)
        off += n * l
        b = params[off:off + l].astype(F64)
        off += l
        h = h @ W.T + b
        if i < len(sizes) - 2:
            h = np.maximum(h, 0)
    return h


def propagated_bound(mu_old, mu_new, ls_new):
    """|KL(gpu) − KL(model)| of a Gaussian minibatch when each fp32 forward is within δ = 3·gemm_tol (one GEMM bound
    per layer, three layers, K = 16) of the float64 μ: per column |Δμ| moves by at most 2δ, so the mean-term moves by
    at most (|Δμ|·2δ + ½(2δ)²)·exp(−2·lsn); the σ-term has the same fp32 inputs on both sides.  Plus the fp32
    rounding of the recorded sum and mean."""
    delta = 3 * max(gemm_tol(mu_old, 16), gemm_tol(mu_new, 16))
    dm = np.abs(mu_old - mu_new)
    per_row = ((dm * 2 * delta + 0.5 * (2 * delta) ** 2) * np.exp(-2.0 * ls_new.astype(F64))).sum(1)
    return float(per_row.mean())


@pytest.mark.parametrize("s", [0, 3, 5])
def test_step_values(lib, s):
    sizes = [5, 16, 16, 3]
    first, second = small(lib, "gaussian", EXACT, INF), small(lib, "gaussian", EXACT, INF)
    mu_ptr = first.contents.policy.contents.mu
    params0 = nn_params_packed(lib, mu_ptr)
    ls0 = ppo_ffi.d2h(lib, first.contents.policy.contents.d_log_std, F32, 3)
    lib.ppo_set_step_limit(first, -1, s)
    lib.ppo_set_step_limit(second, -1, s + 1)
    update(lib, first)
    update(lib, second)
    params_s = nn_params_packed(lib, mu_ptr)                  # what step s forwards with
    ls_s = ppo_ffi.d2h(lib, first.contents.policy.contents.d_log_std, F32, 3)
    rows = np.full(B, -1, np.int32)
    assert lib.ppo_adv_norm_read(second, s, rows.ctypes.data_as(C.POINTER(C.c_int)), None, B) == B
    state = ppo_ffi.d2h(lib, second.contents.buffer.contents.state_p, F32, N * 5).reshape(N, 5)[rows]
    mu_old, mu_new = mlp64(params0, sizes, state), mlp64(params_s, sizes, state)
    kl, mag = kx.gaussian(mu_old, ls0, mu_new, ls_s)
    h = history(lib, second, EXACT)
    assert len(h) == s + 1
    want = kl.mean()
    bound = propagated_bound(mu_old, mu_new, ls_s) + 2 * MEAN_TOL * mag.mean()
    print(f"step {s}: exact KL {h[s]!r}, model {want!r}, |diff| {abs(float(h[s]) - want):.3g}, bound {bound:.3g}")
    assert h[s] >= 0 and abs(float(h[s]) - want) <= bound
    if s == 0:
        assert want == 0 and h[0] <= bound                     # tiny, not necessarily 0
    else:
        assert want > 0
    lib.free_ppo(first)
    lib.free_ppo(second)


# ------------------------------------------------------------------------------------ 6. the decision uses it
@pytest.fixture(scope="module")
def measured(lib):
    p = small(lib, "gaussian", EXACT, INF)
    update(lib, p)
    h = history(lib, p)
    lib.free_ppo(p)
    assert len(h) == 2 * NB
    return h


def test_target_kl_stops_on_the_exact_value(lib, measured):
    h = measured
    vals = np.unique(h)
    k = len(vals) // 2
    thr = 0.5 * (float(vals[k - 1]) + float(vals[k]))            # strictly between two of its values
    target = F32(thr / 1.5)
    limit = F32(1.5) * target
    assert vals[k - 1] < limit < vals[k]
    j = int(np.argmax(h > limit))
    assert h[j] > limit and not (h[:j] > limit).any()
    p = small(lib, "gaussian", EXACT, float(target))
    update(lib, p)
    st = stats(lib, p)
    assert st[16] == j and st[15] == j and st[32] == EXACT
    got = history(lib, p)
    assert len(got) > j and got[:j + 1].tobytes() == h[:j + 1].tobytes()
    lib.free_ppo(p)


def test_adaptive_rate_follows_the_exact_value(lib, measured):
    want_kl = float(np.median(measured[1:]))
    lr_min, lr_max = 1e-5, 1e-2
    p = small(lib, "gaussian", EXACT)
    assert lib.ppo_set_lr_schedule(p, 2, want_kl, lr_min, lr_max) == 0
    update(lib, p)
    h = history(lib, p)
    assert len(h) == 2 * NB and h.tobytes() == history(lib, p, EXACT).tobytes()
    rates = np.zeros(2 * NB, F32)
    assert lib.ppo_lr_history(p, rates.ctypes.data_as(C.POINTER(C.c_float)), 2 * NB) == 2 * NB
    ref, _, raised, lowered = lrs.replay(lrs.initial_lr(3e-4, lr_min, lr_max), h, want_kl, lr_min, lr_max)
    assert rates.tobytes() == np.asarray(ref, F32).tobytes()
    assert raised + lowered > 0
    st = stats(lib, p)
    assert st[27] == raised and st[28] == lowered
    k3 = history(lib, p, K3)
    ref_k3 = lrs.replay(lrs.initial_lr(3e-4, lr_min, lr_max), k3, want_kl, lr_min, lr_max)[0]
    print(f"adaptive: exact {h}, k3 {k3}, rates {rates}, a k3 replay would give {np.asarray(ref_k3)}")
    lib.free_ppo(p)


# ------------------------------------------------------------------------------------ 7. loopback data parallelism
CHILD = """
    import ctypes as C, json, sys
    sys.path.insert(0, {pkg!r})
    import ppo_ffi
    lib = ppo_ffi.load()
    assert lib.ppo_set_device(0) == 0
    if {loop}:
        assert lib.ppo_comm_init(0, 1, None) == 0 and lib.ppo_comm_world() == 2
    C.CDLL("libc.so.6").srand(3)
    p = lib.create_ppo(ppo_ffi.c_strings(["relu", "relu", "none"]), ppo_ffi.c_ints([5, 16, 16, 3]), 4, 512, 3e-4, 1e-3,
                       0.95, 0.2, 0.01, 1.0, True)
    lib.ppo_fill_synthetic(p, 4, 128, 99, 1.0 / 100)
    assert lib.ppo_set_kl_estimator(p, {est}) == 0 and lib.ppo_set_target_kl(p, float("inf")) == 0
    lib.ppo_prof_enable(1)
    lib.ppo_prof_reset()
    lib.ppo_update(p, 0.99, 128, 2, 1, 1, 23)
    lib.ppo_synchronize()
    cnt = (C.c_long * 7)()
    lib.ppo_prof_counts(cnt)
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    h = (C.c_double * 16)()
    n = lib.ppo_kl_history(p, h, 16)
    k = (C.c_double * 16)()
    assert lib.ppo_kl_history_est(p, 0, k, 16) == n
    print("RESULT " + json.dumps(dict(kl=[x.hex() for x in h[:n]], k3=[x.hex() for x in k[:n]], comm=cnt[5])))
"""


def run_child(tmp_path, loop, est):
    script = tmp_path / f"kl_exact_loop{int(loop)}_{est}.py"
    script.write_text(textwrap.dedent(CHILD.format(pkg=os.path.join(ROOT, "ppo.c_amd"), loop=bool(loop), est=est)))
    env = {k: v for k, v in os.environ.items() if k not in ("PPO_COMM_LOOPBACK", "PPO_GRAPH", "PPO_SERIAL")}
    env["PPO_NO_TINY"] = "1"
    if loop:
        env.update(PPO_COMM_LOOPBACK="2", PPO_REPLICA_CHECK="1")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_loopback_ranks_decide_from_the_same_bits(lib, tmp_path):
    """Two in-process ranks holding the same shard: the all-reduced sum doubles exactly and so does the row count, so
    the exact (and the k3) history is the single-rank run's bit for bit; the sum rides in the monitor's own four-float
    all-reduce (the replica check passes inside ppo_update)."""
    one, two, two_k3 = run_child(tmp_path, False, EXACT), run_child(tmp_path, True, EXACT), run_child(tmp_path, True, K3)
    assert len(one["kl"]) == 2 * NB and one["kl"] == two["kl"] and one["k3"] == two["k3"] != one["kl"]
    assert float.fromhex(one["kl"][-1]) > 0
    # no collective is added: the same count under either estimator, and k3 keeps its bits beside the exact sum
    assert two["comm"] == two_k3["comm"] > 0 and two_k3["kl"] == two_k3["k3"] == two["k3"]


# ------------------------------------------------------------------------------------ 8. checkpoint
def test_checkpoint_keeps_the_estimator(lib, tmp_path):
    x = small(lib, "gaussian", EXACT, INF)
    update(lib, x, 1)
    path = str(tmp_path / "klest.ckpt").encode()
    assert lib.ppo_save_state(x, path, 0) == 0
    img = open(path, "rb").read()
    assert struct.unpack_from("<I", img, 12)[0] & 16
    assert struct.pack("<IIQ", 9, 0, 8) in img and struct.pack("<II", EXACT, 0) in img
    err = C.create_string_buffer(256)
    y = lib.ppo_load_state(path, err, 256)
    assert y, err.value
    assert lib.ppo_get_kl_estimator(y) == EXACT
    assert lib.ppo_state_hash(y, 0) == lib.ppo_state_hash(x, 0) != 0
    assert lib.ppo_set_kl_estimator(x, K3) == 0
    assert lib.ppo_state_hash(x, 0) != lib.ppo_state_hash(y, 0)
    # a damaged estimator is declined on the host, with a message
    at = img.index(struct.pack("<IIQ", 9, 0, 8)) + 24
    bad = bytearray(img)
    bad[at:at + 4] = struct.pack("<I", 2)
    fnv = 0xcbf29ce484222325
    for byte in bad[at:at + 8]:
        fnv = ((fnv ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    bad[at - 8:at] = struct.pack("<Q", fnv)
    (tmp_path / "bad.ckpt").write_bytes(bytes(bad))
    assert not lib.ppo_load_state(str(tmp_path / "bad.ckpt").encode(), err, 256)
    assert b"KL estimator" in err.value
    no_error(lib)
    lib.free_ppo(x)
    lib.free_ppo(y)


def test_state_hash_of_a_ppo_that_never_set_it_is_the_parent_commits(lib, monkeypatch):
    """tests/golden/kl_exact_parent_hash.json was produced on the parent commit's build by exactly these calls"""
    for k in ("PPO_NO_TINY", "PPO_GRAPH", "PPO_SERIAL"):
        monkeypatch.delenv(k, raising=False)
    gold = json.load(open(GOLDEN))
    C.CDLL("libc.so.6").srand(3)
    p = lib.create_ppo(ppo_ffi.c_strings(["relu", "relu", "none"]), ppo_ffi.c_ints([5, 16, 16, 3]), 4, 512, 3e-4, 1e-3,
                       0.95, 0.2, 0.01, 1.0, True)
    lib.ppo_fill_synthetic(p, 4, 128, 99, 1.0 / 100)
    assert f"{lib.ppo_state_hash(p, 0):016x}" == gold["fresh_0"]
    assert f"{lib.ppo_state_hash(p, 1):016x}" == gold["fresh_1"]
    assert lib.ppo_set_target_kl(p, INF) == 0
    update(lib, p)
    assert f"{lib.ppo_state_hash(p, 0):016x}" == gold["updated_0"]
    assert f"{lib.ppo_state_hash(p, 1):016x}" == gold["updated_1"]
    h = (C.c_double * 8)()
    assert lib.ppo_kl_history(p, h, 8) == 8 and [float(x).hex() for x in h] == gold["kl_hist"]
    # set and set back: still the parent's image
    assert lib.ppo_set_kl_estimator(p, EXACT) == 0 and f"{lib.ppo_state_hash(p, 0):016x}" != gold["updated_0"]
    assert lib.ppo_set_kl_estimator(p, K3) == 0 and f"{lib.ppo_state_hash(p, 0):016x}" == gold["updated_0"]
    lib.free_ppo(p)
