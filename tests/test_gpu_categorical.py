"""The categorical policy on the device (ppo_set_action_dist; csrc/categorical.hip, csrc/discrete.hip) against
tests/categorical_ref.py: the head row by row, the sampler, a whole update, and the argument handling.  Every bound comes from
categorical_ref (derived from the rounding of the listed operations and validated by the fp32 mirror on the CPU in
test_categorical_cpu.py); nothing is taken from a run of the kernels.

Largest error / bound ratios observed on an MI355X (printed by every run): see test_head_rows' docstring."""
import ctypes as C

import numpy as np
import pytest

import categorical_ref as cr
import kl_ref
import ppo_ffi
import tanh_ref
from categorical_ref import ENT, EPS, F32, F64, U
from helpers import dev, empty, gemm_tol, nn_grads_packed, nn_input_rows, nn_params_packed
from test_gpu_update import adam_first_step, assert_adam_delta

pytestmark = pytest.mark.gpu

SIZES_A = [2, 3, 17, 32, 33, 64, 65, 257]
SIZES_M = [1, 63, 64, 257]
WORST = {}


def no_error(lib):
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


def run_head(lib, i, ent=ENT):
    m, A = i["z"].shape
    d = dict(z=dev(lib, i["z"]), act=dev(lib, i["act"]), adv=dev(lib, i["adv"]), old=dev(lib, i["old"]),
             g=empty(lib, m * A), lp=empty(lib, m), H=empty(lib, m))
    try:
        loss = C.c_double(np.nan)
        rc = lib.ppo_categorical_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, m, A, EPS, ent,
                                             d["g"].ptr, d["lp"].ptr, d["H"].ptr, C.byref(loss))
        assert rc == 0
        return dict(grad=d["g"].to_numpy(F32, m * A).reshape(m, A), lp=d["lp"].to_numpy(F32, m),
                    H=d["H"].to_numpy(F32, m), loss=loss.value)
    finally:
        for a in d.values():
            a.free()


@pytest.mark.parametrize("A", SIZES_A)
def test_head_rows(lib, A):
    """lp, row entropy and every element of ∂loss/∂logits against the float64 model within head_bounds, at
    m ∈ {1, 63, 64, 257} (the lane-per-row / wave-per-row switch at A = 32 | 33, the wave width and its neighbours,
    a ragged last workgroup), with the ±30 row and the flat row; the loss within loss_bound.  Rows whose clip branch
    could differ (ratio on 1 ± eps) may be left out, at most 1 %: the inputs hold none.
    Observed on an MI355X: lp 0.53, H 0.22, grad 0.34 of the bound at most (A = 2 … 257, every m)."""
    full = cr.head_inputs(A)
    for m in SIZES_M:
        i = cr.rows_of(full, m)
        ref = cr.head_f64(i["z"], i["act"], i["adv"], i["old"], EPS, ENT)
        b = cr.head_bounds(i["z"], i["act"], i["adv"], i["old"], EPS, ENT)
        got = run_head(lib, i)
        what = f"A {A} m {m}"
        skip = cr.near_clip(ref["ratio"])
        assert skip.mean() <= 0.01, what
        live = ~skip & (i["adv"] != 0)
        dev_clipped = ~(got["grad"] != 0).any(axis=1)
        # with ent_coeff > 0 a clipped row keeps its entropy term: the branch shows in the first term alone
        first = run_head(lib, i, ent=0.0)["grad"]
        np.testing.assert_array_equal((~(first != 0).any(axis=1))[live], ref["clipped"][live], err_msg=what)
        assert not dev_clipped[live & ~ref["clipped"]].any(), what
        for name in ("lp", "H", "grad"):
            err = np.abs(got[name].astype(F64) - ref[name])[~skip]
            ratio = float((err / b[name][~skip]).max())
            WORST[name] = max(WORST.get(name, 0.0), ratio)
            print(f"{what}: {name} error / bound {ratio:.3f}")
            assert (err <= b[name][~skip]).all(), f"{what}: {name} at {ratio:.3g} of the bound"
        bound = cr.loss_bound(ref, b, m, ENT)
        print(f"{what}: loss error / bound {abs(got['loss'] - ref['loss']) / bound:.3f}")
        assert abs(got["loss"] - ref["loss"]) <= bound, f"{what}: loss {got['loss']} vs {ref['loss']} ± {bound}"
    print(f"largest error / bound so far: {WORST}")
    no_error(lib)


@pytest.mark.parametrize("A", [513, 1024, 1025, 2048, 2049, 4096])
def test_head_rows_wide(lib, A):
    """The wave-per-row instantiations above A = 512 (16, 32 and 64 logits per lane) up to the head's limit, 5 rows
    (two workgroups, the second ragged): the same per-row checks against the same bounds."""
    i = cr.head_inputs(A, 5)
    ref = cr.head_f64(i["z"], i["act"], i["adv"], i["old"], EPS, ENT)
    b = cr.head_bounds(i["z"], i["act"], i["adv"], i["old"], EPS, ENT)
    got = run_head(lib, i)
    assert not cr.near_clip(ref["ratio"]).any()
    for name in ("lp", "H", "grad"):
        err = np.abs(got[name].astype(F64) - ref[name])
        print(f"A {A} m 5: {name} error / bound {float((err / b[name]).max()):.3f}")
        assert (err <= b[name]).all(), name
    assert abs(got["loss"] - ref["loss"]) <= cr.loss_bound(ref, b, 5, ENT)
    no_error(lib)


def run_sampler(lib, z, key, offset):
    m, A = z.shape
    d = dict(z=dev(lib, z), act=dev(lib, np.full((m, A), np.nan, F32)), lp=empty(lib, m))
    try:
        assert lib.ppo_categorical_sample_device(d["z"].ptr, m, A, key, offset, d["act"].ptr, d["lp"].ptr) == 0
        return d["act"].to_numpy(F32, m * A).reshape(m, A), d["lp"].to_numpy(F32, m)
    finally:
        for a in d.values():
            a.free()


@pytest.mark.parametrize("A", [2, 6, 65])
def test_sampler(lib, A):
    """65 536 rows: the index equals the mirror's on every row whose threshold is further than the bound from a
    cumulative boundary (the others, under 1 % — the mirror's own count is pinned on the CPU — may differ by the
    device's expf), the log-prob is the chosen index's within head_bounds' lp, columns 1 … A−1 are zero."""
    z = cr.sample_inputs(A)
    m = z.shape[0]
    act, lp = run_sampler(lib, z, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET)
    a_ref, _, margin = cr.sample_f32(z, cr.sample_u(m, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET))
    near = margin <= 2 * (A + 70) * U + 2 * U
    assert near.mean() < 0.01
    a = act[:, 0].astype(np.int64)
    assert (act[:, 0] == a).all() and a.min() >= 0 and a.max() <= A - 1
    assert not act[:, 1:].any() and not np.signbit(act[:, 1:]).any()
    np.testing.assert_array_equal(a[~near], a_ref[~near])
    ref = cr.head_f64(z, act, np.zeros(m), np.zeros(m), EPS, 0.0)
    b = cr.head_bounds(z, act, np.zeros(m), np.zeros(m), EPS, 0.0)
    err = np.abs(lp.astype(F64) - ref["lp"])
    print(f"A {A}: {int((a != a_ref).sum())} rows differ from the mirror ({int(near.sum())} near a boundary); "
          f"lp error / bound {float((err / b['lp']).max()):.3f}")
    assert (err <= b["lp"]).all()
    no_error(lib)


def test_sampler_frequencies(lib):
    """A = 6, every row the same logits: the empirical frequencies within 5 standard deviations of the multinomial."""
    A = 6
    z = cr.sample_inputs(A, shared_row=True)
    m = z.shape[0]
    act, _ = run_sampler(lib, z, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET)
    p = cr.head_f64(z[:1], np.zeros((1, A)), np.zeros(1), np.zeros(1), EPS, 0.0)["p"][0]
    freq = np.bincount(act[:, 0].astype(np.int64), minlength=A) / m
    assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / m)).all(), (freq, p)


# ----------------------------------------------------------------------------------------- the whole update
SIZES, N, B, SEED = [8, 64, 6], 512, 128, 11
ACTS = ["relu", "none"]


def make_ppo(lib, ent_coeff=ENT, cat=True, seed=5):
    C.CDLL("libc.so.6").srand(seed)
    ppo = lib.create_ppo(ppo_ffi.c_strings(ACTS), ppo_ffi.c_ints(SIZES), len(SIZES), N, 3e-4, 3e-4, 0.95, EPS, ent_coeff,
                         1.0, True)
    if cat:
        assert lib.ppo_set_action_dist(ppo, 1) == 0 and lib.ppo_get_action_dist(ppo) == 1
    return ppo


def update(lib, ppo, steps):
    lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 100)
    lib.ppo_reset_stats(ppo)
    lib.ppo_set_step_limit(ppo, 0, steps)
    lib.ppo_update(ppo, 0.99, B, 1, 0, 1, SEED)
    lib.ppo_synchronize()


def read_buffer(lib, ppo):
    b = ppo.contents.buffer.contents
    S, A = SIZES[0], SIZES[-1]
    return dict(state=ppo_ffi.d2h(lib, b.d_state_p, F32, N * S).reshape(N, S),
                act=ppo_ffi.d2h(lib, b.d_action_p, F32, N * A).reshape(N, A),
                old=ppo_ffi.d2h(lib, b.d_logprob_p, F32, N), adv=ppo_ffi.d2h(lib, b.d_advantage_p, F32, N))


def log_std(lib, ppo):
    pol = ppo.contents.policy.contents
    return ppo_ffi.d2h(lib, pol.d_log_std, F32, pol.action_size)


def step_rows(lib, oracle, ppo, buf, k):
    """The buffer rows of policy step k: the first policy epoch's device Feistel order under the first key of SEED
    (no value epoch drew one), positions k·B … k·B + B − 1."""
    perm = oracle.feistel_perm(N, oracle.splitmix64(SEED))
    return perm[k * B:(k + 1) * B]


def model_step(params, buf, rows, ent):
    """The float64 restatement of one policy step from fp32 parameters: forward, the model's head, backward."""
    hs, _ = tanh_ref.forward(SIZES, ACTS, params, buf["state"][rows])
    head = cr.head_f64(hs[-1].astype(F32), buf["act"][rows], buf["adv"][rows], buf["old"][rows], EPS, ent)
    return tanh_ref.backward(SIZES, ACTS, params, hs, head["grad"])[0], head, hs[-1]


def adam_state(lib, ppo):
    ad = ppo.contents.adam_policy.contents
    n = nn_params_packed(lib, ppo.contents.policy.contents.mu).size
    return ppo_ffi.d2h(lib, ad.m, F32, n), ppo_ffi.d2h(lib, ad.v, F32, n), ad.time_step


@pytest.mark.parametrize("engine", [0, 1])
def test_whole_update(lib, oracle, engine):
    """A fresh {8, 64, 6} PPO, buffer 512, batch 128, filled by ppo_fill_synthetic in categorical mode; one
    ppo_update capped at 2 policy steps, on both fp32 GEMM engines.
    Step 1 (a twin capped at 1 step): μ's parameters against Adam's first step of the restated gradient, by
    test_gpu_update.py's own bound for one policy step (assert_adam_delta: exact where |g| is not tiny, 2·lr
    elsewhere; the gradient itself within gemm_tol at K = B).
    Step 2: restated from the twin's device parameters and Adam moments (so only step 2's own gradient error enters)
    with the reference Adam; the bound is that derivation applied to a second step — 1e-6·|θ| + 1e-6·lr plus Adam's
    sensitivity lr·|∂(m̂/√v̂)/∂g|·gemm_tol, never more than 2·lr; as there, at most max(2, n/1000) entries may sit
    beyond it (a tiny gradient's sign flip between the twins' first steps) and none beyond 4·lr.
    log σ stays bit-identical, out[4] is the mirror's mean row entropy, the last step's rows are the Feistel order's."""
    prev = lib.ppo_gemm_f32_engine(engine)
    try:
        one, two = make_ppo(lib), make_ppo(lib)
        mu0 = nn_params_packed(lib, one.contents.policy.contents.mu)
        ls0 = log_std(lib, one)
        update(lib, one, 1)
        update(lib, two, 2)
        buf = read_buffer(lib, one)
        assert read_buffer(lib, two)["act"].tobytes() == buf["act"].tobytes()
        a = buf["act"][:, 0]
        assert (a == a.astype(int)).all() and a.min() >= 0 and a.max() <= 5 and not buf["act"][:, 1:].any()
        assert len(np.unique(a)) == 6
        lr = 3e-4
        # step 1
        r1 = step_rows(lib, oracle, one, buf, 0)
        np.testing.assert_array_equal(nn_input_rows(lib, one.contents.policy.contents.mu, B), buf["state"][r1])
        g1, head1, _ = model_step(mu0, buf, r1, ENT)
        got_g1 = nn_grads_packed(lib, one.contents.policy.contents.mu)
        assert np.abs(got_g1 - g1).max() <= gemm_tol(g1, B)
        mu1 = nn_params_packed(lib, one.contents.policy.contents.mu)
        flips = assert_adam_delta(mu1, adam_first_step(mu0, g1, lr), g1, lr, "step 1")
        assert flips <= max(2, mu1.size // 1000)
        # step 2, from the twin's device state
        m1, v1, t1 = adam_state(lib, one)
        assert t1 == 1 and two.contents.adam_policy.contents.time_step == 2
        r2 = step_rows(lib, oracle, two, buf, 1)
        np.testing.assert_array_equal(nn_input_rows(lib, two.contents.policy.contents.mu, B), buf["state"][r2])
        g2, head2, z2 = model_step(mu1, buf, r2, ENT)
        want, m2, v2 = mu1.copy(), m1.copy(), v1.copy()
        assert oracle.adam_update(want, g2.astype(F32), m2, v2, 1, lr) == 2
        mu2 = nn_params_packed(lib, two.contents.policy.contents.mu)
        tol = gemm_tol(g2, B)
        mh, vh = m2.astype(F64) / (1 - 0.9 ** 2), v2.astype(F64) / (1 - 0.999 ** 2)
        den = np.sqrt(vh) + 1e-8
        dm = 0.1 * tol / (1 - 0.9 ** 2)
        dv = 0.001 * (2 * np.abs(g2) * tol + tol * tol) / (1 - 0.999 ** 2)
        sens = dm / den + np.abs(mh) / den * (dv / (2 * np.maximum(vh, 1e-300))) * (np.sqrt(vh) / den)
        bound = np.minimum(1e-6 * np.abs(want) + 1e-6 * lr + lr * sens, 2 * lr * 1.0001 + 1e-7)
        err = np.abs(mu2.astype(F64) - want)
        over = int((err > bound).sum())
        print(f"engine {engine}: step 2 worst error / bound {float((err / bound).max()):.3f}, {over} entries beyond")
        assert over <= max(2, mu2.size // 1000) and err.max() <= 4 * lr * 1.0001 + 2e-7
        # log σ, the entropy word, the loss word
        assert log_std(lib, two).tobytes() == ls0.tobytes() == log_std(lib, one).tobytes()
        st = (C.c_double * 5)()
        lib.ppo_read_stats(two, st, 5)
        mirror = cr.head_f32(z2.astype(F32), buf["act"][r2], buf["adv"][r2], buf["old"][r2], EPS, ENT)
        Hm = float(mirror["H"].astype(F64).mean())
        b2 = cr.head_bounds(z2.astype(F32), buf["act"][r2], buf["adv"][r2], buf["old"][r2], EPS, ENT)
        # the device's logits differ from the restated ones by the forward's GEMM error: |∂H/∂z| ≤ |log p| + H per
        # column, over A columns
        dz = gemm_tol(z2, SIZES[1])
        slack = (B + 2) * U * np.log(6) + b2["H"].mean() + 6 * dz * (np.abs(np.log(head2["p"])).max() + np.log(6))
        assert st[3] == 2 and abs(st[4] - Hm) <= slack, (st[4], Hm, slack)
        no_error(lib)
        lib.free_ppo(one)
        lib.free_ppo(two)
    finally:
        lib.ppo_gemm_f32_engine(prev)


def test_update_kl_and_clipping(lib, oracle):
    """The same update with ppo_set_target_kl(+inf): ppo_kl_history is the model's k3 estimator at both steps.  Step
    1's x = lp − old_lp is rounding only (the buffer's log-probs are the policy's own); step 2's is the first Adam
    step's effect, restated from the device μ of a twin capped at one step (atomic-free gradient products, so the
    twins' first steps are the same bits).  The bound per step: k3′(x) = expm1(x), so |δk3| ≤ |expm1(x)|·lp_err +
    lp_err² with lp_err the head's lp bound plus the forward's GEMM tolerance on the logits (|∂lp/∂z|₁ ≤ 2), plus the
    record's fp32 storage.
    With ppo_set_max_grad_norm(1e-3) both steps clip (the counters say so); with 0.5 the update only has to run
    and report the restated gradient's norm — whether it clips depends on that norm."""
    lib.ppo_gemm_tune(-1, 1)
    try:
        one, ppo = make_ppo(lib), make_ppo(lib)
        mu0 = nn_params_packed(lib, ppo.contents.policy.contents.mu)
        for p in (one, ppo):
            assert lib.ppo_set_target_kl(p, float("inf")) == 0
        update(lib, one, 1)
        update(lib, ppo, 2)
    finally:
        lib.ppo_gemm_tune(-1, 0)
    hist = (C.c_double * 4)()
    assert lib.ppo_kl_history(ppo, hist, 4) == 2
    buf = read_buffer(lib, ppo)
    mu1 = nn_params_packed(lib, one.contents.policy.contents.mu)
    assert (mu1 != mu0).any()
    for k, params in enumerate((mu0, mu1)):
        r = step_rows(lib, oracle, ppo, buf, k)
        _, head, z = model_step(params, buf, r, ENT)
        want = kl_ref.approx_kl(head["lp"], buf["old"][r])
        lp_err = (cr.head_bounds(z.astype(F32), buf["act"][r], buf["adv"][r], buf["old"][r], EPS, ENT)["lp"].max()
                  + 2 * (gemm_tol(z, SIZES[1]) + U * np.abs(z).max()))
        x = head["lp"] - buf["old"][r].astype(F64)
        bound = np.abs(np.expm1(x)).max() * lp_err + lp_err ** 2 + U * want + 1e-12
        print(f"kl step {k + 1}: device {hist[k]:.6e} model {want:.6e} error / bound {abs(hist[k] - want) / bound:.3f}")
        assert abs(hist[k] - want) <= bound, (k, hist[k], want, bound)
        if k == 1:
            assert want > 2 * bound                          # step 2's KL stands clear of its own bound: a real check
    lib.free_ppo(one)
    lib.free_ppo(ppo)

    ppo = make_ppo(lib)
    assert lib.ppo_set_max_grad_norm(ppo, 1e-3) == 0
    update(lib, ppo, 2)
    st = (C.c_double * 13)()
    lib.ppo_read_stats(ppo, st, 13)
    assert st[3] == 2 and st[12] == 2 and st[10] > 1e-3, list(st)
    lib.free_ppo(ppo)
    ppo = make_ppo(lib)
    assert lib.ppo_set_max_grad_norm(ppo, 0.5) == 0
    update(lib, ppo, 2)
    lib.ppo_read_stats(ppo, st, 13)
    g_last = nn_grads_packed(lib, ppo.contents.policy.contents.mu)
    assert st[3] == 2 and abs(st[10] - np.linalg.norm(g_last.astype(F64))) <= 1e-5 * st[10]
    assert (1 if st[10] > 0.5 else 0) <= st[12] <= 2
    no_error(lib)
    lib.free_ppo(ppo)


def test_off_means_off(lib):
    """dist left at 0, or set to 1 and back to 0: the parameter hash before and after a (Gaussian) update equals that
    of a PPO on which ppo_set_action_dist is never called."""
    hashes = []
    for mode in ("never", "query", "toggle"):
        ppo = make_ppo(lib, cat=False)
        if mode == "query":
            assert lib.ppo_get_action_dist(ppo) == 0
        if mode == "toggle":
            assert lib.ppo_set_action_dist(ppo, 1) == 0 and lib.ppo_set_action_dist(ppo, 0) == 0
            assert lib.ppo_get_action_dist(ppo) == 0
        h0 = lib.ppo_param_hash(ppo)
        lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 100)
        lib.ppo_gemm_tune(-1, 1)                               # atomic-free gradient products: bit-reproducible
        try:
            lib.ppo_update(ppo, 0.99, B, 2, 2, 1, SEED)
        finally:
            lib.ppo_gemm_tune(-1, 0)
        hashes.append((h0, lib.ppo_param_hash(ppo)))
        lib.free_ppo(ppo)
    assert hashes[0] == hashes[1] == hashes[2] and hashes[0][0] != hashes[0][1]
    no_error(lib)


# ------------------------------------------------------------------- the synthetic environment, categorical
def test_synthetic_rollout_categorical(lib, oracle):
    """ppo_rollout_device(kind 1) with A = 6: every step re-simulated from the stored (state, action).  The
    environment reads the index i as c = 2·i/(A − 1) − 1 for every element and −0.01·c² in the reward, which is
    rng_ref.synth_step under the one-column action c (tolerances: test_gpu_rng.py's, from the fp32 restatement);
    the index is the sampler mirror's under the "policy noise" stream at counter e wherever the threshold is further
    from a cumulative boundary than the bound plus the forward's GEMM tolerance; the log-prob is the index's; and a
    fresh twin's evaluation reproduces the rollout's episode statistics bit for bit."""
    import rng_ref as R
    from test_gpu_rng import assert_transcendental, by_step
    from test_gpu_rng import read_buffer as read_rollout

    sizes, E, T, seed = [5, 16, 6], 64, 48, 13
    S, A, n = sizes[0], sizes[-1], E * T
    mk = lambda: lib.create_ppo(ppo_ffi.c_strings(ACTS), ppo_ffi.c_ints(sizes), 3, n, 3e-4, 3e-4, 0.95, EPS, 0.0,  # noqa: E731
                                1.0, True)
    C.CDLL("libc.so.6").srand(8)
    ppo = mk()
    C.CDLL("libc.so.6").srand(8)
    twin = mk()
    for p in (ppo, twin):
        assert lib.ppo_set_action_dist(p, 1) == 0
    lib.ppo_rollout_device(ppo, E, T, 1, seed)
    lib.ppo_synchronize()
    buf = read_rollout(lib, ppo, n, S, A)
    g = np.arange(T)
    obs, act = by_step(buf["state"], E, T), by_step(buf["action"], E, T)
    idx = act[:, :, 0].astype(np.int64)
    assert (act[:, :, 0] == idx).all() and idx.min() >= 0 and idx.max() <= A - 1 and not act[:, :, 1:].any()
    assert len(np.unique(idx)) == A
    c = (F32(2) * idx.astype(F32) / F32(A - 1) - F32(1))[:, :, None]
    assert c.dtype == F32
    n64, r64, done, reset = R.synth_step(obs, c, g, seed, F64)
    n32, r32, _, _ = R.synth_step(obs, c, g, seed, F32)
    nxt, rew = by_step(buf["next_state"], E, T), by_step(buf["reward"], E, T)
    assert_transcendental(nxt, n64, n32, "categorical synthetic next_state", magnitudes=(1.0,))
    assert_transcendental(rew, r64, r32, "categorical synthetic reward")
    np.testing.assert_array_equal(by_step(buf["term"], E, T).astype(bool), done)
    follow = np.where(done[:, :, None], reset, nxt)
    assert (obs[1:].view(np.uint32) == follow[:-1].view(np.uint32)).all()
    # the sampler inside the rollout: logits restated from the stored observations
    params = nn_params_packed(lib, ppo.contents.policy.contents.mu)
    z = tanh_ref.forward(sizes, ACTS, params, obs.reshape(-1, S))[0][-1]
    dz = gemm_tol(z, sizes[1]) + U * np.abs(z).max()
    key = R.rollout_key(seed)
    u = np.concatenate([cr.sample_u(E, key, cr.K_NOISE + int(t)) for t in g])          # [T·E], step-major as obs
    a_ref, _, margin = cr.sample_f32(z.astype(F32), u)
    near = margin <= 2 * (A + 70) * U + 2 * U + 2 * np.expm1(2 * dz)
    assert near.mean() <= 0.01
    np.testing.assert_array_equal(idx.reshape(-1)[~near], a_ref[~near])
    a_rows = act.reshape(-1, A)
    ref = cr.head_f64(z.astype(F32), a_rows, np.zeros(n), np.zeros(n), EPS, 0.0)
    lp_b = cr.head_bounds(z.astype(F32), a_rows, np.zeros(n), np.zeros(n), EPS, 0.0)["lp"] + 2 * dz
    assert (np.abs(by_step(buf["logprob"], E, T).reshape(-1).astype(F64) - ref["lp"]) <= lp_b).all()
    # evaluation of a fresh twin: the same trajectory
    st = (C.c_double * 16)()
    assert lib.ppo_episode_stats(ppo, st, 16) == 16
    ev = (C.c_double * 9)()
    assert lib.ppo_eval_device(twin, E, T, 1, seed, 0, 0.99, ev, 9) == 9
    assert np.array(ev[:8]).tobytes() == np.array(st[8:16]).tobytes()
    no_error(lib)
    lib.free_ppo(ppo)
    lib.free_ppo(twin)


# ------------------------------------------------------------------------------------------------ arguments
def test_arguments(lib):
    C.CDLL("libc.so.6").srand(1)
    mk = lambda sizes: lib.create_ppo(ppo_ffi.c_strings(["relu", "none"]), ppo_ffi.c_ints(sizes), 3, 64, 3e-4, 3e-4,  # noqa: E731
                                      0.95, EPS, 0.0, 1.0, True)
    p = mk([4, 16, 2])
    assert lib.ppo_get_action_dist(p) == 0
    for bad in (-1, 2, 7):
        assert lib.ppo_set_action_dist(p, bad) == -1 and lib.ppo_get_action_dist(p) == 0
    one = mk([3, 16, 1])                                       # A < 2
    assert lib.ppo_set_action_dist(one, 1) == -1 and lib.ppo_get_action_dist(one) == 0
    assert lib.ppo_set_action_dist(one, 0) == 0
    wide = mk([4, 16, 4097])                                   # A above the head's bound
    assert lib.ppo_set_action_dist(wide, 1) == -1 and lib.ppo_get_action_dist(wide) == 0
    # bf16, both orders
    assert lib.ppo_set_action_dist(p, 1) == 0
    assert lib.ppo_set_compute_dtype(p, 1) == -1 and lib.ppo_get_action_dist(p) == 1
    assert lib.ppo_set_action_dist(p, 0) == 0 and lib.ppo_set_compute_dtype(p, 1) == 0
    assert lib.ppo_set_action_dist(p, 1) == -1 and lib.ppo_get_action_dist(p) == 0
    assert lib.ppo_set_compute_dtype(p, 0) == 0 and lib.ppo_set_action_dist(p, 1) == 0
    # kind 2 through the status-returning evaluation: Gaussian, wrong S / A
    out = (C.c_double * 9)()
    ev = lambda q: lib.ppo_eval_device(q, 4, 5, 2, 1, 0, 0.99, out, 9)  # noqa: E731
    assert ev(p) == 9                                          # S = 4, A = 2, categorical: accepted
    assert lib.ppo_set_action_dist(p, 0) == 0 and ev(p) == -1  # Gaussian
    s3 = mk([3, 16, 2])
    a3 = mk([4, 16, 3])
    for q in (s3, a3):
        assert lib.ppo_set_action_dist(q, 1) == 0 and ev(q) == -1
    assert lib.ppo_eval_device(p, 4, 5, 3, 1, 0, 0.99, out, 9) == -1
    # the test entries
    d = empty(lib, 64)
    loss = C.c_double(0)
    head = lib.ppo_categorical_head_device
    assert head(None, d.ptr, d.ptr, d.ptr, 4, 2, EPS, 0.0, d.ptr, d.ptr, d.ptr, C.byref(loss)) == -1
    assert head(d.ptr, d.ptr, d.ptr, d.ptr, 0, 2, EPS, 0.0, d.ptr, d.ptr, d.ptr, C.byref(loss)) == -1
    assert head(d.ptr, d.ptr, d.ptr, d.ptr, 4, 1, EPS, 0.0, d.ptr, d.ptr, d.ptr, C.byref(loss)) == -1
    assert head(d.ptr, d.ptr, d.ptr, d.ptr, 4, 4097, EPS, 0.0, d.ptr, d.ptr, d.ptr, C.byref(loss)) == -1
    assert head(d.ptr, d.ptr, d.ptr, d.ptr, 4, 2, float("nan"), 0.0, d.ptr, d.ptr, d.ptr, C.byref(loss)) == -1
    samp = lib.ppo_categorical_sample_device
    assert samp(None, 4, 2, 1, 0, d.ptr, d.ptr) == -1 and samp(d.ptr, 0, 2, 1, 0, d.ptr, d.ptr) == -1
    assert samp(d.ptr, 4, 1, 1, 0, d.ptr, d.ptr) == -1 and samp(d.ptr, 4, 2, 1, 0, None, d.ptr) == -1
    d.free()
    no_error(lib)
    for q in (p, one, wide, s3, a3):
        lib.free_ppo(q)
