"""The state-dependent-σ Gaussian policy inside the library (ppo_set_action_gaussian_sd): one update against a float64
forward, head and backward over the rows the step gathered; the KL monitor's history under both estimators against
the model from the read-back rows; the rollouts against the sampler entry, the environments' own dense step and
rng_ref's synthetic model; loopback data parallelism.  Models: tanh_ref (the network) and gauss_sd_ref (the head, the
row KL); the GEMM bound is helpers.gemm_tol, the single-step comparison and constants are test_gpu_tanh.py's."""
import ctypes as C
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import gauss_sd_ref as sd
import ppo_ffi
import rng_ref as R
import tanh_ref as T
from gauss_sd_ref import F32, F64, U
from helpers import assert_gemm_close, dev, empty, gemm_tol, nn_grads_packed, nn_input_rows, nn_params_packed
from test_gpu_update import adam_first_step, assert_adam_delta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, EPS, ENT, LO, HI, SEED = 3e-4, 0.2, 0.01, -0.1, 0.1, 7   # bounds inside a fresh network's output range
U64 = np.uint64
# ro_seed: the rollout seed of test_one_update, the first of 5, 6, … at which the float64 model's log-σ outputs over
# the gathered rows keep clear of the clamp bounds (asserted on the model in the test)
CASES = {"pendulum": dict(sizes=[3, 64, 64, 2], acts=["tanh", "tanh", "none"], kind=0, E=8, T=16, B=64, ro_seed=5),
         "synthetic": dict(sizes=[5, 40, 34], acts=["tanh", "none"], kind=1, E=8, T=16, B=64, ro_seed=7)}


def no_error(lib):
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


def make(lib, sizes, acts, cap, lr=LR):
    C.CDLL("libc.so.6").srand(1234)
    ppo = lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), cap, lr, lr, 0.95, EPS, ENT, 0.7, True)
    assert lib.ppo_set_action_gaussian_sd(ppo, LO, HI) == 0
    return ppo


def rows_of(x0, states):
    where = {r.tobytes(): i for i, r in enumerate(np.ascontiguousarray(states, F32))}
    rows = np.array([where[r.tobytes()] for r in x0])
    assert len(set(rows.tolist())) == len(rows)
    return rows


def counts(lib):
    cnt = (C.c_long * 7)()
    lib.ppo_prof_counts(cnt)
    return list(cnt)


def read(lib, ppo, n, S, A):
    b = ppo.contents.buffer.contents
    return dict(state=ppo_ffi.d2h(lib, b.d_state_p, F32, n * S).reshape(n, S).copy(),
                next_state=ppo_ffi.d2h(lib, b.d_next_state_p, F32, n * S).reshape(n, S).copy(),
                action=ppo_ffi.d2h(lib, b.d_action_p, F32, n * A).reshape(n, A).copy(),
                old_lp=ppo_ffi.d2h(lib, b.d_logprob_p, F32, n).copy(),
                reward=ppo_ffi.d2h(lib, b.d_reward_p, F32, n).copy())


def near_bounds(z64, Aa, K):
    """log-σ elements within the forward's GEMM tolerance of a clamp bound: there the device and the model may sit
    on different sides"""
    t, tol = z64[:, Aa:], gemm_tol(z64, K)
    return int(((np.abs(t - LO) <= tol) | (np.abs(t - HI) <= tol)).sum())


class engine:
    def __init__(self, lib, e):
        self.lib, self.e = lib, e

    def __enter__(self):
        self.prev = self.lib.ppo_gemm_f32_engine(self.e)

    def __exit__(self, *exc):
        self.lib.ppo_gemm_f32_engine(self.prev)


# ------------------------------------------------------------------------------------------ 7. one update
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("eng", [1, 0])
def test_one_update(lib, case, eng):
    """Step limit one value step and one policy step.  μ's parameter gradient and the post-Adam parameters against
    the float64 forward (tanh_ref), head (gauss_sd_ref.head_f64) and backward over the rows the step gathered, held
    to test_gpu_tanh.py's single-step bound (gemm_tol at K = B, Adam's first step); out[4] within Aa·gemm_tol of the
    model's mean row entropy (H is a sum of Aa outputs of the forward) plus the fp32 sum's bound; out[34] and out[35]
    exact — the inputs are asserted to hold no log-σ element within the forward's tolerance of a clamp bound; log σ
    bit-identical; exactly two launches of the head class (the value step's MSE and this head), nothing replayed."""
    c = CASES[case]
    sizes, acts, E, Tn, B = c["sizes"], c["acts"], c["E"], c["T"], c["B"]
    S, A = sizes[0], sizes[-1]
    Aa, N = A // 2, E * Tn
    # the input condition, on the model alone: no log-σ element of the gathered rows within the forward's tolerance of
    # a clamp bound (there the device and the model may clamp differently)
    r = _one_update(lib, c, eng, c["ro_seed"])
    what = f"{case}, engine {eng}"
    assert near_bounds(r["z"], Aa, max(sizes)) == 0, f"{what}: a log σ output sits on a clamp bound; choose another ro_seed"
    z, hs, buf, adv, rp, mu0, mu1, gmu, st, cnt, cnt_gae = (r[k] for k in (
        "z", "hs", "buf", "adv", "rp", "mu0", "mu1", "gmu", "st", "cnt", "cnt_gae"))
    ref = sd.head_f64(z, buf["action"][rp], adv[rp], buf["old_lp"][rp], EPS, ENT, LO, HI)
    cl = sd.ls_classes(z, LO, HI)
    assert ref["clamped"] > 0 and cl["inside"] > 0, f"{what}: the step must see clamped and unclamped columns"
    gmu_ref = T.backward(sizes, acts, mu0, hs, ref["grad"])[0]
    assert_gemm_close(gmu, gmu_ref, B, f"{what} policy grads")
    flips = assert_adam_delta(mu1, adam_first_step(mu0, gmu_ref, LR), gmu_ref, LR, f"{what} policy params")
    assert flips <= max(2, mu1.size // 1000)
    assert st[1] == 1 and st[3] == 1 and st[8] == 0
    h_tol = Aa * gemm_tol(z, max(sizes)) + (Aa + 1) * U * (np.abs(ref["H"]).max() + Aa)
    assert abs(st[4] - ref["H"].mean()) <= h_tol, f"{what}: out[4] {st[4]} vs {ref['H'].mean()} ± {h_tol}"
    assert st[34] == ref["clamped"] and st[35] == B * Aa, (st[34], st[35], ref["clamped"])
    assert cnt[4] - cnt_gae[4] == 2, (cnt, cnt_gae)


def _one_update(lib, c, eng, ro_seed):
    """the device side of test_one_update and the model's forward over the rows the policy step gathered"""
    sizes, acts, E, Tn, B = c["sizes"], c["acts"], c["E"], c["T"], c["B"]
    S, A = sizes[0], sizes[-1]
    N = E * Tn
    with engine(lib, eng):
        ppo = make(lib, sizes, acts, N)
        try:
            p = ppo.contents
            pol = p.policy.contents
            lib.ppo_rollout_device(ppo, E, Tn, c["kind"], ro_seed)
            lib.ppo_synchronize()
            mu0 = nn_params_packed(lib, pol.mu)
            ls0 = ppo_ffi.d2h(lib, pol.d_log_std, F32, A).tobytes()
            buf = read(lib, ppo, N, S, A)
            lib.ppo_reset_stats(ppo)
            lib.ppo_prof_enable(1)
            lib.ppo_prof_reset()
            lib.ppo_set_step_limit(ppo, 0, 0)
            lib.ppo_update(ppo, 0.99, B, 1, 1, 1, SEED)
            lib.ppo_synchronize()
            cnt_gae = counts(lib)
            lib.ppo_prof_reset()
            lib.ppo_set_step_limit(ppo, 1, 1)
            lib.ppo_update(ppo, 0.99, B, 1, 1, 1, SEED)
            lib.ppo_synchronize()
            cnt = counts(lib)
            lib.ppo_prof_enable(0)
            no_error(lib)
            st = (C.c_double * 36)()
            lib.ppo_read_stats(ppo, st, 36)
            st = list(st)
            adv = ppo_ffi.d2h(lib, p.buffer.contents.d_advantage_p, F32, N).copy()
            rp = rows_of(nn_input_rows(lib, pol.mu, B), buf["state"])
            gmu, mu1 = nn_grads_packed(lib, pol.mu), nn_params_packed(lib, pol.mu)
            assert ppo_ffi.d2h(lib, pol.d_log_std, F32, A).tobytes() == ls0
            assert (ppo_ffi.d2h(lib, pol.d_log_std_grad, F32, A).view(np.uint32) == 0).all()
            assert p.adam_policy.contents.time_step == 1
        finally:
            lib.ppo_prof_enable(0)
            lib.free_ppo(ppo)
    hs, _ = T.forward(sizes, acts, mu0, buf["state"][rp])
    return dict(z=hs[-1], hs=hs, buf=buf, adv=adv, rp=rp, mu0=mu0, mu1=mu1, gmu=gmu, st=st, cnt=cnt, cnt_gae=cnt_gae)


# ------------------------------------------------------------------------------------------ 8. KL monitor
def kl_run(lib, est, steps):
    """a fresh PPO, one synthetic rollout, an update of `steps` policy steps (no value step) under an infinite target"""
    c = CASES["synthetic"]
    sizes, acts, E, T = c["sizes"], c["acts"], c["E"], c["T"]
    S, A, N, B = sizes[0], sizes[-1], E * T, 64
    ppo = make(lib, sizes, acts, N, lr=1e-2)         # a rate at which one Adam step moves the policy well past δ
    try:
        pol = ppo.contents.policy.contents
        assert lib.ppo_set_target_kl(ppo, float("inf")) == 0 and lib.ppo_set_kl_estimator(ppo, est) == 0
        lib.ppo_rollout_device(ppo, E, T, 1, 5)
        lib.ppo_synchronize()
        out = read(lib, ppo, N, S, A)
        out["mu0"] = nn_params_packed(lib, pol.mu)
        lib.ppo_set_step_limit(ppo, 0, steps)
        lib.ppo_update(ppo, 0.99, B, 2, 1, 1, SEED)
        lib.ppo_synchronize()
        no_error(lib)
        h = (C.c_double * 8)()
        assert lib.ppo_kl_history(ppo, h, 8) == steps
        out["hist"] = list(h)[:steps]
        out["rows"] = rows_of(nn_input_rows(lib, pol.mu, B), out["state"])
        out["mu1"] = nn_params_packed(lib, pol.mu)
        out["hash"] = lib.ppo_param_hash(ppo)
        return out
    finally:
        lib.free_ppo(ppo)


def test_kl_history_against_the_model(lib):
    """ppo_kl_history under k3 and under PPO_KL_EXACT against gauss_sd_ref on the step's read-back rows.  Step 2 of an
    update runs on the parameters step 1 left: a run limited to one policy step gives them (the runs are
    deterministic: same construction, rollout and shuffle seed — the first run's parameters are asserted to be the
    second's after its first step by the equal first history entry and rows), a run limited to two gives the history
    and the second step's rows.  z_old = forward(μ0), z_new = forward(μ1) in float64 over those rows;
        k3    = mean(expm1(x) − x), x = lp_new − old_lp
        exact = mean(sd row KL(z_old ‖ z_new)), clamped on both sides.
    Tolerance: every z carries the forward's δ = gemm_tol.  |Δx_i| ≤ δ·Σ_j(|ζ_j|/σ_j + 1 + ζ_j²) + lp's fp32 bound,
    ζ the standardised action; k3's term moves by (|expm1 x| + |Δx|)·|Δx|.  The row KL moves, for a δ on both rows,
    by 2·Σ_j[(|∂μ| + |∂ls|)·δ + (e^{−2ls_n}(1 + 2Δμ²) + 2e^{2d})·δ²] with ∂μ = Δμ·e^{−2ls_n},
    ∂ls = 1 − e^{2d} − Δμ²e^{−2ls_n}.  Plus 2⁻²³ relative for the fp32 words the sums and the history pass through.
    Parameters are bit-equal under either estimator (an infinite target never stops)."""
    c = CASES["synthetic"]
    sizes, acts = c["sizes"], c["acts"]
    Aa, K = sizes[-1] // 2, max(sizes)
    one = kl_run(lib, 0, 1)
    got = {est: kl_run(lib, est, 2) for est in (0, 1)}
    assert got[0]["hash"] == got[1]["hash"] and got[0]["mu1"].tobytes() == got[1]["mu1"].tobytes()
    assert got[0]["hist"][0] == one["hist"][0] and got[0]["state"].tobytes() == one["state"].tobytes()
    rows = got[0]["rows"]
    np.testing.assert_array_equal(rows, got[1]["rows"])
    x0 = one["state"][rows]
    zo = T.forward(sizes, acts, one["mu0"], x0)[0][-1]
    zn = T.forward(sizes, acts, one["mu1"], x0)[0][-1]
    delta = max(gemm_tol(zo, K), gemm_tol(zn, K))
    act, old = one["action"][rows].astype(F64), one["old_lp"][rows].astype(F64)
    ref = sd.head_f64(zn, act, np.ones(len(rows)), old, EPS, 0.0, LO, HI)
    x = ref["lp"] - old
    zeta = (act[:, :Aa] - zn[:, :Aa]) / np.exp(ref["ls"])
    lp_b = sd.head_bounds(zn.astype(F32), act.astype(F32), np.ones(len(rows), F32), old.astype(F32), EPS, 0.0, LO, HI)["lp"]
    dx = delta * (np.abs(zeta) / np.exp(ref["ls"]) + 1 + zeta ** 2).sum(axis=1) + lp_b + U * np.abs(old)
    k3 = float((np.expm1(x) - x).mean())
    k3_tol = float(((np.abs(np.expm1(x)) + dx) * dx).mean()) + 2 * U * abs(k3)
    lso, lsn = sd.clamp(zo[:, Aa:], LO, HI)[0], sd.clamp(zn[:, Aa:], LO, HI)[0]
    d, dm, e2 = lso - lsn, zo[:, :Aa] - zn[:, :Aa], np.exp(-2 * lsn)
    exact = float(sd.kl_rows_f64(zo, zn, LO, HI).mean())
    first = np.abs(dm) * e2 + np.abs(1 - np.exp(2 * d) - dm * dm * e2)
    second = e2 * (1 + 2 * dm * dm) + 2 * np.exp(2 * d)
    ex_tol = float((2 * (first * delta + second * delta ** 2)).sum(axis=1).mean()) + 2 * U * abs(exact)
    print(f"k3 {got[0]['hist'][1]:.6e} model {k3:.6e} ± {k3_tol:.2e}; exact {got[1]['hist'][1]:.6e} model {exact:.6e} "
          f"± {ex_tol:.2e}")
    assert k3 > 10 * k3_tol and exact > 10 * ex_tol, "the step must move the policy by more than the tolerance"
    assert abs(got[0]["hist"][1] - k3) <= k3_tol
    assert abs(got[1]["hist"][1] - exact) <= ex_tol
    # the first step runs on the rollout's parameters: both estimators read 0 up to the same tolerances
    assert abs(got[0]["hist"][0]) <= k3_tol and abs(got[1]["hist"][0]) <= ex_tol


# -------------------------------------------------------------------------------------------- 9. rollouts
def resample(lib, d_z, m, A, seed, step):
    """the sampler entry on μ's output as the library left it, at the rollout's key and kNoise + step"""
    act, lp = dev(lib, np.full((m, A), np.nan, F32)), empty(lib, m)
    try:
        key = R.rollout_key(seed)
        assert lib.ppo_gauss_sd_sample_device(d_z, m, A, LO, HI, key, R.K_NOISE + step, act.ptr, lp.ptr) == 0
        return act.to_numpy(F32, m * A).reshape(m, A), lp.to_numpy(F32, m)
    finally:
        act.free()
        lp.free()


def test_rollout_device_pendulum_two_calls(lib):
    """ppo_rollout_device on Pendulum with A = 2 over two calls: the torque the environment used is column 0 of the
    stored row — the environments' own dense step (ppo_env_step_device, A = 1, the same device functions) fed that
    column from the same reset reproduces next_state and reward bit for bit over both calls; the last step's stored
    action and log-prob are the sampler entry's on μ's output at kNoise + step; the zero half is +0."""
    c = CASES["pendulum"]
    E, T, S, A = 8, 8, 3, 2
    ppo = make(lib, c["sizes"], c["acts"], E * T)
    nf = lib.ppo_env_state_floats(0, S)
    es, obs = empty(lib, E * nf), empty(lib, E * S)
    nxt, after, rew = empty(lib, E * S), empty(lib, E * S), empty(lib, E)
    term, trunc = dev(lib, np.zeros(E, np.uint8)), dev(lib, np.zeros(E, np.uint8))
    try:
        assert lib.ppo_env_reset_device(0, es.ptr, obs.ptr, E, S, 5) == 0
        mu = ppo.contents.policy.contents.mu.contents
        for call in range(2):
            lib.ppo_rollout_device(ppo, E, T, 0, 5)
            lib.ppo_synchronize()
            buf = read(lib, ppo, E * T, S, A)
            act = buf["action"].reshape(E, T, A)
            assert (act[:, :, 1].view(np.uint32) == 0).all() and np.isfinite(act).all()
            if call == 0:
                assert buf["state"].reshape(E, T, S)[:, 0].tobytes() == obs.to_numpy(F32, E * S).tobytes()
            for t in range(T):
                step = call * T + t
                torque = dev(lib, np.ascontiguousarray(act[:, t, 0]))
                assert lib.ppo_env_step_device(0, es.ptr, torque.ptr, nxt.ptr, after.ptr, rew.ptr, term.ptr, trunc.ptr,
                                               E, S, 1, 0, 5, step) == 0
                torque.free()
                assert nxt.to_numpy(F32, E * S).tobytes() == buf["next_state"].reshape(E, T, S)[:, t].tobytes(), (call, t)
                assert rew.to_numpy(F32, E).tobytes() == buf["reward"].reshape(E, T)[:, t].tobytes(), (call, t)
            a, lp = resample(lib, mu.d_output, E, A, 5, call * T + T - 1)
            assert a.tobytes() == act[:, T - 1].tobytes()
            assert lp.tobytes() == buf["old_lp"].reshape(E, T)[:, T - 1].tobytes()
        no_error(lib)
    finally:
        for d in (es, obs, nxt, after, rew, term, trunc):
            d.free()
        lib.free_ppo(ppo)


def test_rollout_device_synthetic_reads_the_action_half(lib):
    """the synthetic environment under the policy reads column j mod Aa and averages the action term over Aa columns:
    next_state and reward against rng_ref.synth_step handed the Aa action columns, by test_gpu_rng.py's rule (four
    times what numpy's fp32 evaluation misses the float64 one by, at least 4 ulps)."""
    E, T, S, A = 8, 4, 5, 6
    Aa = A // 2
    ppo = make(lib, [S, 32, A], ["tanh", "none"], E * T)
    try:
        lib.ppo_rollout_device(ppo, E, T, 1, 5)
        lib.ppo_synchronize()
        buf = read(lib, ppo, E * T, S, A)
        no_error(lib)
    finally:
        lib.free_ppo(ppo)
    st = buf["state"].reshape(E, T, S).transpose(1, 0, 2)
    ac = buf["action"].reshape(E, T, A).transpose(1, 0, 2)
    assert (ac[:, :, Aa:].view(np.uint32) == 0).all() and (np.abs(ac[:, :, :Aa]) > 0).all()
    g = np.arange(T)
    n64, r64, _, _ = R.synth_step(st, np.ascontiguousarray(ac[:, :, :Aa]), g, 5, F64)
    n32, r32, _, _ = R.synth_step(st, np.ascontiguousarray(ac[:, :, :Aa]), g, 5, F32)
    for got, r64_, r32_, name in ((buf["next_state"].reshape(E, T, S).transpose(1, 0, 2), n64, n32, "next_state"),
                                  (buf["reward"].reshape(E, T).T, r64, r32, "reward")):
        tol = max(4.0 * float(np.abs(r32_.astype(F64) - r64_).max()), 4.0 * float(np.spacing(F32(np.abs(r64_).max()))))
        err = float(np.abs(got.astype(F64) - r64_).max())
        assert err <= tol, f"{name}: {err:.3g} > {tol:.3g}"
    # a model that read all A columns (zeros included) is far outside: the check tells the two apart
    wrong = R.synth_step(st, ac, g, 5, F64)[1]
    assert np.abs(wrong - r64).max() > 100 * tol


def test_open_rollout_with_a_host_environment(lib):
    """The open rollout driven by a caller-side environment kept in host arrays (obs ← 0.9·obs + 0.1·tanh(action half
    tiled), reward = −mean a², an episode ends every 3rd step of environment 0).  Every act is the sampler entry's on
    μ's output at kNoise + step, bit for bit, for the action handed out and the stored log-prob; ppo_act_device
    sampled at the same seed and step reproduces it bit for bit; deterministic returns the mean half of μ's output
    bit for bit with zeros after it; ppo_eval_device leaves the training state hash unchanged; CartPole declines."""
    E, T, S, A, seed = 8, 4, 5, 6, 9
    Aa = A // 2
    ppo = make(lib, [S, 32, A], ["tanh", "none"], E * T)
    rng = np.random.default_rng(2)
    obs = rng.uniform(-1, 1, (E, S)).astype(F32)
    d_act, d_act2, d_lp = empty(lib, E * A), empty(lib, E * A), empty(lib, E)
    try:
        mu = ppo.contents.policy.contents.mu.contents
        d_obs = dev(lib, obs)
        assert lib.ppo_rollout_begin(ppo, E, T, d_obs.ptr, seed) == 0
        d_obs.free()
        for t in range(T):
            step = lib.ppo_rollout_act(ppo, d_act.ptr)
            assert step >= 0
            a = d_act.to_numpy(F32, E * A).reshape(E, A).copy()
            z = ppo_ffi.d2h(lib, mu.d_output, F32, E * A).reshape(E, A).copy()
            want_a, want_lp = resample(lib, mu.d_output, E, A, seed, step)
            assert a.tobytes() == want_a.tobytes() and (a[:, Aa:].view(np.uint32) == 0).all()
            b = ppo.contents.buffer.contents
            assert ppo_ffi.d2h(lib, b.d_logprob_p, F32, E * T).reshape(E, T)[:, t].tobytes() == want_lp.tobytes()
            assert ppo_ffi.d2h(lib, b.d_action_p, F32, E * T * A).reshape(E, T, A)[:, t].tobytes() == a.tobytes()
            d_now = dev(lib, obs)
            assert lib.ppo_act_device(ppo, d_now.ptr, E, 0, seed, step, d_act2.ptr, d_lp.ptr) == 0
            assert d_act2.to_numpy(F32, E * A).tobytes() == a.tobytes()
            assert d_lp.to_numpy(F32, E).tobytes() == want_lp.tobytes()
            assert lib.ppo_act_device(ppo, d_now.ptr, E, 1, seed, step, d_act2.ptr, None) == 0
            mean = d_act2.to_numpy(F32, E * A).reshape(E, A)
            assert mean[:, :Aa].tobytes() == np.ascontiguousarray(z[:, :Aa]).tobytes()
            assert (mean[:, Aa:].view(np.uint32) == 0).all()
            d_now.free()
            # the caller's environment, on the host
            nxt = (F32(0.9) * obs + F32(0.1) * np.tanh(a[:, np.arange(S) % Aa])).astype(F32)
            rew = (-(a[:, :Aa] ** 2).mean(axis=1)).astype(F32)
            term = np.zeros(E, np.uint8)
            term[0] = t % 3 == 2
            after = nxt.copy()
            after[term == 1] = rng.uniform(-1, 1, (int(term.sum()), S)).astype(F32)
            ds = [dev(lib, rew), dev(lib, nxt), dev(lib, term), dev(lib, np.zeros(E, np.uint8)), dev(lib, after)]
            assert lib.ppo_rollout_store(ppo, *(x.ptr for x in ds)) == 0
            for x in ds:
                x.free()
            obs = after
        assert lib.ppo_rollout_end(ppo) == 0
        h1 = lib.ppo_state_hash(ppo, 1)
        out = (C.c_double * 9)()
        assert lib.ppo_eval_device(ppo, E, T, 1, 3, 0, 0.99, out, 9) == 9
        assert lib.ppo_eval_device(ppo, E, T, 1, 3, 1, 0.99, out, 9) == 9
        assert lib.ppo_eval_device(ppo, E, T, 2, 3, 0, 0.99, out, 9) == -1
        assert lib.ppo_state_hash(ppo, 1) == h1 != 0
        no_error(lib)
    finally:
        for d in (d_act, d_act2, d_lp):
            d.free()
        lib.free_ppo(ppo)


# ------------------------------------------------------------------------- 11. loopback data parallelism
CHILD = """
    import ctypes as C, json, sys
    sys.path.insert(0, {pkg!r})
    import ppo_ffi
    lib = ppo_ffi.load()
    assert lib.ppo_set_device(0) == 0
    if {loop}:
        assert lib.ppo_comm_init(0, 1, None) == 0 and lib.ppo_comm_world() == 2
    C.CDLL("libc.so.6").srand(3)
    p = lib.create_ppo(ppo_ffi.c_strings(["tanh", "tanh", "none"]), ppo_ffi.c_ints([5, 16, 16, 6]), 4, 512, 3e-4, 1e-3,
                       0.95, 0.2, 0.01, 1.0, True)
    if {on}:
        assert lib.ppo_set_action_gaussian_sd(p, -1.0, 0.5) == 0
    assert lib.ppo_set_target_kl(p, float("inf")) == 0 and lib.ppo_set_kl_estimator(p, {est}) == 0
    lib.ppo_fill_synthetic(p, 4, 128, 99, 1.0 / 100)
    lib.ppo_prof_enable(1)
    lib.ppo_prof_reset()
    lib.ppo_update(p, 0.99, 128, 2, 1, 1, 23)
    lib.ppo_synchronize()
    cnt = (C.c_long * 7)()
    lib.ppo_prof_counts(cnt)
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    h = (C.c_double * 16)()
    n = lib.ppo_kl_history(p, h, 16)
    st = (C.c_double * 36)()
    lib.ppo_read_stats(p, st, 36)
    print("RESULT " + json.dumps(dict(kl=[x.hex() for x in h[:n]], comm=cnt[5], mode=lib.ppo_comm_mode().decode(),
                                      elems=st[35], clamped=st[34], steps=st[3], hash=lib.ppo_param_hash(p))))
"""


def run_child(tmp_path, loop, on, est):
    script = tmp_path / f"sd_loop{int(loop)}_{int(on)}_{est}.py"
    script.write_text(textwrap.dedent(CHILD.format(pkg=os.path.join(ROOT, "ppo.c_amd"), loop=bool(loop), on=bool(on),
                                                   est=est)))
    env = {k: v for k, v in os.environ.items() if k not in ("PPO_COMM_LOOPBACK", "PPO_GRAPH", "PPO_SERIAL")}
    env["PPO_NO_TINY"] = "1"
    if loop:
        env.update(PPO_COMM_LOOPBACK="2", PPO_REPLICA_CHECK="1")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])


@pytest.mark.parametrize("est", [0, 1])
def test_loopback_data_parallel(lib, tmp_path, est):
    """PPO_COMM_LOOPBACK=2, each run in a fresh child process: one update completes with the replica check on;
    ppo_comm_mode and the collective count are the same with the feature on and off; the two ranks hold the same
    shard, so the all-reduced gradient and KL sums double with the row count and the run is the single-rank one bit
    for bit in its KL history; out[35] counts THIS RANK's rows."""
    on, off, single = run_child(tmp_path, True, True, est), run_child(tmp_path, True, False, est), \
        run_child(tmp_path, False, True, est)
    assert on["mode"] == off["mode"] and on["comm"] == off["comm"] > 0
    assert on["steps"] == off["steps"] == 8 and len(on["kl"]) == 8
    assert on["kl"] == single["kl"] and float.fromhex(on["kl"][-1]) > 0
    assert on["elems"] == 128 * 3 and 0 <= on["clamped"] <= on["elems"] and on["clamped"] == single["clamped"]
    assert off["elems"] == 0 and off["clamped"] == 0
