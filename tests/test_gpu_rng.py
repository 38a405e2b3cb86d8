"""The device random streams, bit for bit, against tests/rng_ref.py (csrc/rng.h, sample.hip, rollout.hip).

Everything goes through the public exports ppo_fill_synthetic, ppo_sample_action_device and
ppo_rollout_device.  Equality rules:
  * uniform outputs (affine maps of u01 by powers of two), copies and flags: assert_array_equal;
  * outputs that pass through logf / cosf / sinf / tanhf / expf: a tolerance computed per check (tol()):
    4 × the worst distance of a numpy-fp32 evaluation of the same formula from the float64 reference on the
    same inputs, and never below 4 fp32 ulps of the largest magnitude involved.  The 4 allows the device's
    libm a couple of ulps per function where numpy has about one; a wrong stream is an O(1) error.
Each check prints its worst error / tolerance (and appends it to $PPO_TOL_REPORT when set).

Groups: the synthetic fill (small, and just over the 8192 × 256 elements where the fill kernels start
their grid-stride loop) at p_terminate 0, 1/200, 1; the batched sample (launch-geometry independence,
offset as a stream selector, 64-bit seed and offset); the synthetic rollout re-simulated step by step
with the GLOBAL step g = call·T + t, over two calls under one seed; Pendulum's time-limit resets over
three calls under one seed.
"""
import os

import numpy as np
import pytest

import ppo_ffi
import rng_ref as R
from helpers import F32, assert_rel_close, dev, empty, gemm_tol, nn_params_packed, nn_set_params_packed

pytestmark = pytest.mark.gpu

F64 = np.float64


def tol(ref64, np32, *magnitudes):
    worst = float(np.abs(np.asarray(np32, F64) - ref64).max())
    big = max([float(np.abs(ref64).max())] + [float(np.abs(np.asarray(m, F64)).max()) for m in magnitudes])
    return max(4.0 * worst, 4.0 * float(np.spacing(F32(big))))


def report(what, err, bound):
    ratio = err / bound
    print(f"[rng] {what}: err {err:.3e} tol {bound:.3e} err/tol {ratio:.3f}")
    path = os.environ.get("PPO_TOL_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(f"{ratio:.5f}\t{err:.3e}\t{bound:.3e}\trng\t"
                    f"{os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]}\t{what}\n")


def assert_transcendental(got, ref64, np32, what, magnitudes=()):
    assert got.dtype == F32 and got.shape == ref64.shape, what
    err = float(np.abs(got.astype(F64) - ref64).max())
    bound = tol(ref64, np32, *magnitudes)
    report(what, err, bound)
    assert err <= bound, f"{what}: max |err| {err:.3g} > tol {bound:.3g}"


def make_ppo(lib, sizes, N, seed=3):
    ppo_ffi.C.CDLL("libc.so.6").srand(seed)
    acts = ["relu"] * (len(sizes) - 2) + ["none"]
    return lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), N, 3e-4, 3e-4, 0.95, 0.2, 0.0,
                          1.0, True)


def read_buffer(lib, ppo, N, S, A):
    b = ppo.contents.buffer.contents
    return dict(state=ppo_ffi.d2h(lib, b.d_state_p, F32, N * S).reshape(N, S),
                next_state=ppo_ffi.d2h(lib, b.d_next_state_p, F32, N * S).reshape(N, S),
                action=ppo_ffi.d2h(lib, b.d_action_p, F32, N * A).reshape(N, A),
                logprob=ppo_ffi.d2h(lib, b.d_logprob_p, F32, N),
                reward=ppo_ffi.d2h(lib, b.d_reward_p, F32, N),
                term=ppo_ffi.d2h(lib, b.d_terminated_p, np.uint8, N),
                trunc=ppo_ffi.d2h(lib, b.d_truncated_p, np.uint8, N))


def oracle_mu(lib, oracle, ppo, sizes, state):
    pol = ppo.contents.policy.contents
    relu = [1] * (len(sizes) - 2) + [0]
    acts = oracle.mlp_forward(sizes, relu, nn_params_packed(lib, pol.mu), state)
    return oracle.mlp_layer_outputs(sizes, acts, len(state))[-1], ppo_ffi.d2h(lib, pol.d_log_std, F32, sizes[-1])


def assert_noise(z_got, mu_ref, sigma, K, n64, n32, what):
    """Standardised noise (a − μ_oracle)/σ against the reference draw: the oracle's μ differs from the
    device's by at most the GEMM tolerance, a's own fp32 rounding is within the ulps of max |a|/σ."""
    err = float(np.abs(z_got.astype(F64) - n64).max())
    a_over_sigma = (np.abs(mu_ref).max() + np.abs(n64).max() * sigma.max()) / sigma.min()
    bound = gemm_tol(mu_ref, K) / float(sigma.min()) + tol(n64, n32, a_over_sigma)
    report(what, err, bound)
    assert err <= bound, f"{what}: max |err| {err:.3g} > tol {bound:.3g}"


# ------------------------------------------------------------------------------------------------
# ppo_fill_synthetic
# ------------------------------------------------------------------------------------------------
FILL_SEED = 1234
# the second case: 8 · 8192 · 33 = 2,162,688 state elements > 8192 · 256 = 2,097,152, so fill_uniform_kernel and
# link_next_kernel run their grid-stride loop a second time for the first 65,536 threads
FILL_CASES = {"small": ([7, 8, 2], 3, 5), "grid_stride": ([33, 8, 2], 8, 8192)}


@pytest.mark.parametrize("p", [0.0, 1.0 / 200, 1.0], ids=["p0", "p1_200", "p1"])
@pytest.mark.parametrize("case", list(FILL_CASES))
def test_fill_synthetic(lib, oracle, case, p):
    sizes, E, T = FILL_CASES[case]
    S, A, N = sizes[0], sizes[-1], E * T
    if case == "grid_stride":
        assert N * S > 8192 * 256
    ref = R.fill_synthetic(E, T, S, FILL_SEED, p)
    ppo = make_ppo(lib, sizes, N)
    lib.ppo_fill_synthetic(ppo, E, T, FILL_SEED, p)
    lib.ppo_synchronize()
    buf = read_buffer(lib, ppo, N, S, A)
    np.testing.assert_array_equal(buf["state"], ref["state"])
    np.testing.assert_array_equal(buf["term"].astype(bool), ref["term"])
    np.testing.assert_array_equal(buf["trunc"].astype(bool), ref["trunc"])
    if p == 0.0:
        assert not buf["term"].any()
    if p == 1.0:                                # the reference decides which rows, if any, drew u01 == 1
        assert ref["term"].sum() >= N - 1
    link = np.nonzero(~ref["unlinked"])[0]
    assert (buf["next_state"][link].view(np.uint32) == buf["state"][link + 1].view(np.uint32)).all()
    np.testing.assert_array_equal(buf["next_state"][ref["unlinked"]], ref["next_state"][ref["unlinked"]])
    assert ref["unlinked"].sum() >= E
    r64, r32 = R.fill_reward(N, FILL_SEED, F64), R.fill_reward(N, FILL_SEED, F32)
    assert_transcendental(buf["reward"], r64, r32, f"fill {case} reward")
    # the actions: the fifth key, counter i·A + j, offset 0
    mu, log_std = oracle_mu(lib, oracle, ppo, sizes, buf["state"])
    sigma = np.exp(log_std.astype(F64))
    key = R.fill_key(FILL_SEED, R.FILL_ACTION)
    assert_noise((buf["action"] - mu) / sigma, mu, sigma, sizes[-2], R.sample_noise(N, A, key, 0, F64),
                 R.sample_noise(N, A, key, 0, F32), f"fill {case} action noise")
    lib.free_ppo(ppo)


# ------------------------------------------------------------------------------------------------
# ppo_sample_action_device
# ------------------------------------------------------------------------------------------------
SAMPLE_SEED = (0x9E3779B9 << 32) | 0x1234ABCD           # non-zero high word
SAMPLE_MS = (1, 255, 257, 1000)                         # one thread, a block less one, a block plus one, four blocks
S_IN = 5


def zero_weight_policy(lib, A, rng):
    """A policy whose μ is known exactly: every weight zero, so μ is the last layer's bias."""
    sizes = [S_IN, 8, A]
    pol = lib.create_gaussian_policy(ppo_ffi.c_ints(sizes), ppo_ffi.c_strings(["relu", "none"]), 3, 1.0)
    bias = rng.uniform(-1, 1, A).astype(F32)
    params = np.zeros(S_IN * 8 + 8 + 8 * A + A, F32)
    params[S_IN * 8:S_IN * 8 + 8] = rng.uniform(-1, 1, 8).astype(F32)      # hidden biases: multiplied by zero
    params[-A:] = bias
    nn_set_params_packed(lib, pol.contents.mu, params)
    log_std = rng.uniform(-0.5, 0.5, A).astype(F32)
    ppo_ffi.h2d(lib, pol.contents.d_log_std, log_std)
    return pol, bias, log_std


def run_sample(lib, pol, dstate, m, A, seed, offset):
    da, dlp = empty(lib, m * A), empty(lib, m)
    lib.ppo_sample_action_device(pol, dstate.ptr, da.ptr, dlp.ptr, m, seed, offset)
    lib.ppo_synchronize()
    out = da.to_numpy(F32, m * A).reshape(m, A), dlp.to_numpy(F32, m)
    da.free()
    dlp.free()
    return out


@pytest.mark.parametrize("offset", [0, 7, (1 << 32) + 3], ids=["off0", "off7", "off2p32_3"])
@pytest.mark.parametrize("A", [1, 6, 17])
def test_sample_action_device(lib, oracle, A, offset):
    rng = np.random.default_rng(100 + A)
    pol, bias, log_std = zero_weight_policy(lib, A, rng)
    m_max = max(SAMPLE_MS)
    dstate = dev(lib, rng.uniform(-1, 1, (m_max, S_IN)).astype(F32))
    eps64 = R.sample_noise(m_max, A, SAMPLE_SEED, offset, F64)
    eps32 = R.sample_noise(m_max, A, SAMPLE_SEED, offset, F32)
    mu = np.broadcast_to(bias, (m_max, A))
    a64 = R.sample_action(mu, log_std, eps64, F64)
    a32 = R.sample_action(mu, log_std, eps32, F32)
    assert a32.dtype == F32
    full = None
    for m in sorted(SAMPLE_MS, reverse=True):
        act, lp = run_sample(lib, pol, dstate, m, A, SAMPLE_SEED, offset)
        got_mu = ppo_ffi.d2h(lib, pol.contents.mu.contents.d_output, F32, m * A).reshape(m, A)
        np.testing.assert_array_equal(got_mu, mu[:m])                          # μ is the bias, exactly
        assert_transcendental(act, a64[:m], a32[:m], f"sample A={A} offset={offset} m={m} action",
                              magnitudes=(mu, eps64 * np.exp(log_std.astype(F64))))
        assert_rel_close(lp, oracle.log_prob(np.ascontiguousarray(mu[:m]), log_std, act), 2e-6, 2e-6,
                         f"sample A={A} m={m} log_prob")
        if full is None:
            full = (act, lp)
        else:                                   # independent of the launch geometry: bit for bit
            assert (act.view(np.uint32) == full[0][:m].view(np.uint32)).all()
            assert (lp.view(np.uint32) == full[1][:m].view(np.uint32)).all()
    dstate.free()
    lib.free_gaussian_policy(pol)


def test_sample_offset_selects_a_stream(lib):
    """(i, offset = 1) is not (i + 1, offset = 0): the offset is a counter word of its own."""
    rng = np.random.default_rng(5)
    pol, bias, log_std = zero_weight_policy(lib, 1, rng)
    m = 257
    dstate = dev(lib, np.zeros((m, S_IN), F32))
    a0, _ = run_sample(lib, pol, dstate, m, 1, SAMPLE_SEED, 0)
    a1, _ = run_sample(lib, pol, dstate, m, 1, SAMPLE_SEED, 1)
    assert (a1[:-1] != a0[1:]).mean() > 0.99 and (a1 != a0).mean() > 0.99
    # and a seed's high word is part of the key
    ah, _ = run_sample(lib, pol, dstate, m, 1, SAMPLE_SEED ^ (1 << 63), 0)
    assert (ah != a0).mean() > 0.99
    dstate.free()
    lib.free_gaussian_policy(pol)


# ------------------------------------------------------------------------------------------------
# ppo_rollout_device, synthetic environment
# ------------------------------------------------------------------------------------------------
def by_step(x, E, T):
    """Buffer rows e·T + t → [T, E, ...]."""
    return np.ascontiguousarray(np.swapaxes(x.reshape((E, T) + x.shape[1:]), 0, 1))


SYNTH = dict(sizes=[70, 16, 3], E=64, T=64, seed=7, calls=2)


@pytest.fixture(scope="module")
def synth_rollouts(lib, oracle):
    """Two consecutive synthetic rollouts of a fresh PPO under one seed, read back once: per call the buffer
    and the oracle's μ at the stored observations."""
    sizes, E, T, seed = SYNTH["sizes"], SYNTH["E"], SYNTH["T"], SYNTH["seed"]
    N = E * T
    ppo = make_ppo(lib, sizes, N)
    out = []
    for _ in range(SYNTH["calls"]):
        lib.ppo_rollout_device(ppo, E, T, 1, seed)
        lib.ppo_synchronize()
        buf = read_buffer(lib, ppo, N, sizes[0], sizes[-1])
        buf["mu"], buf["log_std"] = oracle_mu(lib, oracle, ppo, sizes, buf["state"])
        for v in buf.values():
            v.setflags(write=False)
        out.append(buf)
    lib.free_ppo(ppo)
    return out


def test_synthetic_rollout_streams(synth_rollouts):
    """Every step re-simulated from the stored (state, action) with the global step g = call·T + t."""
    sizes, E, T, seed = SYNTH["sizes"], SYNTH["E"], SYNTH["T"], SYNTH["seed"]
    S, A = sizes[0], sizes[-1]
    # the terminations depend on (e, g) alone: the done branch must be exercised in both rollouts
    dones = [R.synth_done(E, np.arange(c * T, (c + 1) * T), seed) for c in range(2)]
    assert all(d.sum() >= 5 for d in dones), [int(d.sum()) for d in dones]
    prev = None
    for call, buf in enumerate(synth_rollouts):
        g = np.arange(call * T, (call + 1) * T)
        obs, act = by_step(buf["state"], E, T), by_step(buf["action"], E, T)
        nxt, rew = by_step(buf["next_state"], E, T), by_step(buf["reward"], E, T)
        term, trunc = by_step(buf["term"], E, T).astype(bool), by_step(buf["trunc"], E, T).astype(bool)
        n64, r64, done, reset = R.synth_step(obs, act, g, seed, F64)
        n32, r32, _, _ = R.synth_step(obs, act, g, seed, F32)
        assert n32.dtype == F32 and r32.dtype == F32
        np.testing.assert_array_equal(done, dones[call])
        np.testing.assert_array_equal(term, done, err_msg=f"call {call}: terminated")
        last = np.zeros((T, E), bool)
        last[T - 1] = True
        np.testing.assert_array_equal(trunc, last & ~done, err_msg=f"call {call}: truncated")
        assert_transcendental(nxt, n64, n32, f"synthetic rollout call {call} next_state", magnitudes=(1.0,))
        assert_transcendental(rew, r64, r32, f"synthetic rollout call {call} reward")
        # the next row: this row's next observation (bitwise), or the reset draw (exact) after a done step
        follow = np.where(done[:, :, None], reset, nxt)
        assert (obs[1:].view(np.uint32) == follow[:-1].view(np.uint32)).all(), f"call {call}: state[row + 1]"
        if call == 0:
            np.testing.assert_array_equal(obs[0], R.synth_first_obs(E, S, seed))
        else:                                   # episodes continue across calls
            assert (obs[0].view(np.uint32) == prev.view(np.uint32)).all()
        prev = follow[-1]
        sigma = np.exp(buf["log_std"].astype(F64))
        z = by_step((buf["action"] - buf["mu"]) / sigma, E, T)
        assert_noise(z, buf["mu"], sigma, sizes[-2], R.policy_noise(E, A, g, seed, F64),
                     R.policy_noise(E, A, g, seed, F32), f"synthetic rollout call {call} policy noise")


def test_synthetic_rollouts_differ(synth_rollouts):
    """A constant seed must not replay the environment's draws: the two rollouts terminate at different cells
    and add different reward noise (r + 0.01·mean(a²))/0.1."""
    E, T = SYNTH["E"], SYNTH["T"]
    masks = [by_step(b["term"], E, T).astype(bool) for b in synth_rollouts]
    assert masks[0].any() and masks[1].any()
    assert (masks[0] != masks[1]).any(), "both rollouts terminate at the same (e, t) cells"
    noise = [(b["reward"].astype(F64) + 0.01 * (b["action"].astype(F64) ** 2).mean(-1)) / 0.1 for b in synth_rollouts]
    assert np.abs(noise[0] - noise[1]).max() > 1.0, "both rollouts add the same reward noise"
    assert (synth_rollouts[0]["state"] != synth_rollouts[1]["state"]).any()


# ------------------------------------------------------------------------------------------------
# ppo_rollout_device, Pendulum-v1
# ------------------------------------------------------------------------------------------------
PENDULUM = dict(sizes=[3, 16, 1], E=8, seed=11)
_pendulum_cache = {}


def pendulum_rollouts(lib, T, calls):
    """`calls` consecutive Pendulum rollouts of a fresh PPO under one seed, read back once per (T, calls)."""
    if (T, calls) not in _pendulum_cache:
        E, N = PENDULUM["E"], PENDULUM["E"] * T
        ppo = make_ppo(lib, PENDULUM["sizes"], N)
        out = []
        for _ in range(calls):
            lib.ppo_rollout_device(ppo, E, T, 0, PENDULUM["seed"])
            lib.ppo_synchronize()
            buf = read_buffer(lib, ppo, N, 3, 1)
            for v in buf.values():
                v.setflags(write=False)
            out.append(buf)
        lib.free_ppo(ppo)
        _pendulum_cache[(T, calls)] = out
    return _pendulum_cache[(T, calls)]


@pytest.mark.parametrize("T,calls", [(200, 3), (256, 2)], ids=["T200x3", "T256x2"])
def test_pendulum_resets(lib, T, calls):
    """Every time-limit reset is the reference draw at its GLOBAL step.  T = 200 lines up with the 200-step
    limit: each call ends with a reset, whose observation opens the next call.  T = 256 puts resets inside
    a call (t = 199, then global step 399), where the draw is written to the next row."""
    E, seed = PENDULUM["E"], PENDULUM["seed"]
    theta, thetadot = R.pendulum_first_reset(E, seed)
    steps, pending, n_resets = 0, (theta, thetadot, "first reset"), 0
    for call, buf in enumerate(pendulum_rollouts(lib, T, calls)):
        obs = by_step(buf["state"], E, T)
        trunc = by_step(buf["trunc"], E, T).astype(bool)
        for t in range(T):
            if pending is not None:             # the observation after a reset: (cos θ, sin θ, θ̇) of the draw
                th, thd, what = pending
                o64, o32 = R.pendulum_obs(th, thd, F64), R.pendulum_obs(th, thd, F32)
                np.testing.assert_array_equal(obs[t][:, 2], thd, err_msg=f"{what}: θ̇")
                assert_transcendental(obs[t][:, :2], o64[:, :2], o32[:, :2], f"pendulum T={T} {what} cos/sin",
                                      magnitudes=(1.0,))
                pending = None
            steps += 1
            limit = steps >= 200
            assert (trunc[t] == (limit or t == T - 1)).all()
            if limit:
                g = call * T + t
                th, thd = R.pendulum_reset(E, [g], seed)
                pending, steps = (th[0], thd[0], f"reset at global step {g}"), 0
                n_resets += 1
        assert not buf["term"].any()
    assert n_resets >= 2


def test_pendulum_starts_differ(lib):
    """T = 200 with one seed for every call: calls 2 and 3 must not restart every episode from one state."""
    E, T = PENDULUM["E"], 200
    starts = [by_step(b["state"], E, T)[0] for b in pendulum_rollouts(lib, T, 3)]
    assert (starts[1] != starts[2]).any(), "calls 2 and 3 start from the same states"
    assert (starts[1][:, 2] != starts[2][:, 2]).all()
