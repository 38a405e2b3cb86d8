"""CartPole-v1 as env_kind 2 of the device rollout (csrc/rollout.hip) with the categorical policy: every transition
recomputed in float64 from the buffer's own state and action (one step, so nothing accumulates), the flags, the
segment ends, cont[] and the episode tracker against a host scan, and the evaluation guarantees extended to kind 2.
Bounds: tests/categorical_ref.py cartpole_bounds, validated by the fp32 mirror in test_cartpole_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import categorical_ref as cr
import episode_ref
import ppo_ffi
from categorical_ref import F32, F64

pytestmark = pytest.mark.gpu

SIZES, E, T, SEED = [4, 32, 2], 64, 600, 21


def make_ppo(lib, N=E * T, seed=4):
    C.CDLL("libc.so.6").srand(seed)
    ppo = lib.create_ppo(ppo_ffi.c_strings(["tanh", "none"]), ppo_ffi.c_ints(SIZES), 3, N, 3e-4, 3e-4, 0.95, 0.2, 0.0,
                         1.0, True)
    assert lib.ppo_set_action_dist(ppo, 1) == 0
    return ppo


def ep_stats(lib, ppo):
    out = (C.c_double * 16)()
    assert lib.ppo_episode_stats(ppo, out, 16) == 16
    return np.array(out[:])


@pytest.fixture(scope="module")
def rollout(lib):
    """One fresh PPO's first rollout, read back once and shared."""
    ppo = make_ppo(lib)
    h0 = lib.ppo_param_hash(ppo)
    lib.ppo_rollout_device(ppo, E, T, 2, SEED)
    b = ppo.contents.buffer.contents
    n = E * T
    out = dict(state=ppo_ffi.d2h(lib, b.d_state_p, F32, n * 4).reshape(E, T, 4),
               nxt=ppo_ffi.d2h(lib, b.d_next_state_p, F32, n * 4).reshape(E, T, 4),
               act=ppo_ffi.d2h(lib, b.d_action_p, F32, n * 2).reshape(E, T, 2),
               lp=ppo_ffi.d2h(lib, b.d_logprob_p, F32, n).reshape(E, T),
               r=ppo_ffi.d2h(lib, b.d_reward_p, F32, n).reshape(E, T),
               term=ppo_ffi.d2h(lib, b.d_terminated_p, np.uint8, n).reshape(E, T),
               trunc=ppo_ffi.d2h(lib, b.d_truncated_p, np.uint8, n).reshape(E, T),
               stats=ep_stats(lib, ppo), hash0=h0, hash1=lib.ppo_param_hash(ppo), pos=(b.idx, bool(b.full)))
    assert lib.ppo_last_error() in (b"", None)
    lib.free_ppo(ppo)
    return out


def host_steps(ro):
    """The TimeLimit counter a host would keep: steps since the last reset, after each row's step."""
    steps = np.zeros((E, T), np.int64)
    run = np.zeros(E, np.int64)
    for t in range(T):
        run = run + 1
        steps[:, t] = run
        run[(ro["term"][:, t] != 0) | (steps[:, t] >= 500)] = 0
    return steps


def test_every_transition(rollout):
    ro = rollout
    s, a = ro["state"].reshape(-1, 4), ro["act"].reshape(-1, 2)
    assert ((a[:, 0] == 0) | (a[:, 0] == 1)).all() and not a[:, 1].any()
    assert 0.2 < a[:, 0].mean() < 0.8                      # a fresh policy is near uniform: both actions occur
    assert (ro["r"] == 1).all()
    want, term64 = cr.cartpole_f64(s, a[:, 0].astype(int))
    b = cr.cartpole_bounds(s, a[:, 0].astype(int))
    err = np.abs(ro["nxt"].reshape(-1, 4).astype(F64) - want)
    print(f"next_state error / bound {float((err / b).max()):.3f}")
    assert (err <= b).all()
    near = ((np.abs(np.abs(want[:, 0]) - cr.X_LIMIT) <= b[:, 0] + cr.LIMIT_SLACK[0])
            | (np.abs(np.abs(want[:, 2]) - cr.TH_LIMIT) <= b[:, 2] + cr.LIMIT_SLACK[1]))
    assert near.mean() <= 0.01
    term = ro["term"].reshape(-1).astype(bool)
    np.testing.assert_array_equal(term[~near], term64[~near])
    assert term.sum() > 50                                  # a random policy falls over within a few dozen steps
    # the log-prob is the categorical one of the stored index: within ln 2 ± a little for a fresh policy
    assert (ro["lp"] < 0).all() and (ro["lp"] > -3).all()


def test_flags_segments_and_continuity(rollout):
    ro = rollout
    steps = host_steps(ro)
    limit = steps >= 500
    want_trunc = limit.copy()
    want_trunc[:, T - 1] = True                             # segment ends are truncated
    np.testing.assert_array_equal(ro["trunc"].astype(bool), want_trunc)
    done = (ro["term"] != 0) | limit
    # where the episode went on, the next row starts from this row's next_state, bit for bit
    go = ~done[:, :-1]
    assert ro["state"][:, 1:][go].tobytes() == ro["nxt"][:, :-1][go].tobytes()
    # where it ended, the next row is a fresh reset: inside ±0.05
    fresh = ro["state"][:, 1:][~go]
    assert fresh.size and (np.abs(fresh) <= 0.05).all()
    assert (np.abs(ro["state"][:, 0]) <= 0.05).all()
    assert ro["pos"] == (0, True)


def test_time_limit_is_reached(lib):
    """A policy that balances long enough meets the 500-step limit: steered by the sign of θ + θ̇ through one tanh
    layer, deterministic evaluation runs 600 steps with a truncation at step 500 in most environments."""
    ppo = make_ppo(lib, N=64)
    mu = ppo.contents.policy.contents.mu.contents
    W0 = np.zeros((32, 4), F32)
    W0[0] = [0, 0.5, 10, 3]                                 # unit 0: a PD term on the pole (and a little on ẋ)
    W1 = np.zeros((2, 32), F32)
    W1[0, 0], W1[1, 0] = -5, 5                              # leaning right → push right
    for ly, W in ((mu.layers[0], W0), (mu.layers[1], W1)):
        ppo_ffi.h2d(lib, ly.d_weights, W)
        ppo_ffi.h2d(lib, ly.d_biases, np.zeros(ly.output_size, F32))
    h = lib.ppo_param_hash(ppo)
    out = (C.c_double * 9)()
    assert lib.ppo_eval_device(ppo, 16, 600, 2, 3, 1, 0.99, out, 9) == 9
    assert lib.ppo_param_hash(ppo) == h                     # deterministic evaluation leaves the parameters alone
    print(f"PD policy: {out[0]:.0f} episodes, mean return {out[1]:.1f}, max {out[4]:.0f}")
    assert out[4] == 500.0                                   # the longest episode is the limit, never more
    lib.free_ppo(ppo)


def test_tracker_and_cont_against_a_host_scan(rollout):
    ro = rollout
    done_last = (ro["term"][:, -1] != 0) | (host_steps(ro)[:, -1] >= 500)
    cont = (~done_last).astype(np.uint8)
    ref = episode_ref.scan(ro["r"].reshape(-1), ro["term"].reshape(-1), ro["trunc"].reshape(-1), cont, E, T, 0.99)
    want = episode_ref.report(ref["agg"])
    assert episode_ref.bits(ro["stats"][8:16]).tobytes() == episode_ref.bits(want).tobytes(), (ro["stats"][8:], want)
    assert ro["stats"][8] > 50 and ro["stats"][12] <= 500
    assert ro["hash0"] == ro["hash1"]                       # a rollout moves no parameter


def test_eval_reproduces_the_first_rollout(lib, rollout):
    """deterministic = 0 on a fresh PPO: the first training rollout's episode statistics bit for bit (the existing
    guarantee, for kind 2); deterministic = 1 leaves ppo_param_hash unchanged."""
    ppo = make_ppo(lib)
    out = (C.c_double * 9)()
    assert lib.ppo_eval_device(ppo, E, T, 2, SEED, 0, 0.99, out, 9) == 9
    ev = np.array(out[:])
    assert episode_ref.bits(ev[:8]).tobytes() == episode_ref.bits(rollout["stats"][8:16]).tobytes()
    h = lib.ppo_param_hash(ppo)
    assert h == rollout["hash0"]
    assert lib.ppo_eval_device(ppo, E, 100, 2, SEED, 1, 0.99, out, 9) == 9
    assert lib.ppo_param_hash(ppo) == h
    assert lib.ppo_last_error() in (b"", None)
    lib.free_ppo(ppo)
