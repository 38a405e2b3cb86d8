"""Episode-return statistics of device rollouts and device evaluation (ppo_episode_stats, ppo_eval_device,
csrc/episode.hip) through the C ABI.

The reference is tests/episode_ref.py (pinned on the CPU in test_episode_cpu.py); every comparison of the scan and
of the tracker is bit for bit.  The scan kernel stages tiles of TILE_E = 64 environments × TILE_T = 64 rows
through LDS: the shapes below straddle both."""
import ctypes as C
import functools

import numpy as np
import pytest

import ppo_ffi
from episode_ref import F32, NBATCH, bits, fresh, merge, report, scan, zero
from helpers import dev, empty
from test_episode_cpu import SYNTH_E, SYNTH_ROLLOUTS, SYNTH_SEED, SYNTH_T, mixed_rewards
from test_gpu_obsnorm import get_state as obs_get_state
from test_gpu_obsnorm import known_triple
from test_gpu_obsnorm import set_state as obs_set_state
from test_gpu_rewnorm import get_state as rew_get_state
from test_gpu_rng import make_ppo

pytestmark = pytest.mark.gpu

TILE_E, TILE_T = 64, 64
SHAPES = [(1, 1), (1, 7), (3, 1), (5, 7), (63, 65), (64, 64), (65, 63), (130, 257)]
GAMMAS = [0.0, 0.99, 1.0]
MODES = ["none", "all", "random", "edge"]
BUFFER_ARRAYS = [("d_state_p", F32, "S"), ("d_next_state_p", F32, "S"), ("d_action_p", F32, "A"),
                 ("d_logprob_p", F32, 1), ("d_reward_p", F32, 1), ("d_advantage_p", F32, 1),
                 ("d_adv_target_p", F32, 1), ("d_terminated_p", np.uint8, 1), ("d_truncated_p", np.uint8, 1)]


def no_error(lib):
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


def same_bits(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    bad = np.nonzero(bits(got).ravel() != bits(ref).ravel())[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: " \
                          f"{got.ravel()[bad[0]]!r} != {ref.ravel()[bad[0]]!r}"


def ep_stats(lib, ppo):
    out = (C.c_double * 16)()
    assert lib.ppo_episode_stats(ppo, out, 16) == 16
    return np.array(out[:])


def read_stats(lib, ppo, n=25):
    st = (C.c_double * n)()
    lib.ppo_read_stats(ppo, st, n)
    return np.array(st[:])


# ----------------------------------------------------------------------------- 1. the scan alone
@functools.lru_cache(maxsize=None)
def scan_inputs(E, T, mode):
    rng = np.random.default_rng(1000 * E + 7 * T + len(mode))
    n = E * T
    r = mixed_rewards(rng, n)
    term, trunc = np.zeros((E, T), np.uint8), np.zeros((E, T), np.uint8)
    if mode == "all":
        term[:] = rng.random((E, T)) < 0.5
        trunc[:] = 1 - term
        term.reshape(-1)[::5] = 1                        # both flags set on some rows
    elif mode == "random":
        term[:] = rng.random((E, T)) < 0.05
        trunc[:] = rng.random((E, T)) < 0.05
    elif mode == "edge":
        term[::2, 0] = 1                                 # ends at t = 0,
        if T >= 2:
            trunc[::3, T - 2] = 1                        # at T − 2
        trunc[:, T - 1] = 1                              # and the segment's own truncation at T − 1
        term[1::4, T - 1] = 1                            # with a termination beside it on some
    conts = {"mixed": rng.integers(0, 2, E).astype(np.uint8)}
    if mode == "edge":
        conts.update(zeros=np.zeros(E, np.uint8), ones=np.ones(E, np.uint8), null=None)
    g = 0.97
    k = rng.integers(1, 50, E)
    state = np.stack([1e3 * rng.normal(size=E), 1e2 * rng.normal(size=E), g ** k, k.astype(np.float64)], 1)
    for a in (r, term, trunc, state):
        a.setflags(write=False)
    return dict(r=r, term=term.reshape(-1), trunc=trunc.reshape(-1), conts=conts, state=state)


@functools.lru_cache(maxsize=None)
def scan_ref(E, T, gamma, mode, cont_name, with_state):
    c = scan_inputs(E, T, mode)
    return scan(c["r"], c["term"], c["trunc"], c["conts"][cont_name], E, T, gamma, c["state"] if with_state else None)


def scan_dev(lib, d, cont, E, T, gamma, state, rows=True):
    """One ppo_episode_scan_device call → (row_ret, row_disc, state out, aggregate); None for what was not asked."""
    n = E * T
    out = (C.c_double * NBATCH)()
    d_ret, d_disc = (empty(lib, n, np.float64), empty(lib, n, np.float64)) if rows else (None, None)
    d_cont = dev(lib, cont) if cont is not None else None
    d_state = dev(lib, state) if state is not None else None
    try:
        rc = lib.ppo_episode_scan_device(d["r"].ptr, d["term"].ptr, d["trunc"].ptr, d_cont.ptr if d_cont else None, E, T,
                                         gamma, d_state.ptr if d_state else None, d_ret.ptr if rows else None,
                                         d_disc.ptr if rows else None, out)
        assert rc == 0
        res = (d_ret.to_numpy(np.float64, n).reshape(E, T) if rows else None,
               d_disc.to_numpy(np.float64, n).reshape(E, T) if rows else None,
               d_state.to_numpy(np.float64, 4 * E).reshape(E, 4) if d_state else None, np.array(out[:]))
    finally:
        for a in (d_ret, d_disc, d_cont, d_state):
            if a:
                a.free()
    return res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("E,T", SHAPES)
def test_scan(lib, E, T, gamma, mode):
    c = scan_inputs(E, T, mode)
    d = {k: dev(lib, c[k]) for k in ("r", "term", "trunc")}
    try:
        for cont_name, cont in c["conts"].items():
            for with_state in (False, True):
                ref = scan_ref(E, T, gamma, mode, cont_name, with_state)
                what = f"{E} x {T} gamma {gamma} {mode} cont {cont_name} state {with_state}"
                row_ret, row_disc, st, agg = scan_dev(lib, d, cont, E, T, gamma, c["state"] if with_state else None)
                same_bits(row_ret, ref["row_ret"], what + ": ret after each row")
                same_bits(row_disc, ref["row_disc"], what + ": disc after each row")
                if with_state:
                    same_bits(st, ref["state"], what + ": state out")
                same_bits(agg, ref["agg"], what + ": aggregate")
                if mode == "none":
                    assert agg.tolist() == [0.0] * NBATCH
                # the aggregate alone, without the per-row outputs
                _, _, st2, agg2 = scan_dev(lib, d, cont, E, T, gamma, c["state"] if with_state else None, rows=False)
                same_bits(agg2, ref["agg"], what + ": aggregate, no row outputs")
                if with_state:
                    same_bits(st2, ref["state"], what + ": state out, no row outputs")
    finally:
        for a in d.values():
            a.free()
    no_error(lib)


def test_scan_bad_arguments(lib):
    c = scan_inputs(5, 7, "random")
    d = {k: dev(lib, c[k]) for k in ("r", "term", "trunc")}
    out = (C.c_double * NBATCH)()
    r, te, tr = d["r"].ptr, d["term"].ptr, d["trunc"].ptr
    f = lib.ppo_episode_scan_device
    assert f(None, te, tr, None, 5, 7, 0.99, None, None, None, out) == -1
    assert f(r, None, tr, None, 5, 7, 0.99, None, None, None, out) == -1
    assert f(r, te, None, None, 5, 7, 0.99, None, None, None, out) == -1
    assert f(r, te, tr, None, 5, 7, 0.99, None, None, None, None) == -1
    for E, T in ((0, 7), (5, 0), (-1, 7), (5, -3)):
        assert f(r, te, tr, None, E, T, 0.99, None, None, None, out) == -1
    no_error(lib)
    assert f(r, te, tr, None, 5, 7, 0.99, None, None, None, out) == 0
    for a in d.values():
        a.free()


# ----------------------------------------------------------------------------- 2. the tracker
def read_flags(lib, ppo, N):
    b = ppo.contents.buffer.contents
    return (ppo_ffi.d2h(lib, b.d_reward_p, F32, N), ppo_ffi.d2h(lib, b.d_terminated_p, np.uint8, N),
            ppo_ffi.d2h(lib, b.d_truncated_p, np.uint8, N))


class Tracker:
    """The reference tracker: the carried per-environment state, the window and the last rollout's aggregate."""

    def __init__(self, E, gamma=0.99):
        self.state, self.window, self.last, self.gamma = fresh(E), zero(), zero(), gamma

    def rollout(self, r, term, trunc, cont, E, T):
        res = scan(r, term, trunc, cont, E, T, self.gamma, self.state)
        self.state, self.last = res["state"], res["agg"]
        self.window = merge(self.window, res["agg"])
        return res

    def check(self, lib, ppo, what):
        got = ep_stats(lib, ppo)
        same_bits(got[:8], report(self.window), what + ": since the last reset")
        same_bits(got[8:], report(self.last), what + ": the last rollout")
        return got


def test_tracker_pendulum(lib):
    E, T = 5, 64
    ppo = make_ppo(lib, [3, 16, 16, 1], E * T)
    assert ep_stats(lib, ppo).tolist() == [0.0] * 16
    ref = Tracker(E)
    for k in range(1, 5):
        lib.ppo_rollout_device(ppo, E, T, 0, 21)
        r, term, trunc = read_flags(lib, ppo, E * T)
        # the 200-step limit: an environment is reset behind the segment's last step iff it was its 200th
        cont = np.full(E, 0 if (k * T) % 200 == 0 else 1, np.uint8)
        ref.rollout(r, term, trunc, cont, E, T)
        got = ref.check(lib, ppo, f"pendulum rollout {k}")
        assert got[8] == (5 if k == 4 else 0)
    assert got[0] == 5 and got[5] == 200.0 and got[13] == 200.0
    assert got[3] <= got[1] <= got[4] < 0.0
    no_error(lib)
    lib.free_ppo(ppo)


def test_tracker_synthetic(lib):
    E, T, S, A = SYNTH_E, SYNTH_T, 5, 2
    ppo = make_ppo(lib, [S, 16, 16, A], E * T)
    ref = Tracker(E)
    kinds = set()
    for k in range(SYNTH_ROLLOUTS):
        began = ref.state[:, 3].copy()                   # rows each environment's episode already has
        lib.ppo_rollout_device(ppo, E, T, 1, SYNTH_SEED)
        r, term, trunc = read_flags(lib, ppo, E * T)
        cont = 1 - term.reshape(E, T)[:, T - 1]
        res = ref.rollout(r, term, trunc, cont, E, T)
        ref.check(lib, ppo, f"synthetic rollout {k}")
        for e, t, _, _, ln in res["episodes"]:
            kinds.add("last row" if t == T - 1 else "inside")
            if ln > t + 1:
                assert ln == began[e] + t + 1
                kinds.add("spans")
    assert kinds == {"inside", "last row", "spans"}, kinds      # what test_episode_cpu.py chose the seed for
    no_error(lib)
    lib.free_ppo(ppo)


def test_tracker_reset_envs_and_gamma(lib):
    E, T = 3, 150
    ppo = make_ppo(lib, [3, 8, 1], E * T)
    g0 = lib.ppo_episode_gamma(ppo, 0.5)
    assert g0 == float(F32(0.99)) and lib.ppo_episode_gamma(ppo, float("nan")) == 0.5
    assert lib.ppo_episode_gamma(ppo, 1.5) == 0.5 and lib.ppo_episode_gamma(ppo, -0.25) == 0.5
    assert lib.ppo_episode_gamma(ppo, 0.75) == 0.5 and lib.ppo_episode_gamma(ppo, 2.0) == 0.75
    ref = Tracker(E, 0.75)
    cont = np.ones(E, np.uint8)                          # 150, 300, 450 steps: never the 200th on a last row

    def roll(E_now, what):
        lib.ppo_rollout_device(ppo, E_now, T, 0, 8)
        r, term, trunc = read_flags(lib, ppo, E_now * T)
        res = ref.rollout(r, term, trunc, cont[:E_now], E_now, T)
        return res, ref.check(lib, ppo, what)

    roll(E, "first rollout")
    _, got = roll(E, "second rollout")
    assert got[0] == 3 and got[5] == 200.0
    lib.ppo_episode_reset_stats(ppo)
    ref.window = zero()                                  # the window alone: the state stays
    got = ref.check(lib, ppo, "after the reset")
    assert got[:8].tolist() == [0.0] * 8 and got[8] == 3
    res, got = roll(E, "third rollout")
    # the episode that ends at step 400 began at step 200, before the reset: its return includes those rows
    assert got[0] == 3 and got[5] == 200.0 and all(ln == 200.0 and t == 99 for _, t, _, _, ln in res["episodes"])
    # a change of n_envs drops the episodes in progress (50 rows each) and keeps the window
    ref.state = fresh(2)
    _, got = roll(2, "fewer environments, first rollout")
    assert got[0] == 3 and got[8] == 0
    _, got = roll(2, "fewer environments, second rollout")
    assert got[0] == 5 and got[8] == 2 and got[13] == 200.0
    no_error(lib)
    lib.free_ppo(ppo)


# ----------------------------------------------------------------------------- 3. evaluation
KINDS = {0: dict(sizes=[3, 16, 16, 1], E=6, T=210), 1: dict(sizes=[5, 16, 16, 2], E=SYNTH_E, T=SYNTH_T)}


def evaluate(lib, ppo, E, T, kind, seed, deterministic, gamma=0.99, n=9):
    out = (C.c_double * max(n, 1))()
    rc = lib.ppo_eval_device(ppo, E, T, kind, seed, deterministic, gamma, out, n)
    return rc, np.array(out[:])


def read_all(lib, ppo, N, S, A):
    b = ppo.contents.buffer.contents
    width = dict(S=S, A=A)
    arrays = {name: ppo_ffi.d2h(lib, getattr(b, name), dt, N * width.get(w, w)) for name, dt, w in BUFFER_ARRAYS}
    return arrays, (b.idx, bool(b.full))


@pytest.mark.parametrize("kind", [0, 1])
def test_eval_sees_the_first_training_rollout(lib, kind):
    cfg = KINDS[kind]
    E, T, seed = cfg["E"], cfg["T"], SYNTH_SEED
    a, b = make_ppo(lib, cfg["sizes"], E * T), make_ppo(lib, cfg["sizes"], E * T)
    rc, ev = evaluate(lib, a, E, T, kind, seed, 0)
    assert rc == 9
    lib.ppo_rollout_device(b, E, T, kind, seed)
    tr = ep_stats(lib, b)
    same_bits(ev[:8], tr[8:], f"kind {kind}: evaluation against the twin's first training rollout")
    assert ev[0] >= 1
    r, term, trunc = read_flags(lib, b, E * T)
    last_open = ~(term.reshape(E, T)[:, -1].astype(bool)) if kind == 1 else np.full(E, T % 200 != 0)
    assert ev[8] == last_open.sum()
    no_error(lib)
    lib.free_ppo(a)
    lib.free_ppo(b)


@pytest.mark.parametrize("obs_norm", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_eval_leaves_the_training_state_alone(lib, kind, obs_norm):
    cfg = KINDS[kind]
    sizes, E, T = cfg["sizes"], cfg["E"], 70
    S, A, N = sizes[0], sizes[-1], E * 70
    a, c = make_ppo(lib, sizes, N), make_ppo(lib, sizes, N)
    for p in (a, c):
        if obs_norm:
            assert lib.ppo_set_obs_norm(p, 5.0) == 0 and lib.ppo_set_reward_norm(p, 10.0) == 0
            assert obs_set_state(lib, p, known_triple(S, 0.1 * np.arange(S), 0.5 + 0.1 * np.arange(S))) == 0
        lib.ppo_rollout_device(p, E, T, kind, 5)         # a training state worth protecting
    before = read_stats(lib, a)
    hash_before = lib.ppo_param_hash(a)
    for det in (0, 1):
        rc, ev = evaluate(lib, a, E + 3, 55, kind, 77, det)
        assert rc == 9 and np.isfinite(ev).all()
    assert lib.ppo_param_hash(a) == hash_before == lib.ppo_param_hash(c)
    np.testing.assert_array_equal(read_stats(lib, a)[19:22], before[19:22])
    assert (before[19] > 0) == obs_norm             # the warmed normaliser's count
    for k in range(2):                                   # what the next rollouts lay depends on every carried part
        if k == 0:
            buf_a, pos_a = read_all(lib, a, N, S, A)
            buf_c, pos_c = read_all(lib, c, N, S, A)
            assert pos_a == pos_c
            for name in buf_a:
                assert buf_a[name].tobytes() == buf_c[name].tobytes(), f"{name} changed under the evaluation"
        for p in (a, c):
            lib.ppo_rollout_device(p, E, T, kind, 5)
        buf_a, pos_a = read_all(lib, a, N, S, A)
        buf_c, pos_c = read_all(lib, c, N, S, A)
        assert pos_a == pos_c
        for name in buf_a:
            assert buf_a[name].tobytes() == buf_c[name].tobytes(), f"rollout {k} after the evaluation: {name}"
        same_bits(ep_stats(lib, a), ep_stats(lib, c), "tracker")
        same_bits(obs_get_state(lib, a, S), obs_get_state(lib, c, S), "observation normaliser")
        same_bits(rew_get_state(lib, a), rew_get_state(lib, c), "reward normaliser")
        assert lib.ppo_param_hash(a) == lib.ppo_param_hash(c)
    no_error(lib)
    lib.free_ppo(a)
    lib.free_ppo(c)


def set_output_bias(lib, ppo, value):
    mu = ppo.contents.policy.contents.mu.contents
    ly = mu.layers[mu.num_layers - 2]
    ppo_ffi.h2d(lib, ly.d_biases, np.full(ly.output_size, value, F32))


@pytest.mark.parametrize("kind", [0, 1])
def test_eval_deterministic(lib, kind):
    cfg = KINDS[kind]
    E, T = cfg["E"], cfg["T"]
    a, twin = make_ppo(lib, cfg["sizes"], 64), make_ppo(lib, cfg["sizes"], 64)
    # a non-zero output bias: |μ| stays far above σ·|ε| = e⁻⁶⁰·|ε| ≈ 1e-26·|ε|, so μ + σ·ε rounds to μ
    for p in (a, twin):
        set_output_bias(lib, p, 0.25)
    pol = twin.contents.policy.contents
    ppo_ffi.h2d(lib, pol.d_log_std, np.full(cfg["sizes"][-1], -60.0, F32))
    rc1, d1 = evaluate(lib, a, E, T, kind, 9, 1)
    rc2, d2 = evaluate(lib, a, E, T, kind, 9, 1)
    rc3, st = evaluate(lib, twin, E, T, kind, 9, 0)
    rc4, noisy = evaluate(lib, a, E, T, kind, 9, 0)
    assert rc1 == rc2 == rc3 == rc4 == 9 and d1[0] >= 1
    same_bits(d1, d2, "two deterministic evaluations")
    same_bits(d1, st, "deterministic against the twin whose sigma is e^-60")
    assert bits(noisy[1]) != bits(d1[1])                 # sigma = 1 does change the returns
    no_error(lib)
    lib.free_ppo(a)
    lib.free_ppo(twin)


def test_eval_pendulum_horizon(lib):
    E = 7
    ppo = make_ppo(lib, [3, 8, 1], 64)
    rc, ev = evaluate(lib, ppo, E, 200, 0, 4, 1)
    assert rc == 9 and ev[0] == E and ev[8] == 0 and ev[5] == 200.0
    rc, ev = evaluate(lib, ppo, E, 199, 0, 4, 1)
    assert rc == 9 and ev[0] == 0 and ev[8] == E and ev[:8].tolist() == [0.0] * 8
    no_error(lib)
    lib.free_ppo(ppo)


def test_eval_bad_arguments(lib):
    pend, synth = make_ppo(lib, [3, 8, 1], 64), make_ppo(lib, [5, 8, 2], 64)
    out = (C.c_double * 9)()
    f = lib.ppo_eval_device
    assert f(None, 4, 10, 0, 1, 1, 0.99, out, 9) == -1
    assert f(pend, 4, 10, 0, 1, 1, 0.99, None, 9) == -1
    assert f(pend, 4, 10, 0, 1, 1, 0.99, out, 8) == -1
    assert f(pend, 0, 10, 0, 1, 1, 0.99, out, 9) == -1
    assert f(pend, -2, 10, 0, 1, 1, 0.99, out, 9) == -1
    assert f(pend, 4, 0, 0, 1, 1, 0.99, out, 9) == -1
    assert f(pend, 4, 10, 2, 1, 1, 0.99, out, 9) == -1
    assert f(pend, 4, 10, -1, 1, 1, 0.99, out, 9) == -1
    assert f(pend, 4, 10, 0, 1, 1, float("nan"), out, 9) == -1
    assert f(synth, 4, 10, 0, 1, 1, 0.99, out, 9) == -1          # Pendulum needs S = 3, A = 1
    no_error(lib)
    assert f(pend, 4, 10, 0, 1, 1, 0.99, out, 9) == 9 and f(synth, 4, 10, 1, 1, 0, 0.99, out, 9) == 9
    lib.free_ppo(pend)
    lib.free_ppo(synth)
