"""tests/rng_ref.py against what is known without a GPU (test_gpu_rng.py then pins the kernels to it).

  * Philox-4x32-10's published known-answer vectors (Random123's kat_vectors: the zero, all-ones and
    π-digits inputs);
  * u01's range and rounding: minimum 2⁻²⁵, maximum exactly 1.0, exact and strictly increasing in
    x >> 8 below 2²³, round-to-even (hence only non-decreasing) from there on;
  * splitmix64 against the oracle's restatement of host/ppo.c;
  * stream disjointness over the shapes test_gpu_rng.py runs: under one key no two consumers — policy
    noise, env decision, env ε, reset — draw the same (counter, offset) pair, across calls too;
  * the synthetic rollout's terminations depend on (e, g) alone: their counts at the GPU test's shape
    are pinned, and two rollouts under one seed differ.
"""
import numpy as np

import rng_ref as R

F32, U64 = np.float32, np.uint64


def _words(lo_hi_pairs):
    return [lo | (hi << 32) for lo, hi in lo_hi_pairs]


def test_philox_known_answers():
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
         (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for ctr, key, want in kat:
        counter, offset = _words([(ctr[0], ctr[1]), (ctr[2], ctr[3])])
        seed, = _words([key])
        got = tuple(int(w) for w in R.philox4x32_10(counter, offset, seed))
        assert got == want, (ctr, key, [hex(g) for g in got])
    # vectorised: the three at once give the three
    ctrs = np.array([_words([(c[0], c[1])])[0] for c, _, _ in kat], dtype=U64)
    offs = np.array([_words([(c[2], c[3])])[0] for c, _, _ in kat], dtype=U64)
    keys = np.array([_words([k])[0] for _, k, _ in kat], dtype=U64)
    out = np.stack(R.philox4x32_10(ctrs, offs, keys), 1)
    np.testing.assert_array_equal(out, np.array([w for _, _, w in kat], dtype=U64))


def test_philox_words_are_32_bit_and_inputs_matter():
    c = np.arange(1000, dtype=U64)
    base = np.stack(R.philox4x32_10(c, 5, 9))
    assert base.max() < 2 ** 32
    for other in (R.philox4x32_10(c + U64(1), 5, 9), R.philox4x32_10(c, 6, 9), R.philox4x32_10(c, 5, 10),
                  R.philox4x32_10(c + U64(1 << 32), 5, 9), R.philox4x32_10(c, 5 + (1 << 32), 9),
                  R.philox4x32_10(c, 5, 9 + (1 << 32))):
        assert (np.stack(other) != base).mean() > 0.99
    # the offset selects a stream; it is not added to the counter
    assert (np.stack(R.philox4x32_10(c, 1, 9)) != np.stack(R.philox4x32_10(c + U64(1), 0, 9))).mean() > 0.99


def test_u01_range_and_rounding():
    two23 = 1 << 23
    assert R.u01(0) == F32(2.0 ** -25) and R.u01(0xFF) == F32(2.0 ** -25)       # low 8 bits dropped
    assert R.u01(0xFFFFFFFF) == F32(1.0)                                          # the closed end
    assert R.u01(0xFFFFFFFF).dtype == F32
    n = np.concatenate([np.arange(0, 4096), np.arange(two23 - 4096, two23),
                        np.random.default_rng(0).integers(0, two23, 100000)]).astype(U64)
    u = R.u01(n << U64(8))
    np.testing.assert_array_equal(u.astype(np.float64), (n.astype(np.float64) + 0.5) / 2.0 ** 24)   # exact
    lo = np.arange(two23 - 70000, two23, dtype=U64) << U64(8)
    assert (np.diff(R.u01(lo)) > 0).all()                                         # strictly monotone
    hi = np.arange(two23, two23 + 70000, dtype=U64)
    uh = R.u01(hi << U64(8))
    assert (np.diff(uh) >= 0).all() and (np.diff(uh) == 0).any()                  # ties: neighbours share a value
    # round-to-even: n + 0.5 goes to the even neighbour
    even = np.where(hi % U64(2) == 0, hi, hi + U64(1)).astype(np.float64)
    np.testing.assert_array_equal(uh.astype(np.float64), even / 2.0 ** 24)
    top = R.u01(np.arange(2 ** 24 - 8, 2 ** 24, dtype=U64) << U64(8))
    assert top.max() == F32(1.0) and (top <= F32(1.0)).all() and (R.u01(np.arange(0, 1 << 16, dtype=U64)) > 0).all()


def test_splitmix64_matches_oracle(oracle):
    for z in (0, 1, 7, 1234, 7 ^ R.ROLLOUT_XOR, (1 << 64) - 1, 0xDEADBEEF12345678):
        assert R.splitmix64(z) == oracle.splitmix64(z)
    assert R.rollout_key(7) == oracle.splitmix64(7 ^ 0x524F4C4C) and R.reset_key(7) == oracle.splitmix64(7)
    assert R.rollout_key(7) != R.reset_key(7)


def test_normal_at_dtypes_agree():
    """The fp32 evaluation sits within a few ulps of the float64 reference: the distance that sizes the
    GPU tests' tolerance is small, so that tolerance cannot hide a wrong stream (an O(1) error)."""
    idx = np.arange(200000, dtype=U64)
    n64 = R.normal_at(idx, R.K_NOISE + 3, 99, np.float64)
    n32 = R.normal_at(idx, R.K_NOISE + 3, 99, np.float32)
    assert n32.dtype == F32 and n64.dtype == np.float64
    assert np.abs(n32 - n64).max() < 8 * np.spacing(F32(np.abs(n64).max()))
    assert abs(n64.mean()) < 0.01 and abs(n64.std() - 1) < 0.01


def _pairs(key, counter, offset):
    c, o = np.broadcast_arrays(counter, offset)
    return {(key, int(a), int(b)) for a, b in zip(c.ravel().tolist(), o.ravel().tolist())}


def _assert_disjoint(groups):
    total, seen = 0, set()
    for name, s in groups.items():
        assert not (seen & s), f"{name} shares a (key, counter, offset) with an earlier consumer"
        seen |= s
        total += len(s)
    assert len(seen) == total


def test_rollout_streams_disjoint():
    """test_gpu_rng.py's rollouts: synthetic [70, 16, 3] E = 64, T = 64, two calls; Pendulum E = 8,
    T = 200, three calls.  Each consumer's own pairs are distinct too (its set has as many members as
    it makes draws)."""
    seed = 7
    E, S, A, T, calls = 64, 70, 3, 64, 2
    g = np.arange(calls * T)
    key, key0 = R.rollout_key(seed), R.reset_key(seed)
    groups = dict(first=_pairs(key0, *R.addr_first_reset(E * S)),
                  noise=_pairs(key, *R.addr_policy_noise(E, A, g)),
                  decision=_pairs(key, *R.addr_env_decision(E, g)),
                  eps=_pairs(key, *R.addr_env_eps(E, S, g)),
                  reset=_pairs(key, *R.addr_reset(E * S, g)))
    want = dict(first=E * S, noise=len(g) * E * A, decision=len(g) * E, eps=len(g) * E * S, reset=len(g) * E * S)
    assert {k: len(v) for k, v in groups.items()} == want
    _assert_disjoint(groups)

    E, T, calls = 8, 200, 3
    g = np.arange(calls * T)
    groups = dict(first=_pairs(key0, *R.addr_first_reset(E)), noise=_pairs(key, *R.addr_policy_noise(E, 1, g)),
                  reset=_pairs(key, *R.addr_reset(E, g)))
    assert {k: len(v) for k, v in groups.items()} == dict(first=E, noise=len(g) * E, reset=len(g) * E)
    _assert_disjoint(groups)


def test_stream_bands_do_not_meet():
    """The offset bands kNoise, kEnv (two offsets per step) and kReset stay apart for 2³⁸ steps, and the
    first reset's offset kReset − 1 lies under another key."""
    steps = 1 << 38
    assert R.K_NOISE + steps <= R.K_ENV and R.K_ENV + 2 * steps + 1 < R.K_RESET
    assert R.K_ENV + 2 * steps + 1 < R.K_RESET - 1


def test_fill_streams_disjoint():
    """ppo_fill_synthetic: five keys s0 ^ 1 … s0 ^ 5, one per consumer, at the small fill case."""
    seed, E, T, S, A = 1234, 3, 5, 7, 2
    N = E * T
    keys = [R.fill_key(seed, c) for c in (R.FILL_STATE, R.FILL_FLAGS, R.FILL_NEXT, R.FILL_REWARD, R.FILL_ACTION)]
    assert len(set(keys)) == 5
    groups = dict(state=_pairs(keys[0], np.arange(N * S), R.OFF_UNIFORM), flags=_pairs(keys[1], np.arange(N), R.OFF_FLAGS),
                  nxt=_pairs(keys[2], np.arange(N * S), R.OFF_NEXT), reward=_pairs(keys[3], np.arange(N), R.OFF_NORMAL),
                  action=_pairs(keys[4], np.arange(N * A), 0))
    _assert_disjoint(groups)
    assert len({R.OFF_UNIFORM, R.OFF_FLAGS, R.OFF_NEXT, R.OFF_NORMAL, 0}) == 5


def test_fill_model_structure():
    for p in (0.0, 1 / 200, 1.0):
        f = R.fill_synthetic(3, 5, 7, 1234, p)
        assert f["state"].dtype == F32 and f["next_state"].dtype == F32 and np.abs(f["state"]).max() <= 1
        last = np.arange(15) % 5 == 4
        np.testing.assert_array_equal(f["trunc"], last & ~f["term"])
        link = ~f["unlinked"]
        np.testing.assert_array_equal(f["next_state"][link], f["state"][np.nonzero(link)[0] + 1])
        assert not (f["next_state"][~link] == f["state"][~link]).all()
        if p == 0.0:
            assert not f["term"].any()
        if p == 1.0:
            assert f["term"].all()              # no u01 == 1 among 15 rows


def test_synthetic_terminations_follow_the_global_step():
    """[70, 16, 3], E = 64, T = 64, seed 7: 14 terminations in the first rollout, 10 in the second, at
    different cells — the done branch is exercised in both and the two rollouts differ."""
    E, T, seed = 64, 64, 7
    d0 = R.synth_done(E, np.arange(0, T), seed)
    d1 = R.synth_done(E, np.arange(T, 2 * T), seed)
    assert (int(d0.sum()), int(d1.sum())) == (14, 10)
    assert (d0 != d1).any()
    n0 = R.synth_reward_noise(E, np.arange(0, T), seed)
    n1 = R.synth_reward_noise(E, np.arange(T, 2 * T), seed)
    assert np.abs(n0 - n1).max() > 1.0


def test_pendulum_resets_follow_the_global_step():
    E, T = 8, 200
    th = [R.pendulum_reset(E, [c * T + T - 1], 11) for c in range(3)]
    assert (th[0][0] != th[1][0]).all() and (th[1][0] != th[2][0]).all() and (th[0][1] != th[1][1]).all()
    t0, d0 = R.pendulum_first_reset(E, 11)
    assert (np.abs(t0) <= R.PI_F).all() and (np.abs(d0) <= 1).all() and t0.dtype == F32 and d0.dtype == F32
