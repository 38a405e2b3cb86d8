"""tests/episode_ref.py pinned on the CPU with hand-computed answers, its aggregates against math.fsum-exact values,
the seed of the GPU tracker test's synthetic case chosen through rng_ref, and the export check of the episode
statistics' entry points (ppo_ext.h ppo_episode_stats …)."""
import math
import subprocess
from fractions import Fraction

import numpy as np

import ppo_ffi
import rng_ref
from episode_ref import F32, NBATCH, bits, ends, episode, fold, fresh, merge, report, scan, zero
from obsnorm_ref import stats64
from rewnorm_ref import bound
from test_obsnorm_cpu import check_triple

NEW_EXPORTS = ["ppo_episode_stats", "ppo_episode_reset_stats", "ppo_episode_gamma", "ppo_episode_scan_device",
               "ppo_eval_device"]
ORDINARY = np.zeros(1, int)      # check_triple's ordinary-column kind

# the GPU tracker test's synthetic case (test_gpu_episode.py): E × T, three rollouts under one seed
SYNTH_E, SYNTH_T, SYNTH_ROLLOUTS, SYNTH_SEED = 37, 129, 3, 1


def u8(*v):
    return np.array(v, np.uint8)


def test_episode_spanning_two_calls():
    """E = 1, T = 2, γ = ½ (every product exact).  Call 1: rewards 1, 2, the segment's truncation continues (cont
    1): nothing is emitted, the state is {3, 1 + ½·2, ¼, 2}.  Call 2: rewards 4, 8; row 0 terminates: episode
    (ret 7, disc 2 + ¼·4 = 3, len 3); row 1 is truncated with cont 0: episode (8, 8, 1)."""
    a = scan([1, 2], u8(0, 0), u8(0, 1), u8(1), 1, 2, 0.5)
    assert a["episodes"] == [] and a["open"] == 1
    np.testing.assert_array_equal(a["agg"], zero())
    np.testing.assert_array_equal(a["state"], [[3.0, 2.0, 0.25, 2.0]])
    np.testing.assert_array_equal(a["row_ret"], [[1.0, 3.0]])
    np.testing.assert_array_equal(a["row_disc"], [[1.0, 2.0]])
    b = scan([4, 8], u8(1, 0), u8(0, 1), u8(0), 1, 2, 0.5, a["state"])
    assert b["episodes"] == [(0, 0, 7.0, 3.0, 3.0), (0, 1, 8.0, 8.0, 1.0)] and b["open"] == 0
    np.testing.assert_array_equal(b["row_ret"], [[7.0, 8.0]])          # before the end row's reset
    np.testing.assert_array_equal(b["row_disc"], [[3.0, 8.0]])
    np.testing.assert_array_equal(b["state"], fresh(1))
    # n 2; mean 7 + (8 − 7)·½; M2 0 + 1·1·(1·½); min 7; max 8; Σlen 4; mean disc 3 + (8 − 3)·½
    np.testing.assert_array_equal(b["agg"], [2.0, 7.5, 0.5, 7.0, 8.0, 4.0, 5.5])
    np.testing.assert_array_equal(report(b["agg"]), [2.0, 7.5, 0.5, 7.0, 8.0, 2.0, 5.5, 0.5])
    # without the carried state the first episode of call 2 would be (4, 4, 1)
    assert scan([4, 8], u8(1, 0), u8(0, 1), u8(0), 1, 2, 0.5)["episodes"][0] == (0, 0, 4.0, 4.0, 1.0)


def test_end_on_the_last_row_depends_on_cont():
    r, term, trunc = [1, 2, 3], u8(0, 0, 0), u8(0, 0, 1)
    assert scan(r, term, trunc, u8(1), 1, 3, 1.0)["episodes"] == []
    assert scan(r, term, trunc, u8(0), 1, 3, 1.0)["episodes"] == [(0, 2, 6.0, 6.0, 3.0)]
    assert scan(r, term, trunc, None, 1, 3, 1.0)["episodes"] == [(0, 2, 6.0, 6.0, 3.0)]
    # a truncation before the last row ends whatever cont says; so does a termination on the last row
    assert scan(r, term, u8(0, 1, 1), u8(1), 1, 3, 1.0)["episodes"] == [(0, 1, 3.0, 3.0, 2.0)]
    assert scan(r, u8(0, 0, 1), trunc, u8(1), 1, 3, 1.0)["episodes"] == [(0, 2, 6.0, 6.0, 3.0)]
    np.testing.assert_array_equal(ends(u8(0, 0, 0, 0), u8(0, 1, 0, 1), u8(1, 0), 2, 2), [[False, False], [False, True]])


def test_both_flags_set_end_one_episode():
    a = scan([1, 2, 3], u8(0, 1, 0), u8(0, 1, 0), None, 1, 3, 1.0)
    assert a["episodes"] == [(0, 1, 3.0, 3.0, 2.0)] and a["open"] == 1
    np.testing.assert_array_equal(a["state"], [[3.0, 3.0, 1.0, 1.0]])


def test_gamma_zero_and_one():
    r = [0.5, 3, -2, 7]
    a0 = scan(r, u8(0, 0, 1, 0), u8(0, 0, 0, 1), None, 1, 4, 0.0)
    assert a0["episodes"] == [(0, 2, 1.5, 0.5, 3.0), (0, 3, 7.0, 7.0, 1.0)]      # disc = the first reward alone
    a1 = scan(r, u8(0, 0, 1, 0), u8(0, 0, 0, 1), None, 1, 4, 1.0)
    assert a1["episodes"] == [(0, 2, 1.5, 1.5, 3.0), (0, 3, 7.0, 7.0, 1.0)]      # disc = ret
    np.testing.assert_array_equal(a1["row_ret"], a1["row_disc"])


def test_zero_episodes_give_the_zero_aggregate():
    a = scan(np.ones(6), np.zeros(6, np.uint8), np.zeros(6, np.uint8), None, 2, 3, 0.99)
    np.testing.assert_array_equal(a["agg"], zero())
    np.testing.assert_array_equal(report(a["agg"]), np.zeros(8))
    assert a["open"] == 2
    one = episode(3.0, 2.0, 5.0)
    np.testing.assert_array_equal(merge(zero(), one), one)             # an empty side is the identity
    np.testing.assert_array_equal(merge(one, zero()), one)


def test_fold_order():
    """The documented order, spelled out for E = 600 (per = 3): runs of three, then the tree."""
    rng = np.random.default_rng(3)
    parts = [episode(x, y, 1.0 + i % 5) if i % 7 else zero() for i, (x, y) in enumerate(rng.normal(size=(600, 2)))]
    q = []
    for i in range(256):
        a = zero()
        for p in parts[3 * i:3 * i + 3]:
            a = merge(a, p)
        q.append(a)
    while len(q) > 1:
        q = [merge(q[i], q[i + 1]) for i in range(0, len(q), 2)]
    np.testing.assert_array_equal(bits(fold(np.array(parts))), bits(q[0]))


def mixed_rewards(rng, n):
    """Magnitudes ≈ 1e6 and ≈ 1e-3 side by side: a re-associated or contracted sum changes bits."""
    big = rng.random(n) < 0.5
    return np.where(big, 1e6 * rng.normal(size=n), 1e-3 * rng.normal(size=n)).astype(F32)


def test_aggregates_against_fsum():
    E, T, gamma = 130, 257, 0.99
    rng = np.random.default_rng(11)
    r = mixed_rewards(rng, E * T)
    term = (rng.random(E * T) < 0.05).astype(np.uint8)
    trunc = (rng.random(E * T) < 0.05).astype(np.uint8)
    cont = rng.integers(0, 2, E).astype(np.uint8)
    a = scan(r, term, trunc, cont, E, T, gamma)
    eps = a["episodes"]
    assert len(eps) > 1000 and a["agg"][0] == len(eps)
    # every episode's return and discounted return against exact arithmetic
    g = Fraction(float(np.float64(F32(gamma))))
    r2 = r.reshape(E, T)
    start = {}
    exact_ret, worst = [], 0.0
    for e, t, ret, disc, ln in eps:
        t0 = start.get(e, 0)
        rows = r2[e, t0:t + 1].astype(np.float64)
        assert ln == rows.size
        ex = math.fsum(rows.tolist())
        exact_ret.append(ex)
        assert abs(ret - ex) <= rows.size * 2.0 ** -53 * np.abs(rows).sum()
        exd = float(sum(g ** k * Fraction(float(x)) for k, x in enumerate(rows)))
        # Σ g^k r_k is the recurrence R_i = r_i + g·R_{i−1} over the episode's rows in reverse: rewnorm_ref's bound
        z = np.zeros(rows.size, bool)
        b = bound(rows[::-1].astype(F32), z, z, gamma)[-1]
        assert abs(disc - exd) <= b
        worst = max(worst, abs(disc - exd) / b if b > 0 else 0.0)
        start[e] = t + 1
    print(f"worst discounted-return err / bound {worst:.3g}")
    ref = stats64(np.array(exact_ret).reshape(-1, 1))
    print(check_triple(a["agg"][:3], ref, ORDINARY, "returns' triple against fsum"))
    assert a["agg"][3] == min(x[2] for x in eps) and a["agg"][4] == max(x[2] for x in eps)
    assert a["agg"][5] == sum(x[4] for x in eps)
    md = math.fsum(x[3] for x in eps) / len(eps)
    assert abs(a["agg"][6] - md) <= 1e-10 * np.std([x[3] for x in eps])


def test_synthetic_seed_has_every_kind_of_end():
    """The seed of the GPU tracker test: rng_ref reproduces the synthetic environment's termination draws bit for
    bit, so the three kinds of end are asserted here, without a GPU."""
    E, T, R = SYNTH_E, SYNTH_T, SYNTH_ROLLOUTS
    done = rng_ref.synth_done(E, np.arange(R * T), SYNTH_SEED)          # [global step, env]
    inside = last_row = spans = 0
    for e in range(E):
        prev = -1                                                       # the global step of the previous end
        for s in np.nonzero(done[:, e])[0]:
            last_row += s % T == T - 1
            inside += s % T != T - 1
            spans += (prev + 1) // T < s // T                           # began in an earlier rollout
            prev = s
    print(f"seed {SYNTH_SEED}: {inside} ends inside a segment, {last_row} on a last row, {spans} span a boundary")
    assert inside >= 1 and last_row >= 1 and spans >= 1


def test_new_functions_are_exported(lib_built):
    out = subprocess.run(["nm", "-D", "--defined-only", ppo_ffi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    missing = [n for n in NEW_EXPORTS if n not in exported]
    assert len(NEW_EXPORTS) == 5 and not missing, f"not exported: {missing}"
    for n in NEW_EXPORTS:
        assert getattr(lib_built, n).argtypes is not None, n
    assert NBATCH == 7
