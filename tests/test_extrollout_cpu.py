"""tests/extrollout_ref.py pinned on the CPU, the conditions the GPU test's seeds and shapes must meet, and the
export check of the open-rollout entry points (ppo_ext.h ppo_rollout_begin …)."""
import itertools
import subprocess

import numpy as np

import episode_ref
import extrollout_ref as xr
import ppo_ffi
import rng_ref
from rewnorm_ref import chan, returns64, triple64
from test_obsnorm_cpu import check_triple

NEW_EXPORTS = ["ppo_rollout_begin", "ppo_rollout_act", "ppo_rollout_store", "ppo_rollout_end", "ppo_act_device",
               "ppo_env_state_floats", "ppo_env_reset_device", "ppo_env_step_device"]

# what tests/test_gpu_extrollout.py drives (the shapes are the issue's)
SYNTH_SEED, SYNTH_E, SYNTH_T, SYNTH_ROLLOUTS = 5, 300, 8, 2
PENDULUM_E, PENDULUM_T, PENDULUM_ROLLOUTS = 5, 67, 3
REWNORM_GAMMA = 0.5


def test_store_rule_agrees_with_the_episode_end_predicate():
    """A row ends an episode, by episode_ref.ends over the stored flags and cont[], exactly where the environment
    itself said so: the segment-end truncation the store adds ends nothing.  Every combination of the two flags at
    a mid-segment cell and at the segment end."""
    combos = list(itertools.product([0, 1], repeat=4))               # (term, trunc) mid, (term, trunc) at T − 1
    E, T = len(combos), 3
    term_in = np.zeros((E, T), bool)
    trunc_in = np.zeros((E, T), bool)
    for e, (a, b, c, d) in enumerate(combos):
        term_in[e, 1], trunc_in[e, 1], term_in[e, T - 1], trunc_in[e, T - 1] = a, b, c, d
    term, trunc, cont = xr.store_flags(term_in, trunc_in)
    np.testing.assert_array_equal(term, term_in)
    np.testing.assert_array_equal(trunc[:, :-1], trunc_in[:, :-1])
    assert (term[:, -1] | trunc[:, -1]).all(), "every segment ends done"
    np.testing.assert_array_equal(trunc[:, -1], trunc_in[:, -1] | ~term_in[:, -1])
    np.testing.assert_array_equal(cont, ~(term_in[:, -1] | trunc_in[:, -1]))
    np.testing.assert_array_equal(episode_ref.ends(term, trunc, cont, E, T), term_in | trunc_in)
    # the built-in kernels' variant (truncated = 1 on a terminated segment end) ends the same rows
    trunc_builtin = trunc.copy()
    trunc_builtin[:, -1] = True
    np.testing.assert_array_equal(episode_ref.ends(term, trunc_builtin, cont, E, T), term_in | trunc_in)
    np.testing.assert_array_equal(term | trunc, term | trunc_builtin)


def test_lay_places_rows_env_major():
    E, T, S = 2, 3, 2
    rng = np.random.default_rng(0)
    nxt = rng.integers(0, 50, (E, T, S)).astype(np.float32)
    after = nxt + 100
    first = np.array([[7, 8], [9, 10]], np.float32)
    buf = xr.lay(first, np.arange(E * T).reshape(E, T), nxt, np.zeros((E, T)), np.zeros((E, T)), after)
    for e in range(E):
        np.testing.assert_array_equal(buf["state"][e * T], first[e])
        for t in range(T):
            np.testing.assert_array_equal(buf["next_state"][e * T + t], nxt[e, t])
            assert buf["reward"][e * T + t] == e * T + t
            if t + 1 < T:
                np.testing.assert_array_equal(buf["state"][e * T + t + 1], after[e, t])
    np.testing.assert_array_equal(buf["current"], after[:, -1])
    # obs_after omitted: an environment that never resets
    np.testing.assert_array_equal(xr.lay(first, np.zeros((E, T)), nxt, np.zeros((E, T)), np.zeros((E, T)))["state"]
                                  .reshape(E, T, S)[:, 1:], nxt[:, :-1])


def test_counter_environment():
    tb = xr.counter_tables()
    ended = tb["term"] | tb["trunc"]
    assert tb["term"][:, xr.T - 1].any(), "a termination on the segment end of rollout 1"
    assert tb["trunc"][:, 1:xr.T - 1].any(), "a truncation at a mid-segment cell"
    np.testing.assert_array_equal((tb["obs_after"] != tb["next_obs"]).any(axis=2), ended)
    bufs, stats = xr.counter_expected()
    b1, b2 = bufs
    # hand-checked cells: env 0 terminates at t = 1, so row 2 starts the fresh episode (0.5, 2)
    np.testing.assert_array_equal(b1["state"][0:4], [[0, 0], [0, 1], [0.5, 2], [0, 3]])
    np.testing.assert_array_equal(b1["next_state"][0:4], [[0, 1], [0, 2], [0, 3], [0, 4]])
    np.testing.assert_array_equal(b1["reward"], [0, 1, 2, 3, 10, 11, 12, 13, 20, 21, 22, 23])
    np.testing.assert_array_equal(b1["term"], [0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0])
    np.testing.assert_array_equal(b1["trunc"], [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1])
    np.testing.assert_array_equal(b1["cont"], [1, 0, 1])
    np.testing.assert_array_equal(b2["state"][0::xr.T], [[0, 4], [1.5, 4], [2, 4]])
    np.testing.assert_array_equal(b2["term"], [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0])
    np.testing.assert_array_equal(b2["trunc"], [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1])
    np.testing.assert_array_equal(b2["cont"], [0, 1, 1])
    # episodes: rollout 1 ends (0, 1) {0 + 1}, (1, 3) {10 + 11 + 12 + 13}, (2, 2) {20 + 21 + 22}; rollout 2 ends
    # (2, 5) {23 + 24 + 25} and (0, 7) {2 + … + 7}: the segment ends that merely cut an episode count for nothing
    assert stats[0][8] == 3 and stats[0][0] == 3 and stats[0][11:13].tolist() == [1.0, 63.0]
    assert stats[1][8] == 2 and stats[1][0] == 5 and stats[1][11:13].tolist() == [27.0, 72.0]
    assert stats[1][3:5].tolist() == [1.0, 72.0]
    # the returns' carry the GPU test checks through the reward normaliser: a non-zero carry enters rollout 2, and
    # the expected triples are "ordinary" columns for check_triple's bound
    g = REWNORM_GAMMA
    R1, co1 = returns64(b1["reward"], b1["term"], b1["trunc"], g, xr.T, np.zeros(xr.E), b1["cont"])
    assert (co1[b1["cont"] != 0] != 0).all() and (co1[b1["cont"] == 0] == 0).all()
    R2, _ = returns64(b2["reward"], b2["term"], b2["trunc"], g, xr.T, co1, None)
    R2z, _ = returns64(b2["reward"], b2["term"], b2["trunc"], g, xr.T, np.zeros(xr.E), None)
    assert (R2 != R2z).any()
    ordinary = np.zeros(1, int)
    for want in (triple64(R1), chan(triple64(R1), triple64(R2))):
        check_triple(want, want, ordinary, "the expected triple is ordinary")


def test_conditions_of_the_gpu_cases():
    # synthetic: terminations do not depend on observations or actions, so the seed is checked here
    g = np.arange(SYNTH_T * SYNTH_ROLLOUTS)
    done = rng_ref.synth_done(SYNTH_E, g, SYNTH_SEED)
    assert done.shape == (g.size, SYNTH_E) and done.any(), "SYNTH_SEED gives no termination"
    # Pendulum: every environment meets the 200-step limit once, inside a segment of the last rollout
    steps = PENDULUM_T * PENDULUM_ROLLOUTS
    assert steps > 200
    t_limit = 199 % PENDULUM_T
    assert 199 // PENDULUM_T == PENDULUM_ROLLOUTS - 1 and 0 < t_limit < PENDULUM_T - 1
    assert steps < 400


def test_new_functions_are_exported(lib_built):
    out = subprocess.run(["nm", "-D", "--defined-only", ppo_ffi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert not [n for n in NEW_EXPORTS if n not in exported]
    for n in NEW_EXPORTS:
        assert n in ppo_ffi._SIGS, n
    assert lib_built.ppo_env_state_floats(0, 3) == 3 and lib_built.ppo_env_state_floats(1, 376) == 376
    assert lib_built.ppo_env_state_floats(2, 4) == 5
    assert lib_built.ppo_env_state_floats(3, 4) == -1 and lib_built.ppo_env_state_floats(0, 4) == -1
