"""The open rollout (ppo_ext.h ppo_rollout_begin / _act / _store / _end): a numpy statement of the store rule.

Written from the comment in ppo_ext.h alone.  The caller's environment hands in, per step and environment, a
reward, the transition's next observation, its own terminated / truncated flags and the observation the next step
starts from; `store_flags` turns the flags into the buffer's and into cont[], `lay` lays a whole rollout env-major.
The "counter environment" below is a table-driven stand-in for a foreign simulator whose every value is a small
integer or a half, so each buffer array has one exact expected value.
"""
import numpy as np

import episode_ref

F32 = np.float32


def store_flags(term_in, trunc_in):
    """Environment flags [E, T] → (terminated [E, T], truncated [E, T], cont [E]) as the store writes them:
    terminated = term_in; truncated = trunc_in || (t == T−1 && !terminated); cont[e] = !(term_in || trunc_in) at
    t = T−1 — the environment's own flags alone decide it."""
    term_in = np.asarray(term_in).astype(bool)
    trunc_in = np.asarray(trunc_in).astype(bool)
    term = term_in.copy()
    trunc = trunc_in.copy()
    trunc[:, -1] |= ~term[:, -1]
    cont = ~(term_in[:, -1] | trunc_in[:, -1])
    return term, trunc, cont


def lay(obs_first, reward, next_obs, term_in, trunc_in, obs_after=None):
    """One rollout laid env-major.  obs_first [E, S]: what begin wrote to rows e·T; reward [E, T]; next_obs and
    obs_after [E, T, S] (obs_after None: next_obs); flags [E, T].  Returns dict(state, next_state [E·T, S], reward
    [E·T], term, trunc [E·T] uint8, cont [E] uint8, current [E, S]): row e·T + t, and the observations the next
    rollout continues from."""
    reward = np.asarray(reward, F32)
    next_obs = np.asarray(next_obs, F32)
    after = next_obs if obs_after is None else np.asarray(obs_after, F32)
    E, T, S = next_obs.shape
    state = np.empty((E, T, S), F32)
    state[:, 0] = np.asarray(obs_first, F32)
    state[:, 1:] = after[:, :-1]
    term, trunc, cont = store_flags(term_in, trunc_in)
    return dict(state=state.reshape(E * T, S), next_state=next_obs.reshape(E * T, S).copy(),
                reward=reward.reshape(E * T).copy(), term=term.reshape(E * T).astype(np.uint8),
                trunc=trunc.reshape(E * T).astype(np.uint8), cont=cont.astype(np.uint8), current=after[:, -1].copy())


# ------------------------------------------------------------------------------------------------
# the counter environment: E = 3 environments, S = 2, A = 1, two rollouts of T = 4 (global steps 0 … 7)
# ------------------------------------------------------------------------------------------------
E, T, S, A, ROLLOUTS = 3, 4, 2, 1, 2
G = T * ROLLOUTS
# (e, global step) cells where the environment itself ends the episode
TERMINATED = [(0, 1), (1, T - 1), (2, 5)]        # mid-segment; the segment end of rollout 1; mid-segment of rollout 2
TRUNCATED = [(2, 2), (0, G - 1)]                 # mid-segment; the environment's own limit on a segment end


def counter_tables():
    """The whole run as tables indexed [e, g], g the global step: obs (e, g) before the step, reward 10·e + g,
    next_obs (e, g + 1), the flags, and obs_after = next_obs except where the episode ended, where the fresh
    episode is marked by e + 0.5 in column 0."""
    e = np.arange(E, dtype=F32)[:, None] + np.zeros((1, G), F32)
    g = np.arange(G, dtype=F32)[None, :] + np.zeros((E, 1), F32)
    term = np.zeros((E, G), bool)
    trunc = np.zeros((E, G), bool)
    for cell in TERMINATED:
        term[cell] = True
    for cell in TRUNCATED:
        trunc[cell] = True
    next_obs = np.stack([e, g + 1], 2)
    after = next_obs.copy()
    after[term | trunc, 0] += F32(0.5)
    return dict(obs0=np.stack([e[:, 0], g[:, 0]], 1), reward=10 * e + g, next_obs=next_obs, obs_after=after, term=term,
                trunc=trunc)


def counter_expected():
    """Per rollout the expected buffer (`lay`), then `stats`: the 16 values ppo_episode_stats reports after each
    rollout (window, last rollout), from episode_ref driven with the rollouts' own cont[]."""
    tb = counter_tables()
    bufs, stats = [], []
    first, state, window = tb["obs0"], None, episode_ref.zero()
    for r in range(ROLLOUTS):
        sl = slice(r * T, (r + 1) * T)
        buf = lay(first, tb["reward"][:, sl], tb["next_obs"][:, sl], tb["term"][:, sl], tb["trunc"][:, sl],
                  tb["obs_after"][:, sl])
        sc = episode_ref.scan(buf["reward"], buf["term"], buf["trunc"], buf["cont"], E, T, 0.99, state)
        state, window = sc["state"], episode_ref.merge(window, sc["agg"])
        stats.append(np.concatenate([episode_ref.report(window), episode_ref.report(sc["agg"])]))
        bufs.append(buf)
        first = buf["current"]
    return bufs, stats
