"""Plain numpy restatement of libppo's device random generators and of what they fill.

Written from the algorithm (Philox-4x32-10: Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as
easy as 1, 2, 3", SC'11) and from the stream table at the head of ppo.c_amd/csrc/rng.h, which names
every consumer's (key, counter, offset).  Nothing here reads the device or the library: the CPU
tests (test_rng_cpu.py) pin this file to the published known answers, the GPU tests
(test_gpu_rng.py) pin the kernels to this file.

Numeric convention.  Everything the device computes with +, −, × alone is evaluated here in fp32
with the device's operation order, so it is bit exact.  What goes through logf / cosf / sinf / tanhf
/ expf takes a `dtype`: np.float64 is the reference (fp32 inputs, the transcendental part in double),
np.float32 is the "straightforward numpy-fp32 evaluation" whose distance from the reference sizes
the tests' tolerance.
"""
import functools

import numpy as np

F32 = np.float32
F64 = np.float64
U64 = np.uint64
M32 = U64(0xFFFFFFFF)
M64 = (1 << 64) - 1

PHILOX_M0, PHILOX_M1 = U64(0xD2511F53), U64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = U64(0x9E3779B9), U64(0xBB67AE85)

# rollout streams: the high bits of the offset (rng.h)
K_NOISE, K_ENV, K_RESET = 1 << 40, 2 << 40, 3 << 40
# ppo_fill_synthetic: offset of each fill kernel, and the xor that derives each consumer's key from s0
OFF_UNIFORM, OFF_NORMAL, OFF_FLAGS, OFF_NEXT = 0x5EED, 0xA11CE, 0x7E4, 0x4E57
FILL_STATE, FILL_FLAGS, FILL_NEXT, FILL_REWARD, FILL_ACTION = 1, 2, 3, 4, 5
ROLLOUT_XOR = 0x524F4C4C

PI_F = F32(np.pi)
TWO_PI_F = F32(2) * PI_F                       # 2.f * (float)M_PI: exact


def splitmix64(z):
    """host/ppo.c splitmix64 on a Python int."""
    z = (int(z) + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def fill_key(seed, consumer):
    return splitmix64(seed) ^ consumer


def reset_key(seed):
    """Key of the first reset of ppo_rollout_device."""
    return splitmix64(seed)


def rollout_key(seed):
    """Key of every later draw of ppo_rollout_device: policy noise, env decision, env ε, resets."""
    return splitmix64((int(seed) ^ ROLLOUT_XOR) & M64)


def _u64(a):
    if isinstance(a, (int, np.integer)):
        return np.asarray(int(a) & M64, dtype=U64)
    return np.asarray(a).astype(U64)


def philox4x32_10(counter, offset, seed):
    """Ten Philox-4x32 rounds.  Counter words (lo, hi) of `counter` then (lo, hi) of `offset`, key words
    (lo, hi) of `seed`; uint64 arrays or ints, broadcast against each other.  Returns the four output
    words as uint64 arrays holding 32-bit values."""
    counter, offset, seed = np.broadcast_arrays(_u64(counter), _u64(offset), _u64(seed))
    c0, c1 = counter & M32, counter >> U64(32)
    c2, c3 = offset & M32, offset >> U64(32)
    k0, k1 = seed & M32, seed >> U64(32)
    for _ in range(10):
        p0 = PHILOX_M0 * c0                     # 32 × 32 → 64 bits: no overflow in uint64
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> U64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def u01(x):
    """fp32 ((x >> 8) + 0.5f) · 2⁻²⁴: in (0, 1], exact below 2²³, round-to-even from there on."""
    n = (_u64(x) >> U64(8)).astype(F32)         # < 2²⁴: exact
    return (n + F32(0.5)) * F32(1.0 / 16777216.0)


def box_muller(x, y, dtype=F64):
    """sqrt(−2·log u1)·cos(2π·u2) from two output words: u1, u2 and the cosine's argument are the
    device's fp32 values; log, sqrt and cos in `dtype`."""
    u1, u2 = u01(x), u01(y)
    arg = TWO_PI_F * u2                         # fp32, as the device rounds it
    return np.sqrt(dtype(-2) * np.log(u1.astype(dtype))) * np.cos(arg.astype(dtype))


def normal_at(idx, offset, seed, dtype=F64):
    x, y, _, _ = philox4x32_10(idx, offset, seed)
    return box_muller(x, y, dtype)


def uniform_pm1(word):
    """−1 + 2·u01: exact in fp32."""
    return F32(-1) + F32(2) * u01(word)


# ------------------------------------------------------------------------------------------------
# Addresses: the (counter, offset) pairs each consumer draws.  The models below and the disjointness
# test both go through these.
# ------------------------------------------------------------------------------------------------
def _g(g):
    return np.asarray(g, dtype=U64)


def addr_policy_noise(E, A, g):
    """[len(g), E, A]: counter e·A + j, offset kNoise + g."""
    g = _g(g).reshape(-1, 1, 1)
    c = (np.arange(E, dtype=U64)[:, None] * U64(A) + np.arange(A, dtype=U64)[None, :])[None]
    return np.broadcast_arrays(c, U64(K_NOISE) + g)


def addr_env_decision(E, g):
    """[len(g), E]: counter e, offset kEnv + 2g."""
    g = _g(g).reshape(-1, 1)
    return np.broadcast_arrays(np.arange(E, dtype=U64)[None, :], U64(K_ENV) + U64(2) * g)


def addr_env_eps(E, S, g):
    """[len(g), E, S]: counter e·S + j, offset kEnv + 2g + 1."""
    g = _g(g).reshape(-1, 1, 1)
    c = (np.arange(E, dtype=U64)[:, None] * U64(S) + np.arange(S, dtype=U64)[None, :])[None]
    return np.broadcast_arrays(c, U64(K_ENV) + U64(2) * g + U64(1))


def addr_reset(n, g):
    """[len(g), n]: counter k (n = E·S for the synthetic environment, E for Pendulum), offset kReset + g."""
    g = _g(g).reshape(-1, 1)
    return np.broadcast_arrays(np.arange(n, dtype=U64)[None, :], U64(K_RESET) + g)


def addr_first_reset(n):
    return np.arange(n, dtype=U64), np.full(n, K_RESET - 1, dtype=U64)


# ------------------------------------------------------------------------------------------------
# ppo_fill_synthetic
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _fill_uniforms(n, seed):
    """The two U(−1, 1) element streams of a fill (state, fresh next_state), computed once per (n, seed)
    and shared read-only among the cases that differ only in p_terminate."""
    out = []
    for off, consumer in ((OFF_UNIFORM, FILL_STATE), (OFF_NEXT, FILL_NEXT)):
        a = uniform_pm1(philox4x32_10(np.arange(n, dtype=U64), off, fill_key(seed, consumer))[0])
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def fill_reward(N, seed, dtype=F64):
    return dtype(F32(0.1)) * normal_at(np.arange(N, dtype=U64), OFF_NORMAL, fill_key(seed, FILL_REWARD), dtype)


def fill_synthetic(E, T, S, seed, p_terminate):
    """state [N, S], term [N], trunc [N], next_state [N, S] and unlinked [N] of
    ppo_fill_synthetic(ppo, E, T, seed, p_terminate), N = E·T, row e·T + t.  All exact; the reward is
    fill_reward, the action noise sample_noise(N, A, fill_key(seed, FILL_ACTION), 0)."""
    N = E * T
    state, fresh = (a.reshape(N, S) for a in _fill_uniforms(N * S, seed))
    u = u01(philox4x32_10(np.arange(N, dtype=U64), OFF_FLAGS, fill_key(seed, FILL_FLAGS))[0])
    term = u < F32(p_terminate)                 # fp32 comparison: u01 == 1 does not terminate at p = 1
    last = (np.arange(N) % T) == T - 1
    trunc = last & ~term
    unlinked = last | term
    next_state = fresh.copy()
    link = np.nonzero(~unlinked)[0]
    next_state[link] = state[link + 1]
    return dict(state=state, term=term, trunc=trunc, next_state=next_state, unlinked=unlinked)


# ------------------------------------------------------------------------------------------------
# ppo_sample_action_device
# ------------------------------------------------------------------------------------------------
def sample_noise(m, A, seed, offset, dtype=F64, first=0):
    """ε [m, A] of rows first .. first + m − 1: counter i·A + j, the caller's offset and key."""
    idx = (np.arange(first, first + m, dtype=U64)[:, None] * U64(A) + np.arange(A, dtype=U64)[None, :])
    return normal_at(idx, offset, seed, dtype)


def sample_action(mu, log_std, eps, dtype=F64):
    """a = μ + ε·exp(log_std) with fp32 μ and log_std."""
    return mu.astype(dtype) + eps * np.exp(log_std.astype(dtype))


# ------------------------------------------------------------------------------------------------
# ppo_rollout_device, synthetic environment (kind 1)
# ------------------------------------------------------------------------------------------------
P_DONE = F32(1) / F32(500)


def synth_first_obs(E, S, seed):
    c, o = addr_first_reset(E * S)
    return uniform_pm1(philox4x32_10(c, o, reset_key(seed))[0]).reshape(E, S)


def synth_done(E, g, seed):
    """[len(g), E] terminations of global steps g: independent of observations and actions."""
    c, o = addr_env_decision(E, g)
    return u01(philox4x32_10(c, o, rollout_key(seed))[2]) < P_DONE


def synth_step(obs, action, g, seed, dtype=F64):
    """One synthetic step of every environment at each global step of g.

    obs [G, E, S], action [G, E, A] (fp32, as stored), g [G].  Returns next_obs [G, E, S] and reward
    [G, E] in `dtype`, done [G, E], and reset [G, E, S]: the exact fp32 observation an environment
    restarts from where done."""
    G, E, S = obs.shape
    A = action.shape[2]
    key = rollout_key(seed)
    c, o = addr_env_decision(E, g)
    dx, dy, dz, _ = philox4x32_10(c, o, key)
    done = u01(dz) < P_DONE
    c, o = addr_env_eps(E, S, g)
    eps = normal_at(c, o, key, dtype)
    a = action.astype(dtype)
    t = np.tanh(a)[:, :, np.arange(S) % A]
    c95, c05 = dtype(F32(0.95)), dtype(F32(0.05))
    nxt = np.clip(c95 * obs.astype(dtype) + c05 * t + c05 * eps, dtype(-1), dtype(1))
    ss = np.zeros((G, E), dtype)
    for q in range(A):                          # the device's summation order
        ss = ss + a[:, :, q] * a[:, :, q]
    reward = dtype(F32(-0.01)) * ss / dtype(A) + dtype(F32(0.1)) * np.sqrt(
        dtype(-2) * np.log(u01(dx).astype(dtype))) * np.cos((TWO_PI_F * u01(dy)).astype(dtype))
    c, o = addr_reset(E * S, g)
    reset = uniform_pm1(philox4x32_10(c, o, key)[0]).reshape(G, E, S)
    return nxt, reward, done, reset


def synth_reward_noise(E, g, seed, dtype=F64):
    """The N(0, 1) draw under the synthetic reward, [len(g), E]."""
    c, o = addr_env_decision(E, g)
    dx, dy, _, _ = philox4x32_10(c, o, rollout_key(seed))
    return box_muller(dx, dy, dtype)


def policy_noise(E, A, g, seed, dtype=F64):
    """[len(g), E, A] standard normal under the rollout's actions."""
    c, o = addr_policy_noise(E, A, g)
    return normal_at(c, o, rollout_key(seed), dtype)


# ------------------------------------------------------------------------------------------------
# ppo_rollout_device, Pendulum-v1 (kind 0)
# ------------------------------------------------------------------------------------------------
def _pendulum_from(x, y):
    theta = -PI_F + TWO_PI_F * u01(x)           # fp32, two roundings as on the device
    return theta, uniform_pm1(y)


def pendulum_first_reset(E, seed):
    c, o = addr_first_reset(E)
    x, y, _, _ = philox4x32_10(c, o, reset_key(seed))
    return _pendulum_from(x, y)


def pendulum_reset(E, g, seed):
    """(θ [len(g), E], θ̇ [len(g), E]) fp32: the time-limit reset drawn at global step g."""
    c, o = addr_reset(E, g)
    x, y, _, _ = philox4x32_10(c, o, rollout_key(seed))
    return _pendulum_from(x, y)


def pendulum_obs(theta, thetadot, dtype=F64):
    th = theta.astype(dtype)
    return np.stack([np.cos(th), np.sin(th), thetadot.astype(dtype)], -1)
