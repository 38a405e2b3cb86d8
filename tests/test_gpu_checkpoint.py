"""Training-state checkpoints on the GPU (ppo_ext.h ppo_save_state / ppo_load_state / ppo_state_hash /
ppo_state_image; DESIGN.md §4 "Training-state checkpoints"): a resumed run is the run that was interrupted.

The shared pattern: PPO X runs K = 2 rounds of (rollout, ppo_update with PPO_SHUFFLE_DEVICE, constant seed), saves,
and runs 2 more rounds, recording after each the parameter hash, the state hashes, the buffer's rows, the episode
statistics and both normalisers' states.  PPO Y = ppo_load_state of the file runs the same 2 rounds.  Everything
recorded must be equal byte for byte, and the state hashes already right after the load.  Shapes are the smallest that
exercise each piece of state.  Nothing here provokes a fault: the damaged files of the decline test are rejected by
the host-side validator before any device call.
"""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import checkpoint_ref as ck
import masked_ref as mk
import ppo_ffi
from helpers import dev, empty

pytestmark = pytest.mark.gpu
F32, U8, U32 = np.float32, np.uint8, np.uint32
GAMMA, SEED, USEED, K = 0.99, 41, 17, 2
BUF = 1                                           # PPO_CKPT_BUFFER


def make(lib, sizes, acts, cap, seed=3):
    C.CDLL("libc.so.6").srand(seed)
    return lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), cap, 3e-4, 1e-3, 0.95, 0.2, 0.01,
                          1.0, True)


def load(lib, path):
    err = C.create_string_buffer(256)
    ppo = lib.ppo_load_state(path, err, 256)
    assert ppo, err.value
    assert err.value == b"" and lib.ppo_last_error() == b""
    return ppo


def doubles(n):
    return (C.c_double * n)()


def snapshot(lib, ppo, n):
    """everything the pattern records, as raw bytes"""
    lib.ppo_synchronize()
    b = ppo.contents.buffer.contents
    S, A = b.state_size, b.action_size
    rows = [ppo_ffi.d2h(lib, p, dt, n * w).tobytes() for p, dt, w in
            ((b.d_state_p, F32, S), (b.d_action_p, F32, A), (b.d_logprob_p, F32, 1), (b.d_reward_p, F32, 1),
             (b.d_terminated_p, U8, 1), (b.d_truncated_p, U8, 1))]
    ep, obs, rew = doubles(16), doubles(1 + 2 * S), doubles(3)
    assert lib.ppo_episode_stats(ppo, ep, 16) == 16
    assert lib.ppo_obs_norm_get_state(ppo, obs, 1 + 2 * S) == 1 + 2 * S
    lib.ppo_reward_norm_get_state(ppo, rew)
    return dict(param=lib.ppo_param_hash(ppo), hash0=lib.ppo_state_hash(ppo, 0), hash1=lib.ppo_state_hash(ppo, BUF),
                limit=(b.idx, b.full), state=rows[0], action=rows[1], logprob=rows[2], reward=rows[3], terminated=rows[4],
                truncated=rows[5], episodes=bytes(ep), obs_norm=bytes(obs), rew_norm=bytes(rew))


def assert_same(x, y, what):
    for k in x:
        assert x[k] == y[k], f"{what}: {k} differs"


def resume(lib, tmp_path, ppo, one_round, n, flags=0):
    """the pattern: K rounds, save, 2 more rounds on X; load, the same 2 rounds on Y; returns (X's records, Y)"""
    for r in range(K):
        one_round(ppo, r)
    path = str(tmp_path / "state.ckpt").encode()
    assert lib.ppo_save_state(ppo, path, flags) == 0 and not os.path.exists(path + b".tmp")
    h0 = lib.ppo_state_hash(ppo, flags)
    y = load(lib, path)
    assert lib.ppo_state_hash(y, flags) == h0 != 0
    assert lib.ppo_param_hash(y) == lib.ppo_param_hash(ppo)
    return path, y, h0


# ------------------------------------------------------------------------------------------ 1. Gaussian
PEND = dict(sizes=[3, 32, 32, 1], acts=["relu", "relu", "none"], E=8, T=16, B=32)


def pendulum(lib, every_option=True, sizes=None):
    p = make(lib, sizes or PEND["sizes"], PEND["acts"], PEND["E"] * PEND["T"])
    if every_option:
        assert lib.ppo_set_obs_norm(p, 10.0) == 0 and lib.ppo_set_reward_norm(p, 10.0) == 0
        assert lib.ppo_set_max_grad_norm(p, 0.5) == 0 and lib.ppo_set_value_clip(p, 0.2) == 0
        assert lib.ppo_set_target_kl(p, float("inf")) == 0
    return p


def pendulum_round(lib):
    def one(ppo, r):
        lib.ppo_rollout_device(ppo, PEND["E"], PEND["T"], 0, SEED)
        lib.ppo_update(ppo, GAMMA, PEND["B"], 2, 2, 1, USEED)
    return one


def getters(lib, p, S):
    m, r = np.empty(S, F32), np.empty(S, F32)
    assert lib.ppo_obs_norm_affine(p, m.ctypes.data, r.ctypes.data, S) == 0
    nvec = ppo_ffi.c_ints([0] * 8)
    D = lib.ppo_get_action_nvec(p, nvec, 8)
    vals = [lib.ppo_get_max_grad_norm(p), lib.ppo_get_target_kl(p), lib.ppo_get_value_clip(p), lib.ppo_get_obs_norm(p),
            lib.ppo_get_reward_norm(p), lib.ppo_episode_gamma(p, float("nan")), lib.ppo_reward_norm_scale(p)]
    return (struct.pack("<7f", *vals), lib.ppo_get_action_dist(p), D, list(nvec)[:D], lib.ppo_get_action_mask(p),
            p.contents.V.contents.dtype, p.contents.policy.contents.mu.contents.dtype, m.tobytes(), r.tobytes())


def test_gaussian_every_option(lib, tmp_path):
    """Pendulum-v1, E = 8, T = 16, [3, 32, 32, 1] ReLU, B = 32, 2 + 2 epochs, both normalisers, gradient clipping,
    value clipping and the KL monitor on: env_state, ro_step, cont[], the return carry with rew_scanned = 1, the
    tracker and the shuffle key all cross the file."""
    n, one = PEND["E"] * PEND["T"], pendulum_round(lib)
    x = pendulum(lib)
    assert lib.ppo_episode_gamma(x, 0.97) == pytest.approx(0.99)
    _, y, _ = resume(lib, tmp_path, x, one, n)
    assert getters(lib, y, 3) == getters(lib, x, 3)
    assert lib.ppo_get_target_kl(y) == float("inf") and lib.ppo_get_max_grad_norm(y) == 0.5
    by = y.contents.buffer.contents
    assert by.idx == 0 and not by.full                      # without the flag the rows are not kept
    for r in range(K, K + 2):
        one(x, r)
        one(y, r)
        assert_same(snapshot(lib, x, n), snapshot(lib, y, n), f"round {r}")
    st = doubles(25)
    lib.ppo_read_stats(y, st, 25)
    assert st[19] > 0 and st[22] > 0                        # both normalisers really ran on Y
    assert lib.ppo_last_error() == b""
    lib.free_ppo(x)
    lib.free_ppo(y)


# --------------------------------------------------------------------------------------- 2. categorical
def test_categorical_tanh_cartpole(lib, tmp_path):
    """CartPole-v1, E = 8, T = 32, [4, 32, 2] tanh: episodes end inside the window, others stay open across the save"""
    E, T, B = 8, 32, 32
    x = make(lib, [4, 32, 2], ["tanh", "none"], E * T)
    assert lib.ppo_set_action_dist(x, 1) == 0

    def one(ppo, r):
        lib.ppo_rollout_device(ppo, E, T, 2, SEED)
        lib.ppo_update(ppo, GAMMA, B, 2, 2, 1, USEED)

    path, y, _ = resume(lib, tmp_path, x, one, E * T)
    ro = ck.parse(open(path, "rb").read())["rollout"]
    assert ro["ep_agg"][0] > 0, "no episode ended before the save"
    assert ro["cont"].any() and (ro["ep_state"][:, 3] > 0).any(), "no episode open across the save"
    assert lib.ppo_get_action_dist(y) == 1
    for r in range(K, K + 2):
        one(x, r)
        one(y, r)
        assert_same(snapshot(lib, x, E * T), snapshot(lib, y, E * T), f"round {r}")
    assert lib.ppo_last_error() == b""
    lib.free_ppo(x)
    lib.free_ppo(y)


# ------------------------------------------------------------- 3. multi-discrete, masks, the open rollout
MD = dict(S=5, nvec=[3, 2], A=5, E=4, T=8, B=8, sizes=[5, 16, 5], acts=["relu", "none"])


class Sim:
    """the caller's environment, stepped on the host from the returned actions: a contraction of the observation
    pushed by both components, episodes that terminate or truncate on per-environment counters"""

    def __init__(self):
        E, S = MD["E"], MD["S"]
        self.obs = np.random.default_rng(8).uniform(-1, 1, (E, S)).astype(F32)
        self.count = np.zeros(E, np.int64)

    def copy(self):
        s = Sim()
        s.obs, s.count = self.obs.copy(), self.count.copy()
        return s

    def step(self, act):
        E = MD["E"]
        a0, a1 = act[:, 0].astype(F32), act[:, 1].astype(F32)
        nxt = (F32(0.9) * self.obs + F32(0.1) * (a0 - F32(1))[:, None]).astype(F32)
        nxt[:, 1] += F32(0.05) * a1
        rew = (a1 - F32(0.5) * np.abs(self.obs[:, 0])).astype(F32)
        self.count += 1
        term = (self.count % 5 == 0) & (np.arange(E) % 2 == 0)
        trunc = (self.count % 7 == 0) & ~term
        after = nxt.copy()
        ended = term | trunc
        after[ended] = (F32(0.1) * (np.arange(E, dtype=F32)[:, None] + F32(1)) * np.ones(MD["S"], F32))[ended]
        self.count[ended] = 0
        self.obs = after
        return nxt, after, rew, term.astype(U8), trunc.astype(U8)


def md_ppo(lib):
    p = make(lib, MD["sizes"], MD["acts"], MD["E"] * MD["T"])
    assert lib.ppo_set_action_multidiscrete(p, ppo_ffi.c_ints(MD["nvec"]), 2) == 0
    assert lib.ppo_set_action_mask(p, 1) == 0
    return p


def open_rollout(lib, ppo, sim, r, fresh):
    """one open rollout under seeded masks; returns the actions libppo handed out, as bytes"""
    E, T, S, A = MD["E"], MD["T"], MD["S"], MD["A"]
    d_obs = dev(lib, sim.obs) if fresh else None
    assert lib.ppo_rollout_begin(ppo, E, T, d_obs.ptr if fresh else None, SEED) == 0
    d_act, d_mask = empty(lib, E * A), empty(lib, E * mk.words(A), U32)
    out, held = [], [d_act, d_mask] + ([d_obs] if fresh else [])
    for t in range(T):
        ppo_ffi.h2d(lib, d_mask.ptr, mk.pack(mk.random_masks(MD["nvec"], E, [77, r, t])))
        assert lib.ppo_rollout_act_masked(ppo, d_mask.ptr, d_act.ptr) >= 0
        lib.ppo_synchronize()
        act = d_act.to_numpy(F32, E * A).reshape(E, A)
        out.append(act.tobytes())
        arrs = [dev(lib, a) for a in sim.step(act)]
        nxt, after, rew, term, trunc = arrs
        assert lib.ppo_rollout_store(ppo, rew.ptr, nxt.ptr, term.ptr, trunc.ptr, after.ptr) == 0
        lib.ppo_synchronize()
        held += arrs
    assert lib.ppo_rollout_end(ppo) == 0
    for a in held:
        a.free()
    return b"".join(out)


def test_multidiscrete_masked_open_rollout(lib, tmp_path):
    """S = 5, nvec = {3, 2}, E = 4, T = 8, masking on, the environment stepped by the test: after the load Y continues
    with ppo_rollout_begin(…, NULL, seed) — ext_done / ext_obs crossed the file — and is handed X's actions"""
    n = MD["E"] * MD["T"]
    x, sim_x = md_ppo(lib), Sim()
    acts = {}

    def one(ppo, r, sim=None, who="x"):
        acts[who, r] = open_rollout(lib, ppo, sim or sim_x, r, fresh=(r == 0))
        lib.ppo_update(ppo, GAMMA, MD["B"], 2, 2, 1, USEED)

    path, y, _ = resume(lib, tmp_path, x, one, n)
    sim_y = sim_x.copy()                                   # the environment is the caller's object: it keeps it
    ro = ck.parse(open(path, "rb").read())["rollout"]
    assert ro["kind"] == ck.ENV_EXTERNAL and ro["ext_done"] == 1 and ro["ext_obs"].tobytes() == sim_x.obs.tobytes()
    assert lib.ppo_get_action_mask(y) == 1 and lib.ppo_get_action_dist(y) == 2
    for r in range(K, K + 2):
        one(x, r)
        one(y, r, sim_y, "y")
        assert acts["x", r] == acts["y", r], f"round {r}: actions differ"
        assert_same(snapshot(lib, x, n), snapshot(lib, y, n), f"round {r}")
        W = lib.ppo_action_mask_words(x)
        assert (ppo_ffi.d2h(lib, lib.ppo_action_mask_buffer(x), U32, n * W).tobytes()
                == ppo_ffi.d2h(lib, lib.ppo_action_mask_buffer(y), U32, n * W).tobytes())
    assert lib.ppo_last_error() == b""
    lib.free_ppo(x)
    lib.free_ppo(y)


# --------------------------------------------------------------------------------------- 4. the buffer flag
def test_buffer_flag_resumes_into_the_update(lib, tmp_path):
    """as test 1, saved between the third rollout and its update: with PPO_CKPT_BUFFER Y updates without rolling out
    and lands on X's parameters; the same save without the flag loads with an empty buffer"""
    n, one = PEND["E"] * PEND["T"], pendulum_round(lib)
    x = pendulum(lib)
    for r in range(K):
        one(x, r)
    lib.ppo_rollout_device(x, PEND["E"], PEND["T"], 0, SEED)
    with_rows, without = str(tmp_path / "rows.ckpt").encode(), str(tmp_path / "bare.ckpt").encode()
    assert lib.ppo_save_state(x, with_rows, BUF) == 0 and lib.ppo_save_state(x, without, 0) == 0
    y, z = load(lib, with_rows), load(lib, without)
    assert lib.ppo_state_hash(y, BUF) == lib.ppo_state_hash(x, BUF) != lib.ppo_state_hash(x, 0)
    assert lib.ppo_state_hash(z, 0) == lib.ppo_state_hash(x, 0)
    bz = z.contents.buffer.contents
    assert bz.idx == 0 and not bz.full
    assert ck.parse(open(without, "rb").read())["buffer"] is None
    before = snapshot(lib, x, n)
    assert_same(before, snapshot(lib, y, n), "the loaded rows")
    for p in (x, y):
        lib.ppo_update(p, GAMMA, PEND["B"], 2, 2, 1, USEED)
    after = snapshot(lib, x, n)
    assert_same(after, snapshot(lib, y, n), "after the resumed update")
    assert after["param"] != before["param"]
    # … and the run goes on identically
    one(x, K + 1)
    one(y, K + 1)
    assert_same(snapshot(lib, x, n), snapshot(lib, y, n), "the round after")
    for p in (x, y, z):
        lib.free_ppo(p)


def test_buffer_flag_keeps_the_mask_store(lib, tmp_path):
    """shapes of test 3: the loaded mask store's first limit · W words are X's"""
    n = MD["E"] * MD["T"]
    x, sim = md_ppo(lib), Sim()
    open_rollout(lib, x, sim, 0, fresh=True)
    path = str(tmp_path / "masked.ckpt").encode()
    assert lib.ppo_save_state(x, path, BUF) == 0
    y = load(lib, path)
    W = lib.ppo_action_mask_words(x)
    mx = ppo_ffi.d2h(lib, lib.ppo_action_mask_buffer(x), U32, n * W)
    my = ppo_ffi.d2h(lib, lib.ppo_action_mask_buffer(y), U32, n * W)
    assert (mx != 0xFFFFFFFF).any() and mx.tobytes() == my.tobytes()
    assert ck.parse(open(path, "rb").read())["buffer"]["mask"].tobytes() == mx.tobytes()
    for p in (x, y):
        lib.ppo_update(p, GAMMA, MD["B"], 2, 2, 1, USEED)
    assert_same(snapshot(lib, x, n), snapshot(lib, y, n), "after the resumed update")
    lib.free_ppo(x)
    lib.free_ppo(y)


# ---------------------------------------------------------------------------------- 5. image properties
def image(lib, ppo, flags):
    n = lib.ppo_state_image(ppo, flags, None, 0)
    assert n > 0
    out = C.create_string_buffer(n)
    assert lib.ppo_state_image(ppo, flags, out, n - 1) == -1
    assert lib.ppo_state_image(ppo, flags, out, n) == n
    return out.raw


def test_image_properties(lib, tmp_path):
    one = pendulum_round(lib)
    x = pendulum(lib)
    one(x, 0)
    lib.ppo_rollout_device(x, PEND["E"], PEND["T"], 0, SEED)
    for flags in (0, BUF):
        img = image(lib, x, flags)
        assert image(lib, x, flags) == img, "the image of an idle PPO changed"
        assert lib.ppo_state_hash(x, flags) == ck.fnv1a64(img)
        a, b = str(tmp_path / f"a{flags}").encode(), str(tmp_path / f"b{flags}").encode()
        assert lib.ppo_save_state(x, a, flags) == 0
        assert open(a, "rb").read() == img
        y = load(lib, a)
        assert lib.ppo_save_state(y, b, flags) == 0
        assert open(b, "rb").read() == img, "save, load, save again changed the file"
        lib.free_ppo(y)
    legacy = str(tmp_path / "legacy.bin").encode()
    lib.save_ppo(x, legacy)
    p = ck.parse(img)
    assert p["legacy"] == open(legacy, "rb").read()
    assert p["version"] == 1 and p["flags"] == ck.F_BUFFER | ck.F_ROLLOUT and p["unknown"] == []
    s = p["settings"]
    assert (s["max_grad_norm"], s["target_kl"], s["value_clip"], s["obs_clip"], s["rew_clip"]) == (
        lib.ppo_get_max_grad_norm(x), lib.ppo_get_target_kl(x), lib.ppo_get_value_clip(x), lib.ppo_get_obs_norm(x),
        lib.ppo_get_reward_norm(x))
    assert s["ep_gamma"] == lib.ppo_episode_gamma(x, float("nan")) and s["action_dist"] == 0 and s["nvec"] == []
    assert (s["mask_on"], s["dtype_V"], s["dtype_mu"], s["obs_frozen"], s["rew_frozen"]) == (0, 0, 0, 0, 0)
    obs, rew = doubles(7), doubles(3)
    assert lib.ppo_obs_norm_get_state(x, obs, 7) == 7
    lib.ppo_reward_norm_get_state(x, rew)
    assert p["normalisers"][0].tobytes() == bytes(obs) and p["normalisers"][1].tobytes() == bytes(rew)
    assert obs[0] == PEND["E"] * PEND["T"] and rew[0] > 0
    ro, bf = p["rollout"], p["buffer"]
    assert (ro["E"], ro["T"], ro["kind"], ro["step"], ro["laid"], ro["rew_scanned"]) == (8, 16, 0, 32, 1, 0)
    b = x.contents.buffer.contents
    assert bf["limit"] == 128 and bf["reward"].tobytes() == ppo_ffi.d2h(lib, b.d_reward_p, F32, 128).tobytes()
    assert p["shuffle"]["seed"] == USEED and p["shuffle"]["seeded"] == 1
    lib.free_ppo(x)


# --------------------------------------------------------------------------------------------- 6. declines
def test_declines_leave_the_process_alive(lib, tmp_path):
    one = pendulum_round(lib)
    x = pendulum(lib)
    one(x, 0)
    good = str(tmp_path / "good.ckpt").encode()
    assert lib.ppo_save_state(x, good, BUF) == 0
    img = open(good, "rb").read()
    # a save while a rollout is open, a NULL argument, an unwritable path: −1, no file
    m = md_ppo(lib)
    d_obs = dev(lib, Sim().obs)
    assert lib.ppo_rollout_begin(m, MD["E"], MD["T"], d_obs.ptr, SEED) == 0
    mid = str(tmp_path / "mid.ckpt").encode()
    assert lib.ppo_save_state(m, mid, 0) == -1 and lib.ppo_state_image(m, 0, None, 0) == -1
    assert lib.ppo_state_hash(m, 0) == 0
    assert not os.path.exists(mid) and not os.path.exists(mid + b".tmp")
    assert lib.ppo_save_state(None, mid, 0) == -1 and lib.ppo_save_state(x, None, 0) == -1
    assert lib.ppo_save_state(x, str(tmp_path / "no" / "such" / "dir.ckpt").encode(), 0) == -1
    # damaged files: NULL, a message, nothing recorded
    _, flags, secs = ck.read_image(img)
    cuts, pos = [0, 7, ck.HEADER], ck.HEADER
    for _, payload in secs:
        cuts += [pos + ck.SECTION, pos + ck.SECTION + len(payload) // 2]       # the boundary, the middle of a payload
        pos += ck.SECTION + ck.pad8(len(payload))
        cuts.append(pos)
    assert cuts.pop() == len(img)
    bad = {f"truncated to {c} bytes": img[:c] for c in cuts}
    flip = bytearray(img)
    flip[ck.HEADER + ck.SECTION + 100] ^= 0x40
    bad["one flipped payload byte"] = bytes(flip)
    bad["a wrong magic"] = b"PPOSTATS" + img[8:]
    bad["version 2"] = ck.write_image(secs, flags=flags, version=2)
    wrong = [(t, ck.pack_normalisers(np.ones(6), [1.0, 0.0, 0.0]) if t == ck.NORMALISERS else p) for t, p in secs]
    bad["an observation triple of the wrong length"] = ck.write_image(wrong, flags=flags)
    assert ck.write_image(secs, flags=flags) == img
    err = C.create_string_buffer(256)
    assert not lib.ppo_load_state(str(tmp_path / "missing.ckpt").encode(), err, 256) and err.value
    for what, data in bad.items():
        path = str(tmp_path / "bad.ckpt").encode()
        open(path, "wb").write(data)
        err = C.create_string_buffer(256)
        assert not lib.ppo_load_state(path, err, 256), what
        assert err.value.startswith(b"ppo_load_state: "), what
        assert lib.ppo_last_error() == b"", what
    assert not lib.ppo_load_state(good[:-1], None, 0)                      # no room for a message: still NULL
    # the process is alive and the GPU well: the good file loads and updates
    y = load(lib, good)
    lib.ppo_update(y, GAMMA, PEND["B"], 1, 1, 1, USEED)
    lib.ppo_update(x, GAMMA, PEND["B"], 1, 1, 1, USEED)
    lib.ppo_synchronize()
    assert lib.ppo_param_hash(x) == lib.ppo_param_hash(y) and lib.ppo_last_error() == b""
    d_obs.free()
    for p in (x, y, m):
        lib.free_ppo(p)


# ------------------------------------------------------------------------------------------------ 7. bf16
def test_bf16_mode(lib, tmp_path):
    """ppo_set_compute_dtype(ppo, 1) on a ReLU Gaussian [3, 64, 64, 1]: after save and load one more round agrees"""
    one = pendulum_round(lib)
    x = pendulum(lib, every_option=False, sizes=[3, 64, 64, 1])
    assert lib.ppo_set_compute_dtype(x, 1) == 0
    _, y, _ = resume(lib, tmp_path, x, one, PEND["E"] * PEND["T"])
    assert y.contents.V.contents.dtype == 1 and y.contents.policy.contents.mu.contents.dtype == 1
    one(x, K)
    one(y, K)
    lib.ppo_synchronize()
    assert lib.ppo_param_hash(x) == lib.ppo_param_hash(y)
    assert lib.ppo_state_hash(x, BUF) == lib.ppo_state_hash(y, BUF)
    assert lib.ppo_last_error() == b""
    lib.free_ppo(x)
    lib.free_ppo(y)
