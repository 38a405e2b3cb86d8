"""The open rollout (ppo_rollout_begin / _act / _store / _end), ppo_act_device and the built-in environments on
dense arrays (ppo_env_reset_device / ppo_env_step_device), through the C ABI.

No comparison here needs a tolerance: the counter environment's expected buffer is exact small integers
(tests/extrollout_ref.py), and the built-in environments driven from outside run the same device functions on the
same inputs as ppo_rollout_device, so every array is compared as raw bytes.  The one deliberate difference — a
terminated row on a segment end gets truncated = 0 from the store where CartPole's kernel writes 1 — is compared
as ppo_ext.h states it: `truncated` where terminated == 0, and terminated | truncated everywhere."""
import ctypes as C

import numpy as np
import pytest

import extrollout_ref as xr
import ppo_ffi
import test_gpu_rollout
from helpers import F32, dev, empty
from rewnorm_ref import chan, returns64, triple64
from test_extrollout_cpu import (PENDULUM_E, PENDULUM_ROLLOUTS, PENDULUM_T, REWNORM_GAMMA, SYNTH_E, SYNTH_ROLLOUTS,
                                 SYNTH_SEED, SYNTH_T)
from test_obsnorm_cpu import check_triple

pytestmark = pytest.mark.gpu

SEED = 21
UPDATE_SEED = 9
NSTAT = 25
ORDINARY = np.zeros(1, int)


def no_error(lib):
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


def ep_stats(lib, ppo):
    out = (C.c_double * 16)()
    assert lib.ppo_episode_stats(ppo, out, 16) == 16
    return np.array(out[:])


def read_stats(lib, ppo):
    st = (C.c_double * NSTAT)()
    lib.ppo_read_stats(ppo, st, NSTAT)
    return np.array(st[:])


def rew_state(lib, ppo):
    out = (C.c_double * 3)()
    lib.ppo_reward_norm_get_state(ppo, out)
    return np.array(out[:])


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=what)


class Arrays:
    """The dense device arrays one vectorised environment hands over per step."""

    def __init__(self, lib, E, S, A, state_floats=0):
        self.all = dict(obs=empty(lib, E * S), act=empty(lib, E * A), nxt=empty(lib, E * S), after=empty(lib, E * S),
                        rew=empty(lib, E), term=empty(lib, E, np.uint8), trunc=empty(lib, E, np.uint8),
                        es=empty(lib, max(E * state_floats, 1)))
        for k, v in self.all.items():
            setattr(self, k, v)

    def free(self):
        for v in self.all.values():
            v.free()


# ----------------------------------------------------------------------------- 1. the counter environment
def test_counter_environment(lib):
    E, T, S, A, cap = xr.E, xr.T, xr.S, xr.A, 16
    tb = xr.counter_tables()
    want, want_stats = xr.counter_expected()
    ppo = test_gpu_rollout.make(lib, [S, 8, A], cap)
    assert lib.ppo_set_reward_norm(ppo, 10.0) == 0
    lib.ppo_set_step_limit(ppo, 0, 0)
    ar = Arrays(lib, E, S, A)
    ppo_ffi.h2d(lib, ar.obs.ptr, tb["obs0"].astype(F32))
    g = REWNORM_GAMMA
    triple, carry = np.zeros(3), np.zeros(E)
    first_step = None
    for r in range(xr.ROLLOUTS):
        assert lib.ppo_rollout_begin(ppo, E, T, ar.obs.ptr if r == 0 else None, SEED) == 0
        for t in range(T):
            gs = r * T + t
            step = lib.ppo_rollout_act(ppo, ar.act.ptr)
            first_step = step if first_step is None else first_step
            assert step == first_step + gs, "one position per step, across rollouts"
            ppo_ffi.h2d(lib, ar.rew.ptr, tb["reward"][:, gs].astype(F32))
            ppo_ffi.h2d(lib, ar.nxt.ptr, tb["next_obs"][:, gs].astype(F32))
            ppo_ffi.h2d(lib, ar.after.ptr, tb["obs_after"][:, gs].astype(F32))
            ppo_ffi.h2d(lib, ar.term.ptr, tb["term"][:, gs].astype(np.uint8))
            ppo_ffi.h2d(lib, ar.trunc.ptr, tb["trunc"][:, gs].astype(np.uint8) * 7)      # any non-zero byte is set
            dense = ar.act.to_numpy(F32, E * A).reshape(E, A)
            assert lib.ppo_rollout_store(ppo, ar.rew.ptr, ar.nxt.ptr, ar.term.ptr, ar.trunc.ptr, ar.after.ptr) == 0
            rows = np.arange(E) * T + t
            b = ppo.contents.buffer.contents
            same_bits(dense, ppo_ffi.d2h(lib, b.d_action_p, F32, cap * A).reshape(cap, A)[rows], "d_action = the rows")
        assert lib.ppo_rollout_end(ppo) == 0
        lib.ppo_synchronize()
        got = test_gpu_rollout.read_buffer(lib, ppo, E * T, S, A)
        w = want[r]
        for k in ("state", "next_state", "reward", "term", "trunc"):
            same_bits(got[k], w[k], f"rollout {r}: {k}")
        assert np.isfinite(got["action"]).all() and np.isfinite(got["logprob"]).all()
        b = ppo.contents.buffer.contents
        assert (b.idx, bool(b.full)) == (E * T, False)
        same_bits(ep_stats(lib, ppo), want_stats[r], f"rollout {r}: ppo_episode_stats")
        # the carries, seen through the reward normaliser's fold of this rollout's returns
        lib.ppo_update(ppo, g, E * T // 4, 1, 1, 1, UPDATE_SEED)
        lib.ppo_synchronize()
        R, carry_out = returns64(w["reward"], w["term"], w["trunc"], g, T, carry, w["cont"])
        if r == 1:
            assert (carry != 0).any()
            Rz, _ = returns64(w["reward"], w["term"], w["trunc"], g, T, np.zeros(E), None)
            with pytest.raises(AssertionError):     # control: without the carry the fold does not match
                check_triple(rew_state(lib, ppo), chan(triple, triple64(Rz)), ORDINARY, "control")
        triple = chan(triple, triple64(R))
        check_triple(rew_state(lib, ppo), triple, ORDINARY, f"reward normaliser after rollout {r}")
        carry = carry_out
    no_error(lib)
    # obs_after omitted means next_obs: one more rollout of an environment that never resets
    assert lib.ppo_rollout_begin(ppo, E, 1, None, SEED) == 0
    assert lib.ppo_rollout_act(ppo, ar.act.ptr) == first_step + xr.G
    ppo_ffi.h2d(lib, ar.term.ptr, np.zeros(E, np.uint8))
    ppo_ffi.h2d(lib, ar.trunc.ptr, np.zeros(E, np.uint8))
    assert lib.ppo_rollout_store(ppo, ar.rew.ptr, ar.nxt.ptr, ar.term.ptr, ar.trunc.ptr, None) == 0
    assert lib.ppo_rollout_end(ppo) == 0
    assert lib.ppo_rollout_begin(ppo, E, 1, None, SEED) == 0
    lib.ppo_synchronize()
    b = ppo.contents.buffer.contents
    same_bits(ppo_ffi.d2h(lib, b.d_state_p, F32, E * S).reshape(E, S), tb["next_obs"][:, xr.G - 1].astype(F32),
              "continues from next_obs")
    no_error(lib)
    lib.ppo_set_step_limit(ppo, -1, -1)
    ar.free()
    lib.free_ppo(ppo)


# ----------------------------------------------------------------------------- 2. built-ins driven from outside
CASES = {
    "pendulum": dict(kind=0, sizes=[3, 16, 1], E=PENDULUM_E, T=PENDULUM_T, rollouts=PENDULUM_ROLLOUTS, cat=0,
                     seed=SEED),
    "pendulum-257": dict(kind=0, sizes=[3, 16, 1], E=257, T=3, rollouts=1, cat=0, seed=SEED),
    "cartpole": dict(kind=2, sizes=[4, 32, 2], E=257, T=32, rollouts=2, cat=1, seed=SEED),
    "synthetic-gaussian": dict(kind=1, sizes=[5, 16, 3], E=SYNTH_E, T=SYNTH_T, rollouts=SYNTH_ROLLOUTS, cat=0,
                               seed=SYNTH_SEED),
    "synthetic-categorical": dict(kind=1, sizes=[5, 16, 4], E=SYNTH_E, T=SYNTH_T, rollouts=SYNTH_ROLLOUTS, cat=1,
                                  seed=SYNTH_SEED),
}
# One case per kind also trains (both normalisers on, an update after each rollout) and compares ppo_param_hash.
# That comparison needs an update that is itself bit-reproducible run to run, which is a property of ppo_update, not
# of the rollout: grad_W's split-K atomics are switched off around the update (ppo_gemm_tune(-1, 1), as
# test_gpu_categorical.py does), and every Gaussian head adds its log σ gradient with one floating-point atomic per
# workgroup, so a Gaussian minibatch wider than one workgroup (synthetic: B = 600) gives log σ in the last bit or
# two differently on two runs of ppo_rollout_device alone (measured: two of four identical runs differed in log σ
# and in nothing else).  Pendulum's B = 83 is one workgroup; the categorical head writes no log σ gradient.  So
# the synthetic kind trains in its categorical case.
TRAINED = ["pendulum", "cartpole", "synthetic-categorical"]


def make_case(lib, c, train):
    ppo = test_gpu_rollout.make(lib, c["sizes"], c["E"] * c["T"])
    if c["cat"]:
        assert lib.ppo_set_action_dist(ppo, 1) == 0
    if train:
        assert lib.ppo_set_obs_norm(ppo, 10.0) == 0
        assert lib.ppo_set_reward_norm(ppo, 10.0) == 0
    return ppo


def record(lib, ppo, c, train):
    E, T, S, A = c["E"], c["T"], c["sizes"][0], c["sizes"][-1]
    lib.ppo_synchronize()
    out = test_gpu_rollout.read_buffer(lib, ppo, E * T, S, A)
    out["stats"] = ep_stats(lib, ppo)
    b = ppo.contents.buffer.contents
    out["pos"] = (b.idx, bool(b.full))
    if train:
        lib.ppo_gemm_tune(-1, 1)                # atomic-free gradient products: the update is bit-reproducible
        try:
            lib.ppo_update(ppo, 0.99, E * T // 4, 1, 1, 1, UPDATE_SEED)
        finally:
            lib.ppo_gemm_tune(-1, 0)
        out["hash"] = lib.ppo_param_hash(ppo)
    return out


def run_internal(lib, c, train):
    ppo = make_case(lib, c, train)
    recs = []
    for _ in range(c["rollouts"]):
        lib.ppo_rollout_device(ppo, c["E"], c["T"], c["kind"], c["seed"])
        recs.append(record(lib, ppo, c, train))
    no_error(lib)
    lib.free_ppo(ppo)
    return recs


def drive(lib, ppo, c, ar, first, each_step=None):
    """One external rollout of a built-in environment: begin, T × (act, the dense step at act's position, store), end."""
    E, T, S, A = c["E"], c["T"], c["sizes"][0], c["sizes"][-1]
    assert lib.ppo_rollout_begin(ppo, E, T, ar.obs.ptr if first else None, c["seed"]) == 0
    for t in range(T):
        step = lib.ppo_rollout_act(ppo, ar.act.ptr)
        assert step >= 0
        if each_step:
            each_step(t, step)
        assert lib.ppo_env_step_device(c["kind"], ar.es.ptr, ar.act.ptr, ar.nxt.ptr, ar.after.ptr, ar.rew.ptr,
                                       ar.term.ptr, ar.trunc.ptr, E, S, A, c["cat"], c["seed"], step) == 0
        assert lib.ppo_rollout_store(ppo, ar.rew.ptr, ar.nxt.ptr, ar.term.ptr, ar.trunc.ptr, ar.after.ptr) == 0
    assert lib.ppo_rollout_end(ppo) == 0


def run_external(lib, c, train):
    E, S, A = c["E"], c["sizes"][0], c["sizes"][-1]
    ppo = make_case(lib, c, train)
    nf = lib.ppo_env_state_floats(c["kind"], S)
    assert nf > 0
    ar = Arrays(lib, E, S, A, nf)
    assert lib.ppo_env_reset_device(c["kind"], ar.es.ptr, ar.obs.ptr, E, S, c["seed"]) == 0
    recs = []
    for r in range(c["rollouts"]):
        drive(lib, ppo, c, ar, r == 0)
        recs.append(record(lib, ppo, c, train))
    no_error(lib)
    ar.free()
    lib.free_ppo(ppo)
    return recs


def check_condition(name, c, recs):
    """What the case is there to meet, asserted on ppo_rollout_device's own buffers."""
    E, T = c["E"], c["T"]
    term = np.stack([r["term"].reshape(E, T) for r in recs])
    trunc = np.stack([r["trunc"].reshape(E, T) for r in recs])
    if name == "pendulum":        # every environment meets the 200-step limit once, inside a segment
        assert (trunc[:, :, :T - 1].sum(axis=(0, 2)) == 1).all() and trunc[-1, :, 199 % T].all()
    elif name == "cartpole":
        assert term[:, :, :T - 1].any() and term[:, :, T - 1].any()
    elif name.startswith("synthetic"):
        assert term.any()


@pytest.mark.parametrize("name,train", [(n, False) for n in CASES] + [(n, True) for n in TRAINED])
def test_builtin_from_outside_equals_rollout_device(lib, name, train):
    c = CASES[name]
    inner = run_internal(lib, c, train)
    outer = run_external(lib, c, train)
    if not train:
        check_condition(name, c, inner)
    for r, (a, b) in enumerate(zip(inner, outer)):
        what = f"{name} rollout {r}"
        for k in ("state", "action", "logprob", "next_state", "reward", "term"):
            same_bits(a[k], b[k], f"{what}: {k}")
        live = a["term"] == 0
        same_bits(a["trunc"][live], b["trunc"][live], f"{what}: truncated where not terminated")
        same_bits(a["term"] | a["trunc"], b["term"] | b["trunc"], f"{what}: terminated | truncated")
        same_bits(a["stats"], b["stats"], f"{what}: ppo_episode_stats")
        assert a["pos"] == b["pos"] == (0, True)
        if train:
            assert a["hash"] == b["hash"], f"{what}: ppo_param_hash after the update"
    if train:
        assert len({r["hash"] for r in inner}) == len(inner), "the updates moved the parameters"


# ----------------------------------------------------------------------------- 3. ppo_act_device
def known_obs_state(S):
    """A warmed observation normaliser: n = 100, mean 0.1·(j + 1), variance 0.25·(j + 1)."""
    j = np.arange(S) + 1.0
    return np.concatenate([[100.0], 0.1 * j, 100.0 * 0.25 * j])


@pytest.mark.parametrize("cat", [0, 1])
@pytest.mark.parametrize("norm", [0, 1])
def test_act_device_reproduces_the_rollouts_step(lib, cat, norm):
    c = dict(kind=1, sizes=[5, 16, 4 if cat else 3], E=257, T=3, cat=cat, seed=SEED)
    E, T, S, A = c["E"], c["T"], 5, c["sizes"][-1]
    ppo = make_case(lib, c, False)
    if norm:
        assert lib.ppo_set_obs_norm(ppo, 1.5) == 0
        st = known_obs_state(S)
        assert lib.ppo_obs_norm_set_state(ppo, st.ctypes.data_as(C.POINTER(C.c_double)), st.size) == 0
    ar = Arrays(lib, E, S, A, S)
    assert lib.ppo_env_reset_device(1, ar.es.ptr, ar.obs.ptr, E, S, SEED) == 0
    d_obs, d_act, d_lp = empty(lib, E * S), empty(lib, E * A), empty(lib, E)
    b = ppo.contents.buffer.contents
    seen = []

    def each_step(t, step):
        rows = np.arange(E) * T + t
        buf = test_gpu_rollout.read_buffer(lib, ppo, E * T, S, A)
        before = (lib.ppo_param_hash(ppo), read_stats(lib, ppo))
        ppo_ffi.h2d(lib, d_obs.ptr, buf["state"][rows])
        assert lib.ppo_act_device(ppo, d_obs.ptr, E, 0, SEED, step, d_act.ptr, d_lp.ptr) == 0
        lib.ppo_synchronize()
        same_bits(d_act.to_numpy(F32, E * A).reshape(E, A), buf["action"][rows], f"step {t}: action")
        same_bits(d_lp.to_numpy(F32, E), buf["logprob"][rows], f"step {t}: log-prob")
        # another position or another seed draws something else
        assert lib.ppo_act_device(ppo, d_obs.ptr, E, 0, SEED, step + 1, d_act.ptr, None) == 0
        assert (d_act.to_numpy(F32, E * A).reshape(E, A) != buf["action"][rows]).any()
        # deterministic: μ's output as it stands after the call
        assert lib.ppo_act_device(ppo, d_obs.ptr, E, 1, SEED, step, d_act.ptr, None) == 0
        lib.ppo_synchronize()
        mu = ppo_ffi.d2h(lib, ppo.contents.policy.contents.mu.contents.d_output, F32, E * A).reshape(E, A)
        act = d_act.to_numpy(F32, E * A).reshape(E, A)
        if cat:
            same_bits(act[:, 0], mu.argmax(axis=1).astype(F32), f"step {t}: argmax")      # numpy: the first maximum
            assert (act[:, 1:] == 0).all()
        else:
            same_bits(act, mu, f"step {t}: deterministic action")
        after = test_gpu_rollout.read_buffer(lib, ppo, E * T, S, A)
        for k in buf:
            same_bits(buf[k], after[k], f"step {t}: buffer {k} untouched")
        assert lib.ppo_param_hash(ppo) == before[0]
        same_bits(read_stats(lib, ppo), before[1], "ppo_read_stats untouched")
        seen.append(step)

    drive(lib, ppo, c, ar, True, each_step)
    assert seen == [0, 1, 2] and (b.idx, bool(b.full)) == (0, True)
    if norm:       # the normaliser did something: the clamp at 1.5 bites somewhere on U(−1, 1) inputs of column 0
        sh = known_obs_state(S)
        assert (np.abs((test_gpu_rollout.read_buffer(lib, ppo, E * T, S, A)["state"][:, 0] - sh[1])
                       / np.sqrt(sh[1 + S] / sh[0])) > 1.5).any()
    no_error(lib)
    for a in (d_obs, d_act, d_lp):
        a.free()
    ar.free()
    lib.free_ppo(ppo)


def test_act_device_argmax_takes_the_lowest_of_a_tie(lib):
    sizes, m = [5, 16, 4], 300
    c = dict(sizes=sizes, E=m, T=1, cat=1)
    ppo = make_case(lib, c, False)
    mu = ppo.contents.policy.contents.mu.contents
    last = mu.layers[mu.num_layers - 2]
    ppo_ffi.h2d(lib, last.d_weights, np.zeros(last.input_size * last.output_size, F32))
    ppo_ffi.h2d(lib, last.d_biases, np.array([0, 1, 1, 0], F32))         # logits (0, 1, 1, 0) on every row
    obs = np.random.default_rng(0).uniform(-1, 1, (m, 5)).astype(F32)
    d_obs, d_act = dev(lib, obs), empty(lib, m * 4)
    assert lib.ppo_act_device(ppo, d_obs.ptr, m, 1, SEED, 0, d_act.ptr, None) == 0
    lib.ppo_synchronize()
    logits = ppo_ffi.d2h(lib, mu.d_output, F32, m * 4).reshape(m, 4)
    same_bits(logits, np.tile(np.array([0, 1, 1, 0], F32), (m, 1)), "the forced logits")
    same_bits(d_act.to_numpy(F32, m * 4).reshape(m, 4), np.tile(np.array([1, 0, 0, 0], F32), (m, 1)), "lowest argmax")
    no_error(lib)
    d_obs.free()
    d_act.free()
    lib.free_ppo(ppo)


# ----------------------------------------------------------------------------- 4. sequence and argument errors
def test_errors_return_minus_one(lib):
    c = CASES["pendulum"]
    E, T, S, A = 4, 3, 3, 1
    c = dict(c, E=E, T=T)
    ppo = test_gpu_rollout.make(lib, c["sizes"], E * T)
    ar = Arrays(lib, E, S, A, 3)
    assert lib.ppo_env_reset_device(0, ar.es.ptr, ar.obs.ptr, E, S, SEED) == 0
    store = lambda after=None: lib.ppo_rollout_store(ppo, ar.rew.ptr, ar.nxt.ptr, ar.term.ptr, ar.trunc.ptr, after)
    env = lambda step: lib.ppo_env_step_device(0, ar.es.ptr, ar.act.ptr, ar.nxt.ptr, ar.after.ptr, ar.rew.ptr,
                                               ar.term.ptr, ar.trunc.ptr, E, S, A, 0, SEED, step)
    # nothing open yet
    assert lib.ppo_rollout_act(ppo, ar.act.ptr) == -1
    assert store() == -1 and lib.ppo_rollout_end(ppo) == -1
    assert lib.ppo_rollout_begin(ppo, E, T, None, SEED) == -1, "nothing to continue from"
    # capacity and shapes
    assert lib.ppo_rollout_begin(ppo, E, T + 1, ar.obs.ptr, SEED) == -1
    assert lib.ppo_rollout_begin(ppo, 0, T, ar.obs.ptr, SEED) == -1
    assert lib.ppo_rollout_begin(ppo, E, 0, ar.obs.ptr, SEED) == -1
    assert lib.ppo_rollout_begin(None, E, T, ar.obs.ptr, SEED) == -1
    # begin(NULL) after a built-in rollout
    lib.ppo_rollout_device(ppo, E, T, 0, SEED)
    assert lib.ppo_rollout_begin(ppo, E, T, None, SEED) == -1
    # an open rollout: NULL arrays, store before act, store twice, end early
    assert lib.ppo_rollout_begin(ppo, E, T, ar.obs.ptr, SEED) == 0
    assert store() == -1, "store before act"
    assert lib.ppo_rollout_act(ppo, None) == -1
    for t in range(T):
        step = lib.ppo_rollout_act(ppo, ar.act.ptr)
        assert step >= 0
        assert lib.ppo_rollout_act(ppo, ar.act.ptr) == -1, "act twice"
        assert env(step) == 0
        assert lib.ppo_rollout_store(ppo, None, ar.nxt.ptr, ar.term.ptr, ar.trunc.ptr, None) == -1
        assert lib.ppo_rollout_store(ppo, ar.rew.ptr, None, ar.term.ptr, ar.trunc.ptr, None) == -1
        assert lib.ppo_rollout_store(ppo, ar.rew.ptr, ar.nxt.ptr, None, ar.trunc.ptr, None) == -1
        assert lib.ppo_rollout_store(ppo, ar.rew.ptr, ar.nxt.ptr, ar.term.ptr, None, None) == -1
        assert store(ar.after.ptr) == 0
        assert store(ar.after.ptr) == -1, "store twice"
        if t == T - 2:
            assert lib.ppo_rollout_end(ppo) == -1, "end after T − 1 steps"
            assert lib.ppo_rollout_begin(ppo, E, T, None, SEED) == -1, "continue from an open rollout"
    assert lib.ppo_rollout_act(ppo, ar.act.ptr) == -1, "a (T + 1)-th act"
    assert lib.ppo_rollout_end(ppo) == 0
    assert lib.ppo_rollout_end(ppo) == -1
    b = ppo.contents.buffer.contents
    assert (b.idx, bool(b.full)) == (0, True)
    # continuing wants the same E
    assert lib.ppo_rollout_begin(ppo, E - 1, T, None, SEED) == -1
    assert lib.ppo_rollout_begin(ppo, E, T, None, SEED) == 0
    # a built-in rollout closes the open one; nothing continues from it
    lib.ppo_rollout_device(ppo, E, T, 0, SEED)
    assert lib.ppo_rollout_act(ppo, ar.act.ptr) == -1
    assert lib.ppo_rollout_begin(ppo, E, T, None, SEED) == -1
    # ppo_fill_synthetic closes one too
    assert lib.ppo_rollout_begin(ppo, E, T, ar.obs.ptr, SEED) == 0
    lib.ppo_fill_synthetic(ppo, E, T, 3, 0.0)
    assert lib.ppo_rollout_act(ppo, ar.act.ptr) == -1
    assert lib.ppo_rollout_begin(ppo, E, T, None, SEED) == -1
    # the stateless act and the dense environments
    assert lib.ppo_act_device(ppo, None, E, 0, SEED, 0, ar.act.ptr, None) == -1
    assert lib.ppo_act_device(ppo, ar.obs.ptr, E, 0, SEED, 0, None, None) == -1
    assert lib.ppo_act_device(ppo, ar.obs.ptr, 0, 0, SEED, 0, ar.act.ptr, None) == -1
    assert lib.ppo_act_device(None, ar.obs.ptr, E, 0, SEED, 0, ar.act.ptr, None) == -1
    assert lib.ppo_env_reset_device(0, None, ar.obs.ptr, E, S, SEED) == -1
    assert lib.ppo_env_reset_device(0, ar.es.ptr, None, E, S, SEED) == -1
    assert lib.ppo_env_reset_device(0, ar.es.ptr, ar.obs.ptr, E, 4, SEED) == -1
    assert lib.ppo_env_reset_device(7, ar.es.ptr, ar.obs.ptr, E, S, SEED) == -1
    assert lib.ppo_env_step_device(0, ar.es.ptr, None, ar.nxt.ptr, ar.after.ptr, ar.rew.ptr, ar.term.ptr,
                                   ar.trunc.ptr, E, S, A, 0, SEED, 0) == -1
    assert lib.ppo_env_step_device(0, ar.es.ptr, ar.act.ptr, ar.nxt.ptr, ar.after.ptr, ar.rew.ptr, ar.term.ptr,
                                   ar.trunc.ptr, E, S, 2, 0, SEED, 0) == -1
    assert lib.ppo_env_step_device(2, ar.es.ptr, ar.act.ptr, ar.nxt.ptr, ar.after.ptr, ar.rew.ptr, ar.term.ptr,
                                   ar.trunc.ptr, E, 4, 2, 0, SEED, 0) == -1, "CartPole takes categorical actions"
    lib.ppo_synchronize()
    no_error(lib)
    ar.free()
    lib.free_ppo(ppo)


# ----------------------------------------------------------------------------- 5. launch count
def prof_total(lib, run):
    lib.ppo_synchronize()
    lib.ppo_prof_enable(1)
    lib.ppo_prof_reset()
    try:
        run()
        lib.ppo_synchronize()
        cnt = (C.c_long * 7)()
        lib.ppo_prof_counts(cnt)
    finally:
        lib.ppo_prof_enable(0)
    return sum(cnt)


def test_launch_count(lib):
    """The open loop adds, per step, the dense copy of the actions and the store in place of the built-in
    environment kernel: at most 2·T launches over ppo_rollout_device, plus begin's (the copy of d_obs0, the first
    rows, the carry, the row map: 4 at the most) — end adds none over the internal tail."""
    c = dict(CASES["pendulum"], E=64, T=16)
    E, T = c["E"], c["T"]
    inner = test_gpu_rollout.make(lib, c["sizes"], E * T)
    n_in = prof_total(lib, lambda: lib.ppo_rollout_device(inner, E, T, 0, SEED))
    outer = test_gpu_rollout.make(lib, c["sizes"], E * T)
    ar = Arrays(lib, E, 3, 1, 3)
    assert lib.ppo_env_reset_device(0, ar.es.ptr, ar.obs.ptr, E, 3, SEED) == 0
    n_out = prof_total(lib, lambda: drive(lib, outer, c, ar, True)) - T       # the T dense environment launches
    print(f"launches: ppo_rollout_device {n_in}, open rollout without its environment {n_out}, T = {T}")
    assert n_in >= 3 * T
    assert n_out <= n_in + 2 * T + 4
    no_error(lib)
    ar.free()
    lib.free_ppo(inner)
    lib.free_ppo(outer)
