"""Learning-rate schedules on the GPU (ppo_set_lr_schedule, csrc/kl.hip decide(), csrc/adam.hip's kernels over RateWord;
DESIGN.md §4 "Learning-rate schedules").

Everything here is bit for bit.  The adaptive rule is replayed from the update's own ppo_kl_history through the fp32
numpy model (tests/lr_schedule_ref.py); the Adam kernels' pointer variants are compared with the by-value kernels on
identical inputs; whole updates are compared with updates of a PPO whose rate was set by hand.  Where a PPO under the
adaptive schedule is compared with one under the constant schedule, the latter runs the KL monitor
(ppo_set_target_kl(+inf)), so that both take the multi-launch loop — the schedule's documented path.

Shapes: [3, 64, 64, 1], capacity 512, B = 128 (four minibatches per epoch), 2 + 2 epochs, device shuffle, synthetic
fill.  lr_policy = 3e-3 (test_gpu_kl.py's, so that the KL moves visibly within 8 steps), lr_V = 1e-3.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import lr_schedule_ref as lr
import ppo_ffi
from test_gpu_adam import EDGE, TensorList, align4, normal_grads
from test_gpu_update import make_ppo

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, N, B = [3, 64, 64, 1], 512, 128
NB = N // B
NPE = NVE = 2
STEPS = NPE * NB
LR_P, LR_V, LO, HI = F32(3e-3), F32(1e-3), F32(1e-5), F32(1e-2)
SEED, INF = 4321, float("inf")


def set_schedule(lib, ppo, kind, p0, p1, p2):
    return lib.ppo_set_lr_schedule(ppo, int(kind), float(p0), float(p1), float(p2))


def fresh(lib, oracle, sizes=SIZES, cap=N, fill=True):
    ppo = make_ppo(lib, oracle, sizes, cap, seed=1234, init_std=0.7, ent_coeff=0.01)
    ppo.contents.lr_policy = float(LR_P)
    ppo.contents.lr_V = float(LR_V)
    if fill:
        lib.ppo_fill_synthetic(ppo, 4, cap // 4, 99, 1.0 / 500)
    lib.ppo_synchronize()
    return ppo


def update(lib, ppo, batch=B):
    lib.ppo_update(ppo, 0.99, batch, NPE, NVE, 1, SEED)
    lib.ppo_synchronize()
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


def stats(lib, ppo):
    st = (C.c_double * 29)()
    lib.ppo_read_stats(ppo, st, 29)
    return list(st)


def kl_hist(lib, ppo):
    h = (C.c_double * 64)()
    n = lib.ppo_kl_history(ppo, h, 64)
    out = np.array(h[:n]).astype(F32)
    assert (out.astype(np.float64) == np.array(h[:n])).all()          # the history holds fp32 values
    return out


def lr_hist(lib, ppo):
    h = (C.c_float * 64)()
    n = lib.ppo_lr_history(ppo, h, 64)
    return np.array(h[:n], F32)


def get_lr(lib, ppo):
    out = (C.c_double * 2)()
    assert lib.ppo_get_lr(ppo, out) == 0
    return F32(out[0]), F32(out[1])


def get_schedule(lib, ppo):
    out = (C.c_float * 4)()
    return lib.ppo_get_lr_schedule(ppo, out), list(out)


def nets(lib, ppo):
    """the raw parameter bytes: (μ, log σ), V"""
    c = ppo.contents
    pol = c.policy.contents
    mu, V = pol.mu.contents, c.V.contents
    p = ppo_ffi.d2h(lib, mu.d_params, F32, mu.num_params).tobytes() + \
        ppo_ffi.d2h(lib, pol.d_log_std, F32, pol.action_size).tobytes()
    return p, ppo_ffi.d2h(lib, V.d_params, F32, V.num_params).tobytes()


def assert_replays(lib, ppo, lr0, desired, stop_step=-1, what=""):
    """ppo_lr_history, ppo_get_lr and out[25], out[27], out[28] against the model's replay of ppo_kl_history"""
    kls, got = kl_hist(lib, ppo), lr_hist(lib, ppo)
    want, last, up, down = lr.replay(lr0, kls, desired, LO, HI, stop_step)
    st = stats(lib, ppo)
    print(f"{what}: kl {' '.join(f'{k:.3e}' for k in kls)}\n{what}: lr {' '.join(f'{x:.4e}' for x in got)}; "
          f"raised {st[27]:.0f} lowered {st[28]:.0f}")
    assert len(kls) == len(got) > 0
    assert got.tobytes() == want.tobytes(), f"{what}: lr history {got} != model {want}"
    assert get_lr(lib, ppo)[0].tobytes() == last.tobytes() and F32(st[25]).tobytes() == last.tobytes()
    assert st[25] == float(last) and (st[27], st[28]) == (up, down)
    return kls, got, last, up, down


# ----------------------------------------------------------------------------- 0. the setter
def test_setter_return_codes(lib, oracle):
    ppo = fresh(lib, oracle, fill=False)
    nan = float("nan")
    assert get_schedule(lib, ppo) == (lr.CONSTANT, [0.0] * 4)
    assert set_schedule(lib, ppo, lr.ADAPTIVE, 0.01, LO, HI) == 0
    want = (lr.ADAPTIVE, [F32(0.01), LO, HI, 0.0])
    assert get_schedule(lib, ppo) == want and get_lr(lib, ppo) == (LR_P, LR_V)
    bad = [(3, 1.0, 1.0, 1.0), (-1, 1.0, 1.0, 1.0),
           (lr.CONSTANT, nan, 0, 0), (lr.LINEAR, 4, nan, 0), (lr.ADAPTIVE, 0.01, 1e-5, nan),
           (lr.LINEAR, 0.5, 0.1, 0), (lr.LINEAR, 0, 0.1, 0), (lr.LINEAR, INF, 0.1, 0), (lr.LINEAR, 4, -0.1, 0),
           (lr.LINEAR, 4, 1.5, 0),
           (lr.ADAPTIVE, 0.0, 1e-5, 1e-2), (lr.ADAPTIVE, -1.0, 1e-5, 1e-2), (lr.ADAPTIVE, INF, 1e-5, 1e-2),
           (lr.ADAPTIVE, 0.01, 0.0, 1e-2), (lr.ADAPTIVE, 0.01, 1e-2, 1e-5), (lr.ADAPTIVE, 0.01, 1e-5, INF),
           (lr.ADAPTIVE, 0.01, INF, INF)]
    for args in bad:
        assert set_schedule(lib, ppo, *args) == -1, args
        assert get_schedule(lib, ppo) == want, args                   # the setting is unchanged
    assert lib.ppo_lr_couple_value(ppo, 1) == 0 and lib.ppo_lr_couple_value(ppo, 0) == 1
    assert set_schedule(lib, ppo, lr.ADAPTIVE, 0.01, 5e-3, 5e-3) == 0           # lr_max == lr_min is a range
    assert get_lr(lib, ppo)[0] == F32(5e-3)                                           # clamp(3e-3, 5e-3, 5e-3)
    assert ppo.contents.lr_policy == LR_P                                             # the base is never written
    assert set_schedule(lib, ppo, lr.LINEAR, 4, 0.1, 123.0) == 0
    assert get_schedule(lib, ppo) == (lr.LINEAR, [4.0, F32(0.1), 0.0, 0.0])
    assert lib.ppo_lr_history(ppo, None, 0) == 0
    assert set_schedule(lib, ppo, lr.CONSTANT, 1, 2, 3) == 0
    assert get_schedule(lib, ppo) == (lr.CONSTANT, [0.0] * 4) and get_lr(lib, ppo) == (LR_P, LR_V)
    lib.free_ppo(ppo)


# ----------------------------------------------------------------------------- 1. Adam through the pointer
RATES = [F32(3e-4), F32(1e-5) * F32(1.5) * F32(1.5) * F32(1.5)]
LAYOUTS = {"flat": lambda n: ([n], "separate", 0, 1), "flat-unaligned": lambda n: ([n], "separate", 1, 1),
           "gapped": lambda n: ([n, 5, n], ("gaps", (4, 5, 9)), 0, 0)}


def grads_with_edges(rng, n):
    """test_gpu_adam's regime: ±10^U(−12, 6) with exact zeros, and the EDGE values (zeros, subnormals, ±inf, NaN)
    at seeded positions"""
    g = normal_grads(rng, n)
    k = min(n, len(EDGE))
    g[rng.choice(n, k, replace=False)] = rng.permutation(EDGE)[:k]
    return g


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1023, 4099])
def test_adam_pointer_equals_by_value(lib, n, layout):
    """adam_update_cuda(adam, r) against ppo_adam_update_lr_device(adam, &r) on identical copies: p (the whole
    allocations, sentinels included), m and v byte for byte after each of 3 steps; the vectorised span kernel, the
    scalar one (an unaligned span) and the multi-tensor kernel (a list with gaps)."""
    lengths, lay, lead, flat = LAYOUTS[layout](n)
    for rate in RATES:
        rng = np.random.default_rng([n, len(lengths), int(rate.view(np.uint32))])
        d_rate = ppo_ffi.DeviceArray.from_numpy(lib, np.array([rate], F32))
        tls = [TensorList(lib, lengths, lay, lead=lead) for _ in range(2)]
        p0 = rng.uniform(-1, 1, tls[0].size).astype(F32)
        adams = []
        for tl in tls:
            tl.set_params(p0, upload=True)
            adams.append(lib.create_adam_cuda(*tl.args(), tl.n, tl.size, 0.9, 0.999))
        try:
            assert adams[0].contents.flat == flat and adams[1].contents.flat == flat
            for step in range(3):
                g = grads_with_edges(rng, tls[0].size)
                for tl in tls:
                    tl.set_grads(g)
                lib.adam_update_cuda(adams[0], float(rate))
                assert lib.ppo_adam_update_lr_device(adams[1], d_rate.ptr) == 0
                lib.ppo_synchronize()
                for a, b in zip(tls[0].dp, tls[1].dp):
                    assert a.to_numpy(np.uint8, a.nbytes).tobytes() == b.to_numpy(np.uint8, b.nbytes).tobytes(), \
                        f"p differs at step {step + 1}"
                span = align4(adams[0].contents.span)
                for name in ("m", "v"):
                    x, y = (ppo_ffi.d2h(lib, getattr(ad.contents, name), F32, span).tobytes() for ad in adams)
                    assert x == y, f"{name} differs at step {step + 1}"
                assert adams[0].contents.time_step == adams[1].contents.time_step == step + 1
            if n >= 15:                                                # the steps were taken (n = 1 may draw g = 0 thrice)
                moved = tls[0].dp[0].to_numpy(F32, tls[0].pb[0].size)
                assert (moved != tls[0].pb[0]).any()
        finally:
            for ad in adams:
                lib.free_adam_cuda(ad)
            for tl in tls:
                tl.free()
            d_rate.free()
    assert lib.ppo_adam_update_lr_device(None, None) == -1


# ----------------------------------------------------------------------------- 2. schedule off is the parent's path
def test_constant_schedule_is_the_untouched_path(lib, oracle):
    a, b = fresh(lib, oracle), fresh(lib, oracle)
    assert set_schedule(lib, b, lr.CONSTANT, 0, 0, 0) == 0
    for _ in range(2):
        update(lib, a)
        update(lib, b)
    assert lib.ppo_param_hash(a) == lib.ppo_param_hash(b)
    assert lib.ppo_state_hash(a, 0) == lib.ppo_state_hash(b, 0) != 0
    sa, sb = stats(lib, a), stats(lib, b)
    assert sa[25:29] == sb[25:29] == [float(LR_P), float(LR_V), 0.0, 0.0]
    assert sa[13:17] == [0.0] * 4 and lib.ppo_lr_history(a, None, 0) == 0          # no monitor, no history
    lib.free_ppo(a)
    lib.free_ppo(b)


# ----------------------------------------------------------------------------- 3. the rule, replayed
@pytest.fixture(scope="module")
def measured(lib, oracle):
    """a measure-only run (constant schedule, KL monitor): its KL history, and its networks after the update"""
    ppo = fresh(lib, oracle)
    assert lib.ppo_set_target_kl(ppo, INF) == 0
    update(lib, ppo)
    out = dict(kl=kl_hist(lib, ppo), nets=nets(lib, ppo))
    lib.free_ppo(ppo)
    assert len(out["kl"]) == STEPS
    return out


@pytest.mark.parametrize("case", ["always-lower", "always-raise", "median"])
def test_rule_replayed(lib, oracle, measured, case):
    desired = {"always-lower": 1e-12, "always-raise": 1e3, "median": float(np.median(measured["kl"]))}[case]
    ppo = fresh(lib, oracle)
    assert set_schedule(lib, ppo, lr.ADAPTIVE, desired, LO, HI) == 0
    assert get_lr(lib, ppo) == (LR_P, LR_V)
    lib.ppo_reset_stats(ppo)
    update(lib, ppo)
    kls, got, last, up, down = assert_replays(lib, ppo, LR_P, desired, what=case)
    st = stats(lib, ppo)
    assert len(got) == STEPS == st[3] and st[15] == STEPS and st[16] == -1          # the monitor ran, nothing stopped
    assert st[26] == float(LR_V) and ppo.contents.lr_policy == LR_P
    if case == "always-lower":
        # step 0 sees the parameters that sampled the buffer: its kl is rounding noise (≈ 1e-13) and may sit under
        # the band; every later step lowers
        assert (kls[1:] > 2e-12).all() and down >= STEPS - 1 and up <= 1 and last < LR_P
    elif case == "always-raise":
        assert down == 0 and up == int((kls > 0).sum()) >= STEPS - 1 and last == HI           # 3e-3 · 1.5³ > 1e-2
    else:
        assert up >= 1 and down >= 1, f"the median case is vacuous: raised {up}, lowered {down}"
    lib.ppo_reset_stats(ppo)
    assert stats(lib, ppo)[27:29] == [0.0, 0.0] and get_lr(lib, ppo)[0] == last     # counters cleared, the rate stays
    lib.free_ppo(ppo)


@pytest.mark.parametrize("desired", [1e-20, 1e3])
def test_adapted_rate_is_the_one_adam_used(lib, oracle, desired):
    """one policy step (and one value step) under the schedule against a PPO whose lr_policy was set by hand to the
    first step's adapted rate: the pair kernel's pointer variant read the word decide() had just written"""
    a, b = fresh(lib, oracle), fresh(lib, oracle)
    assert set_schedule(lib, a, lr.ADAPTIVE, desired, LO, HI) == 0
    lib.ppo_set_step_limit(a, 1, 1)
    update(lib, a)
    rate = lr_hist(lib, a)
    assert len(rate) == 1 and rate[0] != LR_P and rate[0] == get_lr(lib, a)[0]
    assert lib.ppo_set_target_kl(b, INF) == 0
    b.contents.lr_policy = float(rate[0])
    lib.ppo_set_step_limit(b, 1, 1)
    update(lib, b)
    assert nets(lib, a) == nets(lib, b)
    c = fresh(lib, oracle)                                             # … and the base rate gives other parameters
    assert lib.ppo_set_target_kl(c, INF) == 0
    lib.ppo_set_step_limit(c, 1, 1)
    update(lib, c)
    assert nets(lib, c)[0] != nets(lib, a)[0] and nets(lib, c)[1] == nets(lib, a)[1]
    for p in (a, b, c):
        lib.free_ppo(p)


# ----------------------------------------------------------------------------- 4. coupling
def test_value_rate_coupling(lib, oracle, measured):
    desired = 1e-12                                                    # every step lowers: the rate moves for sure
    x, y, z = fresh(lib, oracle), fresh(lib, oracle), fresh(lib, oracle)
    for p in (x, y):
        assert set_schedule(lib, p, lr.ADAPTIVE, desired, LO, HI) == 0
    assert lib.ppo_lr_couple_value(x, 1) == 0
    assert get_schedule(lib, x)[1][3] == 1.0
    assert lib.ppo_set_target_kl(z, INF) == 0                          # the constant schedule on the same loop
    for p in (x, y, z):
        update(lib, p)
    # update 1: the ratio is exactly 1
    assert stats(lib, x)[26] == float(LR_V) == stats(lib, y)[26]
    assert nets(lib, x) == nets(lib, y)
    # coupling off: the value network is the constant schedule's, bit for bit (the policy's is not: its rate moved)
    assert nets(lib, y)[1] == nets(lib, z)[1] == measured["nets"][1] and nets(lib, y)[0] != nets(lib, z)[0]
    rate1 = get_lr(lib, x)[0]
    assert rate1 < LR_P
    want = lr.coupled_value_lr(LR_V, rate1, LR_P, LO, HI)
    assert want != LR_V
    y.contents.lr_V = float(want)                                             # by hand, by value
    update(lib, x)
    update(lib, y)
    st = stats(lib, x)
    assert F32(st[26]).tobytes() == want.tobytes() and st[26] == float(want) and get_lr(lib, x)[1] == want
    assert nets(lib, x) == nets(lib, y)
    assert x.contents.lr_V == LR_V
    for p in (x, y, z):
        lib.free_ppo(p)


# ----------------------------------------------------------------------------- 5. with the target-KL stop
def test_with_target_kl_stop(lib, oracle):
    """desired_kl = 1e3 raises at every step, so the KL grows; a finite target between an interior step's KL and
    everything before it stops the update there.  The stop step still adapts (the rule runs ahead of the stop test),
    every later step leaves the rate alone; out[15] / out[16] keep their meaning."""
    a = fresh(lib, oracle)
    assert set_schedule(lib, a, lr.ADAPTIVE, 1e3, LO, HI) == 0
    update(lib, a)
    kls = kl_hist(lib, a)
    lib.free_ppo(a)
    cand = [s for s in range(1, STEPS) if s % NB not in (0, NB - 1) and kls[s] > 1.2 * kls[:s].max() > 0]
    assert cand, f"no interior step rises 20 % above its predecessors: {kls}"
    s = cand[0]
    target = float(np.sqrt(float(kls[:s].max()) * float(kls[s]))) / 1.5
    b = fresh(lib, oracle)
    assert set_schedule(lib, b, lr.ADAPTIVE, 1e3, LO, HI) == 0 and lib.ppo_set_target_kl(b, target) == 0
    lib.ppo_reset_stats(b)
    update(lib, b)
    st = stats(lib, b)
    issued = (s // NB + 1) * NB
    assert st[16] == s and st[15] == s and st[3] == issued
    _, got, last, _, _ = assert_replays(lib, b, LR_P, 1e3, stop_step=s, what=f"stop at {s}")
    assert len(got) == issued and (got[s:] == got[s]).all() and last == got[s]
    assert (kl_hist(lib, b)[:s + 1] == kls[:s + 1]).all()
    ap = b.contents.adam_policy.contents
    assert ap.time_step == s == b.contents.adam_entropy.contents.time_step
    lib.free_ppo(b)


def test_pointer_pair_with_clip_and_stop(lib, oracle):
    """The pair kernel with both rates through device words, a clip coefficient and the stop word together, against the
    by-value pair kernel byte for byte over a whole update that stops part-way.  The adaptive range is the single rate
    R (lr_min == lr_max), so decide() writes R at every step and a PPO on the constant schedule with lr_policy = R set
    by hand takes the same steps: the steps before the stop scale their gradients by the step's coefficient, the stop
    step and those behind it only clear them.  The value rate is coupled, so the value Adam (the vector kernel, with
    its own coefficient) reads lr_V · (R / R) from its word.  Parameters, log σ, and m, v and the step count of all
    three Adams."""
    R, NORM = F32(5e-3), 1e-2

    def run(adaptive, target):
        ppo = fresh(lib, oracle)
        if adaptive:
            assert set_schedule(lib, ppo, lr.ADAPTIVE, 0.01, R, R) == 0 and get_lr(lib, ppo)[0] == R
            assert lib.ppo_lr_couple_value(ppo, 1) == 0              # lr_v = lr_V · (R / R): the value Adam's word
        else:
            ppo.contents.lr_policy = float(R)
        assert lib.ppo_set_max_grad_norm(ppo, NORM) == 0 and lib.ppo_set_target_kl(ppo, target) == 0
        lib.ppo_reset_stats(ppo)
        update(lib, ppo)
        c = ppo.contents
        out = dict(nets=nets(lib, ppo), kl=kl_hist(lib, ppo), lr=lr_hist(lib, ppo), st=stats(lib, ppo))
        for k, ad in (("V", c.adam_V), ("mu", c.adam_policy), ("ls", c.adam_entropy)):
            a = ad.contents
            out[k] = (a.time_step, ppo_ffi.d2h(lib, a.m, F32, a.span).tobytes(),
                      ppo_ffi.d2h(lib, a.v, F32, a.span).tobytes())
        lib.free_ppo(ppo)
        return out

    kls = run(False, INF)["kl"]
    assert len(kls) == STEPS
    # a step that stops the update with at least one issued step behind it: its KL stands clear of all before it
    cand = [s for s in range(1, STEPS) if s % NB != NB - 1 and kls[s] > 1.2 * max(float(kls[:s].max()), 1e-12)]
    assert cand, f"no step rises 20 % above its predecessors: {kls}"
    s = cand[-1]
    target = float(np.sqrt(max(float(kls[:s].max()), 1e-12) * float(kls[s]))) / 1.5
    a, b = run(True, target), run(False, target)
    print(f"stop at {s} of {STEPS}, target {target:.3e}; clipped value / policy steps {b['st'][11]:.0f} / "
          f"{b['st'][12]:.0f}, last norms {b['st'][9]:.3e} / {b['st'][10]:.3e}; kl {kls}")
    for r in (a, b):
        assert r["st"][16] == s and r["st"][15] == s and r["st"][3] == (s // NB + 1) * NB > s + 1
        assert r["st"][12] >= s and r["st"][11] >= 1           # every policy step that ran was clipped (coef < 1)
        assert r["st"][26] == float(LR_V) and r["V"][0] == NVE * NB
        assert r["mu"][0] == s == r["ls"][0] and (r["kl"][:s + 1] == kls[:s + 1]).all()
    assert len(a["lr"]) == a["st"][3] and (a["lr"] == R).all() and len(b["lr"]) == 0
    for k in ("nets", "V", "mu", "ls"):
        assert a[k] == b[k], f"{k} differs between the device-word and the by-value update"


# ----------------------------------------------------------------------------- 6. linear
def test_linear_decay(lib, oracle):
    n_updates, f = 4, 0.1
    a, b = fresh(lib, oracle), fresh(lib, oracle)
    assert set_schedule(lib, a, lr.LINEAR, n_updates, f, 0) == 0
    after = []
    for u in range(5):
        want = (lr.linear_lr(LR_P, u, n_updates, f), lr.linear_lr(LR_V, u, n_updates, f))
        got = get_lr(lib, a)
        st = stats(lib, a)
        print(f"update {u}: policy {got[0]:.9g} value {got[1]:.9g}")
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert (st[25], st[26]) == (float(want[0]), float(want[1]))
        update(lib, a)
        after.append(lib.ppo_param_hash(a))
    assert get_lr(lib, a) == (F32(float(LR_P) * float(F32(f))), F32(float(LR_V) * float(F32(f))))     # u = 5 > N
    assert a.contents.lr_policy == LR_P and a.contents.lr_V == LR_V and stats(lib, a)[13:17] == [0.0] * 4
    update(lib, b)                                                     # update 0 runs at the base rates
    assert lib.ppo_param_hash(b) == after[0]
    b.contents.lr_policy = float(lr.linear_lr(LR_P, 1, n_updates, f))
    b.contents.lr_V = float(lr.linear_lr(LR_V, 1, n_updates, f))
    update(lib, b)
    assert lib.ppo_param_hash(b) == after[1]
    c = fresh(lib, oracle)                                             # … which the base rates do not give
    update(lib, c)
    update(lib, c)
    assert lib.ppo_param_hash(c) != after[1]
    for p in (a, b, c):
        lib.free_ppo(p)


# ----------------------------------------------------------------------------- 7. data-parallel loopback
DP_CHILD = """
    import ctypes as C, json, sys
    sys.path.insert(0, {pkg!r})
    import ppo_ffi
    lib = ppo_ffi.load()
    assert lib.ppo_set_device(0) == 0
    assert lib.ppo_comm_init(0, 1, None) == 0 and lib.ppo_comm_world() == 2
    C.CDLL("libc.so.6").srand(1234)
    sizes = {sizes!r}
    ppo = lib.create_ppo(ppo_ffi.c_strings(["relu", "relu", "none"]), ppo_ffi.c_ints(sizes), 4, {cap}, {lr_p!r}, {lr_v!r},
                         0.95, 0.2, 0.01, 0.7, True)
    lib.ppo_fill_synthetic(ppo, 4, {cap} // 4, 99, 1.0 / 500)
    assert lib.ppo_set_lr_schedule(ppo, 2, {desired!r}, {lo!r}, {hi!r}) == 0
    assert lib.ppo_lr_couple_value(ppo, 1) == 0
    h0 = lib.ppo_param_hash(ppo)
    lib.ppo_update(ppo, 0.99, {batch}, 2, 2, 1, {seed})            # the replica check runs behind it (PPO_REPLICA_CHECK=1)
    lib.ppo_synchronize()
    kl, rate, st, now = (C.c_double * 64)(), (C.c_float * 64)(), (C.c_double * 29)(), (C.c_double * 2)()
    n, m = lib.ppo_kl_history(ppo, kl, 64), lib.ppo_lr_history(ppo, rate, 64)
    lib.ppo_read_stats(ppo, st, 29)
    lib.ppo_get_lr(ppo, now)
    h1 = lib.ppo_param_hash(ppo)
    same = lib.ppo_comm_check_replicas(ppo)
    peer = (C.c_ulonglong * 1)(h1 ^ 1)                              # a peer whose rate word (or anything) differs
    assert lib.ppo_comm_loopback_peer_hash(peer, 1) == 0
    differs = lib.ppo_comm_check_replicas(ppo)
    lib.ppo_clear_error()
    lib.ppo_comm_loopback_clear()
    print("RESULT " + json.dumps(dict(kl=list(kl[:n]), lr=[float(x) for x in rate[:m]], st=list(st), now=list(now),
                                      same=same, differs=differs, moved=h0 != h1, err=(lib.ppo_last_error() or b"").decode())))
    lib.ppo_comm_finalize()
"""


def test_data_parallel_loopback(lib, measured, tmp_path):
    """two identical in-process ranks in a fresh child process: decide() runs in kl_decide_kernel on the all-reduced
    sums (2m rows), the rate history replays from that rank's KL history, and the replica check — which covers the
    rate words while the schedule is on — passes"""
    desired = float(np.median(measured["kl"]))
    script = tmp_path / "dp_lr.py"
    script.write_text(textwrap.dedent(DP_CHILD.format(pkg=os.path.join(ROOT, "ppo.c_amd"), sizes=SIZES, cap=N, batch=B,
                                                      lr_p=float(LR_P), lr_v=float(LR_V), desired=desired, lo=float(LO),
                                                      hi=float(HI), seed=SEED)))
    env = dict(os.environ, PPO_COMM_LOOPBACK="2", PPO_REPLICA_CHECK="1")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    kls, got = np.array(out["kl"]).astype(F32), np.array(out["lr"], F32)
    want, last, up, down = lr.replay(LR_P, kls, desired, LO, HI)
    print(f"loopback: kl {kls}\nloopback: lr {got}; raised {up} lowered {down}")
    assert len(got) == STEPS and got.tobytes() == want.tobytes()
    assert up + down >= 1 and (out["st"][27], out["st"][28]) == (up, down)
    assert F32(out["now"][0]).tobytes() == last.tobytes() and out["st"][26] == float(LR_V)
    assert out["same"] == 0 and out["differs"] == -1 and out["moved"] and out["err"] == ""
    # the mean runs over the global minibatch (doubled sums over 2m rows): step 0, before any rate has acted, is the
    # one-rank run's
    one = measured["kl"]
    assert abs(float(kls[0]) - float(one[0])) <= 1e-3 * float(one[0])


# ----------------------------------------------------------------------------- 8. checkpoint
def test_checkpoint_resumes_the_schedule(lib, oracle, tmp_path):
    E, T = 8, N // 8

    def one(p):
        lib.ppo_rollout_device(p, E, T, 0, 41)
        update(lib, p)

    x = fresh(lib, oracle, fill=False)
    off = lib.ppo_state_image(x, 0, None, 0)
    assert set_schedule(lib, x, lr.ADAPTIVE, 1e-4, LO, HI) == 0 and lib.ppo_lr_couple_value(x, 1) == 0
    assert lib.ppo_state_image(x, 0, None, 0) == off + 24 + 48         # one more section: header + 48 bytes
    one(x)
    one(x)
    path = str(tmp_path / "lr.ckpt").encode()
    assert lib.ppo_save_state(x, path, 0) == 0
    err = C.create_string_buffer(256)
    y = lib.ppo_load_state(path, err, 256)
    assert y, err.value
    assert lib.ppo_state_hash(y, 0) == lib.ppo_state_hash(x, 0) != 0
    assert get_schedule(lib, y) == get_schedule(lib, x) == (lr.ADAPTIVE, [F32(1e-4), LO, HI, 1.0])
    assert get_lr(lib, y) == get_lr(lib, x) and get_lr(lib, x)[0] != LR_P
    assert stats(lib, y)[27:29] == stats(lib, x)[27:29] != [0.0, 0.0]
    one(x)
    one(y)
    assert lib.ppo_state_hash(y, 0) == lib.ppo_state_hash(x, 0)
    assert get_lr(lib, y) == get_lr(lib, x) and lr_hist(lib, x).tobytes() == lr_hist(lib, y).tobytes()
    assert nets(lib, x) == nets(lib, y)
    # a damaged schedule section is declined by the validator, before anything is allocated
    img = bytearray(open(path, "rb").read())
    img[-40] ^= 0x01
    bad = str(tmp_path / "bad.ckpt").encode()
    open(bad, "wb").write(bytes(img))
    assert not lib.ppo_load_state(bad, err, 256) and b"section 7" in err.value
    # the linear schedule keeps its update counter
    z = fresh(lib, oracle, fill=False)
    assert set_schedule(lib, z, lr.LINEAR, 4, 0.1, 0) == 0
    one(z)
    assert lib.ppo_save_state(z, path, 0) == 0
    w = lib.ppo_load_state(path, err, 256)
    assert w, err.value
    assert get_lr(lib, w) == get_lr(lib, z) == (lr.linear_lr(LR_P, 1, 4, 0.1), lr.linear_lr(LR_V, 1, 4, 0.1))
    assert lib.ppo_state_hash(w, 0) == lib.ppo_state_hash(z, 0)
    for p in (x, y, z, w):
        lib.free_ppo(p)


# ----------------------------------------------------------------------------- 9. categorical policy
def test_categorical_policy(lib, oracle):
    E, T, cap, batch = 8, 32, 256, 64
    runs = {}
    for desired in (INF, None):
        ppo = make_ppo(lib, oracle, [4, 32, 2], cap, seed=1234)
        ppo.contents.lr_policy = float(LR_P)
        assert lib.ppo_set_action_dist(ppo, 1) == 0
        if desired is INF:
            assert lib.ppo_set_target_kl(ppo, INF) == 0
        else:
            d = float(np.median(runs[INF]))
            assert set_schedule(lib, ppo, lr.ADAPTIVE, d, LO, HI) == 0
        lib.ppo_rollout_device(ppo, E, T, 2, 41)
        lib.ppo_reset_stats(ppo)
        update(lib, ppo, batch)
        if desired is INF:
            runs[INF] = kl_hist(lib, ppo)
        else:
            _, got, _, up, down = assert_replays(lib, ppo, LR_P, d, what="categorical")
            assert len(got) == NPE * (cap // batch) and up + down >= 1
        lib.free_ppo(ppo)


# ----------------------------------------------------------------------------- 10. linear decay under graph replay
def test_linear_decay_under_graph_replay(lib, oracle, monkeypatch):
    """PPO_GRAPH=1 ([17, 256, 256, 6], N = 1024, B = 64, 1 + 1 epochs: steps 1 … 14 of each phase replay captured
    graphs whose Adam step sizes come from the device step table): the table is built from the decayed rates.  Update
    1 of a linear schedule (N = 4, f = 0.1: 0.775 of the base) against a PPO given those rates by hand on the same
    path — V bit for bit (one workgroup per sum at B = 64), the policy to test_graph_replay_matches_eager's bound (the
    fused head's log σ fp32 atomics) — and against a PPO left at the base rates, which must differ."""
    sizes, cap, batch = [17, 256, 256, 6], 1024, 64
    monkeypatch.setenv("PPO_NO_CLUSTER", "1")
    monkeypatch.setenv("PPO_GRAPH", "1")
    monkeypatch.setenv("PPO_GRAPH_STEPS", "16")
    rates = (lr.linear_lr(LR_P, 1, 4, 0.1), lr.linear_lr(LR_V, 1, 4, 0.1))
    assert rates[0] < F32(0.8) * LR_P
    out = {}
    for mode in ("linear", "by hand", "base"):
        ppo = fresh(lib, oracle, sizes=sizes, cap=cap)
        if mode == "linear":
            assert set_schedule(lib, ppo, lr.LINEAR, 4, 0.1, 0) == 0
        lib.ppo_reset_stats(ppo)
        for u in range(2):
            if mode == "by hand" and u == 1:
                ppo.contents.lr_policy, ppo.contents.lr_V = float(rates[0]), float(rates[1])
            lib.ppo_update(ppo, 0.99, batch, 1, 1, 1, SEED)
            lib.ppo_synchronize()
        st = stats(lib, ppo)
        assert st[8] == 2 * 2 * (cap // batch - 2), st[8]              # both phases of both updates replayed graphs
        p, v = nets(lib, ppo)
        out[mode] = (np.frombuffer(p, F32), v)
        lib.free_ppo(ppo)
    assert out["linear"][1] == out["by hand"][1] and out["linear"][1] != out["base"][1]
    n_steps = 2 * cap // batch

    def close(a, b):
        err = np.abs(a.astype(np.float64) - b)
        return err.max() <= 2 * float(LR_P) * n_steps and (err <= 0.1 * float(LR_P)).mean() >= 0.99

    assert close(out["linear"][0], out["by hand"][0])
    assert not close(out["linear"][0], out["base"][0])
