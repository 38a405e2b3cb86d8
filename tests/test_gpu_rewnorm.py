"""Running return-based reward normalisation in the device PPO update (ppo_set_reward_norm, csrc/retnorm.hip).

The oracle has no such option: the reference is tests/rewnorm_ref.py (pinned on the CPU in test_rewnorm_cpu.py).
The update is checked against itself: an update with the feature on over raw rewards must equal an update with it
off over rewards scaled on the host by the bit-comparable fp32 model — the same GAE kernels run on the same bits.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ppo_ffi
import test_gpu_rollout
from helpers import F32, assert_gemm_close, dev, empty, nn_grads_packed, nn_params_packed
from rewnorm_ref import bound, chan, returns64, scale_f32, scale_of, triple64
from test_gpu_obsnorm import CONFIGS
from test_gpu_obsnorm import known_triple as obs_known_triple
from test_gpu_obsnorm import set_state as obs_set_state
from test_gpu_update import make_ppo
from test_obsnorm_cpu import check_triple
from test_rewnorm_cpu import flags, rewards

pytestmark = pytest.mark.gpu

SEED = 77
NSTAT = 25
CHUNK = 2048                    # rows one workgroup of the scan composes (ppo_ext.h PPO_RET_CHUNK)
ORDINARY = np.zeros(1, int)     # check_triple's ordinary-column kind


def stats(lib, ppo, n=NSTAT):
    st = (C.c_double * n)()
    lib.ppo_read_stats(ppo, st, n)
    return list(st)


def set_state(lib, ppo, triple):
    t = np.ascontiguousarray(triple, np.float64)
    assert t.size == 3
    return lib.ppo_reward_norm_set_state(ppo, t.ctypes.data_as(C.POINTER(C.c_double)))


def get_state(lib, ppo):
    out = (C.c_double * 3)()
    lib.ppo_reward_norm_get_state(ppo, out)
    return np.array(out[:])


def no_error(lib):
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


# ----------------------------------------------------------------------------- 1. the scan alone
class Shifted:
    """A device address inside an allocation someone else owns."""

    def __init__(self, ptr):
        self.ptr = ptr


def scan_dev(lib, d, n, gamma, seg_len, want_returns=True, want_carry=True):
    """One ppo_reward_returns_device call over the device arrays of `d` → (R, carry_out, out3)."""
    out3 = (C.c_double * 3)()
    E = n // seg_len if seg_len else 0
    dR = empty(lib, max(n, 1), np.float64) if want_returns else None
    dco = empty(lib, max(E, 1), np.float64) if seg_len and want_carry else None
    rc = lib.ppo_reward_returns_device(d["r"].ptr, d["term"].ptr, d["trunc"].ptr, n, gamma, seg_len,
                                       d["ci"].ptr if seg_len else None, d["cont"].ptr if seg_len else None,
                                       dR.ptr if dR else None, dco.ptr if dco else None, out3)
    assert rc == 0
    R = dR.to_numpy(np.float64, n) if dR else None
    co = dco.to_numpy(np.float64, E) if dco else None
    for a in (dR, dco):
        if a:
            a.free()
    return R, co, np.array(out3[:])


SHAPES = [(1, 0), (CHUNK - 1, 0), (CHUNK, 0), (CHUNK + 1, 0), (3 * CHUNK + 17, 0),
          (5 * 7, 7), (3 * (CHUNK + 1), CHUNK + 1), (64 * 64, 64)]
CASES = [(n, T, g, "rate") for n, T in SHAPES for g in (0.0, 0.99, 1.0)]
# no end flag for more than two chunks; a flag on the last row of a chunk and on the first row of the next; all set
CASES += [(3 * CHUNK + 17, 0, g, "none") for g in (0.99, 1.0)]
CASES += [(3 * CHUNK + 17, 0, 0.99, "edge"), (3 * (CHUNK + 1), CHUNK + 1, 0.99, "edge")]
CASES += [(3 * CHUNK + 17, 0, 0.99, "all"), (64 * 64, 64, 1.0, "all")]


@functools.lru_cache(maxsize=None)
def scan_case(n, T, gamma, mode):
    rng = np.random.default_rng(7 * n + 13 * T + len(mode))
    r = rewards(rng, n)
    term, trunc = flags(rng, n, 1 / 50)
    if mode == "none":
        term[:], trunc[:] = False, False
    elif mode == "edge":
        term[:], trunc[:] = False, False
        term[CHUNK - 1], trunc[CHUNK] = True, True
        trunc[2 * CHUNK - 1], term[2 * CHUNK] = True, True
    elif mode == "all":
        term[:] = rng.random(n) < 0.5
        trunc[:] = ~term
        term[::5] = True                      # both flags set on some rows
    E = n // T if T else 0
    ci = (10.0 * rewards(rng, E)).astype(np.float64) if T else None
    cont = rng.integers(0, 2, E).astype(np.uint8) if T else None
    if T and E > 1:
        cont[0], cont[1] = 0, 1               # mixed
    R, co = returns64(r, term, trunc, gamma, T, ci, cont)
    b = bound(r, term, trunc, gamma, T, ci)
    for a in (r, term, trunc, R, b):
        a.setflags(write=False)
    return dict(r=r, term=term.astype(np.uint8), trunc=trunc.astype(np.uint8), ci=ci, cont=cont, R=R, co=co, b=b)


@pytest.mark.parametrize("n,T,gamma,mode", CASES)
def test_scan(lib, n, T, gamma, mode):
    c = scan_case(n, T, gamma, mode)
    # the special cases start one element into their allocations: the kernel's unaligned (scalar-load) path
    pad = 0 if mode == "rate" else 1
    own = {k: dev(lib, np.concatenate([np.zeros(pad, c[k].dtype), c[k]])) for k in ("r", "term", "trunc")}
    if T:
        own["ci"], own["cont"] = dev(lib, c["ci"]), dev(lib, c["cont"])
    d = {k: Shifted(a.ptr + (pad * c[k].itemsize if k in ("r", "term", "trunc") else 0)) for k, a in own.items()}
    try:
        R, co, o3 = scan_dev(lib, d, n, gamma, T)
        R2, co2, o3b = scan_dev(lib, d, n, gamma, T)
        _, _, o3c = scan_dev(lib, d, n, gamma, T, want_returns=False, want_carry=False)
    finally:
        for a in own.values():
            a.free()
    err = np.abs(R - c["R"])
    worst = float((err[c["b"] > 0] / c["b"][c["b"] > 0]).max(initial=0.0))
    print(f"n {n} T {T} gamma {gamma} {mode}: worst err / bound {worst:.3g}")
    assert (err <= c["b"]).all(), worst
    if T:
        last = np.arange(T - 1, n, T)
        assert (np.abs(co - c["co"]) <= c["b"][last]).all()
        assert (co[c["cont"] == 0] == 0).all() and (co[c["cont"] == 1] == R[last][c["cont"] == 1]).all()
        np.testing.assert_array_equal(co.view(np.uint64), co2.view(np.uint64))
    # determinism: the same bits on every run, with or without the optional outputs
    np.testing.assert_array_equal(R.view(np.uint64), R2.view(np.uint64))
    np.testing.assert_array_equal(o3.view(np.uint64), o3b.view(np.uint64))
    np.testing.assert_array_equal(o3.view(np.uint64), o3c.view(np.uint64))
    # the triple is the exact one of the device's own returns
    check_triple(o3, triple64(R), ORDINARY, f"ppo_reward_returns_device n {n} T {T} gamma {gamma} {mode}")
    no_error(lib)


def test_scan_bad_arguments(lib):
    out3 = (C.c_double * 3)(1, 1, 1)
    r, f = empty(lib, 16), empty(lib, 16, np.uint8)
    ci = dev(lib, np.zeros(4))
    f_ = lib.ppo_reward_returns_device
    assert f_(r.ptr, f.ptr, f.ptr, 0, 0.99, 0, None, None, None, None, out3) == 0 and list(out3) == [0.0] * 3
    assert f_(None, None, None, 0, 0.99, 0, None, None, None, None, out3) == 0 and list(out3) == [0.0] * 3
    assert f_(r.ptr, f.ptr, f.ptr, -1, 0.99, 0, None, None, None, None, out3) == -1
    assert f_(None, f.ptr, f.ptr, 8, 0.99, 0, None, None, None, None, out3) == -1
    assert f_(r.ptr, None, f.ptr, 8, 0.99, 0, None, None, None, None, out3) == -1
    assert f_(r.ptr, f.ptr, None, 8, 0.99, 0, None, None, None, None, out3) == -1
    assert f_(r.ptr, f.ptr, f.ptr, 8, 0.99, 0, None, None, None, None, None) == -1
    assert f_(r.ptr, f.ptr, f.ptr, 8, 0.99, -2, ci.ptr, f.ptr, None, None, out3) == -1
    assert f_(r.ptr, f.ptr, f.ptr, 9, 0.99, 4, ci.ptr, f.ptr, None, None, out3) == -1       # n % T != 0
    assert f_(r.ptr, f.ptr, f.ptr, 8, 0.99, 4, None, f.ptr, None, None, out3) == -1         # no carry_in
    assert f_(r.ptr, f.ptr, f.ptr, 8, 0.99, 4, ci.ptr, None, None, ci.ptr, out3) == -1      # carry_out, no cont
    assert f_(r.ptr, f.ptr, f.ptr, 8, float("nan"), 0, None, None, None, None, out3) == -1
    assert f_(r.ptr, f.ptr, f.ptr, 8, 0.99, 4, ci.ptr, None, None, None, out3) == 0 and out3[0] == 8
    for a in (r, f, ci):
        a.free()
    no_error(lib)


# ----------------------------------------------------------------------------- 2. scale and counters
def gae_run(lib, oracle, rew, setup=None, sizes=(5, 16, 2), envs=2):
    """A PPO over a synthetic fill whose rewards are replaced by `rew`, `setup(ppo)` applied, one update with
    step limit (0, 0) — GAE only."""
    N = rew.size
    ppo = make_ppo(lib, oracle, list(sizes), N)
    lib.ppo_fill_synthetic(ppo, envs, N // envs, 3, 0.0)
    lib.ppo_synchronize()
    b = ppo.contents.buffer.contents
    ppo_ffi.h2d(lib, b.d_reward_p, rew)
    if setup:
        setup(ppo)
    lib.ppo_set_step_limit(ppo, 0, 0)
    lib.ppo_update(ppo, 0.99, N, 1, 1, 1, SEED)
    lib.ppo_synchronize()
    no_error(lib)
    lib.ppo_set_step_limit(ppo, -1, -1)
    return dict(ppo=ppo, st=stats(lib, ppo), adv=ppo_ffi.d2h(lib, b.d_advantage_p, F32, N),
                tgt=ppo_ffi.d2h(lib, b.d_adv_target_p, F32, N), rew=ppo_ffi.d2h(lib, b.d_reward_p, F32, N))


def test_scale_of_a_known_state(lib, oracle):
    ppo = make_ppo(lib, oracle, [5, 16, 2], 8)
    assert lib.ppo_get_reward_norm(ppo) == 0.0 and lib.ppo_reward_norm_scale(ppo) == 1.0
    rng = np.random.default_rng(5)
    for _ in range(20):
        tri = np.array([float(rng.integers(1, 10 ** 6)), rng.normal() * 100, 0.0])
        tri[2] = tri[0] * (10.0 ** rng.uniform(-3, 3)) ** 2
        assert set_state(lib, ppo, tri) == 0
        np.testing.assert_array_equal(get_state(lib, ppo), tri)
        s, s_ref = lib.ppo_reward_norm_scale(ppo), scale_of(tri)
        assert abs(float(s) - float(s_ref)) <= np.spacing(s_ref), (s, s_ref)
    assert set_state(lib, ppo, np.zeros(3)) == 0 and lib.ppo_reward_norm_scale(ppo) == 1.0
    for clip in (10.0, 0.5, float("inf")):
        assert lib.ppo_set_reward_norm(ppo, clip) == 0 and lib.ppo_get_reward_norm(ppo) == F32(clip)
    # bad arguments: −1, the setting and the state unchanged
    tri = np.array([4.0, 0.25, 8.0])
    assert set_state(lib, ppo, tri) == 0
    assert lib.ppo_set_reward_norm(ppo, float("nan")) == -1 and lib.ppo_get_reward_norm(ppo) == float("inf")
    for bad in ([-1.0, 0, 1], [4, 0, -1.0], [np.nan, 0, 1], [4, np.nan, 1], [4, 0, np.nan], [np.inf, 0, 1],
                [4, np.inf, 1], [4, 0, np.inf]):
        assert set_state(lib, ppo, np.array(bad, np.float64)) == -1
    assert lib.ppo_reward_norm_set_state(ppo, None) == -1
    np.testing.assert_array_equal(get_state(lib, ppo), tri)
    assert lib.ppo_reward_norm_freeze(ppo, 1) == 0 and lib.ppo_reward_norm_freeze(ppo, 0) == 1
    # turning it off keeps the state, and the first 22 statistics do not change with the length asked for
    s_on = stats(lib, ppo)
    assert s_on[22:] == [4, 0, 0]
    assert lib.ppo_set_reward_norm(ppo, 0.0) == 0 and lib.ppo_get_reward_norm(ppo) == 0.0
    np.testing.assert_array_equal(get_state(lib, ppo), tri)
    assert stats(lib, ppo)[22:] == [0, 0, 0]
    assert stats(lib, ppo, 22) == stats(lib, ppo)[:22] == s_on[:22]
    no_error(lib)
    lib.free_ppo(ppo)


def test_identity_boundary_nan_and_counters(lib, oracle):
    rew = np.array([0.5, -0.5, 0.25, 0.50000006, -0.75, 3.0, 0.1, -0.2], F32)
    off = gae_run(lib, oracle, rew)
    assert off["st"][22:] == [0, 0, 0]
    # an empty state is the bitwise identity even with clip 0.5, frozen or not … (not frozen: it folds first)
    ident = gae_run(lib, oracle, rew, lambda p: (lib.ppo_set_reward_norm(p, 0.5), lib.ppo_reward_norm_freeze(p, 1)))
    for k in ("adv", "tgt"):
        np.testing.assert_array_equal(ident[k].view(np.uint32), off[k].view(np.uint32))
    assert ident["st"][22:] == [0, 0, 8] and lib.ppo_reward_norm_scale(ident["ppo"]) == 1.0
    # s = 1 exactly: elements exactly at ±c pass through uncounted; out[22..24] after a frozen update
    one = np.array([4.0, 0.0, 4.0 * (1.0 - 1e-8)])

    def frozen_half(p):
        assert lib.ppo_set_reward_norm(p, 0.5) == 0 and set_state(lib, p, one) == 0
        assert lib.ppo_reward_norm_scale(p) == 1.0
        assert lib.ppo_reward_norm_freeze(p, 1) == 0

    y, cl = scale_f32(rew, F32(1.0), 0.5)
    assert cl.tolist() == [False, False, False, True, True, True, False, False]
    a = gae_run(lib, oracle, rew, frozen_half)
    b = gae_run(lib, oracle, y)
    for k in ("adv", "tgt"):
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
    assert not np.array_equal(a["tgt"], off["tgt"])
    assert a["st"][22:] == [4, 3, 8]
    np.testing.assert_array_equal(a["rew"].view(np.uint32), rew.view(np.uint32))
    np.testing.assert_array_equal(get_state(lib, a["ppo"]), one)           # frozen: no fold
    # a NaN reward propagates and is not counted
    rew_nan = rew.copy()
    rew_nan[6] = np.nan
    y_nan, cl_nan = scale_f32(rew_nan, F32(1.0), 0.5)
    assert np.isnan(y_nan[6]) and not cl_nan[6]
    an = gae_run(lib, oracle, rew_nan, frozen_half)
    bn = gae_run(lib, oracle, y_nan)
    assert an["st"][22:] == [4, 3, 8] and np.isnan(an["tgt"]).any()
    np.testing.assert_array_equal(np.isnan(an["tgt"]), np.isnan(bn["tgt"]))
    ok = ~np.isnan(an["tgt"])
    np.testing.assert_array_equal(an["tgt"][ok].view(np.uint32), bn["tgt"][ok].view(np.uint32))
    for r_ in (off, ident, a, b, an, bn):
        lib.free_ppo(r_["ppo"])


# ----------------------------------------------------------------------------- 3. update == update on pre-scaled rewards
TRI0 = np.array([1e6, 0.0, 1e6 * 0.8 ** 2])


def one_update(lib, oracle, sizes, B, N, clip, pre=None):
    ppo = make_ppo(lib, oracle, sizes, N, seed=4242)
    lib.ppo_fill_synthetic(ppo, 8, N // 8, 9, 1.0 / 200)
    lib.ppo_synchronize()
    b = ppo.contents.buffer.contents
    raw = (ppo_ffi.d2h(lib, b.d_reward_p, F32, N) * F32(50.0)).astype(F32)     # so that the scale matters
    out = dict(ppo=ppo, raw=raw, term=ppo_ffi.d2h(lib, b.d_terminated_p, np.uint8, N),
               trunc=ppo_ffi.d2h(lib, b.d_truncated_p, np.uint8, N))
    if pre is not None:                                    # run B: rewards scaled on the host, feature off
        ppo_ffi.h2d(lib, b.d_reward_p, scale_f32(raw, pre, clip)[0])
    else:
        ppo_ffi.h2d(lib, b.d_reward_p, raw)
        assert lib.ppo_set_reward_norm(ppo, clip) == 0 and set_state(lib, ppo, TRI0) == 0
    lib.ppo_set_step_limit(ppo, 1, 1)
    lib.ppo_reset_stats(ppo)
    oracle.srand(99)
    lib.ppo_update(ppo, 0.99, B, 1, 1, 1, SEED)
    lib.ppo_synchronize()
    no_error(lib)
    pol = ppo.contents.policy.contents
    out["mu_forward_m"] = pol.mu.contents.cache_m_forward
    out.update(st=stats(lib, ppo), adv=ppo_ffi.d2h(lib, b.d_advantage_p, F32, N),
               tgt=ppo_ffi.d2h(lib, b.d_adv_target_p, F32, N), gV=nn_grads_packed(lib, ppo.contents.V),
               gmu=nn_grads_packed(lib, pol.mu), gls=ppo_ffi.d2h(lib, pol.d_log_std_grad, F32, sizes[-1]),
               buf_rew=ppo_ffi.d2h(lib, b.d_reward_p, F32, N), s=lib.ppo_reward_norm_scale(ppo))
    return out


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_update_equals_prescaled(lib, oracle, cfg, monkeypatch):
    sizes, B, tiny = CONFIGS[cfg]
    monkeypatch.delenv("PPO_NO_TINY", raising=False)
    N, clip = 2 * B, 5.0
    a = one_update(lib, oracle, sizes, B, N, clip)
    # A folds first: the scale the reference predicts, which is also A's
    R_ref, _ = returns64(a["raw"], a["term"], a["trunc"], 0.99)
    want = chan(TRI0, triple64(R_ref))
    s = scale_of(want)
    assert a["s"] == s, (a["s"], s)
    bb = one_update(lib, oracle, sizes, B, N, clip, pre=s)
    try:
        np.testing.assert_array_equal(a["raw"], bb["raw"])
        # the path the configuration is here for was the one taken, with the feature on as with it off
        assert a["mu_forward_m"] == bb["mu_forward_m"] == (N if tiny else B), (a["mu_forward_m"], bb["mu_forward_m"])
        assert a["st"][1] == 1 and a["st"][3] == 1
        for k in ("adv", "tgt"):
            np.testing.assert_array_equal(a[k].view(np.uint32), bb[k].view(np.uint32))
        assert_gemm_close(a["gV"], bb["gV"], B, f"{cfg}: value grads, feature on vs pre-scaled")
        assert_gemm_close(a["gmu"], bb["gmu"], B, f"{cfg}: policy grads, feature on vs pre-scaled")
        assert_gemm_close(a["gls"], bb["gls"], B, f"{cfg}: log-std grads, feature on vs pre-scaled")
        assert np.abs(bb["gV"]).max() > 0 and np.abs(bb["gmu"]).max() > 0
        # the caller's buffer is never written
        np.testing.assert_array_equal(a["buf_rew"].view(np.uint32), a["raw"].view(np.uint32))
        # counters and the folded state
        _, cl = scale_f32(a["raw"], s, clip)
        st = a["st"]
        print(f"{cfg}: scale {s}, clamped {int(st[23])} of {int(st[24])} (model {int(cl.sum())}), count {st[22]}")
        assert cl.sum() > 0 and st[23] == cl.sum() and st[24] == N and bb["st"][22:] == [0, 0, 0]
        got = get_state(lib, a["ppo"])
        check_triple(got, want, ORDINARY, f"{cfg}: running state after the update")
        assert st[22] == want[0] == got[0]
        # a frozen repeat scales and leaves the state's bits alone
        assert lib.ppo_reward_norm_freeze(a["ppo"], 1) == 0
        lib.ppo_update(a["ppo"], 0.99, B, 1, 1, 1, SEED)
        lib.ppo_synchronize()
        np.testing.assert_array_equal(get_state(lib, a["ppo"]).view(np.uint64), got.view(np.uint64))
        assert stats(lib, a["ppo"])[22:] == [want[0], cl.sum(), N]
        no_error(lib)
    finally:
        for r_ in (a, bb):
            lib.ppo_set_step_limit(r_["ppo"], -1, -1)
            lib.free_ppo(r_["ppo"])


# ----------------------------------------------------------------------------- 4. fold order
def test_fold_order(lib, oracle):
    """Fold first, scale with the refreshed state: from an empty state the first update is already scaled."""
    N = 4096
    rng = np.random.default_rng(21)
    rew = (5.0 * rng.normal(size=N)).astype(F32)
    off = gae_run(lib, oracle, rew, sizes=(17, 64, 6), envs=8)
    on = gae_run(lib, oracle, rew, lambda p: lib.ppo_set_reward_norm(p, 5.0), sizes=(17, 64, 6), envs=8)
    b = on["ppo"].contents.buffer.contents
    R_ref, _ = returns64(rew, ppo_ffi.d2h(lib, b.d_terminated_p, np.uint8, N),
                         ppo_ffi.d2h(lib, b.d_truncated_p, np.uint8, N), 0.99)
    want = triple64(R_ref)
    assert on["st"][22] == N and on["st"][24] == N
    check_triple(get_state(lib, on["ppo"]), want, ORDINARY, "state after the first update")
    s = lib.ppo_reward_norm_scale(on["ppo"])
    assert s == scale_of(want) and s < 0.5, (s, scale_of(want))
    assert np.abs(on["tgt"] - off["tgt"]).max() > 1.0
    # … and a second update over the same buffer folds again but scales the raw rewards once
    lib.ppo_set_step_limit(on["ppo"], 0, 0)
    lib.ppo_update(on["ppo"], 0.99, N, 1, 1, 1, SEED)
    lib.ppo_synchronize()
    assert stats(lib, on["ppo"])[22] == 2 * N
    np.testing.assert_array_equal(ppo_ffi.d2h(lib, b.d_reward_p, F32, N).view(np.uint32), rew.view(np.uint32))
    for r_ in (off, on):
        lib.free_ppo(r_["ppo"])


# ----------------------------------------------------------------------------- 5. device rollout carry
@pytest.mark.parametrize("sizes,kind", [([3, 64, 64, 1], 0), ([17, 64, 64, 6], 1)])
def test_rollout_carry(lib, oracle, sizes, kind):
    E = T = 64
    N, S, A, g = E * T, sizes[0], sizes[-1], 0.99
    ppo = test_gpu_rollout.make(lib, sizes, N)
    assert lib.ppo_set_reward_norm(ppo, 10.0) == 0
    lib.ppo_set_step_limit(ppo, 0, 0)
    bufs = []
    for _ in range(2):
        lib.ppo_rollout_device(ppo, E, T, kind, 11)
        lib.ppo_synchronize()
        bufs.append(test_gpu_rollout.read_buffer(lib, ppo, N, S, A))
        lib.ppo_update(ppo, g, N // 4, 1, 1, 1, SEED)
        lib.ppo_synchronize()
        no_error(lib)
    b1, b2 = bufs
    got = get_state(lib, ppo)
    # cont, reconstructed: the episode of env e continues when rollout 2 starts from rollout 1's last next_state
    last = b1["next_state"][T - 1::T].view(np.uint32)
    first = b2["state"][0::T].view(np.uint32)
    cont = (last == first).all(axis=1)
    assert cont.any()
    R1, co1 = returns64(b1["reward"], b1["term"], b1["trunc"], g, T, np.zeros(E), cont)
    assert (co1[cont] != 0).any()
    R2, _ = returns64(b2["reward"], b2["term"], b2["trunc"], g, T, co1, None)
    want = chan(triple64(R1), triple64(R2))
    check_triple(got, want, ORDINARY, f"kind {kind}: state after two rollouts, carried")
    assert stats(lib, ppo)[22] == 2 * N
    # control: without the carry the fold does not match
    R2z, _ = returns64(b2["reward"], b2["term"], b2["trunc"], g, T, np.zeros(E), None)
    with pytest.raises(AssertionError):
        check_triple(got, chan(triple64(R1), triple64(R2z)), ORDINARY, "control")
    # a rollout after ppo_fill_synthetic starts from zero carry
    lib.ppo_fill_synthetic(ppo, E, T, 13, 1.0 / 200)
    lib.ppo_update(ppo, g, N // 4, 1, 1, 1, SEED)
    lib.ppo_synchronize()
    before = get_state(lib, ppo)
    assert before[0] == 3 * N
    lib.ppo_rollout_device(ppo, E, T, kind, 11)
    lib.ppo_synchronize()
    b3 = test_gpu_rollout.read_buffer(lib, ppo, N, S, A)
    lib.ppo_update(ppo, g, N // 4, 1, 1, 1, SEED)
    lib.ppo_synchronize()
    R3, _ = returns64(b3["reward"], b3["term"], b3["trunc"], g, T, np.zeros(E), None)
    check_triple(get_state(lib, ppo), chan(before, triple64(R3)), ORDINARY, f"kind {kind}: rollout after a fill")
    no_error(lib)
    lib.ppo_set_step_limit(ppo, -1, -1)
    lib.free_ppo(ppo)


# ----------------------------------------------------------------------------- 6. with the other options and paths
def test_with_other_options(lib, oracle, monkeypatch):
    monkeypatch.setenv("PPO_NO_TINY", "1")
    sizes, N, B = [17, 64, 64, 6], 1024, 256
    S = sizes[0]
    ppo = make_ppo(lib, oracle, sizes, N, seed=1234)
    assert lib.ppo_set_obs_norm(ppo, 5.0) == 0
    assert obs_set_state(lib, ppo, obs_known_triple(S, 0.1 * np.random.default_rng(3).normal(size=S), 1.0)) == 0
    assert lib.ppo_set_reward_norm(ppo, 5.0) == 0 and set_state(lib, ppo, [5000.0, 0.0, 5000.0 * 0.01]) == 0
    lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 500)
    assert lib.ppo_set_max_grad_norm(ppo, 0.5) == 0 and lib.ppo_set_target_kl(ppo, float("inf")) == 0
    assert lib.ppo_set_value_clip(ppo, 0.2) == 0
    lib.ppo_reset_stats(ppo)
    lib.ppo_update(ppo, 0.99, B, 1, 2, 1, SEED)
    lib.ppo_synchronize()
    no_error(lib)
    st = stats(lib, ppo)
    lib.free_ppo(ppo)
    assert np.isfinite(st).all()
    assert st[1] == 8 and st[3] == 4 and st[18] == 2 * 1024 and st[15] == 4
    assert st[19] == 5000 + 1024 and st[21] == 1024 * 17
    assert st[22] == 5000 + 1024 and st[24] == 1024


def test_graph_replay(lib, oracle, monkeypatch):
    """The feature keeps graph replay available (test_gpu_update.test_graph_replay_matches_eager's shape)."""
    sizes, N, B = [17, 256, 256, 6], 1024, 64
    monkeypatch.setenv("PPO_NO_CLUSTER", "1")
    out = {}
    for mode in ("eager", "graph"):
        if mode == "eager":
            monkeypatch.delenv("PPO_GRAPH", raising=False)
        else:
            monkeypatch.setenv("PPO_GRAPH", "1")
            monkeypatch.setenv("PPO_GRAPH_STEPS", "16")
        ppo = make_ppo(lib, oracle, sizes, N, init_std=0.7, ent_coeff=0.01)
        assert lib.ppo_set_reward_norm(ppo, 5.0) == 0 and set_state(lib, ppo, [5000.0, 0.0, 5000.0 * 0.01]) == 0
        lib.ppo_fill_synthetic(ppo, 8, N // 8, 44, 1.0 / 200)
        lib.ppo_reset_stats(ppo)
        lib.ppo_update(ppo, 0.99, B, 1, 2, 1, SEED)
        lib.ppo_synchronize()
        no_error(lib)
        pol = ppo.contents.policy.contents
        out[mode] = dict(st=stats(lib, ppo), v=nn_params_packed(lib, ppo.contents.V), mu=nn_params_packed(lib, pol.mu))
        lib.free_ppo(ppo)
    a, b = out["eager"], out["graph"]
    assert a["st"][8] == 0 and b["st"][8] > 0, b["st"][8]
    assert b["st"][24] == N and b["st"][22] == 5000 + N and b["st"][23] == a["st"][23]
    assert_gemm_close(b["v"], a["v"], B, "value parameters, graph replay vs eager")
    assert_gemm_close(b["mu"], a["mu"], B, "policy parameters, graph replay vs eager")


# ----------------------------------------------------------------------------- 7. data parallelism in loopback
def test_loopback_fold_and_hash(lib, oracle, monkeypatch):
    sizes, N, B = [17, 64, 64, 6], 1024, 256
    monkeypatch.setenv("PPO_COMM_LOOPBACK", "2")
    assert lib.ppo_comm_init(0, 1, None) == 0, lib.ppo_last_error()
    try:
        assert lib.ppo_comm_world() == 2
        ppo = make_ppo(lib, oracle, sizes, N, seed=1234)
        assert lib.ppo_set_reward_norm(ppo, 5.0) == 0
        lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 500)
        b = ppo.contents.buffer.contents
        out3 = (C.c_double * 3)()
        assert lib.ppo_reward_returns_device(b.d_reward_p, b.d_terminated_p, b.d_truncated_p, N, 0.99, 0, None, None,
                                             None, None, out3) == 0
        one = np.array(out3[:])
        lib.ppo_set_step_limit(ppo, 1, 1)
        lib.ppo_update(ppo, 0.99, B, 1, 1, 1, SEED)
        lib.ppo_synchronize()                              # returns: no collective left waiting
        no_error(lib)
        got = get_state(lib, ppo)
        assert got[0] == 2 * N and stats(lib, ppo)[22] == 2 * N
        np.testing.assert_allclose(got[1], one[1], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(got[2], 2 * one[2], rtol=1e-12, atol=0)
        lib.ppo_set_step_limit(ppo, -1, -1)
        lib.free_ppo(ppo)
    finally:
        lib.ppo_comm_finalize()
        monkeypatch.delenv("PPO_COMM_LOOPBACK")
    # the hash covers the state while the feature is on, and only then
    p1, p2 = (make_ppo(lib, oracle, sizes, N, seed=1234) for _ in range(2))
    assert lib.ppo_param_hash(p1) == lib.ppo_param_hash(p2)
    h_off = lib.ppo_param_hash(p1)
    # a function of the state only: on and never touched hashes like on and set to the empty state
    assert lib.ppo_set_reward_norm(p1, 5.0) == 0 and lib.ppo_set_reward_norm(p2, 5.0) == 0
    assert set_state(lib, p2, np.zeros(3)) == 0
    assert lib.ppo_param_hash(p1) == lib.ppo_param_hash(p2) != h_off
    for p, mean in ((p1, 0.25), (p2, 0.5)):
        assert set_state(lib, p, [5000.0, mean, 5000.0]) == 0
    assert lib.ppo_param_hash(p1) != lib.ppo_param_hash(p2)
    assert set_state(lib, p2, [5000.0, 0.25, 5000.0]) == 0
    assert lib.ppo_param_hash(p1) == lib.ppo_param_hash(p2) != h_off
    for p in (p1, p2):
        assert lib.ppo_set_reward_norm(p, 0.0) == 0
    assert lib.ppo_param_hash(p1) == lib.ppo_param_hash(p2) == h_off
    lib.free_ppo(p1)
    lib.free_ppo(p2)
