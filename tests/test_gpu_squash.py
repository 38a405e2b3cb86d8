"""The squashed Gaussian policy on the device (csrc/squash.hip, csrc/kl.hip) within tests/squash_ref.py's bounds."""
import ctypes as C

import numpy as np
import pytest

import gauss_sd_ref as sd
import ppo_ffi
import rng_ref
import squash_ref as sq
from gauss_sd_ref import ENT, EPS, F32, F64, LS_MAX, LS_MIN, U
from helpers import nn_params_packed
from test_gpu_beta import make, on_device

pytestmark = pytest.mark.gpu
KEY, OFF = 0x1234ABCD5678, 77


def run_head(lib, i, ent=ENT):
    m, A = i["z"].shape
    with on_device(lib, z=i["z"], act=i["act"], adv=i["adv"], old=i["old"], g=np.full((m, A), np.nan, F32),
                   lp=np.zeros(m, F32), H=np.zeros(m, F32)) as d:
        loss, cnt = C.c_double(np.nan), (C.c_longlong * 2)(-1, -1)
        assert lib.ppo_squash_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, m, A, LS_MIN, LS_MAX, EPS,
                                          ent, KEY, OFF, d["g"].ptr, d["lp"].ptr, d["H"].ptr, C.byref(loss), cnt) == 0
        return dict(grad=d["g"].to_numpy(F32, m * A).reshape(m, A), lp=d["lp"].to_numpy(F32, m),
                    H=d["H"].to_numpy(F32, m), loss=loss.value, counts=(cnt[0], cnt[1]))


def run_sampler(lib, z, det=0):
    m, A = z.shape
    with on_device(lib, z=z, act=np.full((m, A), np.nan, F32), lp=np.zeros(m, F32)) as d:
        assert lib.ppo_squash_sample_device(d["z"].ptr, m, A, LS_MIN, LS_MAX, KEY, OFF, det, d["act"].ptr,
                                            None if det else d["lp"].ptr) == 0
        return d["act"].to_numpy(F32, m * A).reshape(m, A), d["lp"].to_numpy(F32, m)


@pytest.mark.parametrize("Aa,m", [(Aa, m) for Aa in sd.HEAD_AA for m in sd.HEAD_M] + [(3, 32768 + 65)])
def test_head_rows(lib, Aa, m):
    """32833 rows: 1027 tiles of 32 rows for a grid capped at 1024 — the grid-stride path and the fold of 1024
    partials, where run-to-run byte identity is asserted too.  At ent_coeff = 0 a clipped row's gradient is all zero"""
    src = sd.smallest_covering(Aa, m) if m <= sd.ROWS else sd.head_inputs(Aa, m)
    assert m == 1 or sd.check_input_condition(src, f"Aa {Aa} m {m}")
    i = sq.squashed(src)
    ref = sq.head_f64(i["z"], i["act"], i["adv"], i["old"], EPS, ENT, LS_MIN, LS_MAX, KEY, OFF)
    assert not sd.near_clip(ref["ratio"]).any()
    got = run_head(lib, i)
    for name in ("lp", "H", "grad", "loss"):
        err, bound = np.abs(np.asarray(got[name], F64) - ref[name]), ref["b_" + name]
        print(f"Aa {Aa} m {m}: {name} error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all(), name
    assert got["counts"] == (ref["clamped"], ref["elems"])
    assert (got["grad"][:, Aa:][~ref["inside"]].view(np.uint32) == 0).all()
    np.testing.assert_array_equal(~(run_head(lib, i, ent=0.0)["grad"] != 0).any(axis=1), ref["clipped"])
    if m > 32768:
        again = run_head(lib, i)
        assert again["loss"] == got["loss"] and all(again[k].tobytes() == got[k].tobytes() for k in ("grad", "lp", "H"))


@pytest.mark.parametrize("Aa", sd.HEAD_AA)
def test_sampler(lib, Aa):
    """u against the model; a the device's own tanhf(u), element for element (the deterministic form over μ = u); the
    stored log-prob the head's bits; finite where |u| > 10 and a rounds to ±1"""
    m, z = 300, np.array(sd.smallest_covering(Aa, 300)["z"])
    z[:8, 0], z[:8, Aa] = [12, -12, 15, -15, 11, -11, 30, -30], LS_MIN               # σ = e⁻²: |u| stays above 10
    act, lp = run_sampler(lib, z)
    u, a = act[:, Aa:], act[:, :Aa]
    want, bound = sq.sample_f64(z, LS_MIN, LS_MAX, KEY, OFF)
    print(f"Aa {Aa}: u error / bound {float((np.abs(u - want) / bound).max()):.3f}")
    assert (np.abs(u - want) <= bound).all()
    det, _ = run_sampler(lib, np.concatenate([u, z[:, Aa:]], axis=1), det=1)
    assert det[:, :Aa].tobytes() == a.tobytes() and det[:, Aa:].tobytes() == u.tobytes()
    assert (np.abs(a - np.tanh(u.astype(F64))) <= 10 * U).all()                      # a 5-ulp tanhf, |a| <= 1
    assert (np.abs(u[:8, 0]) > 10).all() and (np.abs(a[:8, 0]) == 1).all() and np.isfinite(lp).all()
    assert run_head(lib, dict(z=z, act=act, adv=np.ones(m, F32), old=lp))["lp"].tobytes() == lp.tobytes()


@pytest.mark.parametrize("Aa", [3, 32])
def test_kl(lib, Aa):
    """k3, the clip fraction (exact: no ratio within 0.05 of a boundary, asserted) and the closed form against the
    model; the closed form the state-dependent-σ entry's bits on the same rows; means pass through fp32 words"""
    m, rng = 300, np.random.default_rng(70 + Aa)
    i = sq.squashed(sd.smallest_covering(Aa, m))
    zo, rows = (i["z"] + rng.normal(scale=0.3, size=i["z"].shape)).astype(F32), rng.permutation(m).astype(np.int32)
    with on_device(lib, n=i["z"], o=zo, r=rows, a=i["act"], old=i["old"], k=np.zeros(m, F64), k3=np.zeros(m, F64)) as d:
        out, mean = (C.c_double * 3)(), C.c_double()
        assert lib.ppo_squash_kl_device(d["n"].ptr, d["o"].ptr, d["r"].ptr, d["a"].ptr, d["old"].ptr, m, 2 * Aa, LS_MIN,
                                        LS_MAX, EPS, d["k"].ptr, out) == 0
        assert lib.ppo_gauss_sd_kl_exact_device(d["n"].ptr, d["o"].ptr, d["r"].ptr, m, 2 * Aa, LS_MIN, LS_MAX,
                                                d["k3"].ptr, C.byref(mean)) == 0
        got, same = d["k"].to_numpy(F64, m), d["k3"].to_numpy(F64, m)
    ref = sq.kl_f64(i["z"], zo[rows], i["act"], i["old"], EPS, LS_MIN, LS_MAX)
    assert (np.abs(np.abs(np.expm1(ref["x"])) - EPS) > 0.05).all()
    print(f"Aa {Aa}: k3 error / bound {abs(out[0] - ref['k3']) / (ref['b_k3'] + 2 * U * ref['k3']):.3f}")
    assert abs(out[0] - ref["k3"]) <= ref["b_k3"] + 2 * U * ref["k3"] and out[1] == ref["clip"]
    assert (np.abs(got - ref["rows"]) <= 1e-12 * np.maximum(1.0, ref["rows"])).all()
    assert got.tobytes() == same.tobytes() and out[2] == mean.value


def test_one_update_and_resume(lib, tmp_path):
    """one policy step from ppo_fill_synthetic: ratios of exactly 1 (clip fraction 0, k3 0), finite parameters, out[4]
    the model's mean H over the step's z under the update's entropy stream; then save → load → update hashes equal"""
    A, N, seed = 6, 300, 7
    x = make(lib, [5, 40, A], ["tanh", "none"], N, None)
    assert lib.ppo_set_action_squashed_gaussian(x, LS_MIN, LS_MAX) == 0 == lib.ppo_set_target_kl(x, float("inf"))
    lib.ppo_fill_synthetic(x, 10, 30, 3, 0.02)
    lib.ppo_set_step_limit(x, 1, 1)
    lib.ppo_update(x, 0.99, N, 1, 1, 1, seed)
    out, mu = (C.c_double * 36)(), x.contents.policy.contents.mu
    lib.ppo_read_stats(x, out, 36)
    z = ppo_ffi.d2h(lib, mu.contents.d_output, F32, N * A).reshape(N, A).copy()
    # the policy epoch's shuffle key follows the value epoch's: splitmix64(seed) + 1 (rng.h, the entropy stream)
    key = rng_ref.splitmix64(((int(rng_ref.splitmix64(seed)) + 1) ^ seed ^ 0x5351454E54) & (2 ** 64 - 1))
    ref = sq.head_f64(z, np.zeros((N, A), F32), np.ones(N), np.zeros(N), EPS, ENT, LS_MIN, LS_MAX, int(key), 0)
    print(f"update: mean H error / bound {abs(out[4] - ref['H'].mean()) / ref['b_H'].mean():.3f}")
    assert abs(out[4] - ref["H"].mean()) <= ref["b_H"].mean() and out[35] == N * A // 2
    assert out[14] == 0 and out[13] == 0 and np.isfinite(nn_params_packed(lib, mu)).all()
    path, err, b2 = str(tmp_path / "sq.ckpt").encode(), C.create_string_buffer(256), (C.c_float * 2)()
    assert lib.ppo_get_action_dist(x) == 5 and lib.ppo_save_state(x, path, 1) == 0
    y = lib.ppo_load_state(path, err, 256)
    assert y and lib.ppo_get_action_dist(y) == 5 and lib.ppo_get_action_squashed_gaussian(y, b2) == 1, err.value
    assert (b2[0], b2[1]) == (LS_MIN, LS_MAX)
    for p in (x, y):
        lib.ppo_set_step_limit(p, -1, -1)
        lib.ppo_rollout_device(p, 10, 30, 1, 41)
        lib.ppo_update(p, 0.99, 100, 2, 2, 1, seed)
    assert lib.ppo_state_hash(y, 1) == lib.ppo_state_hash(x, 1) != 0 and lib.ppo_param_hash(y) == lib.ppo_param_hash(x)
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    lib.free_ppo(x), lib.free_ppo(y)


@pytest.mark.parametrize("A,lo,hi,bf16", [(5, -20, 2, 0), (66, -20, 2, 0), (4, 1, 1, 0), (4, float("nan"), 1, 0),
                                          (4, -21, 1, 0), (4, -1, 21, 0), (4, -20, 2, 1)])
def test_setter_declines(lib, A, lo, hi, bf16):
    ppo = make(lib, [3, 16, A], ["relu", "none"], 64, None)
    assert lib.ppo_set_compute_dtype(ppo, bf16) == 0
    assert lib.ppo_set_action_squashed_gaussian(ppo, lo, hi) == -1 and lib.ppo_get_action_dist(ppo) == 0
    if A == 4 and not bf16:
        assert lib.ppo_set_action_squashed_gaussian(ppo, -20, 2) == 0 and lib.ppo_get_action_dist(ppo) == 5
        assert lib.ppo_set_action_dist(ppo, 5) == lib.ppo_set_action_mask(ppo, 1) == lib.ppo_set_compute_dtype(ppo, 1) == -1
        assert lib.ppo_set_action_dist(ppo, 0) == 0 and lib.ppo_get_action_squashed_gaussian(ppo, None) == 0
    assert lib.ppo_squash_sample_device(None, 1, 2, -1.0, 1.0, 0, 0, 0, None, None) == -1      # nothing launched
    assert lib.ppo_last_error() in (b"", None)
    lib.free_ppo(ppo)
