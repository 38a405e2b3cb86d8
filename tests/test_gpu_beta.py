"""The Beta policy on the device (csrc/beta.hip, csrc/kl.hip) against tests/beta_ref.py, whose bounds these are."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import beta_ref as br
import ppo_ffi
import tanh_ref as T
from beta_ref import ENT, EPS, F32, F64, U, Z_MAX
from helpers import assert_gemm_close, dev, nn_grads_packed, nn_input_rows, nn_params_packed
from test_beta_cpu import SAMPLER_PAIRS
from test_gpu_gauss_sd_update import engine, read, rows_of
from test_gpu_update import adam_first_step, assert_adam_delta

pytestmark = pytest.mark.gpu
LR = 3e-4


@contextlib.contextmanager
def on_device(lib, **arrays):
    d = {k: dev(lib, v) for k, v in arrays.items()}
    try:
        yield d
    finally:
        assert [a.free() for a in d.values()] and lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


def run_head(lib, i, skew=0):
    m, A = i["z"].shape
    pad = lambda a: np.concatenate([np.zeros(skew, a.dtype), a.ravel()])                        # noqa: E731
    with on_device(lib, z=pad(i["z"]), act=pad(i["act"]), adv=i["adv"], old=i["old"], g=np.full(m * A + skew, np.nan, F32),
                   lp=np.zeros(m, F32), H=np.zeros(m, F32)) as d:
        loss, cnt = C.c_double(np.nan), (C.c_longlong * 2)(-1, -1)
        assert lib.ppo_beta_head_device(d["z"].ptr + 4 * skew, d["act"].ptr + 4 * skew, d["adv"].ptr, d["old"].ptr, m, A,
                                        Z_MAX, EPS, ENT, d["g"].ptr + 4 * skew, d["lp"].ptr, d["H"].ptr, C.byref(loss),
                                        cnt) == 0
        return dict(grad=d["g"].to_numpy(F32, m * A + skew)[skew:].reshape(m, A), lp=d["lp"].to_numpy(F32, m),
                    H=d["H"].to_numpy(F32, m), loss=loss.value, counts=(cnt[0], cnt[1]))


@pytest.mark.parametrize("Aa,m,skew", [(Aa, m, 0) for Aa in (1, 3, 17, 32) for m in (1, 63, 64, 65, 300)] +
                         [(3, 65536 + 129, 0), (17, 65, 1)])
def test_head_rows(lib, Aa, m, skew):
    """65665 rows: 1027 tiles for a grid capped at 1024; skew: every pointer 4 bytes off a 16-byte boundary"""
    i = br.head_inputs(Aa, m)
    got = run_head(lib, i, skew)
    ref = br.head_f64(i["z"], i["act"], i["adv"], i["old"], EPS, ENT, Z_MAX, lp_for_g=got["lp"])
    for name in ("lp", "H", "grad"):
        err, bound = np.abs(got[name].astype(F64) - ref[name]), ref["b_" + name]
        print(f"Aa {Aa} m {m}: {name} worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all(), name
    print(f"Aa {Aa} m {m}: loss err / bound {abs(got['loss'] - ref['loss']) / ref['b_loss']:.3f}")
    assert abs(got["loss"] - ref["loss"]) <= ref["b_loss"]
    assert got["counts"] == (ref["clamped"], ref["elems"]) and (got["grad"][~ref["inside"]].view(np.uint32) == 0).all()


@pytest.mark.parametrize("Aa", [3, 32])
def test_deterministic_and_nan_isolated(lib, Aa):
    i = br.head_inputs(Aa, 300)
    a, b = run_head(lib, i), run_head(lib, i)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("grad", "lp", "H", "loss"))
    z = np.array(i["z"])
    z[131, 0] = np.nan
    c, keep = run_head(lib, dict(i, z=z)), np.arange(300) != 131
    assert all(c[k][keep].tobytes() == a[k][keep].tobytes() for k in ("grad", "lp", "H")) and np.isnan(c["lp"][131])


def test_sampler(lib):
    """6 standard errors at n = 65536 (numpy's own sampler stays inside them: test_beta_cpu.py); lp is the head's bits"""
    logit = lambda s: -Z_MAX if s == 1 else np.log(np.expm1(s - 1))                             # noqa: E731
    row = np.array([logit(a) for a, _ in SAMPLER_PAIRS] + [logit(b) for _, b in SAMPLER_PAIRS], F32)
    n, z = 65536, np.ascontiguousarray(np.broadcast_to(row, (65536, 6)))
    a, b = (v[0] for v in br.shapes(z[:1], Z_MAX)[:2])
    with on_device(lib, z=z, act=np.full((n, 6), np.nan, F32), lp=np.zeros(n, F32)) as d:
        assert lib.ppo_beta_sample_device(d["z"].ptr, n, 6, Z_MAX, 0x1234ABCD5678, 77, 0, d["act"].ptr, d["lp"].ptr) == 0
        act, lp = d["act"].to_numpy(F32, n * 6).reshape(n, 6), d["lp"].to_numpy(F32, n)
        assert lib.ppo_beta_sample_device(d["z"].ptr, n, 6, Z_MAX, 0, 0, 1, d["act"].ptr, None) == 0
        mean = d["act"].to_numpy(F32, n * 6).reshape(n, 6)
    assert (act[:, :3] >= br.X_LO).all() and (act[:, :3] <= br.X_HI).all() and (act[:, 3:].view(np.uint32) == 0).all()
    for p in (1, 2):
        se = np.sqrt((br.moments(a, b, 2 * p) - br.moments(a, b, p) ** 2) / n)
        off_by = np.abs((act[:, :3].astype(F64) ** p).mean(axis=0) - br.moments(a, b, p)) / se
        print(f"sampler: mean of x^{p} off by {off_by} standard errors")
        assert (off_by <= 6).all(), p
    assert run_head(lib, dict(z=z, act=act, adv=np.ones(n, F32), old=lp))["lp"].tobytes() == lp.tobytes()
    assert (np.abs(mean[:, :3] - a / (a + b)) <= 2 * U * a / (a + b)).all() and (mean[:, 3:].view(np.uint32) == 0).all()


@pytest.mark.parametrize("Aa", [3, 32])
def test_kl_both_estimators(lib, Aa):
    """k3 = mean(expm1(x) − x): x = lp_new − old_lp carries lp's bound Δ, so a term moves by (|expm1 x| + Δ)·Δ; the clip
    count is exact (no ratio within 0.05 of a boundary, asserted); the means pass through fp32 words, 2⁻²³ more."""
    m, i, rng = 300, br.head_inputs(Aa, 300), np.random.default_rng(70 + Aa)
    zo, rows = (i["z"] + rng.normal(scale=0.3, size=i["z"].shape)).astype(F32), rng.permutation(m).astype(np.int32)
    with on_device(lib, n=i["z"], o=zo, r=rows, a=i["act"], old=i["old"], k=np.zeros(m, F64)) as d:
        out = (C.c_double * 3)()
        assert lib.ppo_beta_kl_device(d["n"].ptr, d["o"].ptr, d["r"].ptr, d["a"].ptr, d["old"].ptr, m, 2 * Aa, Z_MAX, EPS,
                                      d["k"].ptr, out) == 0
        got = d["k"].to_numpy(F64, m)
    ref = br.head_f64(i["z"], i["act"], i["adv"], i["old"], EPS, 0.0, Z_MAX)
    x, dx = ref["lp"] - i["old"].astype(F64), ref["b_lp"]
    want, bound = br.kl_rows_f64(zo[rows], i["z"], Z_MAX)
    assert (np.abs(np.abs(np.expm1(x)) - EPS) > 0.05).all()
    k3, k3_tol = (np.expm1(x) - x).mean(), ((np.abs(np.expm1(x)) + dx) * dx).mean()
    print(f"Aa {Aa}: err / bound: k3 {abs(out[0] - k3) / (k3_tol + 2 * U * k3):.3g}, closed form {float((np.abs(got - want) / bound).max()):.3g}")
    assert abs(out[0] - k3) <= k3_tol + 2 * U * k3 and out[1] == float((np.abs(np.expm1(x)) > EPS).sum()) / m
    assert (np.abs(got - want) <= bound).all() and abs(out[2] - want.mean()) <= bound.mean() + 2 * U * want.mean()


def make(lib, sizes, acts, cap, zmax=15.0):
    C.CDLL("libc.so.6").srand(1234)
    ppo = lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), cap, LR, LR, 0.95, EPS, ENT, 0.7, True)
    assert zmax is None or lib.ppo_set_action_beta(ppo, zmax) == 0
    return ppo


def test_setter(lib):
    ppo, odd, wide = (make(lib, [3, 16, A], ["relu", "none"], 64, None) for A in (4, 5, 66))
    for p, zmax in [(odd, 15), (wide, 15)] + [(ppo, bad) for bad in (float("nan"), float("inf"), 0.0, -1.0)]:
        assert lib.ppo_set_action_beta(p, zmax) == -1 and lib.ppo_get_action_dist(p) == 0
    assert lib.ppo_set_compute_dtype(ppo, 1) == 0 and lib.ppo_set_action_beta(ppo, 15) == -1        # bf16 mode
    assert lib.ppo_set_compute_dtype(ppo, 0) == 0 and lib.ppo_set_action_beta(ppo, 15) == 0
    assert lib.ppo_get_action_dist(ppo) == 4 and lib.ppo_last_error() in (b"", None)
    lib.free_ppo(ppo), lib.free_ppo(odd), lib.free_ppo(wide)


@pytest.mark.parametrize("eng", [1, 0])
def test_one_update(lib, eng):
    """one policy step at m = 300, A = 6, the KL monitor on under estimator `eng`; test_gpu_gauss_sd_update.py's bounds"""
    sizes, acts, E, Tn, B, N = [5, 40, 6], ["tanh", "none"], 10, 30, 300, 300
    with engine(lib, eng):
        ppo = make(lib, sizes, acts, N)
        pol = ppo.contents.policy.contents
        lib.ppo_rollout_device(ppo, E, Tn, 1, 5)
        mu0, buf = nn_params_packed(lib, pol.mu), read(lib, ppo, N, 5, 6)
        assert lib.ppo_set_target_kl(ppo, float("inf")) == 0 and lib.ppo_set_kl_estimator(ppo, eng) == 0
        lib.ppo_set_step_limit(ppo, 1, 1)
        lib.ppo_update(ppo, 0.99, B, 1, 1, 1, 7)
        assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
        adv = ppo_ffi.d2h(lib, ppo.contents.buffer.contents.d_advantage_p, F32, N).copy()
        rp = rows_of(nn_input_rows(lib, pol.mu, B), buf["state"])
        gmu, mu1 = nn_grads_packed(lib, pol.mu), nn_params_packed(lib, pol.mu)
        lib.free_ppo(ppo)
    hs, _ = T.forward(sizes, acts, mu0, buf["state"][rp])
    ref = br.head_f64(hs[-1], buf["action"][rp], adv[rp], buf["old_lp"][rp], EPS, ENT, 15.0)
    gmu_ref = T.backward(sizes, acts, mu0, hs, ref["grad"])[0]
    assert_gemm_close(gmu, gmu_ref, B, f"engine {eng} policy grads")
    flips = assert_adam_delta(mu1, adam_first_step(mu0, gmu_ref, LR), gmu_ref, LR, f"engine {eng} policy params")
    assert flips <= max(2, mu1.size // 1000)


def test_pendulum_and_checkpoint_resume(lib, tmp_path):
    """Pendulum with A = 2: the reward is that of the torque 2·(2x − 1); a save / load resumes bit for bit"""
    E, Tn, sizes, acts = 8, 16, [3, 32, 32, 2], ["relu", "relu", "none"]

    def one_round(p, r):
        lib.ppo_rollout_device(p, E, Tn, 0, 41)
        lib.ppo_update(p, 0.99, 64, 2, 2, 1, 17 + r)

    x = make(lib, sizes, acts, E * Tn)
    one_round(x, 0)
    buf = read(lib, x, E * Tn, 3, 2)
    a, s = buf["action"], buf["state"].astype(F64)
    assert (a[:, 0] >= br.X_LO).all() and (a[:, 0] <= br.X_HI).all() and (a[:, 1].view(np.uint32) == 0).all()
    u = 2 * (2 * a[:, 0].astype(F64) - 1)            # reward −(θ² + 0.1·θ̇² + 0.001·u²), θ from the stored (cos, sin)
    want = -(np.arctan2(s[:, 1], s[:, 0]) ** 2 + 0.1 * s[:, 2] ** 2 + 0.001 * u ** 2)
    assert np.abs(buf["reward"] - want).max() <= 1e-4 * (1 + np.abs(want).max()) and np.std(u) > 0.1
    path, err, out = str(tmp_path / "beta.ckpt").encode(), C.create_string_buffer(256), C.c_float()
    assert lib.ppo_save_state(x, path, 1) == 0
    y = lib.ppo_load_state(path, err, 256)
    assert y and lib.ppo_get_action_dist(y) == 4 and lib.ppo_get_action_beta(y, C.byref(out)) == 1 and out.value == 15.0
    one_round(x, 1)
    one_round(y, 1)
    assert lib.ppo_state_hash(y, 1) == lib.ppo_state_hash(x, 1) != 0 and lib.ppo_param_hash(y) == lib.ppo_param_hash(x)
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    lib.free_ppo(x), lib.free_ppo(y)
