"""The state-dependent-σ Gaussian policy on the device (ppo_set_action_gaussian_sd; csrc/gauss_sd.hip, csrc/kl.hip)
against tests/gauss_sd_ref.py: the head row by row, constant-σ equivalence with the Gaussian head, the sampler,
determinism and NaN isolation, the closed-form KL, the setter and a checkpoint (the update, the KL monitor, the
rollouts and data parallelism are in test_gpu_gauss_sd_update.py).  Every bound
comes from gauss_sd_ref (derived from the rounding of the listed operations and validated by the fp32 mirror on the
CPU in test_gauss_sd_cpu.py); nothing is taken from a run of the kernels."""
import ctypes as C

import numpy as np
import pytest

import gauss_sd_ref as sd
import ppo_ffi
import rng_ref
from gauss_sd_ref import ENT, EPS, F32, F64, LS_MAX, LS_MIN, U
from helpers import dev, empty

pytestmark = pytest.mark.gpu
U64 = np.uint64


def no_error(lib):
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


def run_head(lib, i, ent=ENT, lo=LS_MIN, hi=LS_MAX):
    m, A = i["z"].shape
    d = dict(z=dev(lib, i["z"]), act=dev(lib, i["act"]), adv=dev(lib, i["adv"]), old=dev(lib, i["old"]),
             g=dev(lib, np.full((m, A), np.nan, F32)), lp=empty(lib, m), H=empty(lib, m))
    try:
        loss, cnt = C.c_double(np.nan), (C.c_longlong * 2)(-1, -1)
        rc = lib.ppo_gauss_sd_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, m, A, lo, hi, EPS, ent,
                                          d["g"].ptr, d["lp"].ptr, d["H"].ptr, C.byref(loss), cnt)
        assert rc == 0
        return dict(grad=d["g"].to_numpy(F32, m * A).reshape(m, A), lp=d["lp"].to_numpy(F32, m),
                    H=d["H"].to_numpy(F32, m), loss=loss.value, counts=(cnt[0], cnt[1]))
    finally:
        for a in d.values():
            a.free()


# ------------------------------------------------------------------------------------------ 1. head rows
@pytest.mark.parametrize("Aa", sd.HEAD_AA)
def test_head_rows(lib, Aa):
    """lp, both gradient halves, the row entropy and the loss within the derived bounds of the float64 model at
    m ∈ {1, 63, 64, 65, 300}; the counters exact; a clamped column's gradient the bits of +0."""
    for m in sd.HEAD_M:
        i = sd.smallest_covering(Aa, m)
        what = f"Aa {Aa} m {m}"
        args = (i["z"], i["act"], i["adv"], i["old"], EPS, ENT, LS_MIN, LS_MAX)
        ref = sd.check_input_condition(i, what) if m > 1 else sd.head_f64(*args)
        b = sd.head_bounds(*args)
        got = run_head(lib, i)
        for name in ("lp", "H", "grad"):
            err = np.abs(got[name].astype(F64) - ref[name])
            print(f"{what}: {name} error / bound {float((err / np.maximum(b[name], 1e-300)).max()):.3f}")
            assert (err <= b[name]).all(), f"{what}: {name}"
        bound = sd.loss_bound(ref, b, m, ENT)
        print(f"{what}: loss error / bound {abs(got['loss'] - ref['loss']) / bound:.3f}")
        assert abs(got["loss"] - ref["loss"]) <= bound, f"{what}: loss {got['loss']} vs {ref['loss']} ± {bound}"
        assert got["counts"] == (ref["clamped"], ref["elems"]), what
        assert (got["grad"][:, Aa:][~ref["inside"]].view(np.uint32) == 0).all(), what
        # the clip branch per row: with ent_coeff = 0 a clipped row's gradient is all zero, an unclipped one's is not
        first = run_head(lib, i, ent=0.0)["grad"]
        np.testing.assert_array_equal(~(first != 0).any(axis=1), ref["clipped"], err_msg=what)
    no_error(lib)


def test_head_rows_past_the_grid_cap(lib):
    """m = 65536 + 129 rows are 1027 tiles for a grid capped at 1024 workgroups: three workgroups take a second tile
    (the grid-stride path) and the last arriver folds 1024 partials in runs of 16 — the only shape at which either
    can go wrong.  The same checks as test_head_rows, at Aa = 3."""
    Aa, m = 3, 65536 + 129
    i = sd.head_inputs(Aa, m)
    args = (i["z"], i["act"], i["adv"], i["old"], EPS, ENT, LS_MIN, LS_MAX)
    ref, b = sd.check_input_condition(i, f"m {m}"), sd.head_bounds(*args)
    got = run_head(lib, i)
    for name in ("lp", "H", "grad"):
        err = np.abs(got[name].astype(F64) - ref[name])
        print(f"m {m}: {name} error / bound {float((err / np.maximum(b[name], 1e-300)).max()):.3f}")
        assert (err <= b[name]).all(), name
    bound = sd.loss_bound(ref, b, m, ENT)
    print(f"m {m}: loss error / bound {abs(got['loss'] - ref['loss']) / bound:.3f}")
    assert abs(got["loss"] - ref["loss"]) <= bound
    assert got["counts"] == (ref["clamped"], ref["elems"])
    again = run_head(lib, i)
    assert again["loss"] == got["loss"] and again["grad"].tobytes() == got["grad"].tobytes()
    no_error(lib)


# ------------------------------------------------------------------------------ 2. constant-σ equivalence
def run_gauss_head(lib, form, mu, L, act, adv, old, ent):
    m, A = mu.shape
    d = dict(ls=dev(lib, L), act=dev(lib, act), adv=dev(lib, adv), old=dev(lib, old), mu=dev(lib, mu), lp=empty(lib, m),
             g=empty(lib, m * A), gls=empty(lib, A))
    try:
        loss = C.c_double(np.nan)
        rc = lib.ppo_policy_head_device(form, m, A, 0, 0, EPS, ent, d["ls"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr,
                                        d["mu"].ptr, None, None, None, d["lp"].ptr, d["g"].ptr, None, None, d["gls"].ptr,
                                        C.byref(loss))
        assert rc == 0
        return dict(lp=d["lp"].to_numpy(F32, m), grad=d["g"].to_numpy(F32, m * A).reshape(m, A),
                    gls=d["gls"].to_numpy(F32, A))
    finally:
        for a in d.values():
            a.free()


@pytest.mark.parametrize("Aa", sd.HEAD_AA)
def test_constant_sigma_is_the_gaussian_head(lib, Aa):
    """every row's raw log σ = one in-range vector L: lp (form 0 writes it; forms 0 and 1 share the row arithmetic)
    and the mean-half gradient are the Gaussian head's bits at width Aa; the column sums of the log-σ half agree with
    form 1's d_grad_log_std (which holds −ent_coeff per column, as Σ_rows −ent_coeff/m does) within the bound of a sum
    of m fp32 terms: (m + 2)·2⁻²⁴·Σ|term| plus the terms' own."""
    rng = np.random.default_rng(50 + Aa)
    L = rng.uniform(LS_MIN + 0.05, LS_MAX - 0.05, Aa).astype(F32)
    for m in (64, 300):
        i = sd.smallest_covering(Aa, m)
        z = np.array(i["z"])
        z[:, Aa:] = L
        j = dict(z=z, act=i["act"], adv=i["adv"], old=i["old"])
        got = run_head(lib, j)
        mu, act = np.ascontiguousarray(z[:, :Aa]), np.ascontiguousarray(i["act"][:, :Aa])
        g1 = run_gauss_head(lib, 1, mu, L, act, i["adv"], i["old"], ENT)
        g0 = run_gauss_head(lib, 0, mu, L, act, i["adv"], i["old"], ENT)
        assert got["lp"].tobytes() == g0["lp"].tobytes(), f"Aa {Aa} m {m}: lp"
        assert got["grad"][:, :Aa].tobytes() == g1["grad"].tobytes(), f"Aa {Aa} m {m}: mean gradient"
        assert got["counts"] == (0, m * Aa)
        args = (z, i["act"], i["adv"], i["old"], EPS, ENT, LS_MIN, LS_MAX)
        ref, b = sd.head_f64(*args), sd.head_bounds(*args)
        terms = np.abs(ref["grad"][:, Aa:]) + ENT / m
        bound = 2 * b["grad"][:, Aa:].sum(axis=0) + (m + 2) * U * terms.sum(axis=0)
        err = np.abs(got["grad"][:, Aa:].astype(F64).sum(axis=0) - g1["gls"].astype(F64))
        assert (err <= bound).all(), f"Aa {Aa} m {m}: log σ column sums {err} vs {bound}"
    no_error(lib)


# -------------------------------------------------------------------------------------------- 3. sampler
def run_sampler(lib, z, key, offset, lo=LS_MIN, hi=LS_MAX):
    m, A = z.shape
    d = dict(z=dev(lib, z), act=dev(lib, np.full((m, A), np.nan, F32)), lp=empty(lib, m))
    try:
        assert lib.ppo_gauss_sd_sample_device(d["z"].ptr, m, A, lo, hi, key, offset, d["act"].ptr, d["lp"].ptr) == 0
        return d["act"].to_numpy(F32, m * A).reshape(m, A), d["lp"].to_numpy(F32, m)
    finally:
        for a in d.values():
            a.free()


@pytest.mark.parametrize("Aa", sd.HEAD_AA)
def test_sampler(lib, Aa):
    """a = μ + normal·expf(ls) with rng_ref's normals at counter e·Aa + j (the fp32 normal's and expf's rounding:
    8·2⁻²⁴ relative on the noise term plus the sum's), zeros after the action, the log-prob the head's bits on the
    same (z, action), repeatable under (key, offset), different under another offset."""
    m, key, off = 300, 0x1234ABCD5678, 77
    z = sd.smallest_covering(Aa, m)["z"]
    act, lp = run_sampler(lib, z, key, off)
    assert (act[:, Aa:].view(np.uint32) == 0).all()
    cnt = (np.arange(m, dtype=U64)[:, None] * U64(Aa) + np.arange(Aa, dtype=U64)[None, :])
    n = rng_ref.normal_at(cnt, U64(off), U64(key))
    n32 = rng_ref.normal_at(cnt, U64(off), U64(key), F32)
    ls = sd.clamp(z[:, Aa:].astype(F64), LS_MIN, LS_MAX)[0]
    noise = n * np.exp(ls)
    want = z[:, :Aa].astype(F64) + noise
    # the normal: test_gpu_rng.py's rule — four times what numpy's own fp32 evaluation of Box–Muller misses the
    # float64 one by, at least 4 ulps of the largest draw; then expf (2 ulp), the product and the sum
    n_tol = max(4.0 * float(np.abs(n32.astype(F64) - n).max()), 4.0 * float(np.spacing(F32(np.abs(n).max()))))
    bound = (n_tol + 8 * U * np.abs(n)) * np.exp(ls) + 2 * U * np.abs(want)
    assert (np.abs(act[:, :Aa] - want) <= bound).all()
    head = run_head(lib, dict(z=z, act=act, adv=np.ones(m, F32), old=lp))
    assert head["lp"].tobytes() == lp.tobytes()
    act2, lp2 = run_sampler(lib, z, key, off)
    assert act2.tobytes() == act.tobytes() and lp2.tobytes() == lp.tobytes()
    act3, _ = run_sampler(lib, z, key, off + 1)
    assert (act3[:, :Aa] != act[:, :Aa]).mean() > 0.99
    no_error(lib)


# ------------------------------------------------------------------------- 4. determinism and isolation
@pytest.mark.parametrize("Aa", [3, 32])
def test_deterministic_and_nan_isolated(lib, Aa):
    m = 300
    i = sd.smallest_covering(Aa, m)
    a, b = run_head(lib, i), run_head(lib, i)
    for k in ("grad", "lp", "H"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["loss"] == b["loss"] and a["counts"] == b["counts"]
    z = np.array(i["z"])
    z[131, 0] = np.nan                                   # a mean: the row's lp, its gradient and the loss
    c = run_head(lib, dict(z=z, act=i["act"], adv=i["adv"], old=i["old"]))
    keep = np.arange(m) != 131
    assert c["grad"][keep].tobytes() == a["grad"][keep].tobytes()
    assert c["lp"][keep].tobytes() == a["lp"][keep].tobytes() and c["H"].tobytes() == a["H"].tobytes()
    assert np.isnan(c["lp"][131]) and np.isnan(c["loss"]) and c["counts"] == a["counts"]
    no_error(lib)


# ------------------------------------------------------------------------------------------- 5. exact KL
@pytest.mark.parametrize("Aa", sd.HEAD_AA)
def test_exact_kl_rows(lib, Aa):
    m = 300
    rng = np.random.default_rng(70 + Aa)
    zo = sd.smallest_covering(Aa, m)["z"]
    zn = (zo + rng.normal(scale=0.3, size=zo.shape)).astype(F32)
    rows = rng.permutation(m).astype(np.int32)

    def run(new, old, r):
        d = dict(n=dev(lib, new), o=dev(lib, old), r=dev(lib, r) if r is not None else None, k=empty(lib, m, F64))
        try:
            mean = C.c_double(np.nan)
            assert lib.ppo_gauss_sd_kl_exact_device(d["n"].ptr, d["o"].ptr, d["r"].ptr if r is not None else None, m,
                                                    2 * Aa, LS_MIN, LS_MAX, d["k"].ptr, C.byref(mean)) == 0
            return d["k"].to_numpy(F64, m), mean.value
        finally:
            for a in d.values():
                if a is not None:
                    a.free()

    got, mean = run(zn, zo, rows)
    want = sd.kl_rows_f64(zo[rows], zn, LS_MIN, LS_MAX)
    assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, want)).all()
    assert abs(mean - want.mean()) <= 1e-6 * max(1.0, want.mean())      # the sum leaves through an fp32 word
    same, mean0 = run(zo, zo, None)
    assert (same == 0).all() and mean0 == 0
    # clamping on both sides: moving a raw log σ further outside the bounds changes nothing
    far_o, far_n = np.array(zo), np.array(zn)
    far_o[:, Aa:][zo[:, Aa:] > LS_MAX] += 3
    far_n[:, Aa:][zn[:, Aa:] < LS_MIN] -= 3
    again, _ = run(far_n, far_o, rows)
    assert again.tobytes() == got.tobytes()
    no_error(lib)


# -------------------------------------------------------------------------------------------- 6. setter
def make(lib, sizes, acts, cap, ent=0.01):
    C.CDLL("libc.so.6").srand(3)
    return lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), cap, 3e-4, 1e-3, 0.95, 0.2, ent,
                          1.0, True)


def test_setter(lib):
    ppo = make(lib, [3, 16, 4], ["relu", "none"], 64)
    odd = make(lib, [3, 16, 5], ["relu", "none"], 64)
    wide = make(lib, [3, 16, 66], ["relu", "none"], 64)
    try:
        out = (C.c_float * 2)(9, 9)
        assert lib.ppo_get_action_gaussian_sd(ppo, out) == 0 and lib.ppo_get_action_dist(ppo) == 0
        for lo, hi in ((float("nan"), 1), (-1, float("nan")), (1, 1), (2, 1), (-21, 1), (-1, 21)):
            assert lib.ppo_set_action_gaussian_sd(ppo, lo, hi) == -1 and lib.ppo_get_action_dist(ppo) == 0
        assert lib.ppo_set_action_gaussian_sd(None, -20, 2) == -1
        assert lib.ppo_set_action_gaussian_sd(odd, -20, 2) == -1 and lib.ppo_set_action_gaussian_sd(wide, -20, 2) == -1
        assert lib.ppo_set_action_gaussian_sd(ppo, -20, 2) == 0
        assert lib.ppo_get_action_dist(ppo) == 3 and lib.ppo_get_action_gaussian_sd(ppo, out) == 1
        assert (out[0], out[1]) == (-20.0, 2.0) and lib.ppo_get_action_gaussian_sd(ppo, None) == 1
        assert lib.ppo_set_action_gaussian_sd(ppo, 3, 1) == -1 and lib.ppo_get_action_gaussian_sd(ppo, out) == 1
        assert (out[0], out[1]) == (-20.0, 2.0)
        assert lib.ppo_set_action_mask(ppo, 1) == -1 and lib.ppo_set_action_dist(ppo, 3) == -1
        assert lib.ppo_set_compute_dtype(ppo, 1) == -1
        for dist in (0, 1):
            assert lib.ppo_set_action_dist(ppo, dist) == 0 and lib.ppo_get_action_dist(ppo) == dist
            assert lib.ppo_get_action_gaussian_sd(ppo, out) == 0
            assert lib.ppo_set_action_gaussian_sd(ppo, -5, 1) == 0 and lib.ppo_get_action_dist(ppo) == 3
        assert lib.ppo_set_action_dist(ppo, 0) == 0
        assert lib.ppo_set_compute_dtype(ppo, 1) == 0
        assert lib.ppo_set_action_gaussian_sd(ppo, -20, 2) == -1 and lib.ppo_get_action_dist(ppo) == 0
        # the test entries decline bad arguments before any launch
        assert lib.ppo_gauss_sd_head_device(None, None, None, None, 1, 2, -1.0, 1.0, 0.2, 0.0, None, None, None, None,
                                            None) == -1
        assert lib.ppo_gauss_sd_sample_device(None, 1, 2, -1.0, 1.0, 0, 0, None, None) == -1
        assert lib.ppo_gauss_sd_kl_exact_device(None, None, None, 1, 2, -1.0, 1.0, None, None) == -1
        no_error(lib)
    finally:
        for p in (ppo, odd, wide):
            lib.free_ppo(p)


# ----------------------------------------------------------------------------------------- 10. checkpoint
def test_checkpoint_resume(lib, tmp_path):
    E, T, B = 8, 16, 64
    sizes, acts = [3, 32, 32, 2], ["relu", "relu", "none"]

    def one_round(p, r):
        lib.ppo_rollout_device(p, E, T, 0, 41)
        lib.ppo_update(p, 0.99, B, 2, 2, 1, 17 + r)

    x = make(lib, sizes, acts, E * T)
    plain = make(lib, sizes, acts, E * T)
    y = None
    try:
        h_plain = lib.ppo_state_hash(plain, 1)
        assert lib.ppo_set_action_gaussian_sd(plain, -20, 2) == 0 and lib.ppo_state_hash(plain, 1) != h_plain
        assert lib.ppo_set_action_dist(plain, 0) == 0 and lib.ppo_state_hash(plain, 1) == h_plain
        assert lib.ppo_set_action_gaussian_sd(x, -2.0, 0.5) == 0
        one_round(x, 0)
        path = str(tmp_path / "sd.ckpt").encode()
        assert lib.ppo_save_state(x, path, 1) == 0
        err = C.create_string_buffer(256)
        y = lib.ppo_load_state(path, err, 256)
        assert y, err.value
        out = (C.c_float * 2)()
        assert lib.ppo_get_action_dist(y) == 3 and lib.ppo_get_action_gaussian_sd(y, out) == 1
        assert (out[0], out[1]) == (-2.0, 0.5)
        assert lib.ppo_state_hash(y, 1) == lib.ppo_state_hash(x, 1)
        one_round(x, 1)
        one_round(y, 1)
        assert lib.ppo_state_hash(y, 1) == lib.ppo_state_hash(x, 1) != 0
        assert lib.ppo_param_hash(y) == lib.ppo_param_hash(x)
        no_error(lib)
    finally:
        for p in (x, plain, y):
            if p:
                lib.free_ppo(p)
