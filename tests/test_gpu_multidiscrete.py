"""The multi-discrete policy on the device (ppo_set_action_multidiscrete; csrc/discrete.hip) against
tests/multidiscrete_ref.py: the head row by row, D = 1 against the categorical head bit for bit, the sampler, a
whole update, bit-identity with the categorical policy through the whole library, the synthetic rollout, the open
rollout and the argument handling.  Every bound comes from multidiscrete_ref / categorical_ref (derived from the
rounding of the listed operations and validated by the fp32 mirror on the CPU in test_multidiscrete_cpu.py);
nothing is taken from a run of the kernels."""
import ctypes as C

import numpy as np
import pytest

import categorical_ref as cr
import kl_ref
import multidiscrete_ref as md
import ppo_ffi
import tanh_ref
from categorical_ref import ENT, EPS, F32, F64, U
from helpers import dev, empty, gemm_tol, nn_grads_packed, nn_input_rows, nn_params_packed
from test_gpu_update import adam_first_step, assert_adam_delta

pytestmark = pytest.mark.gpu


def no_error(lib):
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


def set_md(lib, ppo, nvec):
    assert lib.ppo_set_action_multidiscrete(ppo, ppo_ffi.c_ints(nvec), len(nvec)) == 0
    assert lib.ppo_get_action_dist(ppo) == 2


def run_head(lib, i, nvec, ent=ENT):
    m, A = i["z"].shape
    d = dict(z=dev(lib, i["z"]), act=dev(lib, i["act"]), adv=dev(lib, i["adv"]), old=dev(lib, i["old"]),
             g=empty(lib, m * A), lp=empty(lib, m), H=empty(lib, m))
    try:
        loss = C.c_double(np.nan)
        rc = lib.ppo_multidiscrete_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, m, A,
                                               ppo_ffi.c_ints(nvec), len(nvec), EPS, ent, d["g"].ptr, d["lp"].ptr,
                                               d["H"].ptr, C.byref(loss))
        assert rc == 0
        return dict(grad=d["g"].to_numpy(F32, m * A).reshape(m, A), lp=d["lp"].to_numpy(F32, m),
                    H=d["H"].to_numpy(F32, m), loss=loss.value)
    finally:
        for a in d.values():
            a.free()


def run_cat_head(lib, i, ent=ENT):
    m, A = i["z"].shape
    d = dict(z=dev(lib, i["z"]), act=dev(lib, i["act"]), adv=dev(lib, i["adv"]), old=dev(lib, i["old"]),
             g=empty(lib, m * A), lp=empty(lib, m), H=empty(lib, m))
    try:
        loss = C.c_double(np.nan)
        assert lib.ppo_categorical_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, m, A, EPS, ent,
                                               d["g"].ptr, d["lp"].ptr, d["H"].ptr, C.byref(loss)) == 0
        return dict(grad=d["g"].to_numpy(F32, m * A).reshape(m, A), lp=d["lp"].to_numpy(F32, m),
                    H=d["H"].to_numpy(F32, m))
    finally:
        for a in d.values():
            a.free()


def check_head(lib, i, nvec, what):
    m = i["z"].shape[0]
    args = (i["z"], i["act"], i["adv"], i["old"], EPS, ENT, nvec)
    ref, b = md.head_f64(*args), md.head_bounds(*args)
    got = run_head(lib, i, nvec)
    skip = cr.near_clip(ref["ratio"])
    assert skip.mean() <= 0.01 and not skip.any(), what       # the cap, and these inputs contain none
    live = ~skip & (i["adv"] != 0)
    # with ent_coeff > 0 a clipped row keeps its entropy term: the branch shows in the first term alone
    first = run_head(lib, i, nvec, ent=0.0)["grad"]
    np.testing.assert_array_equal((~(first != 0).any(axis=1))[live], ref["clipped"][live], err_msg=what)
    assert (got["grad"] != 0).any(axis=1)[live & ~ref["clipped"]].all(), what
    for name in ("lp", "H", "grad"):
        err = np.abs(got[name].astype(F64) - ref[name])[~skip]
        ratio = float((err / b[name][~skip]).max())
        print(f"{what}: {name} error / bound {ratio:.3f}")
        assert (err <= b[name][~skip]).all(), f"{what}: {name} at {ratio:.3g} of the bound"
    bound = md.loss_bound(ref, b, m, ENT)
    print(f"{what}: loss error / bound {abs(got['loss'] - ref['loss']) / bound:.3f}")
    assert abs(got["loss"] - ref["loss"]) <= bound, f"{what}: loss {got['loss']} vs {ref['loss']} ± {bound}"


ids = lambda nv: f"{nv[0]}x{len(nv)}-A{sum(nv)}"        # noqa: E731


# ------------------------------------------------------------------------------------------ 1. head rows
@pytest.mark.parametrize("nvec", md.HEAD_NVEC, ids=ids)
def test_head_rows(lib, nvec):
    """lp, H and every element of ∂loss/∂logits within head_bounds of the float64 model, the loss within
    loss_bound, at m ∈ {1, 63, 64, 257}; row 0 (D >= 2) has a flat and a peaked component, on which a head that took
    the row's H for H_d is far outside the gradient bound (test_multidiscrete_cpu.py asserts it); the clip branch per
    row from a second run at ent_coeff = 0."""
    full = md.head_inputs(nvec)
    for m in md.HEAD_M:
        check_head(lib, md.rows_of(full, m), nvec, f"nvec {ids(nvec)} m {m}")
    no_error(lib)


@pytest.mark.parametrize("nvec", md.HEAD_NVEC_WIDE, ids=ids)
def test_head_rows_wide(lib, nvec):
    """D at the cap and components up to the head's limit, 5 rows."""
    check_head(lib, md.head_inputs(nvec, 5), nvec, f"nvec {ids(nvec)} m 5")
    no_error(lib)


# ------------------------------------------------------------------------------------ 2. D = 1 is dist 1
@pytest.mark.parametrize("A", [2, 3, 17, 32, 33, 257])
def test_one_component_is_categorical(lib, A):
    """nvec = {A}: for A <= 32 lp, H and the gradient are the categorical head's bits; above, within the bounds."""
    i = cr.head_inputs(A)
    got, cat = run_head(lib, i, [A]), run_cat_head(lib, i)
    if A <= 32:
        for name in ("lp", "H", "grad"):
            assert got[name].tobytes() == cat[name].tobytes(), f"A {A}: {name}"
    else:
        args = (i["z"], i["act"], i["adv"], i["old"], EPS, ENT)
        ref, b = cr.head_f64(*args), cr.head_bounds(*args)
        for name in ("lp", "H", "grad"):
            assert (np.abs(got[name].astype(F64) - ref[name]) <= b[name]).all(), f"A {A}: {name}"
    no_error(lib)


# -------------------------------------------------------------------------------------------- 3. sampler
def run_sampler(lib, z, nvec, key, offset):
    m, A = z.shape
    d = dict(z=dev(lib, z), act=dev(lib, np.full((m, A), np.nan, F32)), lp=empty(lib, m))
    try:
        assert lib.ppo_multidiscrete_sample_device(d["z"].ptr, m, A, ppo_ffi.c_ints(nvec), len(nvec), key, offset,
                                                   d["act"].ptr, d["lp"].ptr) == 0
        return d["act"].to_numpy(F32, m * A).reshape(m, A), d["lp"].to_numpy(F32, m)
    finally:
        for a in d.values():
            a.free()


def test_sampler_one_component(lib):
    """nvec = {6}: action and log-prob are the categorical sampler's bits under the same key and offset."""
    z = cr.sample_inputs(6)
    m = z.shape[0]
    act, lp = run_sampler(lib, z, [6], cr.SAMPLE_KEY, cr.SAMPLE_OFFSET)
    d = dict(z=dev(lib, z), act=dev(lib, np.full((m, 6), np.nan, F32)), lp=empty(lib, m))
    assert lib.ppo_categorical_sample_device(d["z"].ptr, m, 6, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET, d["act"].ptr,
                                             d["lp"].ptr) == 0
    assert act.tobytes() == d["act"].to_numpy(F32, m * 6).tobytes()
    assert lp.tobytes() == d["lp"].to_numpy(F32, m).tobytes()
    for a in d.values():
        a.free()
    no_error(lib)


def test_sampler(lib):
    """D = 9, 65 536 rows: every index equals the mirror's wherever the threshold is further from a cumulative
    boundary than the bound (under 1 % per component may differ), columns D … A−1 are +0, the joint log-prob of the
    stored indices is within the lp bound."""
    nvec = md.SAMPLE_NVEC
    A, D = sum(nvec), len(nvec)
    z = md.sample_inputs(nvec)
    m = z.shape[0]
    act, lp = run_sampler(lib, z, nvec, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET)
    a_ref, _, margin = md.sample_f32(z, md.sample_u(m, D, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET), nvec)
    near = md.near_boundary(margin, nvec)
    assert (near.mean(axis=0) < 0.01).all()
    a = act[:, :D].astype(np.int64)
    assert (act[:, :D] == a).all() and a.min() >= 0 and (a.max(axis=0) <= np.asarray(nvec) - 1).all()
    assert not act[:, D:].any() and not np.signbit(act[:, D:]).any()
    np.testing.assert_array_equal(a[~near], a_ref[~near])
    zero = np.zeros(m)
    ref = md.head_f64(z, act, zero, zero, EPS, 0.0, nvec)
    b = md.head_bounds(z, act, zero, zero, EPS, 0.0, nvec)
    err = np.abs(lp.astype(F64) - ref["lp"])
    print(f"{int((a != a_ref).sum())} indices differ from the mirror ({int(near.sum())} near a boundary); "
          f"lp error / bound {float((err / b['lp']).max()):.3f}")
    assert (err <= b["lp"]).all()
    no_error(lib)


def test_sampler_joint_frequencies(lib):
    """nvec = [6, 3], every row the same logits: the 18 joint cell frequencies within 5 standard deviations of
    m·p_a·p_b — the two components draw independently."""
    nvec = [6, 3]
    z = md.sample_inputs(tuple(nvec), shared_row=True)
    m = z.shape[0]
    act, _ = run_sampler(lib, z, nvec, cr.SAMPLE_KEY, cr.SAMPLE_OFFSET)
    p = md.head_f64(z[:1], np.zeros((1, 9)), np.zeros(1), np.zeros(1), EPS, 0.0, nvec)["p"][0]
    cell = np.outer(p[:6], p[6:]).reshape(-1)
    freq = np.bincount(act[:, 0].astype(np.int64) * 3 + act[:, 1].astype(np.int64), minlength=18) / m
    assert (np.abs(freq - cell) <= 5 * np.sqrt(cell * (1 - cell) / m)).all(), (freq, cell)


# ---------------------------------------------------------------------- 4. one policy step, a short update
SIZES, NVEC, N, B, SEED = [5, 16, 9], [3, 4, 2], 256, 64, 11
ACTS = ["relu", "none"]


def make_ppo(lib, sizes=SIZES, n=N, ent_coeff=ENT, nvec=NVEC, seed=5):
    C.CDLL("libc.so.6").srand(seed)
    ppo = lib.create_ppo(ppo_ffi.c_strings(ACTS), ppo_ffi.c_ints(sizes), len(sizes), n, 3e-4, 3e-4, 0.95, EPS,
                         ent_coeff, 1.0, True)
    if nvec is not None:
        set_md(lib, ppo, nvec)
    return ppo


def update(lib, ppo, steps):
    lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 100)
    lib.ppo_reset_stats(ppo)
    lib.ppo_set_step_limit(ppo, 0, steps)
    lib.ppo_update(ppo, 0.99, B, 1, 0, 1, SEED)
    lib.ppo_synchronize()


def read_buffer(lib, ppo):
    b = ppo.contents.buffer.contents
    S, A = SIZES[0], SIZES[-1]
    return dict(state=ppo_ffi.d2h(lib, b.d_state_p, F32, N * S).reshape(N, S),
                act=ppo_ffi.d2h(lib, b.d_action_p, F32, N * A).reshape(N, A),
                old=ppo_ffi.d2h(lib, b.d_logprob_p, F32, N), adv=ppo_ffi.d2h(lib, b.d_advantage_p, F32, N))


def model_step(params, buf, rows, ent):
    hs, _ = tanh_ref.forward(SIZES, ACTS, params, buf["state"][rows])
    head = md.head_f64(hs[-1].astype(F32), buf["act"][rows], buf["adv"][rows], buf["old"][rows], EPS, ent, NVEC)
    return tanh_ref.backward(SIZES, ACTS, params, hs, head["grad"])[0], head, hs[-1]


@pytest.mark.parametrize("engine", [0, 1])
def test_whole_update(lib, oracle, engine):
    """A fresh {5, 16, 9} PPO with nvec = [3, 4, 2], buffer 256, batch 64, filled by ppo_fill_synthetic; ppo_update
    capped at one policy step, on both fp32 GEMM engines: μ's gradient is the float64 head's pushed through the
    restated backward (gemm_tol at K = B), the parameters Adam's first step of it (test_gpu_update's bound), log σ
    untouched, out[4] the mean joint row entropy within the H bound (plus the forward's GEMM tolerance on the
    logits), and the buffer holds D index columns then zeros."""
    prev = lib.ppo_gemm_f32_engine(engine)
    try:
        one = make_ppo(lib)
        mu = one.contents.policy.contents.mu
        mu0 = nn_params_packed(lib, mu)
        pol = one.contents.policy.contents
        ls0 = ppo_ffi.d2h(lib, pol.d_log_std, F32, pol.action_size)
        update(lib, one, 1)
        buf = read_buffer(lib, one)
        a = buf["act"][:, :3]
        assert (a == a.astype(int)).all() and a.min() >= 0 and (a.max(axis=0) == np.array(NVEC) - 1).all()
        assert not buf["act"][:, 3:].any()
        lr = 3e-4
        r1 = oracle.feistel_perm(N, oracle.splitmix64(SEED))[:B]
        np.testing.assert_array_equal(nn_input_rows(lib, mu, B), buf["state"][r1])
        g1, head1, z1 = model_step(mu0, buf, r1, ENT)
        got_g1 = nn_grads_packed(lib, mu)
        assert np.abs(got_g1 - g1).max() <= gemm_tol(g1, B)
        mu1 = nn_params_packed(lib, mu)
        flips = assert_adam_delta(mu1, adam_first_step(mu0, g1, lr), g1, lr, "step 1")
        assert flips <= max(2, mu1.size // 1000)
        assert ppo_ffi.d2h(lib, pol.d_log_std, F32, pol.action_size).tobytes() == ls0.tobytes()
        st = (C.c_double * 5)()
        lib.ppo_read_stats(one, st, 5)
        mirror = md.head_f32(z1.astype(F32), buf["act"][r1], buf["adv"][r1], buf["old"][r1], EPS, ENT, NVEC)
        Hm = float(mirror["H"].astype(F64).mean())
        b1 = md.head_bounds(z1.astype(F32), buf["act"][r1], buf["adv"][r1], buf["old"][r1], EPS, ENT, NVEC)
        # the device's logits differ from the restated ones by the forward's GEMM error: |∂H/∂z| ≤ |log p| + H_d per
        # column, over A columns
        dz = gemm_tol(z1, SIZES[1])
        Hmax = np.log(np.array(NVEC, F64)).sum()
        slack = (B + 2) * U * Hmax + b1["H"].mean() + 9 * dz * (np.abs(np.log(head1["p"])).max() + np.log(4))
        assert st[3] == 1 and abs(st[4] - Hm) <= slack, (st[4], Hm, slack)
        no_error(lib)
        lib.free_ppo(one)
    finally:
        lib.ppo_gemm_f32_engine(prev)


def test_update_kl(lib, oracle):
    """With ppo_set_target_kl(+inf): ppo_kl_history is the model's k3 estimator on the JOINT lp at both steps
    (test_gpu_categorical's derivation of the bound, with the joint lp's bound)."""
    lib.ppo_gemm_tune(-1, 1)
    try:
        one, ppo = make_ppo(lib), make_ppo(lib)
        mu0 = nn_params_packed(lib, ppo.contents.policy.contents.mu)
        for p in (one, ppo):
            assert lib.ppo_set_target_kl(p, float("inf")) == 0
        update(lib, one, 1)
        update(lib, ppo, 2)
    finally:
        lib.ppo_gemm_tune(-1, 0)
    hist = (C.c_double * 4)()
    assert lib.ppo_kl_history(ppo, hist, 4) == 2
    buf = read_buffer(lib, ppo)
    mu1 = nn_params_packed(lib, one.contents.policy.contents.mu)
    assert (mu1 != mu0).any()
    perm = oracle.feistel_perm(N, oracle.splitmix64(SEED))
    for k, params in enumerate((mu0, mu1)):
        r = perm[k * B:(k + 1) * B]
        _, head, z = model_step(params, buf, r, ENT)
        want = kl_ref.approx_kl(head["lp"], buf["old"][r])
        lp_err = (md.head_bounds(z.astype(F32), buf["act"][r], buf["adv"][r], buf["old"][r], EPS, ENT, NVEC)["lp"].max()
                  + 2 * len(NVEC) * (gemm_tol(z, SIZES[1]) + U * np.abs(z).max()))
        x = head["lp"] - buf["old"][r].astype(F64)
        bound = np.abs(np.expm1(x)).max() * lp_err + lp_err ** 2 + U * want + 1e-12
        print(f"kl step {k + 1}: device {hist[k]:.6e} model {want:.6e} error / bound {abs(hist[k] - want) / bound:.3f}")
        assert abs(hist[k] - want) <= bound, (k, hist[k], want, bound)
    no_error(lib)
    lib.free_ppo(one)
    lib.free_ppo(ppo)


# --------------------------------------------------------------- 5. bit-identity through the whole library
def rollout_and_update(lib, sizes, kind, E, T, setup):
    import test_gpu_rng

    n = E * T
    C.CDLL("libc.so.6").srand(21)
    ppo = lib.create_ppo(ppo_ffi.c_strings(ACTS), ppo_ffi.c_ints(sizes), 3, n, 3e-4, 3e-4, 0.95, EPS, ENT, 1.0, True)
    setup(ppo)
    lib.ppo_rollout_device(ppo, E, T, kind, 17)
    lib.ppo_update(ppo, 0.99, 64, 2, 2, 1, SEED)
    lib.ppo_synchronize()
    buf = test_gpu_rng.read_buffer(lib, ppo, n, sizes[0], sizes[-1])
    st = (C.c_double * 16)()
    assert lib.ppo_episode_stats(ppo, st, 16) == 16
    out = ({k: v.tobytes() for k, v in buf.items()}, np.array(st[:]).tobytes(), lib.ppo_param_hash(ppo))
    lib.free_ppo(ppo)
    return out


@pytest.mark.parametrize("case", [("cartpole", [4, 16, 2], 2, [2]), ("synthetic", [5, 16, 6], 1, [6])],
                         ids=lambda c: c[0])
def test_one_component_through_the_library(lib, case):
    """E = 8, T = 32, the same seed and the same srand: one ppo_rollout_device plus one ppo_update leave the same
    buffers, episode statistics and parameter hash under dist 1 and under nvec = {A}."""
    _, sizes, kind, nvec = case
    lib.ppo_gemm_tune(-1, 1)
    try:
        cat = rollout_and_update(lib, sizes, kind, 8, 32, lambda p: lib.ppo_set_action_dist(p, 1))
        one = rollout_and_update(lib, sizes, kind, 8, 32, lambda p: set_md(lib, p, nvec))
    finally:
        lib.ppo_gemm_tune(-1, 0)
    for name in cat[0]:
        assert cat[0][name] == one[0][name], name
    assert cat[1] == one[1] and cat[2] == one[2]
    no_error(lib)


# --------------------------------------------------------------------------------- 6. synthetic rollout
def test_synthetic_rollout(lib, oracle):
    """ppo_rollout_device(kind 1) with nvec = [3, 4]: every step re-simulated from the stored (state, action) —
    element j reads c_{j mod D} = 2·a_d/(n_d − 1) − 1, the reward's action term is −0.01·(Σ c_d²)/D, which is
    rng_ref.synth_step under the D-column action c; the indices are the sampler mirror's under the policy-noise
    stream; the log-prob is the joint one; a fresh twin's evaluation reproduces the episode statistics bit for bit;
    deterministic evaluation takes the per-component argmax."""
    import rng_ref as R
    from test_gpu_rng import assert_transcendental, by_step
    from test_gpu_rng import read_buffer as read_rollout

    sizes, nvec, E, T, seed = [5, 16, 7], [3, 4], 64, 48, 13
    S, A, D, n = sizes[0], sizes[-1], 2, E * T
    ppo, twin = (make_ppo(lib, sizes, n, 0.0, nvec, seed=8) for _ in range(2))
    lib.ppo_rollout_device(ppo, E, T, 1, seed)
    lib.ppo_synchronize()
    buf = read_rollout(lib, ppo, n, S, A)
    g = np.arange(T)
    obs, act = by_step(buf["state"], E, T), by_step(buf["action"], E, T)
    idx = act[:, :, :D].astype(np.int64)
    assert (act[:, :, :D] == idx).all() and idx.min() >= 0 and not act[:, :, D:].any()
    assert [len(np.unique(idx[:, :, d])) for d in range(D)] == nvec
    c = md.synth_centres(idx, nvec)
    n64, r64, done, reset = R.synth_step(obs, c, g, seed, F64)
    n32, r32, _, _ = R.synth_step(obs, c, g, seed, F32)
    nxt, rew = by_step(buf["next_state"], E, T), by_step(buf["reward"], E, T)
    assert_transcendental(nxt, n64, n32, "multi-discrete synthetic next_state", magnitudes=(1.0,))
    assert_transcendental(rew, r64, r32, "multi-discrete synthetic reward")
    np.testing.assert_array_equal(by_step(buf["term"], E, T).astype(bool), done)
    follow = np.where(done[:, :, None], reset, nxt)
    assert (obs[1:].view(np.uint32) == follow[:-1].view(np.uint32)).all()
    # the sampler inside the rollout: logits restated from the stored observations
    params = nn_params_packed(lib, ppo.contents.policy.contents.mu)
    z = tanh_ref.forward(sizes, ACTS, params, obs.reshape(-1, S))[0][-1]
    dz = gemm_tol(z, sizes[1]) + U * np.abs(z).max()
    key = R.rollout_key(seed)
    u = np.concatenate([md.sample_u(E, D, key, cr.K_NOISE + int(t)) for t in g])            # [T·E, D], step-major
    a_ref, _, margin = md.sample_f32(z.astype(F32), u, nvec)
    near = margin <= 2 * (np.asarray(nvec, F64)[None, :] + 70) * U + 2 * U + 2 * np.expm1(2 * dz)
    assert (near.mean(axis=0) <= 0.01).all()
    np.testing.assert_array_equal(idx.reshape(-1, D)[~near], a_ref[~near])
    a_rows = act.reshape(-1, A)
    zero = np.zeros(n)
    ref = md.head_f64(z.astype(F32), a_rows, zero, zero, EPS, 0.0, nvec)
    lp_b = md.head_bounds(z.astype(F32), a_rows, zero, zero, EPS, 0.0, nvec)["lp"] + 2 * D * dz
    assert (np.abs(by_step(buf["logprob"], E, T).reshape(-1).astype(F64) - ref["lp"]) <= lp_b).all()
    # evaluation of a fresh twin: the same trajectory
    st = (C.c_double * 16)()
    assert lib.ppo_episode_stats(ppo, st, 16) == 16
    ev = (C.c_double * 9)()
    assert lib.ppo_eval_device(twin, E, T, 1, seed, 0, 0.99, ev, 9) == 9
    assert np.array(ev[:8]).tobytes() == np.array(st[8:16]).tobytes()
    # deterministic evaluation writes the per-component argmax: with the logits forced to (−100, 100, −100 | 100,
    # −100, −100, −100) on every row the sampler draws (1, 0) with certainty (the other e_k are 0 in fp32), so the
    # sampled and the deterministic evaluation walk one trajectory; other peaks walk another
    mu = twin.contents.policy.contents.mu.contents
    last = mu.layers[mu.num_layers - 2]
    ppo_ffi.h2d(lib, last.d_weights, np.zeros((A, sizes[1]), F32))

    def evaluate(peaks, deterministic):
        bias = np.full(A, -100, F32)
        bias[[peaks[0], 3 + peaks[1]]] = 100
        ppo_ffi.h2d(lib, last.d_biases, bias)
        assert lib.ppo_eval_device(twin, E, T, 1, seed, deterministic, 0.99, ev, 9) == 9
        return np.array(ev[:]).tobytes()

    assert evaluate((1, 0), 1) == evaluate((1, 0), 0)
    assert evaluate((2, 3), 1) == evaluate((2, 3), 0) != evaluate((1, 0), 1)
    assert evaluate((1, 1), 1) != evaluate((1, 0), 1)          # the second component acts too (c² = 1/9 against 1)
    no_error(lib)
    lib.free_ppo(ppo)
    lib.free_ppo(twin)


# -------------------------------------------------------------------------------------- 7. open rollout
def test_open_rollout_and_act(lib):
    """Under the multi-discrete policy ppo_rollout_act and ppo_act_device agree bit for bit at the same seed and
    step on the same observations; deterministic = 1 gives the per-component argmax, lowest index on ties."""
    sizes, nvec, E, T, seed = [5, 16, 7], [3, 4], 40, 2, 29
    S, A = sizes[0], sizes[-1]
    ppo = make_ppo(lib, sizes, E * T, 0.0, nvec, seed=9)
    obs = np.random.default_rng(3).uniform(-1, 1, (E, S)).astype(F32)
    d_obs, d_act, d_act2, d_lp = dev(lib, obs), empty(lib, E * A), empty(lib, E * A), empty(lib, E)
    assert lib.ppo_rollout_begin(ppo, E, T, d_obs.ptr, seed) == 0
    step = lib.ppo_rollout_act(ppo, d_act.ptr)
    assert step >= 0
    lib.ppo_synchronize()
    b = ppo.contents.buffer.contents
    rows = np.arange(E) * T
    lp_buf = ppo_ffi.d2h(lib, b.d_logprob_p, F32, E * T)[rows]
    act = d_act.to_numpy(F32, E * A).reshape(E, A)
    assert lib.ppo_act_device(ppo, d_obs.ptr, E, 0, seed, step, d_act2.ptr, d_lp.ptr) == 0
    lib.ppo_synchronize()
    assert d_act2.to_numpy(F32, E * A).tobytes() == act.tobytes()
    assert d_lp.to_numpy(F32, E).tobytes() == lp_buf.tobytes()
    assert (act[:, :2] == act[:, :2].astype(int)).all() and not act[:, 2:].any()
    assert len(np.unique(act[:, 0])) > 1 and len(np.unique(act[:, 1])) > 1
    # deterministic, with ties forced: logits (0, 1, 1 | 2, 0, 2, 1) on every row → (1, 0)
    mu = ppo.contents.policy.contents.mu.contents
    last = mu.layers[mu.num_layers - 2]
    ppo_ffi.h2d(lib, last.d_weights, np.zeros((A, sizes[1]), F32))
    ppo_ffi.h2d(lib, last.d_biases, np.array([0, 1, 1, 2, 0, 2, 1], F32))
    assert lib.ppo_act_device(ppo, d_obs.ptr, E, 1, seed, step, d_act2.ptr, None) == 0
    lib.ppo_synchronize()
    want = np.tile(np.array([1, 0, 0, 0, 0, 0, 0], F32), (E, 1))
    assert d_act2.to_numpy(F32, E * A).tobytes() == want.tobytes()
    no_error(lib)
    for a in (d_obs, d_act, d_act2, d_lp):
        a.free()
    lib.free_ppo(ppo)


# -------------------------------------------------------------------------------------- 8. off means off
def test_off_means_off(lib):
    """Multi-discrete set and dist 0 restored: the parameter hashes before and after a Gaussian update equal those
    of a PPO never touched."""
    hashes = []
    for mode in ("never", "toggle"):
        ppo = make_ppo(lib, nvec=None)
        if mode == "toggle":
            set_md(lib, ppo, NVEC)
            assert lib.ppo_set_action_dist(ppo, 0) == 0 and lib.ppo_get_action_dist(ppo) == 0
            assert lib.ppo_get_action_nvec(ppo, None, 0) == 0
        h0 = lib.ppo_param_hash(ppo)
        lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 100)
        lib.ppo_gemm_tune(-1, 1)                               # atomic-free gradient products: bit-reproducible
        try:
            lib.ppo_update(ppo, 0.99, B, 2, 2, 1, SEED)
        finally:
            lib.ppo_gemm_tune(-1, 0)
        hashes.append((h0, lib.ppo_param_hash(ppo)))
        lib.free_ppo(ppo)
    assert hashes[0] == hashes[1] and hashes[0][0] != hashes[0][1]
    no_error(lib)


# ----------------------------------------------------------------------------------------- 9. arguments
def test_arguments(lib):
    C.CDLL("libc.so.6").srand(1)
    mk = lambda sizes: lib.create_ppo(ppo_ffi.c_strings(ACTS), ppo_ffi.c_ints(sizes), 3, 64, 3e-4, 3e-4, 0.95, EPS,  # noqa: E731
                                      0.0, 1.0, True)
    setm = lambda q, nv, D=None: lib.ppo_set_action_multidiscrete(q, ppo_ffi.c_ints(nv), len(nv) if D is None else D)  # noqa: E731
    p = mk([4, 16, 9])
    out = (C.c_int * 4)()
    assert lib.ppo_get_action_nvec(p, out, 4) == 0 and lib.ppo_get_action_nvec(None, out, 4) == 0
    assert lib.ppo_set_action_multidiscrete(None, ppo_ffi.c_ints([9]), 1) == -1
    assert lib.ppo_set_action_multidiscrete(p, None, 1) == -1
    for nv, D in (([9], 0), ([9], -1), ([9], 257), ([8, 1], None), ([3, 4], None), ([3, 4, 3], None),
                  ([2, 2, 2, 2, 2], None), ([10, -1], None)):
        assert setm(p, nv, D) == -1 and lib.ppo_get_action_dist(p) == 0, nv
    assert lib.ppo_set_action_dist(p, 2) == -1 and lib.ppo_get_action_dist(p) == 0
    wide = mk([4, 16, 4098])                                   # A above the head's bound
    assert setm(wide, [2049, 2049]) == -1 and lib.ppo_get_action_dist(wide) == 0
    # accepted; a refused call leaves the setting as it was; the query with a small cap
    assert setm(p, [3, 4, 2]) == 0 and lib.ppo_get_action_dist(p) == 2
    assert setm(p, [3, 4, 3]) == -1 and lib.ppo_get_action_dist(p) == 2
    out[:] = [-7] * 4
    assert lib.ppo_get_action_nvec(p, out, 2) == 3 and list(out) == [3, 4, -7, -7]
    assert lib.ppo_get_action_nvec(p, out, 4) == 3 and list(out) == [3, 4, 2, -7]
    assert lib.ppo_set_action_dist(p, 2) == -1 and lib.ppo_get_action_dist(p) == 2
    # bf16, both orders
    assert lib.ppo_set_compute_dtype(p, 1) == -1 and lib.ppo_get_action_dist(p) == 2
    assert lib.ppo_set_action_dist(p, 1) == 0 and lib.ppo_get_action_dist(p) == 1
    assert lib.ppo_get_action_nvec(p, out, 4) == 0
    assert lib.ppo_set_action_dist(p, 0) == 0 and lib.ppo_set_compute_dtype(p, 1) == 0
    assert setm(p, [3, 4, 2]) == -1 and lib.ppo_get_action_dist(p) == 0
    assert lib.ppo_set_compute_dtype(p, 0) == 0 and setm(p, [9]) == 0 and lib.ppo_get_action_dist(p) == 2
    # the CartPole shape rule through the status-returning evaluation
    ev_out = (C.c_double * 9)()
    ev = lambda q: lib.ppo_eval_device(q, 4, 5, 2, 1, 0, 0.99, ev_out, 9)  # noqa: E731
    cp = mk([4, 16, 2])
    assert ev(cp) == -1                                        # Gaussian
    assert setm(cp, [2]) == 0 and ev(cp) == 9                  # nvec = {2}: accepted
    s3, a4 = mk([3, 16, 2]), mk([4, 16, 4])
    assert setm(s3, [2]) == 0 and ev(s3) == -1
    assert setm(a4, [2, 2]) == 0 and ev(a4) == -1
    # the test entries
    d = empty(lib, 64)
    loss = C.c_double(0)
    head = lambda z, m, A, nv, D, eps=EPS: lib.ppo_multidiscrete_head_device(  # noqa: E731
        z, d.ptr, d.ptr, d.ptr, m, A, nv, D, eps, 0.0, d.ptr, d.ptr, d.ptr, C.byref(loss))
    ok = ppo_ffi.c_ints([2, 2])
    assert head(None, 4, 4, ok, 2) == -1 and head(d.ptr, 0, 4, ok, 2) == -1 and head(d.ptr, 4, 4, None, 2) == -1
    assert head(d.ptr, 4, 5, ok, 2) == -1 and head(d.ptr, 4, 4, ok, 0) == -1 and head(d.ptr, 4, 4, ok, 257) == -1
    assert head(d.ptr, 4, 4, ppo_ffi.c_ints([3, 1]), 2) == -1 and head(d.ptr, 4, 4, ok, 2, float("nan")) == -1
    assert head(d.ptr, 4, 4098, ppo_ffi.c_ints([2049, 2049]), 2) == -1
    samp = lambda z, m, A, nv, D, act=d.ptr: lib.ppo_multidiscrete_sample_device(z, m, A, nv, D, 1, 0, act, d.ptr)  # noqa: E731
    assert samp(None, 4, 4, ok, 2) == -1 and samp(d.ptr, 0, 4, ok, 2) == -1 and samp(d.ptr, 4, 4, None, 2) == -1
    assert samp(d.ptr, 4, 5, ok, 2) == -1 and samp(d.ptr, 4, 4, ok, 2, None) == -1
    d.free()
    no_error(lib)
    for q in (p, wide, cp, s3, a4):
        lib.free_ppo(q)
