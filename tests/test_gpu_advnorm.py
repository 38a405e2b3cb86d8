"""Per-minibatch advantage normalisation on the GPU (ppo_ext.h ppo_set_adv_norm; csrc/advnorm.hip; DESIGN.md §4
"Per-minibatch advantage normalisation").

1. the kernel alone, bit for bit against tests/advnorm_ref.py (outputs and the (m, sd) pairs), in place and out of
   place, with guard words around every array;
2. the update reads what the kernel wrote: every policy step's advantages are advnorm_ref of the buffer's advantages
   at that step's rows, the history and ppo_read_stats out[29..31] agree, and with the mode global the same entry
   returns the plain gathered values;
3. one policy step end to end against a float64 model of the same MLP and head fed the normalised advantages, within
   twice the error the same comparison shows with the feature off (Gaussian, categorical, bf16 mode);
4. nothing changes by default; 5. composition with the other options, graph replay and the single-workgroup shape;
6. checkpoints; 7. loopback data parallelism.
"""
import ctypes as C
import struct

import numpy as np
import pytest

import advnorm_ref as an
import categorical_ref as cr
import ppo_ffi
import tanh_ref
from helpers import nn_grads_packed, nn_input_rows, nn_params_packed

pytestmark = pytest.mark.gpu
F32, F64, U32 = np.float32, np.float64, np.uint32
GAMMA, EPS, ENT = 0.99, 0.2, 0.01
GLOBAL, MINIBATCH = 0, 1
GUARD, G = 0xDEADBEEF, 3           # three guard words: the arrays behind them are 4-byte, not 16-byte, aligned


def make(lib, sizes, acts, cap, seed=3, ent=ENT):
    C.CDLL("libc.so.6").srand(seed)
    return lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), cap, 3e-4, 1e-3, 0.95, EPS, ent,
                          1.0, True)


def stats(lib, ppo, n=32):
    st = (C.c_double * n)()
    lib.ppo_read_stats(ppo, st, n)
    return list(st)


def no_error(lib):
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


def same_bits(got, want, what):
    """bit for bit, except that any NaN equals any NaN (its payload is not part of the definition)"""
    got, want = np.ascontiguousarray(got, F32).ravel(), np.ascontiguousarray(want, F32).ravel()
    assert got.shape == want.shape, what
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), f"{what}: NaNs at other places"
    bad = (got.view(U32) != want.view(U32)) & ~ng
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {int(np.argmax(bad))}: "
                           f"{got[np.argmax(bad)]!r} vs {want[np.argmax(bad)]!r}")


# ----------------------------------------------------------------------------------------- 1. the kernel alone
SHAPES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 4099]
SEGS = [1, 3, 37]
KINDS = ["normal", "offset", "constant", "nan"]


def kernel_data(kind, n_seg, B, rng):
    x = rng.standard_normal((n_seg, B)).astype(F32)
    if kind == "offset":                 # mean 1e4, std 1e-3: an fp32 or single-pass shortcut loses sd
        x = (1e4 + 1e-3 * rng.standard_normal((n_seg, B))).astype(F32)
    elif kind == "constant":             # one constant segment
        x[n_seg // 2] = F32(0.7)
    elif kind == "nan":                  # one NaN, between clean neighbours where there are any
        x[n_seg // 2, B // 2] = np.nan
    return x


def guarded(lib, n, fill=None):
    """a device array of n floats between G guard words on either side → (DeviceArray, pointer to the n floats)"""
    host = np.full(n + 2 * G, GUARD, U32)
    if fill is not None:
        host[G:G + n] = np.ascontiguousarray(fill, F32).ravel().view(U32)
    d = ppo_ffi.DeviceArray.from_numpy(lib, host)
    return d, d.ptr + 4 * G


def read_guarded(d, n, what):
    host = d.to_numpy(U32, n + 2 * G)
    assert (host[:G] == GUARD).all() and (host[G + n:] == GUARD).all(), f"{what}: a guard word was written"
    return host[G:G + n].view(F32)


@pytest.fixture(scope="module")
def kernel_refs():
    """advnorm_ref of every (B, n_seg, kind), computed once: {(B, n_seg, kind): (x, y, stats)}"""
    out = {}
    for B in SHAPES:
        for n_seg in SEGS:
            for k, kind in enumerate(KINDS):
                x = kernel_data(kind, n_seg, B, np.random.default_rng(1000 * B + 10 * n_seg + k))
                y, st = an.normalize(x, B)
                out[B, n_seg, kind] = (x, y, st)
    return out


@pytest.mark.parametrize("B", SHAPES)
def test_kernel_bit_for_bit(lib, kernel_refs, B):
    for n_seg in SEGS:
        for kind in KINDS:
            x, y_ref, st_ref = kernel_refs[B, n_seg, kind]
            n = n_seg * B
            for in_place in (True, False):
                what = f"B={B} n_seg={n_seg} {kind} {'in place' if in_place else 'out of place'}"
                d_in, p_in = guarded(lib, n, x)
                d_out, p_out = (d_in, p_in) if in_place else guarded(lib, n)
                d_st, p_st = guarded(lib, 2 * n_seg)
                assert lib.ppo_adv_normalize_device(p_in, p_out, n_seg, B, p_st) == 0, what
                no_error(lib)
                same_bits(read_guarded(d_out, n, what), y_ref, what)
                same_bits(read_guarded(d_st, 2 * n_seg, what + " stats"), st_ref, what + " (m, sd)")
                if not in_place:
                    same_bits(read_guarded(d_in, n, what + " input"), x, what + ": the input was written")
                    d_out.free()
                d_in.free()
                d_st.free()
    if B == 65:      # the edge cases by value: a constant segment is 0, a NaN stays inside its segment
        x, y, st = kernel_refs[65, 3, "constant"]
        assert not y[1].any() and st[1, 1] == 0
        x, y, st = kernel_refs[65, 3, "nan"]
        assert np.isnan(y[1]).all() and np.isfinite(y[0]).all() and np.isfinite(y[2]).all()


def test_kernel_arguments(lib):
    d, p = guarded(lib, 8, np.arange(8))
    assert lib.ppo_adv_normalize_device(None, p, 1, 8, None) == -1
    assert lib.ppo_adv_normalize_device(p, None, 1, 8, None) == -1
    assert lib.ppo_adv_normalize_device(p, p, 0, 8, None) == -1
    assert lib.ppo_adv_normalize_device(p, p, 1, 0, None) == -1
    assert lib.ppo_adv_normalize_device(p, p, 2, 4, None) == 0           # stats may be NULL
    y, _ = an.normalize(np.arange(8, dtype=F32), 4)
    same_bits(read_guarded(d, 8, "no stats"), y, "no stats")
    d.free()
    no_error(lib)


# ----------------------------------------------------------------------------------------- 2. the update reads it
SMALL = dict(sizes=[3, 8, 8, 2], acts=["relu", "relu", "none"], N=256, B=64)
SEED = 23


def small_ppo(lib, mode, sizes=None, seed=3):
    p = make(lib, sizes or SMALL["sizes"], SMALL["acts"], SMALL["N"], seed)
    if sizes and sizes[-1] == 3:
        assert lib.ppo_set_action_dist(p, 1) == 0
    if mode is not None:
        assert lib.ppo_set_adv_norm(p, mode) == 0 and lib.ppo_get_adv_norm(p) == mode
    lib.ppo_fill_synthetic(p, 4, SMALL["N"] // 4, 99, 1.0 / 100)
    return p


def read_step(lib, ppo, step, B):
    rows, adv = np.full(B, -1, np.int32), np.full(B, np.nan, F32)
    got = lib.ppo_adv_norm_read(ppo, step, rows.ctypes.data_as(C.POINTER(C.c_int)),
                                adv.ctypes.data_as(C.POINTER(C.c_float)), B)
    return got, rows, adv


def history(lib, ppo, n):
    out = np.full(2 * n, np.nan, F32)
    steps = lib.ppo_adv_norm_history(ppo, out.ctypes.data_as(C.POINTER(C.c_float)), n)
    return steps, out.reshape(n, 2)


def buffer_adv(lib, ppo, N):
    return ppo_ffi.d2h(lib, ppo.contents.buffer.contents.d_advantage_p, F32, N)


def check_steps(lib, ppo, N, B, steps):
    """check 2: every step's advantages are advnorm_ref of the buffer's at its rows; history and out[29..31] agree"""
    adv_buf = buffer_adv(lib, ppo, N)
    n_hist, hist = history(lib, ppo, steps)
    assert n_hist == steps
    sds = []
    for s in range(steps):
        got, rows, adv = read_step(lib, ppo, s, B)
        assert got == B and rows.min() >= 0 and rows.max() < N
        y, m, sd = an.normalize_segment(adv_buf[rows])
        same_bits(adv, y, f"step {s}: the head's advantages")
        same_bits(hist[s], [m, sd], f"step {s}: (m, sd)")
        sds.append(float(sd))
    per = N // B
    for e in range(steps // per):       # every whole epoch visits every row once
        rows = np.concatenate([read_step(lib, ppo, e * per + k, B)[1] for k in range(per)])
        assert np.array_equal(np.sort(rows), np.arange(N))
    st = stats(lib, ppo)
    assert st[29] == MINIBATCH and st[30] == min(sds) and st[31] == max(sds)
    assert stats(lib, ppo, 29) == st[:29]                  # callers passing n <= 29 see no change
    return adv_buf


def test_update_reads_the_normalised_segments(lib, monkeypatch):
    N, B = SMALL["N"], SMALL["B"]
    monkeypatch.delenv("PPO_NO_TINY", raising=False)
    p = small_ppo(lib, MINIBATCH)
    lib.ppo_reset_stats(p)
    lib.ppo_update(p, GAMMA, B, 2, 1, 1, SEED)
    lib.ppo_synchronize()
    no_error(lib)
    st = stats(lib, p)
    assert st[3] == 2 * (N // B) and st[1] == N // B and st[8] == 0
    adv_buf = check_steps(lib, p, N, B, 2 * (N // B))
    # the buffer's array is GAE's global normalisation, untouched: mean 0, population std 1
    assert abs(float(adv_buf.astype(F64).mean())) < 1e-6 and abs(float(adv_buf.astype(F64).std()) - 1) < 1e-5
    # bad arguments
    assert read_step(lib, p, -1, B)[0] == -1 and read_step(lib, p, 2 * (N // B), B)[0] == -1
    assert read_step(lib, p, 0, B - 1)[0] == -1
    steps, _ = history(lib, p, 1)                           # a short array is filled as far as it goes
    assert steps == 2 * (N // B)
    lib.free_ppo(p)

    # the mode global (the multi-launch loop forced, which keeps its gather): the plain gathered values, no history
    monkeypatch.setenv("PPO_NO_TINY", "1")
    q = small_ppo(lib, None)
    lib.ppo_update(q, GAMMA, B, 2, 1, 1, SEED)
    lib.ppo_synchronize()
    adv_buf = buffer_adv(lib, q, N)
    for s in range(2 * (N // B)):
        got, rows, adv = read_step(lib, q, s, B)
        assert got == B
        same_bits(adv, adv_buf[rows], f"step {s}, mode global")
    assert history(lib, q, 8)[0] == 0
    assert stats(lib, q)[29:32] == [0, 0, 0]
    no_error(lib)
    lib.free_ppo(q)


def test_setter(lib):
    p = make(lib, SMALL["sizes"], SMALL["acts"], SMALL["N"])
    assert lib.ppo_get_adv_norm(p) == GLOBAL
    assert lib.ppo_set_adv_norm(p, MINIBATCH) == 0 and lib.ppo_get_adv_norm(p) == MINIBATCH
    for bad in (-1, 2, 1 << 20):
        assert lib.ppo_set_adv_norm(p, bad) == -1 and lib.ppo_get_adv_norm(p) == MINIBATCH
    assert lib.ppo_set_adv_norm(p, GLOBAL) == 0 and lib.ppo_get_adv_norm(p) == GLOBAL
    assert read_step(lib, p, 0, 64)[0] == -1 and history(lib, p, 4)[0] == 0      # no update has run
    lib.free_ppo(p)


# ----------------------------------------------------------------------------------------- 3. one policy step
def rel_l2(got, ref):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def one_policy_step(lib, mode, sizes, dtype):
    """one ppo_update capped at one policy step → the relative L2 errors of μ's gradients and of ∂/∂log σ against
    the float64 model fed the advantages the mode prescribes"""
    N, B, acts = SMALL["N"], SMALL["B"], SMALL["acts"]
    cat = sizes[-1] == 3
    p = small_ppo(lib, mode, sizes, seed=7)
    if dtype:
        assert lib.ppo_set_compute_dtype(p, dtype) == 0
    pol = p.contents.policy.contents
    b = p.contents.buffer.contents
    S, A = sizes[0], sizes[-1]
    mu0 = nn_params_packed(lib, pol.mu)
    ls0 = ppo_ffi.d2h(lib, pol.d_log_std, F32, A)
    lib.ppo_set_step_limit(p, 0, 1)
    lib.ppo_update(p, GAMMA, B, 1, 0, 1, SEED)
    lib.ppo_synchronize()
    no_error(lib)
    got, rows, adv_dev = read_step(lib, p, 0, B)
    assert got == B and stats(lib, p)[3] == 1
    state = ppo_ffi.d2h(lib, b.d_state_p, F32, N * S).reshape(N, S)
    act = ppo_ffi.d2h(lib, b.d_action_p, F32, N * A).reshape(N, A)
    old = ppo_ffi.d2h(lib, b.d_logprob_p, F32, N)
    adv = buffer_adv(lib, p, N)[rows]
    if not dtype:                         # the rows the entry reports are the rows μ's forward read
        np.testing.assert_array_equal(nn_input_rows(lib, pol.mu, B), state[rows])
    adv_in = an.normalize_segment(adv)[0] if mode == MINIBATCH else adv
    same_bits(adv_dev, adv_in, "the head's advantages")
    g_dev = nn_grads_packed(lib, pol.mu)
    gls_dev = ppo_ffi.d2h(lib, pol.d_log_std_grad, F32, A)
    if cat:
        hs, _ = tanh_ref.forward(sizes, acts, mu0, state[rows])
        head = cr.head_f64(hs[-1], act[rows], adv_in, old[rows], EPS, ENT)
        g_ref = tanh_ref.backward(sizes, acts, mu0, hs, head["grad"])[0]
        assert not gls_dev.any()          # a discrete policy leaves log σ's gradient zero
        e_ls = 0.0
    else:
        g_ref, gls_ref, _ = tanh_ref.policy_grads(sizes, acts, mu0, ls0, state[rows], act[rows], adv_in, old[rows],
                                                  EPS, ENT)
        e_ls = rel_l2(gls_dev, gls_ref)
    lib.ppo_set_step_limit(p, -1, -1)
    lib.free_ppo(p)
    return rel_l2(g_dev, g_ref), e_ls


@pytest.mark.parametrize("case", ["gaussian", "categorical", "bf16"])
def test_one_policy_step_end_to_end(lib, monkeypatch, case):
    """[3, 8, 8, A] ReLU, 256 rows, B = 64, device shuffle, one policy step; the error is ‖device − model‖₂/‖model‖₂
    over μ's packed gradients, and likewise over ∂/∂log σ.  The floor is the same comparison with the mode global on
    the multi-launch loop — the parent commit's behaviour — and the feature-on error may be twice it.
    Measured on an MI355X (floor → feature on):
        gaussian     μ 2.45e-07 → 2.60e-07,  log σ 1.54e-07 → 7.63e-08
        categorical  μ 1.85e-07 → 1.89e-07   (log σ's gradient is zero on both sides)
        bf16         μ 0.117 → 0.115,        log σ 2.68e-03 → 2.76e-03
    The bf16 floor is that large because the model is exact float64: at width 8 a hidden pre-activation that bf16
    rounding moves across zero flips a ReLU mask bit and with it a whole row's share of a gradient of few terms."""
    monkeypatch.setenv("PPO_NO_TINY", "1")         # both runs on the multi-launch loop
    sizes = [3, 8, 8, 3] if case == "categorical" else SMALL["sizes"]
    dtype = 1 if case == "bf16" else 0
    floor_mu, floor_ls = one_policy_step(lib, GLOBAL, sizes, dtype)
    on_mu, on_ls = one_policy_step(lib, MINIBATCH, sizes, dtype)
    print(f"{case}: relative L2 error of μ's gradients: floor {floor_mu:.3g}, feature on {on_mu:.3g}; "
          f"of log σ's: floor {floor_ls:.3g}, feature on {on_ls:.3g}")
    assert floor_mu > 0 and on_mu <= 2 * floor_mu
    assert on_ls <= 2 * floor_ls


# ----------------------------------------------------------------------------------------- 4. off means off
PEND = dict(sizes=[3, 32, 32, 1], acts=["relu", "relu", "none"], E=8, T=16, B=32)


def pendulum(lib, mode=None, every_option=False):
    p = make(lib, PEND["sizes"], PEND["acts"], PEND["E"] * PEND["T"])
    if every_option:
        assert lib.ppo_set_obs_norm(p, 10.0) == 0 and lib.ppo_set_reward_norm(p, 10.0) == 0
        assert lib.ppo_set_max_grad_norm(p, 0.5) == 0 and lib.ppo_set_value_clip(p, 0.2) == 0
        assert lib.ppo_set_target_kl(p, 0.05) == 0
    if mode is not None:
        assert lib.ppo_set_adv_norm(p, mode) == 0
    return p


def pendulum_rounds(lib, p, n):
    for _ in range(n):
        lib.ppo_rollout_device(p, PEND["E"], PEND["T"], 0, 41)
        lib.ppo_update(p, GAMMA, PEND["B"], 2, 2, 1, 17)
    lib.ppo_synchronize()
    no_error(lib)


def test_nothing_changes_by_default(lib, monkeypatch):
    """Passes with and without the feature: a PPO that never set the mode, one that set it to minibatch and back
    (where the setter exists) and a second untouched one end two updates with equal parameter and state hashes."""
    monkeypatch.delenv("PPO_NO_TINY", raising=False)
    monkeypatch.delenv("PPO_GRAPH", raising=False)
    never, toggled, again = pendulum(lib), pendulum(lib), pendulum(lib)
    if hasattr(lib, "ppo_set_adv_norm"):
        assert lib.ppo_set_adv_norm(toggled, MINIBATCH) == 0 and lib.ppo_set_adv_norm(toggled, GLOBAL) == 0
    h0 = lib.ppo_state_hash(never, 1)
    assert h0 == lib.ppo_state_hash(again, 1) == lib.ppo_state_hash(toggled, 1) != 0
    for p in (never, toggled, again):
        pendulum_rounds(lib, p, 2)
    assert lib.ppo_param_hash(never) == lib.ppo_param_hash(toggled) == lib.ppo_param_hash(again)
    assert lib.ppo_state_hash(never, 1) == lib.ppo_state_hash(toggled, 1) == lib.ppo_state_hash(again, 1) != h0
    n = lib.ppo_state_image(never, 0, None, 0)
    img = C.create_string_buffer(n)
    assert lib.ppo_state_image(never, 0, img, n) == n
    assert struct.unpack_from("<I", img.raw, 12)[0] & 8 == 0          # no advantage-normalisation flag
    for p in (never, toggled, again):
        lib.free_ppo(p)


# ----------------------------------------------------------------------------------------- 5. composition
def finite_params(lib, p):
    c = p.contents
    return all(np.isfinite(nn_params_packed(lib, nn)).all() for nn in (c.V, c.policy.contents.mu))


def test_composition_with_every_option(lib, monkeypatch):
    monkeypatch.delenv("PPO_GRAPH", raising=False)
    a, b = pendulum(lib, MINIBATCH, True), pendulum(lib, MINIBATCH, True)
    off = pendulum(lib, GLOBAL, True)
    for p in (a, b, off):
        pendulum_rounds(lib, p, 3)
    assert finite_params(lib, a)
    assert lib.ppo_param_hash(a) == lib.ppo_param_hash(b) != lib.ppo_param_hash(off)
    st = stats(lib, a)
    assert st[29] == MINIBATCH and 0 < st[30] <= st[31] and st[8] == 0
    assert stats(lib, off)[29:32] == [0, 0, 0]
    for p in (a, b, off):
        lib.free_ppo(p)


def test_graph_replay_falls_back_to_eager_steps(lib, monkeypatch):
    """[17, 256, 256, 6], B = 64 under PPO_GRAPH=1 (the shape test_gpu_update.py replays; the cluster phases set
    aside): with the mode global the steps replay from graphs (out[8] > 0), with it minibatch none does and check 2
    holds."""
    monkeypatch.setenv("PPO_GRAPH", "1")
    monkeypatch.setenv("PPO_GRAPH_STEPS", "16")
    monkeypatch.setenv("PPO_NO_CLUSTER", "1")
    N, B = 1024, 64
    out8 = {}
    for mode in (GLOBAL, MINIBATCH):
        p = make(lib, [17, 256, 256, 6], SMALL["acts"], N, seed=21)
        assert lib.ppo_set_adv_norm(p, mode) == 0
        lib.ppo_fill_synthetic(p, 4, N // 4, 17, 1.0 / 200)
        lib.ppo_reset_stats(p)
        lib.ppo_update(p, GAMMA, B, 1, 1, 1, SEED)
        lib.ppo_synchronize()
        no_error(lib)
        out8[mode] = stats(lib, p)[8]
        if mode == MINIBATCH:
            check_steps(lib, p, N, B, N // B)
        else:
            assert read_step(lib, p, 0, B)[0] == -1        # a replayed update keeps no gather
        lib.free_ppo(p)
    assert out8[GLOBAL] > 0 and out8[MINIBATCH] == 0


def test_single_workgroup_shape_takes_the_loop(lib, monkeypatch):
    """[3, 64, 64, 1] at B = 64 is the single-workgroup phases' shape: with the mode minibatch the update runs the
    multi-launch loop, check 2 holds, and the result differs from the mode global's."""
    monkeypatch.delenv("PPO_NO_TINY", raising=False)
    monkeypatch.delenv("PPO_GRAPH", raising=False)
    N, B = 1024, 64
    hashes = {}
    for mode in (GLOBAL, MINIBATCH):
        p = make(lib, [3, 64, 64, 1], SMALL["acts"], N, seed=21)
        assert lib.ppo_set_adv_norm(p, mode) == 0
        lib.ppo_fill_synthetic(p, 4, N // 4, 17, 1.0 / 200)
        lib.ppo_reset_stats(p)
        lib.ppo_update(p, GAMMA, B, 1, 2, 1, SEED)
        lib.ppo_synchronize()
        no_error(lib)
        st = stats(lib, p)
        assert st[1] == 2 * (N // B) and st[3] == N // B and st[8] == 0
        if mode == MINIBATCH:
            check_steps(lib, p, N, B, N // B)
        else:
            assert read_step(lib, p, 0, B)[0] == -1        # the single-workgroup phases gather for themselves
        hashes[mode] = lib.ppo_param_hash(p)
        lib.free_ppo(p)
    assert hashes[GLOBAL] != hashes[MINIBATCH]


# ----------------------------------------------------------------------------------------- 6. checkpoint
def sections(img):
    """[(tag, payload)] of a checkpoint image (the container of DESIGN.md §4 "Training-state checkpoints")"""
    count = struct.unpack_from("<I", img, 16)[0]
    pos, out = 20, []
    for _ in range(count):
        tag, _, n, _ = struct.unpack_from("<IIQQ", img, pos)
        out.append((tag, img[pos + 24:pos + 24 + n]))
        pos += 24 + ((n + 7) & ~7)
    assert pos == len(img)
    return out


def test_checkpoint_keeps_the_mode(lib, tmp_path):
    x = pendulum(lib, MINIBATCH)
    pendulum_rounds(lib, x, 1)
    path = str(tmp_path / "advnorm.ckpt").encode()
    assert lib.ppo_save_state(x, path, 0) == 0
    img = open(path, "rb").read()
    assert struct.unpack_from("<I", img, 12)[0] & 8
    assert (8, struct.pack("<II", MINIBATCH, 0)) in sections(img)
    err = C.create_string_buffer(256)
    y = lib.ppo_load_state(path, err, 256)
    assert y, err.value
    assert lib.ppo_get_adv_norm(y) == MINIBATCH
    assert lib.ppo_state_hash(y, 0) == lib.ppo_state_hash(x, 0) != 0
    pendulum_rounds(lib, x, 1)
    pendulum_rounds(lib, y, 1)
    assert lib.ppo_param_hash(x) == lib.ppo_param_hash(y)
    assert lib.ppo_state_hash(x, 1) == lib.ppo_state_hash(y, 1)
    assert history(lib, y, 1)[0] == 2 * (PEND["E"] * PEND["T"] // PEND["B"])      # the loaded PPO normalised
    # a damaged mode is declined on the host, with a message
    at = img.index(struct.pack("<IIQ", 8, 0, 8)) + 24
    bad = bytearray(img)
    bad[at:at + 4] = struct.pack("<I", 2)
    fnv = 0xcbf29ce484222325
    for byte in bad[at:at + 8]:
        fnv = ((fnv ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    bad[at - 8:at] = struct.pack("<Q", fnv)
    (tmp_path / "bad.ckpt").write_bytes(bytes(bad))
    assert not lib.ppo_load_state(str(tmp_path / "bad.ckpt").encode(), err, 256)
    assert b"advantage-normalisation mode" in err.value
    no_error(lib)
    lib.free_ppo(x)
    lib.free_ppo(y)


# ----------------------------------------------------------------------------------------- 7. loopback ranks
def test_loopback_replicas(lib, monkeypatch):
    """Two in-process ranks (PPO_COMM_LOOPBACK=2): one update with the mode minibatch, each rank normalising its own
    shard; the replica check passes and the normalisation adds no collective."""
    monkeypatch.setenv("PPO_NO_TINY", "1")
    monkeypatch.setenv("PPO_COMM_LOOPBACK", "2")
    assert lib.ppo_comm_init(0, 1, None) == 0, lib.ppo_last_error()
    try:
        assert lib.ppo_comm_world() == 2
        N, B = 1024, 256
        comm = {}
        for mode in (GLOBAL, MINIBATCH):
            p = make(lib, [17, 64, 64, 6], SMALL["acts"], N, seed=1234)
            assert lib.ppo_set_adv_norm(p, mode) == 0
            lib.ppo_fill_synthetic(p, 4, N // 4, 99, 1.0 / 500)
            lib.ppo_prof_enable(1)
            lib.ppo_prof_reset()
            lib.ppo_update(p, GAMMA, B, 1, 1, 1, SEED)
            lib.ppo_synchronize()
            cnt = (C.c_long * 7)()
            lib.ppo_prof_counts(cnt)
            lib.ppo_prof_enable(0)
            no_error(lib)
            assert lib.ppo_comm_check_replicas(p) == 0
            comm[mode] = cnt[5]
            if mode == MINIBATCH:
                check_steps(lib, p, N, B, N // B)
            lib.free_ppo(p)
        assert comm[GLOBAL] == comm[MINIBATCH] > 0
    finally:
        lib.ppo_comm_finalize()
        monkeypatch.delenv("PPO_COMM_LOOPBACK")
