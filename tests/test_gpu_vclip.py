"""PPO2 value-loss clipping in the device update (ppo_set_value_clip, csrc/vclip.h) in every form of the value
head: the plain MSE kernel, the fused output layer (fp32 and bf16 storage), the folded head as its own kernel and
the head carried by the x3 grad_W launch.

The oracle has no such option: the reference is tests/vclip_ref.py (pinned against torch in test_vclip_cpu.py).
Its fp32 model mirrors the device function operation for operation, so the head is teacher-forced: the model
runs on the GPU's own network output y, and the clipped count must then be exact, the loss equal within fp32
summation and the network's gradients those of the oracle's mlp_backward fed the model's g under the GPU's ReLU
masks.  Old values are supplied by buffer row with N = 2·B, NaN outside the minibatch's rows: a head that
indexed them by minibatch slot would read NaN (which counts as inside) and miss the count.

bf16 storage (form "bf16"): the GEMMs round their operands to bf16, so assert_gemm_close's fp32 bound cannot
hold for the network gradients by the number format (2^-8 per operand); that form is pinned with the bf16
suite's own teacher-forced check (test_gpu_production.check_bf16_layers: every kernel within a bf16 rounding of
fp32 accumulation, the head gradient entering rounded to bf16) and against the fp32 oracle within its 3e-2 bound.
"""
import ctypes as C

import numpy as np
import pytest

import ppo_ffi
from helpers import F32, assert_gemm_close, dev, empty, gpu_relu_masks, nn_grads_packed, nn_params_packed, \
    oracle_grads_with_masks
from bf16_ref import bf16
from test_gpu_production import RELU, check_bf16_layers, close
from test_gpu_update import make_ppo
from vclip_ref import vclip_f32, vclip_f64

pytestmark = pytest.mark.gpu

EPS_V = 0.2
SEED = 77
NSTAT = 19


def stats(lib, ppo, n=NSTAT):
    st = (C.c_double * n)()
    lib.ppo_read_stats(ppo, st, n)
    return list(st)


# ----------------------------------------------------------------------------- 1. the head alone
def head(lib, y, v_old, rows, t, eps):
    m = y.size
    dy, dv, dt, dg = dev(lib, y), dev(lib, v_old), dev(lib, t), empty(lib, m)
    dr = dev(lib, rows.astype(np.int32)) if rows is not None else None
    out = (C.c_double * 3)()
    assert lib.ppo_value_clip_head_device(dy.ptr, dv.ptr, dr.ptr if dr else None, dt.ptr, m, eps, dg.ptr, out) == 0
    g = dg.to_numpy(F32, m)
    for d in (dy, dv, dt, dg, dr):
        if d:
            d.free()
    return g, list(out)


@pytest.mark.parametrize("m,N", [(1, 1), (1000, 1000), (4096, 10000)])
def test_head_bit_for_bit(lib, m, N):
    rng = np.random.default_rng(100 + m)
    y, t = rng.normal(size=m).astype(F32), rng.normal(size=m).astype(F32)
    v_all = rng.normal(size=N).astype(F32)
    rows = rng.permutation(N)[:m] if N > m else None
    v_rows = v_all[rows] if rows is not None else v_all
    if m == 1:
        y[0], t[0], v_all[0], v_rows = 2.0, 1.75, 1.0, v_all        # outside, lc > lu: clipped
    g, out = head(lib, y, v_all, rows, t, EPS_V if m > 1 else 0.25)
    l, g_ref, c = vclip_f32(y, t, v_rows, EPS_V if m > 1 else 0.25)
    np.testing.assert_array_equal(g.view(np.uint32), g_ref.view(np.uint32))
    assert out[1] == c.sum() and out[2] == m
    assert m == 1 or 0.1 < c.mean() < 0.9
    loss64, _, c64 = vclip_f64(y, t, v_rows, float(F32(EPS_V if m > 1 else 0.25)))
    assert (c64 == c).all()
    print(f"m = {m}: loss {out[0]:.9g} vs float64 {loss64:.9g}, clipped {int(out[1])}")
    assert abs(out[0] - loss64) <= 1e-6 * loss64


def test_head_edge_cases(lib):
    e = 0.25
    #            |d| == eps   lu == lc   clipped   NaN y    inside
    y = np.array([1.25, -1.25, 2.0, 2.0, np.nan, 0.5], F32)
    v = np.array([1.0, -1.0, 1.0, 1.0, 0.0, 0.4], F32)
    t = np.array([1.75, -1.75, 1.625, 1.75, 0.0, 3.0], F32)
    g, out = head(lib, y, v, None, t, e)
    l, g_ref, c = vclip_f32(y, t, v, e)
    assert c.tolist() == [False, False, False, True, False, False]
    np.testing.assert_array_equal(g.view(np.uint32), g_ref.view(np.uint32))
    assert np.isnan(g[4]) and g[3] == 0 and out[1] == 1 and out[2] == 6 and np.isnan(out[0])
    # eps_v huge: the plain MSE gradient bit for bit, nothing clipped
    rng = np.random.default_rng(5)
    y, t, v = (rng.normal(size=1000).astype(F32) for _ in range(3))
    for big in (3e38, float("inf")):
        g, out = head(lib, y, v, None, t, big)
        np.testing.assert_array_equal(g, F32(2) * (y - t) / F32(1000))
        assert out[1] == 0 and out[2] == 1000
    # bad arguments
    d = dev(lib, y)
    o = (C.c_double * 3)()
    assert lib.ppo_value_clip_head_device(d.ptr, d.ptr, None, d.ptr, 0, 0.2, d.ptr, o) == -1
    assert lib.ppo_value_clip_head_device(None, d.ptr, None, d.ptr, 4, 0.2, d.ptr, o) == -1
    assert lib.ppo_value_clip_head_device(d.ptr, d.ptr, None, d.ptr, 4, float("nan"), d.ptr, o) == -1
    d.free()


# ----------------------------------------------------------------------------- 2. one value step per head form
FORMS = {
    # name: (policy sizes, B, environment, compute dtype)
    "fold_carried": ([64, 256, 6], 2048, {}, 0),                    # the folded layer is layer 0; head carried
    # two hidden layers, 64×64 forward / grad_x tiles; nn_value_fold_ok needs the x3 engine, which takes
    # minibatches above 1024 rows (neural_network.c use_x3): 1028 rows also leave ragged row tiles
    "fold_64x64": ([17, 256, 256, 6], 1028, {}, 0),
    "fold_head_kernel": ([376, 512, 512, 512, 17], 131072, {}, 0),  # no LDS room: value_head_kernel runs first
    "out_head": ([64, 256, 6], 2048, {"PPO_VALUE_FOLD": "0"}, 0),
    "plain": ([64, 256, 6], 2048, {"PPO_VALUE_FOLD": "0", "PPO_OUT_HEAD": "0"}, 0),
    "bf16": ([64, 256, 6], 2048, {}, 1),                            # bf16 storage: out_head (no fold in bf16 mode)
}


def clip_shifts(rng, n, eps):
    """s with |s| in [0.2, 0.6]·eps (30 % of rows) or [1.5, 3]·eps (70 %), random sign: no row near the inside
    boundary; about half of the outside rows have the clipped value further from the target."""
    out = rng.uniform(size=n) < 0.7
    mag = np.where(out, rng.uniform(1.5, 3.0, n), rng.uniform(0.2, 0.6, n)) * eps
    return (mag * rng.choice([-1.0, 1.0], n)).astype(F32)


def one_step(lib, oracle, form, monkeypatch, clip=True, prof=False):
    sizes, B, env, dtype = FORMS[form]
    for k in ("PPO_VALUE_FOLD", "PPO_OUT_HEAD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PPO_NO_TINY", "1")
    N, S = 2 * B, sizes[0]
    sv = sizes[:-1] + [1]
    if B > 8192:
        oracle.load(use_openblas=True)
        oracle.load().ref_blas_threads(16)
    ppo = make_ppo(lib, oracle, sizes, N, seed=4242)
    assert lib.ppo_set_compute_dtype(ppo, dtype) == 0
    lib.ppo_fill_synthetic(ppo, 8, N // 8, 9, 1.0 / 200)
    lib.ppo_synchronize()
    V = ppo.contents.V
    v0 = nn_params_packed(lib, V)
    b = ppo.contents.buffer.contents
    rows = oracle.feistel_perm(N, oracle.splitmix64(SEED))[:B]
    assert np.unique(rows).size == B and (rows != np.arange(B)).any()      # a slot index is not a row index
    x = ppo_ffi.d2h(lib, b.d_state_p, F32, N * S).reshape(N, S)[rows]
    y_or = oracle.mlp_layer_outputs(sv, oracle.mlp_forward(sv, RELU(sv), v0, x), B)[-1].ravel().astype(F32)
    v_old = np.full(N, np.nan, F32)
    v_old[rows] = y_or + clip_shifts(np.random.default_rng(31), B, EPS_V)
    dv = dev(lib, v_old)
    out = dict(sizes=sizes, sv=sv, B=B, N=N, dtype=dtype, rows=rows, x=x, y_or=y_or, v_old=v_old[rows], v0=v0)
    if clip:
        assert lib.ppo_set_value_clip(ppo, EPS_V) == 0
        assert lib.ppo_value_clip_old_values(ppo, dv.ptr, N) == 0
    lib.ppo_set_step_limit(ppo, 1, 0)
    lib.ppo_reset_stats(ppo)
    if prof:
        lib.ppo_prof_enable(1)
        lib.ppo_prof_reset()
    lib.ppo_update(ppo, 0.99, B, 0, 1, 1, SEED)
    lib.ppo_synchronize()
    if prof:
        cnt = (C.c_long * 7)()
        lib.ppo_prof_counts(cnt)
        lib.ppo_prof_enable(0)
        out["counts"] = list(cnt)
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    out["st"] = stats(lib, ppo)
    out["y"] = ppo_ffi.d2h(lib, V.contents.d_output, F32, B)
    out["tgt"] = ppo_ffi.d2h(lib, b.d_adv_target_p, F32, N)[rows]
    out["gV"] = nn_grads_packed(lib, V)
    if not prof:
        out["check"] = lambda g, what: grads_check(lib, oracle, V, out, g, what)
        out["free"] = lambda: (dv.free(), lib.ppo_set_step_limit(ppo, -1, -1), lib.free_ppo(ppo))
    else:
        dv.free()
        lib.ppo_set_step_limit(ppo, -1, -1)
        lib.free_ppo(ppo)
    return out


def grads_check(lib, oracle, V, r, g, what):
    sv, x, B = r["sv"], r["x"], r["B"]
    gtop = g.reshape(-1, 1)
    if r["dtype"] == 1:                                   # see the module docstring
        gV = check_bf16_layers(lib, V, sv, r["v0"], x, gtop, True, what)
        g_ref, _ = oracle_grads_with_masks(oracle, sv, RELU(sv), r["v0"], x, gtop, None, what)
        close(gV, g_ref, 3e-2, f"{what}: value grads vs the fp32 oracle fed the model's g")
        return bf16(g)
    masks = gpu_relu_masks(lib, V, x)
    assert masks is not None
    g_ref, _ = oracle_grads_with_masks(oracle, sv, RELU(sv), r["v0"], x, gtop, masks, what, max_flips=256)
    assert_gemm_close(r["gV"], g_ref, B, f"{what}: value grads vs the oracle fed the model's g")
    return g


@pytest.mark.parametrize("form", sorted(FORMS))
def test_value_step_forms(lib, oracle, form, monkeypatch):
    r = one_step(lib, oracle, form, monkeypatch)
    try:
        B, y, t, v_old = r["B"], r["y"], r["tgt"], r["v_old"]
        # the construction, from the oracle's forward, on the CPU: 25–75 % clipped, at most 1 % near ties
        lo, _, co = vclip_f32(r["y_or"], t, v_old, EPS_V)

        def near_tie(yy):
            lu = (t.astype(np.float64) - yy) ** 2
            d = yy.astype(np.float64) - v_old
            lc = (t - (v_old + np.copysign(np.float64(F32(EPS_V)), d))) ** 2
            return (np.abs(d) > EPS_V) & (np.abs(lu - lc) < 1e-5 * np.maximum(lu, lc))
        assert 0.25 <= co.mean() <= 0.75, co.mean()
        assert near_tie(r["y_or"]).mean() <= 0.01
        # no row near the inside boundary on the GPU's own y either (bf16 storage moves y by ≈ 1e-2·|y|)
        ad = np.abs(y - v_old) / F32(EPS_V)
        assert ((ad < 0.8) | (ad > 1.2)).all(), "the GPU's y puts a row near the clip boundary"
        # teacher-forced: the fp32 model on the GPU's own y
        l, g, c = vclip_f32(y, t, v_old, EPS_V)
        tie = near_tie(y)
        assert tie.mean() <= 0.01
        st = r["st"]
        print(f"{form}: clipped {int(st[17])} of {int(st[18])} rows (model {int(c.sum())}, oracle forward "
              f"{int(co.sum())}, near ties {int(tie.sum())}); loss {st[0]:.9g} vs model {l.astype(np.float64).sum() / B:.9g}")
        assert st[1] == 1 and st[18] == B
        assert (c & ~tie).sum() <= st[17] <= (c | tie).sum()
        loss = l.astype(np.float64).sum() / B
        assert abs(st[0] - loss) <= 1e-5 * loss
        g_in = r["check"](g, form)                        # every network gradient
        # the output bias gradient (the packed gradient's last entry) is Σ g within fp32 summation: chains of
        # at most 256 additions, 2^-15·Σ|g| (check_bf16_layers' bound for the same sums)
        gb = float(r["gV"][-1])
        s, sa = float(g_in.astype(np.float64).sum()), float(np.abs(g_in).astype(np.float64).sum())
        assert abs(gb - s) <= 2.0 ** -15 * sa + 1e-12, (gb, s)
    finally:
        r["free"]()


# ----------------------------------------------------------------------------- 3. default old values
def default_run(lib, oracle, eps, steps, lr_v, monkeypatch):
    monkeypatch.setenv("PPO_NO_TINY", "1")
    sizes, N, B = [17, 64, 64, 6], 1024, 256
    ppo = make_ppo(lib, oracle, sizes, N, seed=1234)
    ppo.contents.lr_V = lr_v
    lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 500)
    assert lib.ppo_set_value_clip(ppo, eps) == 0
    lib.ppo_set_step_limit(ppo, steps, 0)
    lib.ppo_reset_stats(ppo)
    lib.ppo_update(ppo, 0.99, B, 0, 2, 1, SEED)
    lib.ppo_synchronize()
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    out = dict(st=stats(lib, ppo), g=nn_grads_packed(lib, ppo.contents.V), v=nn_params_packed(lib, ppo.contents.V), B=B)
    lib.ppo_set_step_limit(ppo, -1, -1)
    lib.free_ppo(ppo)
    return out


def test_default_old_values(lib, oracle, monkeypatch):
    """With the update's own GAE values as v_old, the first value step has y = v_old up to the kernels'
    summation order: every row is inside and the step is the plain one.  After a few large steps rows clip."""
    on, off = (default_run(lib, oracle, e, 1, 3e-4, monkeypatch) for e in (EPS_V, 0.0))
    assert on["st"][17] == 0 and on["st"][18] == on["B"] and off["st"][17] == off["st"][18] == 0
    assert abs(on["st"][0] - off["st"][0]) <= 1e-6 * off["st"][0]
    assert_gemm_close(on["g"], off["g"], on["B"], "first value step, clipping on vs off")
    on, off = (default_run(lib, oracle, e, 8, 1e-2, monkeypatch) for e in (1e-3, 0.0))
    print(f"8 steps at lr_V = 1e-2, eps_v = 1e-3: clipped {int(on['st'][17])} of {int(on['st'][18])} rows")
    assert on["st"][17] > 0 and on["st"][18] == 8 * on["B"] and on["st"][1] == 8
    assert not np.array_equal(on["v"], off["v"])


# ----------------------------------------------------------------------------- 4. routing and composition
def test_tiny_shape_takes_the_loop(lib, oracle, monkeypatch):
    """A C2-shaped update (3 → 2×64 → 1, B = 64: the single-workgroup path's shape) with clipping on runs the
    multi-launch loop: the reference's step counts, no graph replay, and the heads counted their rows."""
    monkeypatch.delenv("PPO_NO_TINY", raising=False)
    sizes, N, B = [3, 64, 64, 1], 1024, 64
    ppo = make_ppo(lib, oracle, sizes, N, seed=21)
    lib.ppo_fill_synthetic(ppo, 4, N // 4, 17, 1.0 / 200)
    assert lib.ppo_set_value_clip(ppo, EPS_V) == 0
    lib.ppo_reset_stats(ppo)
    lib.ppo_update(ppo, 0.99, B, 1, 2, 1, SEED)
    lib.ppo_synchronize()
    st = stats(lib, ppo)
    assert st[1] == 2 * (N // B) and st[3] == N // B
    assert st[8] == 0 and st[18] == 2 * N
    assert stats(lib, ppo, 17) == st[:17]                 # callers passing n <= 17 see no change
    # … and together with gradient clipping and KL monitoring
    assert lib.ppo_set_max_grad_norm(ppo, 0.5) == 0 and lib.ppo_set_target_kl(ppo, float("inf")) == 0
    lib.ppo_reset_stats(ppo)
    lib.ppo_update(ppo, 0.99, B, 1, 2, 1, SEED)
    lib.ppo_synchronize()
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    st = stats(lib, ppo)
    assert st[1] == 2 * (N // B) and st[3] == N // B and st[18] == 2 * N and st[15] == N // B
    lib.free_ppo(ppo)


def _loop_run(lib, oracle, eps, monkeypatch):
    monkeypatch.setenv("PPO_NO_TINY", "1")
    sizes, N, B = [17, 64, 64, 6], 1024, 256
    ppo = make_ppo(lib, oracle, sizes, N, seed=1234)
    ppo.contents.lr_V = 1e-2
    lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 500)
    assert lib.ppo_set_value_clip(ppo, eps) == 0
    lib.ppo_reset_stats(ppo)
    lib.ppo_prof_enable(1)
    lib.ppo_prof_reset()
    lib.ppo_update(ppo, 0.99, B, 1, 2, 1, SEED)
    lib.ppo_synchronize()
    cnt = (C.c_long * 7)()
    lib.ppo_prof_counts(cnt)
    lib.ppo_prof_enable(0)
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    out = dict(v=nn_params_packed(lib, ppo.contents.V), st=stats(lib, ppo), comm=cnt[5], hash=lib.ppo_param_hash(ppo))
    lib.free_ppo(ppo)
    return out


def test_loopback_replicas(lib, oracle, monkeypatch):
    """Two identical in-process ranks (PPO_COMM_LOOPBACK=2): the summed gradient is 2g and Adam scales by 1/2,
    both exact, so the value network equals the one-GPU run's wherever the two runs' gradients do (the existing
    loopback property: test_gpu_update.test_comm_rehearsal) — with clipping on as with it off; and the
    head adds no collective."""
    lib.ppo_gemm_tune(-1, 1)                              # atomic-free gradient sums: run-to-run identical bits
    try:
        one = _loop_run(lib, oracle, 1e-3, monkeypatch)
        monkeypatch.setenv("PPO_COMM_LOOPBACK", "2")
        assert lib.ppo_comm_init(0, 1, None) == 0, lib.ppo_last_error()
        try:
            assert lib.ppo_comm_world() == 2
            on = _loop_run(lib, oracle, 1e-3, monkeypatch)
            off = _loop_run(lib, oracle, 0.0, monkeypatch)
        finally:
            lib.ppo_comm_finalize()
            monkeypatch.delenv("PPO_COMM_LOOPBACK")
    finally:
        lib.ppo_gemm_tune(-1, 0)
    assert one["st"][17] > 0 and on["st"][17] == one["st"][17] and on["st"][18] == one["st"][18]
    np.testing.assert_array_equal(on["v"], one["v"])
    assert on["comm"] == off["comm"] > 0


# ----------------------------------------------------------------------------- 5. no extra launches
@pytest.mark.parametrize("form", ["fold_carried", "plain"])
def test_no_extra_launches(lib, oracle, form, monkeypatch):
    on = one_step(lib, oracle, form, monkeypatch, clip=True, prof=True)
    off = one_step(lib, oracle, form, monkeypatch, clip=False, prof=True)
    print(f"{form}: launches per class, on {on['counts']}, off {off['counts']}")
    assert on["counts"] == off["counts"] and sum(on["counts"]) > 0
    assert on["st"][17] > 0 and off["st"][17] == 0 and off["st"][18] == 0


# ----------------------------------------------------------------------------- 6. setters
def test_setters(lib, oracle):
    ppo = make_ppo(lib, oracle, [17, 64, 64, 6], 256)
    assert lib.ppo_get_value_clip(ppo) == 0.0
    assert lib.ppo_set_value_clip(ppo, 0.5) == 0 and lib.ppo_get_value_clip(ppo) == 0.5
    assert lib.ppo_set_value_clip(ppo, float("nan")) == -1 and lib.ppo_get_value_clip(ppo) == 0.5
    for off in (0.0, -1.0, float("inf")):
        assert lib.ppo_set_value_clip(ppo, 0.25) == 0 and lib.ppo_get_value_clip(ppo) == 0.25
        assert lib.ppo_set_value_clip(ppo, off) == 0 and lib.ppo_get_value_clip(ppo) == 0.0
    d = empty(lib, 256)
    assert lib.ppo_value_clip_old_values(ppo, d.ptr, 255) == -1
    assert lib.ppo_value_clip_old_values(ppo, d.ptr, 256) == 0
    assert lib.ppo_value_clip_old_values(ppo, None, 0) == 0
    d.free()
    lib.free_ppo(ppo)
