"""tanh hidden layers in the fp32 networks, on both fp32 GEMM engines, against the float64 model of tanh_ref.py
(the oracle maps "tanh" to the identity, as the reference does, and cannot judge them).

Every kernel is teacher-forced: a layer is compared from the GPU's OWN stored input (forward) or its own upstream
gradient and stored post-activation (backward), so errors do not compound across layers.

Shapes: [12, 72, 40, 3] — at m = 1100 layer 0 (n = 12 ≤ 32) and the output layer (l = 3) run on the exact family's
tiles and the 72 → 40 layer on x3 (m > 1024, n, l > 32; 1100 is ragged against every tile height); at m = 7 every
layer is on the exact family, the 72 → 40 forward on its small-M kernel; engine 0 puts every layer on exact.
[12, 72, 72, 3] at m = 7 adds the small-M grad_x (K = 72 ≥ 64) with the h operand.

Bounds.  Forward: helpers.gemm_tol of the float64 PRE-activation z at K = n — tanh is 1-Lipschitz, so the GEMM's
error passes through undiminished at worst, and tanhf's own few-ulp error on |h| ≤ 1 sits inside gemm_tol's 1e-6
floor.  grad_x: gemm_tol of the float64 product g·W at K = l — the tanh′ factor 1 − h² ≤ 1 scales the product's
error down, and the fp32 statement acc − (acc·h)·h adds ≤ 3·2⁻²⁴·|acc| (test_tanh_cpu.py).  grad_W / grad_b:
gemm_tol at K = m.  tanh is smooth: no mask flips, no case left out."""
import ctypes as C

import numpy as np
import pytest

import ppo_ffi
import tanh_ref as T
from helpers import (F32, assert_gemm_close, assert_rel_close, dev, gemm_tol, nn_grads_packed, nn_input_rows,
                     nn_params_packed, nn_set_params_packed)
from test_gpu_update import adam_first_step, assert_adam_delta

pytestmark = pytest.mark.gpu

F64 = np.float64
SIZES = [12, 72, 40, 3]
TANH = ["tanh", "tanh", "none"]
MIXED = ["relu", "tanh", "none"]
LR = 3e-4
# (sizes, m, engine): engine 1 = x3 (the default), 0 = exact everywhere
LAYER_CASES = [(SIZES, 1100, 1), (SIZES, 7, 1), (SIZES, 1100, 0), (SIZES, 7, 0), ([12, 72, 72, 3], 7, 1)]


class engine:
    """ppo_gemm_f32_engine(e) for the block, the previous setting restored whatever happens."""

    def __init__(self, lib, e):
        self.lib, self.e = lib, e

    def __enter__(self):
        self.old = self.lib.ppo_gemm_f32_engine(self.e)

    def __exit__(self, *exc):
        self.lib.ppo_gemm_f32_engine(self.old)


def _params(sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(len(sizes) - 1):
        n, l = sizes[i], sizes[i + 1]
        out.append(rng.uniform(-1, 1, l * n) * np.sqrt(3.0 / n))        # pre-activations of unit scale
        out.append(rng.uniform(-0.3, 0.3, l))
    return np.concatenate(out).astype(F32)


def _inputs(sizes, m, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (m, sizes[0])).astype(F32)
    x[0] *= 50                      # |z| large: h rounds to ±1 in fp32 for units of this row
    g = rng.uniform(-1, 1, (m, sizes[-1])).astype(F32)
    return x, g


def _net(lib, sizes, acts, params):
    nn = lib.create_neural_network(ppo_ffi.c_ints(sizes), ppo_ffi.c_strings(acts), len(sizes))
    nn_set_params_packed(lib, nn, params)
    return nn


def _stored(lib, nn, m, field):
    """layers[i].<field> of the first m rows, i = 0 … L (m × layers[i].input_size)."""
    c = nn.contents
    return [ppo_ffi.d2h(lib, getattr(c.layers[i], field), F32, m * c.layers[i].input_size)
            .reshape(m, c.layers[i].input_size) for i in range(c.num_layers)]


def _check_forward(lib, nn, sizes, acts, params, m, what):
    hs = _stored(lib, nn, m, "d_input")
    hs[0] = nn_input_rows(lib, nn, m)                 # layer 0's rows as the GEMM read them
    sat = 0
    for i, ((W, b), act) in enumerate(zip(T.unpack(sizes, params), acts)):
        z_ref, h_ref = T.layer_forward(W, b, hs[i], act)
        assert np.isfinite(hs[i + 1]).all()
        # the scaled row 0 on its own: its large pre-activations must not widen the bound of the other rows
        for rows in (slice(0, 1), slice(1, m)):
            err = float(np.abs(hs[i + 1][rows] - h_ref[rows]).max())
            tol = gemm_tol(z_ref[rows], sizes[i])
            print(f"{what} forward layer {i} ({act}) rows {rows.start}:{rows.stop}: max err {err:.3g}, bound {tol:.3g}")
            assert err <= tol, f"{what} forward layer {i} ({act}): max |err| {err:.3g} > {tol:.3g}"
        if act == "tanh":
            assert np.abs(hs[i + 1]).max() <= 1.0
            sat += int((np.abs(hs[i + 1]) == 1).sum())
    return hs, sat


def _check_backward(lib, nn, sizes, acts, params, hs, m, what):
    gs = _stored(lib, nn, m, "d_grad_x")              # gs[i]: the gradient at layer i's input, act′ applied
    layers = T.unpack(sizes, params)
    L = len(layers)
    packed = nn_grads_packed(lib, nn)
    off = 0
    for i in range(L):
        n, l = sizes[i], sizes[i + 1]
        act_in = acts[i - 1] if i > 0 else "none"
        gx_ref, acc_ref, gW_ref, gb_ref = T.layer_backward(layers[i][0], gs[i + 1], hs[i], act_in)
        gW = packed[off:off + n * l].reshape(l, n)
        gb = packed[off + n * l:off + n * l + l]
        off += n * l + l
        assert np.isfinite(gs[i]).all(), f"{what} grad_x layer {i}: NaN / inf"
        err, tol = float(np.abs(gs[i] - gx_ref).max()), gemm_tol(acc_ref, l)
        print(f"{what} grad_x layer {i} (below: {act_in}): max err {err:.3g}, bound {tol:.3g}")
        assert err <= tol, f"{what} grad_x layer {i} (below: {act_in}): max |err| {err:.3g} > {tol:.3g}"
        if act_in == "tanh":                           # a saturated unit passes exactly nothing
            assert (gs[i][np.abs(hs[i]) == 1] == 0).all()
        assert_gemm_close(gW, gW_ref, m, f"{what} grad_W layer {i}")
        assert_gemm_close(gb, gb_ref, m, f"{what} grad_b layer {i}")


def _run_layers(lib, sizes, acts, m, eng, what):
    params = _params(sizes, 100 + m)
    x, g = _inputs(sizes, m, 200 + m)
    nn = _net(lib, sizes, acts, params)
    dx, dg = dev(lib, x), dev(lib, g)
    try:
        with engine(lib, eng):
            lib.forward_propagation_cuda(nn, dx.ptr, m)
            hs, sat = _check_forward(lib, nn, sizes, acts, params, m, what)
            lib.backward_propagation_cuda(nn, dg.ptr, m)
            _check_backward(lib, nn, sizes, acts, params, hs, m, what)
        assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
        return sat
    finally:
        lib.free_neural_network(nn)
        dx.free()
        dg.free()


# ------------------------------------------------------------------------------------- 1, 2: per layer
@pytest.mark.parametrize("sizes,m,eng", LAYER_CASES)
def test_tanh_layers_forward_backward(lib, sizes, m, eng):
    """Tests 1 and 2: every layer's forward and backward, teacher-forced.  Fails on a library where "tanh" is the
    identity (the stored post-activations are then the pre-activations, far outside the bound)."""
    sat = _run_layers(lib, sizes, TANH, m, eng, f"tanh m={m} engine={eng}")
    assert sat > 0, "the scaled row should saturate some units to ±1"


# ------------------------------------------------------------------------------------- 3: mixed network
@pytest.mark.parametrize("m,eng", [(1100, 1), (7, 1), (1100, 0)])
def test_mixed_relu_tanh_network(lib, m, eng):
    """relu below tanh: each derivative lands on its own layer (the per-layer checks), the ReLU′ bits are written
    for the relu layer's output only, and the tanh layer's block of mask words is never touched."""
    _run_layers(lib, SIZES, MIXED, m, eng, f"mixed m={m} engine={eng}")
    params = _params(SIZES, 100 + m)
    x, _ = _inputs(SIZES, m, 200 + m)
    nn = _net(lib, SIZES, MIXED, params)
    dx = dev(lib, x)
    try:
        with engine(lib, eng):
            lib.forward_propagation_cuda(nn, dx.ptr, m)          # allocates the mask words
            c = nn.contents
            cap = c.act_cap_m
            wpr = [(s + 31) // 32 for s in SIZES]
            total = cap * sum(wpr)
            lib.ppo_dev_memset(C.cast(c.d_act_bits, C.c_void_p), 0xA5, 4 * total)
            lib.forward_propagation_cuda(nn, dx.ptr, m)
            lib.ppo_synchronize()
            words = ppo_ffi.d2h(lib, c.d_act_bits, np.uint32, total)
            h1 = ppo_ffi.d2h(lib, c.layers[1].d_input, F32, m * SIZES[1]).reshape(m, SIZES[1])
        off = [cap * sum(wpr[:i]) for i in range(len(SIZES))]
        blk = words[off[1]:off[1] + m * wpr[1]].reshape(m, wpr[1])
        cols = np.arange(SIZES[1])
        bits = (blk[:, cols // 32] >> (cols % 32).astype(np.uint32)) & 1
        np.testing.assert_array_equal(bits.astype(bool), h1 > 0)
        for i in (0, 2, 3):                                      # the input, the tanh output, the network output
            assert (words[off[i]:off[i] + m * wpr[i]] == 0xA5A5A5A5).all(), f"mask words of block {i} were written"
    finally:
        lib.free_neural_network(nn)
        dx.free()


# ------------------------------------------------------------------------------------- 4: reference API
def _act_inputs():
    rng = np.random.default_rng(3)
    x = rng.uniform(-4, 4, (5, 33)).astype(F32)
    x[0, :4] = [0.0, 20.0, -20.0, 1e-6]
    g = rng.normal(size=(5, 33)).astype(F32)
    return x, g


def _check_tanh_values(y, x):
    ref = np.tanh(x.astype(F64))
    # tanhf is accurate to a few ulp (2 documented for the device math library); 4 ulp of the result allowed
    assert (np.abs(y - ref) <= 4 * 2.0 ** -23 * np.abs(ref)).all(), float(np.abs(y - ref).max())
    assert y[0, 0] == 0 and y[0, 1] == 1 and y[0, 2] == -1


def test_reference_api_entry_points(lib):
    x, g = _act_inputs()
    # device-pointer forms
    dx, dg = dev(lib, x), dev(lib, g)
    lib.Tanh_cuda(dx.ptr, 5, 33)
    y = dx.to_numpy(F32, x.size).reshape(x.shape)
    _check_tanh_values(y, x)
    lib.Tanh_derivative_cuda(dx.ptr, dg.ptr, 5, 33)
    gd = dg.to_numpy(F32, g.size).reshape(g.shape)
    np.testing.assert_array_equal(dx.to_numpy(F32, x.size).reshape(x.shape), y)      # x (post-activation) kept
    np.testing.assert_array_equal(gd, T.tanh_bwd_f32(g, y))                          # the stated order, bit for bit
    np.testing.assert_allclose(gd, T.tanh_bwd_f64(g, y), rtol=0, atol=3 * 2.0 ** -24 * float(np.abs(g).max()))
    dx.free()
    dg.free()
    # host-pointer forms
    xh, gh = x.copy(), g.copy()
    lib.Tanh(xh.ctypes.data, 5, 33)
    np.testing.assert_array_equal(xh, y)
    lib.Tanh_derivative(xh.ctypes.data, gh.ctypes.data, 5, 33)
    np.testing.assert_array_equal(gh, gd)
    # the name table: "tanh" maps to the four, device and host
    for build, fwd, bwd in ((lib.build_activation_function_cuda, lib.Tanh_cuda, lib.Tanh_derivative_cuda),
                            (lib.build_activation_function, lib.Tanh, lib.Tanh_derivative)):
        build.restype = C.POINTER(ppo_ffi.ActivationFunction)
        build.argtypes = [C.c_char_p]
        a = build(b"tanh").contents
        assert a.activation == C.cast(fwd, C.c_void_p).value
        assert a.activation_derivative == C.cast(bwd, C.c_void_p).value
        assert build(b"sigmoid").contents.activation is None                        # every other name: identity


def test_tanh_output_layer(lib):
    """The rare output activation: tanh on the last layer goes through phip_tanh_bwd at the top of the backward."""
    sizes, acts, m = [6, 40, 3], ["tanh", "tanh"], 37
    params = _params(sizes, 9)
    x, g = _inputs(sizes, m, 10)
    nn = _net(lib, sizes, acts, params)
    dx, dg = dev(lib, x), dev(lib, g)
    try:
        lib.forward_propagation_cuda(nn, dx.ptr, m)
        hs, _ = _check_forward(lib, nn, sizes, acts, params, m, "tanh output")
        lib.backward_propagation_cuda(nn, dg.ptr, m)
        top = ppo_ffi.d2h(lib, nn.contents.layers[2].d_grad_x, F32, m * 3).reshape(m, 3)
        np.testing.assert_array_equal(top, T.tanh_bwd_f32(g, hs[2]))
        _check_backward(lib, nn, sizes, acts, params, hs, m, "tanh output")
    finally:
        lib.free_neural_network(nn)
        dx.free()
        dg.free()


# ------------------------------------------------------------------------------------- 5: the update
N_UP, B_UP, SEED = 2200, 1100, 77


def _make_ppo(lib, sizes, acts, N, seed=1234, ent_coeff=0.01):
    C.CDLL("libc.so.6").srand(seed)
    return lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), N, LR, LR, 0.95, 0.2, ent_coeff,
                          0.7, True)


def _rows_of(x0, states):
    where = {r.tobytes(): i for i, r in enumerate(np.ascontiguousarray(states, F32))}
    rows = np.array([where[r.tobytes()] for r in x0])
    assert len(set(rows.tolist())) == len(rows)
    return rows


def _gemm_launches(lib):
    cnt = (C.c_long * 7)()
    lib.ppo_prof_counts(cnt)
    return list(cnt)


def _update(lib, eng):
    """One ppo_update of a tanh PPO capped at one value and one policy step, with PPO_GRAPH, PPO_OUT_HEAD and the
    single-workgroup / cluster phases at their defaults, launches counted: everything the tests below read."""
    S, A = SIZES[0], SIZES[-1]
    sv = SIZES[:-1] + [1]
    out = {}
    with engine(lib, eng):
        ppo = _make_ppo(lib, SIZES, TANH, N_UP)
        try:
            p = ppo.contents
            pol = p.policy.contents
            lib.ppo_fill_synthetic(ppo, 4, N_UP // 4, 21, 1.0 / 300)
            lib.ppo_synchronize()
            out["v0"] = nn_params_packed(lib, p.V)
            out["mu0"] = nn_params_packed(lib, pol.mu)
            out["ls0"] = ppo_ffi.d2h(lib, pol.d_log_std, F32, A)
            b = p.buffer.contents
            out["state"] = ppo_ffi.d2h(lib, b.d_state_p, F32, N_UP * S).reshape(N_UP, S)
            out["action"] = ppo_ffi.d2h(lib, b.d_action_p, F32, N_UP * A).reshape(N_UP, A)
            out["old_lp"] = ppo_ffi.d2h(lib, b.d_logprob_p, F32, N_UP)
            # GAE alone first: its launches are the baseline of the step count below
            lib.ppo_reset_stats(ppo)
            lib.ppo_prof_enable(1)
            lib.ppo_prof_reset()
            lib.ppo_set_step_limit(ppo, 0, 0)
            lib.ppo_update(ppo, 0.99, B_UP, 1, 1, 1, SEED)
            lib.ppo_synchronize()
            out["cnt_gae"] = _gemm_launches(lib)
            lib.ppo_prof_reset()
            lib.ppo_set_step_limit(ppo, 1, 1)
            lib.ppo_update(ppo, 0.99, B_UP, 1, 1, 1, SEED)
            lib.ppo_synchronize()
            out["cnt"] = _gemm_launches(lib)
            lib.ppo_prof_enable(0)
            assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
            st = (C.c_double * 9)()
            lib.ppo_read_stats(ppo, st, 9)
            out["st"] = list(st)
            v = np.empty(N_UP, F32)
            assert lib.ppo_gae_state(None, v.ctypes.data, None, N_UP) == N_UP
            out["v"] = v
            out["adv"] = ppo_ffi.d2h(lib, b.d_advantage_p, F32, N_UP)
            out["tgt"] = ppo_ffi.d2h(lib, b.d_adv_target_p, F32, N_UP)
            out["rows_v"] = _rows_of(nn_input_rows(lib, p.V, B_UP), out["state"])
            out["rows_p"] = _rows_of(nn_input_rows(lib, pol.mu, B_UP), out["state"])
            out["gV"], out["v1"] = nn_grads_packed(lib, p.V), nn_params_packed(lib, p.V)
            out["gmu"], out["mu1"] = nn_grads_packed(lib, pol.mu), nn_params_packed(lib, pol.mu)
            out["gls"] = ppo_ffi.d2h(lib, pol.d_log_std_grad, F32, A)
            out["t"] = (p.adam_V.contents.time_step, p.adam_policy.contents.time_step)
        finally:
            lib.ppo_prof_enable(0)
            lib.free_ppo(ppo)
    # the float64 model on the same minibatches (targets and advantages: the GPU's own GAE, whose V is test 5a)
    rv, rp = out["rows_v"], out["rows_p"]
    out["gV_ref"], _ = T.value_grads(sv, TANH, out["v0"], out["state"][rv], out["tgt"][rv])
    out["gmu_ref"], out["gls_ref"], _ = T.policy_grads(SIZES, TANH, out["mu0"], out["ls0"], out["state"][rp],
                                                       out["action"][rp], out["adv"][rp], out["old_lp"][rp], 0.2, 0.01)
    return out


_UPDATES = {}


@pytest.fixture
def updates(lib):
    def get(eng):
        if eng not in _UPDATES:
            _UPDATES[eng] = _update(lib, eng)
        return _UPDATES[eng]
    return get


@pytest.mark.parametrize("eng", [1, 0])
def test_update_gae_values(lib, updates, eng):
    """5a: the V(state) the update's GAE read is the float64 tanh model's.  Fails where "tanh" is the identity."""
    u = updates(eng)
    sv = SIZES[:-1] + [1]
    hs, _ = T.forward(sv, TANH, u["v0"], u["state"])
    assert_gemm_close(u["v"], hs[-1][:, 0], max(sv), f"engine {eng} V(state) of the update's GAE")


@pytest.mark.parametrize("eng", [1, 0])
def test_update_single_steps(lib, updates, eng):
    """5b: one value and one policy step against the float64 model's gradient and Adam's first step — the
    comparison and constants of the relu single-step tests (test_gpu_update.py / test_gpu_production.py)."""
    u = updates(eng)
    assert u["t"] == (1, 1)
    assert_gemm_close(u["gV"], u["gV_ref"], B_UP, f"engine {eng} value grads")
    flips = assert_adam_delta(u["v1"], adam_first_step(u["v0"], u["gV_ref"], LR), u["gV_ref"], LR,
                              f"engine {eng} value params")
    assert flips <= max(2, u["v1"].size // 1000)
    assert_gemm_close(u["gmu"], u["gmu_ref"], B_UP, f"engine {eng} policy grads")
    assert_rel_close(u["gls"], u["gls_ref"], 1e-3, 1e-4 * max(1.0, float(np.abs(u["gls_ref"]).max())), "log_std grad")
    flips = assert_adam_delta(u["mu1"], adam_first_step(u["mu0"], u["gmu_ref"], LR), u["gmu_ref"], LR,
                              f"engine {eng} policy params")
    assert flips <= max(2, u["mu1"].size // 1000)


def test_update_engines_agree(lib, updates):
    """5c: the same update on x3 and on exact, within twice the bound of 5b."""
    a, b = updates(1), updates(0)
    np.testing.assert_array_equal(a["rows_v"], b["rows_v"])
    np.testing.assert_array_equal(a["rows_p"], b["rows_p"])
    for g, ref in (("gV", "gV_ref"), ("gmu", "gmu_ref")):
        err, tol = float(np.abs(a[g] - b[g]).max()), 2 * gemm_tol(a[ref], B_UP)
        assert err <= tol, f"{g}: x3 vs exact {err:.3g} > {tol:.3g}"
    for p1, ref in (("v1", "gV_ref"), ("mu1", "gmu_ref")):
        err = np.abs(a[p1].astype(F64) - b[p1])
        big = np.abs(a[ref]) > 1e-3 * np.abs(a[ref]).max()
        assert (err[big] <= 2 * (1e-6 * np.abs(b[p1][big]) + 1e-6 * LR)).all()
        assert (err <= 2 * (2 * LR * 1.0001 + 1e-7)).all()


@pytest.mark.parametrize("eng", [1, 0])
def test_update_takes_the_multi_launch_loop(lib, updates, eng):
    """5d: with every switch at its default a tanh update takes no fused, folded, single-workgroup, cluster or
    replayed path — seen from outside: no replayed step, one head launch per step (both forms of the head are
    one launch) and, per step, the multi-launch loop's GEMM launches: L forwards, grad_W for every layer and
    grad_x for every layer but the first = 3L − 1 (a fused output head would run 3(L − 1) − 1, the phases 0).
    The result is the one test_update_single_steps checks: both read the same run."""
    u = updates(eng)
    L = len(SIZES) - 1
    assert u["st"][1] == 1 and u["st"][3] == 1                   # one value, one policy step
    assert u["st"][8] == 0                                       # nothing replayed from a captured graph
    gemm = u["cnt"][0] - u["cnt_gae"][0]                         # PPO_K_GEMM beyond the GAE's own forwards
    head = u["cnt"][4] - u["cnt_gae"][4]                         # PPO_K_HEAD
    assert head == 2, u["cnt"]
    assert gemm == 2 * (3 * L - 1), (u["cnt"], u["cnt_gae"])


# ------------------------------------------------------------------------------------- 6: declines
def test_bf16_mode_declines_tanh(lib):
    for acts, want in ((TANH, -1), (MIXED, -1), (["relu", "relu", "none"], 0)):
        ppo = _make_ppo(lib, SIZES, acts, 64)
        try:
            assert lib.ppo_set_compute_dtype(ppo, 1) == want
            V, mu = ppo.contents.V, ppo.contents.policy.contents.mu
            assert V.contents.dtype == mu.contents.dtype == (1 if want == 0 else 0)      # unchanged on a decline
            assert lib.nn_set_compute_dtype(V, 1) == want
            assert lib.ppo_set_compute_dtype(ppo, 0) == 0
        finally:
            lib.free_ppo(ppo)


# ------------------------------------------------------------------------------------- 7: rollout, evaluation
def test_rollout_and_evaluation(lib):
    sizes, E, Tn = [3, 64, 64, 1], 8, 16
    N = E * Tn
    ppo = _make_ppo(lib, sizes, TANH, N, seed=3, ent_coeff=0.0)
    try:
        lib.ppo_rollout_device(ppo, E, Tn, 0, 11)
        lib.ppo_synchronize()
        pol = ppo.contents.policy.contents
        b = ppo.contents.buffer.contents
        state = ppo_ffi.d2h(lib, b.d_state_p, F32, N * 3).reshape(N, 3)
        action = ppo_ffi.d2h(lib, b.d_action_p, F32, N).reshape(N, 1)
        logprob = ppo_ffi.d2h(lib, b.d_logprob_p, F32, N)
        log_std = ppo_ffi.d2h(lib, pol.d_log_std, F32, 1)
        hs, _ = T.forward(sizes, TANH, nn_params_packed(lib, pol.mu), state)
        lp_ref = T.gaussian_log_prob(hs[-1], log_std, action)
        err = np.abs(logprob - lp_ref)
        assert err.max() <= 1e-3 * (1 + np.abs(lp_ref).max()), err.max()      # test_gpu_rollout.py's bound
        out = (C.c_double * 9)()
        assert lib.ppo_eval_device(ppo, E, Tn, 0, 5, 1, 0.99, out, 9) == 9
        assert np.isfinite(np.array(out[:])).all()
        assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    finally:
        lib.free_ppo(ppo)


# ------------------------------------------------------------------------------------- 8: checkpoint
def test_checkpoint_round_trip(lib, tmp_path):
    ppo = _make_ppo(lib, SIZES, TANH, 64)
    x, _ = _inputs(SIZES, 33, 5)
    dx = dev(lib, x)
    loaded = None
    try:
        path = str(tmp_path / "tanh.bin").encode()
        lib.save_ppo(ppo, path)
        loaded = lib.load_ppo(path, True)
        outs = []
        for p in (ppo, loaded):
            for nn in (p.contents.policy.contents.mu, p.contents.V):
                c = nn.contents
                assert [c.activation_functions[i] for i in range(3)] == [b"tanh", b"tanh", b"none"]
                lib.forward_propagation_cuda(nn, dx.ptr, 33)
                outs.append(ppo_ffi.d2h(lib, c.d_output, F32, 33 * c.output_size))
        np.testing.assert_array_equal(outs[0], outs[2])
        np.testing.assert_array_equal(outs[1], outs[3])
        hs, _ = T.forward(SIZES, TANH, nn_params_packed(lib, loaded.contents.policy.contents.mu), x)
        assert np.abs(outs[2].reshape(33, -1) - hs[-1]).max() < 1e-4          # and it is a tanh network
    finally:
        dx.free()
        lib.free_ppo(ppo)
        if loaded:
            lib.free_ppo(loaded)
