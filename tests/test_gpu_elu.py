"""ELU (α = 1) hidden layers in the fp32 networks, on both fp32 GEMM engines, against the float64 model of elu_ref.py.
Method, shapes and inputs of test_gpu_tanh.py: every kernel teacher-forced from the GPU's own stored operands, row 0
scaled ×50 so that some units saturate.  Bounds.  Forward: helpers.gemm_tol of the float64 PRE-activation z at K = n
(ELU is 1-Lipschitz; expm1f's few-ulp error on |h| < 1 sits inside the 1e-6 floor).  grad_x: gemm_tol of the float64
product g·W at K = l (h + 1 ≤ 1 scales its error down; the fp32 statement adds ≤ 2·2⁻²⁴·|acc|, test_elu_cpu.py).
grad_W / grad_b: gemm_tol at K = m.  ELU is C¹: no mask, no flipped case, nothing left out of a comparison."""
import ctypes as C

import numpy as np
import pytest

import elu_ref as E
import ppo_ffi
from helpers import F32, assert_gemm_close, dev, gemm_tol, nn_grads_packed, nn_input_rows, nn_params_packed
from policy_head_ref import policy_head_f64
from test_gpu_adam import LIBC
from test_gpu_tanh import LR, SIZES, _inputs, _make_ppo, _net, _params, _rows_of, _stored, engine
from test_gpu_update import adam_first_step, assert_adam_delta

pytestmark = pytest.mark.gpu

F64 = np.float64
ELU = ["elu", "elu", "none"]


def _layers(lib, sizes, acts, m, eng, saturating=True):
    """Forward and backward of every layer, teacher-forced; below an ELU layer, the exactness conditions."""
    what = f"{acts} {sizes} m={m} engine={eng}"
    params = _params(sizes, 100 + m)
    x, g = _inputs(sizes, m, 200 + m)
    nn = _net(lib, sizes, acts, params)
    dx, dg = dev(lib, x), dev(lib, g)
    try:
        with engine(lib, eng):
            lib.forward_propagation_cuda(nn, dx.ptr, m)
            hs = _stored(lib, nn, m, "d_input")
            hs[0] = nn_input_rows(lib, nn, m)
            lib.backward_propagation_cuda(nn, dg.ptr, m)
            gs = _stored(lib, nn, m, "d_grad_x")
            packed = nn_grads_packed(lib, nn)
        assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    finally:
        lib.free_neural_network(nn)
        dx.free()
        dg.free()
    off = 0
    for i, ((W, b), act) in enumerate(zip(E.unpack(sizes, params), acts)):
        n, l = sizes[i], sizes[i + 1]
        z_ref, h_ref = E.layer_forward(W, b, hs[i], act)
        for rows in (slice(0, 1), slice(1, m)):      # the scaled row on its own: it must not widen the others' bound
            err, tol = float(np.abs(hs[i + 1][rows] - h_ref[rows]).max()), gemm_tol(z_ref[rows], n)
            assert err <= tol, f"{what} forward layer {i} ({act}) rows {rows}: max |err| {err:.3g} > {tol:.3g}"
        act_in = acts[i - 1] if i > 0 else "none"
        gx_ref, acc_ref, gW_ref, gb_ref = E.layer_backward(W, gs[i + 1], hs[i], act_in)
        err, tol = float(np.abs(gs[i] - gx_ref).max()), gemm_tol(acc_ref, l)
        assert np.isfinite(gs[i]).all() and err <= tol, f"{what} grad_x layer {i} ({act_in}): {err:.3g} > {tol:.3g}"
        if act_in == "elu":
            h = hs[i]
            assert (h >= -1).all() and (gs[i][h == -1] == 0).all()     # a saturated unit passes exactly nothing
            # the scaled row saturates some units (checked with elu_ref on the CPU); below a bounded tanh, none
            assert not saturating or ((h == -1).any() and ((h > -1) & (h < 0)).any() and (h > 0).any())
        assert_gemm_close(packed[off:off + n * l].reshape(l, n), gW_ref, m, f"{what} grad_W layer {i}")
        assert_gemm_close(packed[off + n * l:off + n * l + l], gb_ref, m, f"{what} grad_b layer {i}")
        off += n * l + l


@pytest.mark.parametrize("sizes,m,eng", [(SIZES, 1100, 1), (SIZES, 7, 1), (SIZES, 1100, 0), ([12, 72, 72, 3], 7, 1)])
def test_elu_layers_forward_backward(lib, sizes, m, eng):
    """x3 tiles ragged against every tile height, exact tiles, the small-M forward, the small-M grad_x with h.  Fails
    where "elu" is the identity: the stored post-activations are then the pre-activations, many below −1."""
    _layers(lib, sizes, ELU, m, eng)


@pytest.mark.parametrize("below", ["relu", "tanh"])
def test_mixed_networks(lib, below):
    """Each derivative lands on its own layer."""
    _layers(lib, SIZES, [below, "elu", "none"], 1100, 1, saturating=below != "tanh")


def test_reference_api_and_saved_network(lib, tmp_path):
    rng = np.random.default_rng(3)
    x = rng.uniform(-4, 4, (5, 33)).astype(F32)
    x[0, :5] = [0.0, 20.0, -20.0, 1e-6, np.nan]
    g = rng.normal(size=(5, 33)).astype(F32)
    ok = ~np.isnan(x)
    dx, dg = dev(lib, x), dev(lib, g)
    lib.ELU_cuda(dx.ptr, 5, 33)
    y = dx.to_numpy(F32, x.size).reshape(x.shape)
    ref = E.act_f(x.astype(F64), "elu")
    assert (np.abs(y[ok] - ref[ok]) <= 4 * 2.0 ** -23 * np.abs(ref[ok])).all()        # 4 ulp, tanhf's allowance
    assert np.isnan(y[0, 4]) and y[0, 0] == 0 and y[0, 1] == 20 and y[0, 2] == -1
    lib.ELU_derivative_cuda(dx.ptr, dg.ptr, 5, 33)
    gd = dg.to_numpy(F32, g.size).reshape(g.shape)
    np.testing.assert_array_equal(gd, E.elu_bwd_f32(g, y))                   # the stated order, bit for bit, NaN too
    dx.free()
    dg.free()
    xh, gh = x.copy(), g.copy()
    lib.ELU(xh.ctypes.data, 5, 33)
    lib.ELU_derivative(xh.ctypes.data, gh.ctypes.data, 5, 33)
    np.testing.assert_array_equal(xh, y)
    np.testing.assert_array_equal(gh, gd)
    for build, fwd, bwd in ((lib.build_activation_function_cuda, lib.ELU_cuda, lib.ELU_derivative_cuda),
                            (lib.build_activation_function, lib.ELU, lib.ELU_derivative)):
        build.restype, build.argtypes = C.POINTER(ppo_ffi.ActivationFunction), [C.c_char_p]
        a = build(b"elu").contents
        assert (a.activation, a.activation_derivative) == (C.cast(fwd, C.c_void_p).value, C.cast(bwd, C.c_void_p).value)
    # a saved network (its own initial weights) loads as an ELU network: the same forward, bit for bit
    nn = lib.create_neural_network(ppo_ffi.c_ints(SIZES), ppo_ffi.c_strings(ELU), len(SIZES))
    path = str(tmp_path / "elu_nn.bin").encode()
    f = LIBC.fopen(path, b"wb")
    lib.save_neural_network(nn, f)
    LIBC.fclose(f)
    f = LIBC.fopen(path, b"rb")
    nets = (nn, lib.load_neural_network(f))
    LIBC.fclose(f)
    dx, outs = dev(lib, _inputs(SIZES, 33, 5)[0]), []
    for net in nets:
        assert [net.contents.activation_functions[i] for i in range(3)] == [b"elu", b"elu", b"none"]
        lib.forward_propagation_cuda(net, dx.ptr, 33)
        outs.append(ppo_ffi.d2h(lib, net.contents.d_output, F32, 33 * SIZES[-1]))
        lib.free_neural_network(net)
    dx.free()
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.parametrize("eng", [1, 0])
def test_one_update(lib, eng):
    """One value and one policy step of an ELU PPO: both networks' first Adam step against elu_ref's gradients (the
    comparison and constants of test_gpu_tanh.py's 5b); bf16 mode declined, nothing replayed from a graph."""
    N, B, S, A = 2200, 1100, SIZES[0], SIZES[-1]
    with engine(lib, eng):
        ppo = _make_ppo(lib, SIZES, ELU, N)
        try:
            p, pol, b = ppo.contents, ppo.contents.policy.contents, ppo.contents.buffer.contents
            assert lib.ppo_set_compute_dtype(ppo, 1) == -1 and p.V.contents.dtype == pol.mu.contents.dtype == 0
            lib.ppo_fill_synthetic(ppo, 4, N // 4, 21, 1.0 / 300)
            lib.ppo_synchronize()
            v0, mu0 = nn_params_packed(lib, p.V), nn_params_packed(lib, pol.mu)
            ls0, old_lp = ppo_ffi.d2h(lib, pol.d_log_std, F32, A), ppo_ffi.d2h(lib, b.d_logprob_p, F32, N)
            state = ppo_ffi.d2h(lib, b.d_state_p, F32, N * S).reshape(N, S)
            action = ppo_ffi.d2h(lib, b.d_action_p, F32, N * A).reshape(N, A)
            lib.ppo_reset_stats(ppo)
            lib.ppo_set_step_limit(ppo, 1, 1)
            lib.ppo_update(ppo, 0.99, B, 1, 1, 1, 77)
            lib.ppo_synchronize()
            assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
            st = (C.c_double * 9)()
            lib.ppo_read_stats(ppo, st, 9)
            assert st[1] == 1 and st[3] == 1 and st[8] == 0
            adv, tgt = (ppo_ffi.d2h(lib, d, F32, N) for d in (b.d_advantage_p, b.d_adv_target_p))
            rv, rp = (_rows_of(nn_input_rows(lib, nn, B), state) for nn in (p.V, pol.mu))
            gV, v1 = nn_grads_packed(lib, p.V), nn_params_packed(lib, p.V)
            gmu, mu1 = nn_grads_packed(lib, pol.mu), nn_params_packed(lib, pol.mu)
        finally:
            lib.free_ppo(ppo)
    gV_ref = E.grads(SIZES[:-1] + [1], ELU, v0, state[rv], lambda y: 2.0 * (y - tgt[rv].astype(F64)[:, None]) / B)
    gmu_ref = E.grads(SIZES, ELU, mu0, state[rp], lambda mu: policy_head_f64(
        mu, ls0, action[rp], adv[rp], old_lp[rp], 0.2, 0.01)["grad_mu"])
    for name, g, g_ref, p0, p1 in (("value", gV, gV_ref, v0, v1), ("policy", gmu, gmu_ref, mu0, mu1)):
        assert_gemm_close(g, g_ref, B, f"engine {eng} {name} grads")
        flips = assert_adam_delta(p1, adam_first_step(p0, g_ref, LR), g_ref, LR, f"engine {eng} {name} params")
        assert flips <= max(2, p1.size // 1000)
