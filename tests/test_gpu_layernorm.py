"""Layer normalisation of the hidden layers (csrc/layernorm.hip, ppo_set_layer_norm) against the float64 model and the
worst-case bounds of layernorm_ref.py.  Every test needs entry points the parent does not have.

The kernels alone (the two _device entries) on the crafted rows of layernorm_ref.crafted; position and alignment
independence bit for bit; the network teacher-forced from the GPU's own stored operands as in test_gpu_tanh.py; one
update per engine with the checkpoint round trip."""
import ctypes as C

import numpy as np
import pytest

import layernorm_ref as R
import ppo_ffi
from helpers import F32, assert_gemm_close, dev, gemm_tol, nn_grads_packed, nn_input_rows, nn_params_packed
from policy_head_ref import policy_head_f64
from test_gpu_tanh import LR, SIZES, _inputs, _make_ppo, _net, _params, _rows_of, _stored, engine
from test_gpu_update import adam_first_step, assert_adam_delta

pytestmark = pytest.mark.gpu

F64 = np.float64
EPS = 1e-5
WIDTHS = [1, 3, 16, 63, 64, 65, 128, 129, 257, 1024, 1028, 4096]
KERNEL_CASES = ([(9, l, "relu") for l in WIDTHS] + [(9, l, a) for l in (65, 257) for a in ("none", "tanh", "elu")] +
                [(1, 65, "relu"), (70, 65, "relu")])
SENTINEL = F32(-7.25)


def _run(lib, z, g, act, lead=0, rows=None):
    """ln_fwd then ln_bwd on device arrays that start `lead` floats into their allocations, over `rows` rows (default:
    all): (rc, h, stat, dz)."""
    m, l = z.shape
    pad = lambda a: np.concatenate([np.full(lead, SENTINEL, F32), np.asarray(a, F32).ravel()])  # noqa: E731
    dz_, dg, dh, ds = (dev(lib, pad(a)) for a in (z, g, np.full(m * l, SENTINEL), np.full(2 * m, SENTINEL)))
    at = lambda d: d.ptr + 4 * lead  # noqa: E731
    try:
        kind = R.ACT_KINDS[act]
        n = m if rows is None else rows
        rc = (lib.ppo_layer_norm_fwd_device(at(dz_), at(dh), at(ds), n, l, kind, EPS),
              lib.ppo_layer_norm_bwd_device(at(dg), at(dz_), at(dh), at(ds), n, l, kind))
        lib.ppo_synchronize()
        assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
        h, st, dz = (d.to_numpy(F32, lead + n)[lead:] for d, n in ((dh, m * l), (ds, 2 * m), (dg, m * l)))
        return rc, h.reshape(m, l), st.reshape(m, 2), dz.reshape(m, l)
    finally:
        for d in (dz_, dg, dh, ds):
            d.free()


_RUNS = {}


def _case(lib, m, l, act):
    if (m, l, act) not in _RUNS:
        z, g = R.crafted(m, l, 1000 * l + m)
        _RUNS[m, l, act] = (z, g) + _run(lib, z, g, act)
    return _RUNS[m, l, act]


@pytest.mark.parametrize("m,l,act", KERNEL_CASES)
def test_kernel_forward_backward(lib, m, l, act):
    z, g, rc, h, st, dz = _case(lib, m, l, act)
    assert rc == (0, 0) and all(np.isfinite(v).all() for v in (h, st, dz))
    ef = np.abs(h - R.forward(z, EPS, act)[0]) / R.tol_fwd(z, EPS)[0]
    tb = R.tol_bwd(g, z, h, EPS, act)
    eb = np.abs(dz - R.backward(g, z, h, EPS, act)[0])
    print(f"m={m} l={l} {act}: worst err/tol forward {ef.max():.3g}, backward {(eb / np.maximum(tb, 1e-300)).max():.3g}")
    assert (ef <= 1).all() and (eb <= tb).all()
    if act == "relu":
        np.testing.assert_array_equal(h > 0, h != 0)


@pytest.mark.parametrize("m,l,act", [c for c in KERNEL_CASES if c[2] == "relu"])
def test_kernel_stat(lib, m, l, act):
    z, _, _, _, st, _ = _case(lib, m, l, act)
    _, mean, r, _ = R.forward(z, EPS, act)
    _, tm, tr = R.tol_fwd(z, EPS)
    em, er = np.abs(st[:, 0] - mean) / np.maximum(tm, 1e-300), np.abs(st[:, 1] - r) / tr
    print(f"m={m} l={l}: err/tol per row, mean {np.round(em, 3)}, rstd {np.round(er, 3)}")
    assert (np.abs(st[:, 0] - mean) <= tm).all() and (er <= 1).all()


@pytest.mark.parametrize("m,l", [(9, 4097), (0, 65)])
def test_kernel_declines(lib, m, l):
    rc, h, st, dz = _run(lib, np.ones((9, l), F32), np.full((9, l), 2, F32), "relu", rows=m)
    assert rc == (-1, -1) and (h == SENTINEL).all() and (st == SENTINEL).all() and (dz == 2).all()


@pytest.mark.parametrize("act", ["relu", "elu"])
@pytest.mark.parametrize("l", [72, 65])
def test_row_bits_do_not_depend_on_position_or_alignment(lib, l, act):
    z, g = R.crafted(70, l, l)
    z[68], g[68] = z[5] * 3, g[5]
    whole = _run(lib, z, g, act)[1:]
    alone = _run(lib, z[68:69], g[68:69], act)[1:]
    shifted = _run(lib, z[68:69], g[68:69], act, lead=1)[1:]
    again = _run(lib, z, g, act)[1:]
    for w, a, s, w2 in zip(whole, alone, shifted, again):
        assert w[68].tobytes() == a[0].tobytes() == s[0].tobytes() and w.tobytes() == w2.tobytes()


@pytest.mark.parametrize("sizes,acts,m,eng", [(SIZES, a, m, e) for a in (["relu", "relu", "none"], ["elu", "tanh", "none"])
                                              for m in (1100, 7) for e in (1, 0)] +
                         [([12, 72, 72, 3], ["relu", "relu", "none"], 7, 1)])
def test_network_layers(lib, sizes, acts, m, eng):
    what = f"{acts} {sizes} m={m} engine={eng}"
    params = _params(sizes, 100 + m)
    x, gout = _inputs(sizes, m, 200 + m)
    nn = _net(lib, sizes, acts, params)
    dx, dg = dev(lib, x), dev(lib, gout)
    L = len(sizes) - 1
    try:
        assert lib.nn_set_layer_norm(nn, EPS) == 0 and lib.nn_set_compute_dtype(nn, 1) == -1
        with engine(lib, eng):
            lib.forward_propagation_cuda(nn, dx.ptr, m)
            hs = _stored(lib, nn, m, "d_input")
            hs[0] = nn_input_rows(lib, nn, m)
            zs = []
            for i in range(L - 1):
                zs.append(np.empty((m, sizes[i + 1]), F32))
                assert lib.ppo_nn_ln_rows(nn, i, zs[i].ctypes.data, None, m) == 0
            assert lib.ppo_nn_ln_rows(nn, L - 1, None, None, m) == -1
            lib.backward_propagation_cuda(nn, dg.ptr, m)
            gs = _stored(lib, nn, m, "d_grad_x")      # gs[i + 1], i hidden: ∂/∂z of layer i (rewritten in place)
            packed = nn_grads_packed(lib, nn)
        assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    finally:
        lib.free_neural_network(nn)
        dx.free()
        dg.free()
    layers, off = R.E_.unpack(sizes, params), 0
    for i, ((W, b), act) in enumerate(zip(layers, acts)):
        n, l = sizes[i], sizes[i + 1]
        z_ref = hs[i].astype(F64) @ W.T + b
        if i < L - 1:
            for rows in (slice(0, 1), slice(1, m)):
                assert np.abs(zs[i][rows] - z_ref[rows]).max() <= gemm_tol(z_ref[rows], n), f"{what} z layer {i}"
            assert (np.abs(hs[i + 1] - R.forward(zs[i], EPS, act)[0]) <= R.tol_fwd(zs[i], EPS)[0]).all(), f"{what} h {i}"
            g_ref = gs[i + 2].astype(F64) @ layers[i + 1][0]
            dz_ref = R.backward(g_ref, zs[i], hs[i + 1], EPS, act)[0]
            tol = R.tol_bwd(g_ref, zs[i], hs[i + 1], EPS, act, gemm=gemm_tol(g_ref, sizes[i + 2]))
            assert np.isfinite(gs[i + 1]).all() and (np.abs(gs[i + 1] - dz_ref) <= tol).all(), f"{what} dz layer {i}"
        else:
            assert np.abs(hs[i + 1] - z_ref).max() <= gemm_tol(z_ref, n), f"{what} output layer"
        assert_gemm_close(packed[off:off + n * l].reshape(l, n), gs[i + 1].astype(F64).T @ hs[i], m, f"{what} grad_W {i}")
        assert_gemm_close(packed[off + n * l:off + n * l + l], gs[i + 1].astype(F64).sum(axis=0), m, f"{what} grad_b {i}")
        off += n * l + l


@pytest.mark.parametrize("eng", [1, 0])
def test_one_update(lib, eng, tmp_path):
    """One value and one policy step of a normalised ReLU PPO (the shape of test_gpu_elu.py::test_one_update), then the
    checkpoint round trip."""
    N, B, S, A = 2200, 1100, SIZES[0], SIZES[-1]
    RELU = ["relu", "relu", "none"]
    with engine(lib, eng):
        ppo = _make_ppo(lib, SIZES, RELU, N)
        twin = None
        try:
            p, pol, b = ppo.contents, ppo.contents.policy.contents, ppo.contents.buffer.contents
            assert lib.ppo_get_layer_norm(ppo) == 0 and lib.ppo_nn_ln_rows(p.V, 0, None, None, 1) == -1
            assert lib.ppo_set_layer_norm(ppo, -1.0) == -1 and lib.ppo_set_layer_norm(ppo, float("nan")) == -1
            assert lib.ppo_set_layer_norm(ppo, EPS) == 0 and lib.ppo_get_layer_norm(ppo) == F32(EPS)
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
            # the checkpoint keeps the setting; the loaded PPO acts as the original does, bit for bit
            path = str(tmp_path / "ln.ckpt").encode()
            assert lib.ppo_save_state(ppo, path, 0) == 0
            twin = lib.ppo_load_state(path, None, 0)
            assert twin and lib.ppo_get_layer_norm(twin) == F32(EPS)
            dobs, acts = dev(lib, state[:33]), []
            for q in (ppo, twin):
                da = dev(lib, np.zeros((33, A), F32))
                assert lib.ppo_act_device(q, dobs.ptr, 33, 1, 0, 0, da.ptr, None) == 0
                lib.ppo_synchronize()
                acts.append(da.to_numpy(F32, 33 * A))
                da.free()
            dobs.free()
            assert acts[0].tobytes() == acts[1].tobytes() and np.isfinite(acts[0]).all()
            assert lib.ppo_set_layer_norm(ppo, 0.0) == 0 and lib.ppo_get_layer_norm(ppo) == 0
            assert lib.ppo_nn_ln_rows(p.V, 0, None, None, 1) == -1
        finally:
            lib.free_ppo(ppo)
            if twin:
                lib.free_ppo(twin)
    gV_ref = R.grads(SIZES[:-1] + [1], RELU, v0, state[rv], lambda y: 2.0 * (y - tgt[rv].astype(F64)[:, None]) / B, EPS)
    gmu_ref = R.grads(SIZES, RELU, mu0, state[rp], lambda mu: policy_head_f64(
        mu, ls0, action[rp], adv[rp], old_lp[rp], 0.2, 0.01)["grad_mu"], EPS)
    for name, g, g_ref, p0, p1 in (("value", gV, gV_ref, v0, v1), ("policy", gmu, gmu_ref, mu0, mu1)):
        assert_gemm_close(g, g_ref, B, f"engine {eng} {name} grads")
        flips = assert_adam_delta(p1, adam_first_step(p0, g_ref, LR), g_ref, LR, f"engine {eng} {name} params")
        assert flips <= max(2, p1.size // 1000)
