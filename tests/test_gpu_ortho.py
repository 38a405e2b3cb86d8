"""Orthogonal initialisation on the device (csrc/ortho.hip) against numpy.linalg.qr in float64."""
import ctypes as C

import numpy as np
import pytest

import ppo_ffi
from helpers import dev, nn_params_packed

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
SHAPES = [(1, 64), (64, 1), (2, 2), (17, 64), (64, 17), (65, 65), (67, 130), (130, 67), (1025, 3)]


def ortho_ref(G, gain):
    """torch.nn.init.orthogonal_'s definition in float64: Q of the tall orientation, columns signed by diag R"""
    M = G.astype(F64) if G.shape[0] >= G.shape[1] else G.astype(F64).T
    Q, R = np.linalg.qr(M)
    Q = Q * np.where(np.diag(R) < 0, -1.0, 1.0)
    return gain * (Q if G.shape[0] >= G.shape[1] else Q.T)


def gram_error(W, gain):
    Wf = W.astype(F64) / gain
    gram = Wf.T @ Wf if W.shape[0] >= W.shape[1] else Wf @ Wf.T
    return np.abs(gram - np.eye(gram.shape[0])).max()


def run(lib, G, gain):
    d = dev(lib, G)
    try:
        assert lib.ppo_orthogonal_device(d.ptr, G.shape[0], G.shape[1], gain) == 0
        assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
        return d.to_numpy(F32, G.size).reshape(G.shape)
    finally:
        d.free()


@pytest.mark.parametrize("gain", [1.0, float(np.sqrt(2))])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_matches_float64_qr(lib, rows, cols, gain):
    """|W − g·Q| <= 2⁻²⁴|g·Q| + 8·T·2⁻⁵³·κ₂(G)·g: the one fp32 rounding plus the Householder forward error of Q; and
    max|WᵀW/g² − I| <= 2⁻²²: a rounding of 2⁻²⁴ per element moves a Gram entry by at most 2·2⁻²⁴, the bound twice that"""
    G = np.random.default_rng(1000 * rows + cols).standard_normal((rows, cols)).astype(F32)
    g = float(F32(gain))
    W, ref = run(lib, G, g), ortho_ref(G, g)
    bound = 2.0 ** -24 * np.abs(ref) + 8 * max(rows, cols) * 2.0 ** -53 * np.linalg.cond(G.astype(F64)) * g
    err = np.abs(W.astype(F64) - ref)
    print(f"{rows}x{cols} gain {g:.4f}: worst err / bound {float((err / bound).max()):.3f}, {(W != ref.astype(F32)).sum()} "
          f"of {W.size} elements off the rounded reference, Gram error {gram_error(W, g):.3g} of {2.0 ** -22:.3g}")
    assert (err <= bound).all()
    assert gram_error(W, g) <= 2.0 ** -22


def test_zero_column_and_arguments(lib):
    G = np.random.default_rng(5).standard_normal((40, 9)).astype(F32)
    G[:, 4] = 0
    assert np.isfinite(run(lib, G, 1.0)).all() and np.isfinite(run(lib, np.ascontiguousarray(G.T), 1.0)).all()
    d = dev(lib, G)
    bad = [(0, 9, 1.0), (40, 0, 1.0), (-1, 9, 1.0), (1025, 1025, 1.0), (4097, 1, 1.0), (1, 4097, 1.0), (40, 9, 0.0),
           (40, 9, -1.0), (40, 9, float("nan")), (40, 9, float("inf"))]
    assert all(lib.ppo_orthogonal_device(d.ptr, r, c, g) == -1 for r, c, g in bad)
    assert lib.ppo_orthogonal_device(None, 40, 9, 1.0) == -1
    assert d.to_numpy(F32, G.size).tobytes() == G.tobytes() and lib.ppo_last_error() in (b"", None)
    d.free()


def layers_of(lib, nn_ptr):
    """[(W [out, in], b [out])] of a network, from the device"""
    nn, p, out = nn_ptr.contents, nn_params_packed(lib, nn_ptr), []
    for i in range(nn.num_layers - 1):
        n_out, n_in = nn.layers[i].output_size, nn.layers[i].input_size
        out.append((p[:n_out * n_in].reshape(n_out, n_in), p[n_out * n_in:n_out * n_in + n_out]))
        p = p[n_out * n_in + n_out:]
    return out


@pytest.mark.parametrize("dtype", [0, 1])
def test_ppo_init_orthogonal(lib, dtype):
    sizes, acts, gains = [5, 64, 33, 3], ["relu", "relu", "none"], (float(F32(np.sqrt(2))), 0.01, 1.0)

    def make(seed):
        ppo = lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), 4, 256, 3e-4, 3e-4, 0.95, 0.2, 0.0, 0.7, True)
        assert lib.ppo_set_compute_dtype(ppo, dtype) == 0
        assert seed is None or lib.ppo_init_orthogonal(ppo, seed, *gains) == 0
        return ppo

    def bits(ppo):
        pol = ppo.contents.policy.contents
        return b"".join(nn_params_packed(lib, n).tobytes() for n in (pol.mu, ppo.contents.V))

    ppo, plain = make(11), make(None)
    pol = ppo.contents.policy.contents
    log_std = lambda p: ppo_ffi.d2h(lib, p.contents.policy.contents.d_log_std, F32, 3).tobytes()         # noqa: E731
    assert log_std(ppo) == log_std(plain)
    weights = []
    for nn, g_out in ((pol.mu, gains[1]), (ppo.contents.V, gains[2])):
        ls = layers_of(lib, nn)
        for i, (W, b) in enumerate(ls):
            assert gram_error(W, g_out if i == len(ls) - 1 else gains[0]) <= 2.0 ** -22
            assert (b.view(np.uint32) == 0).all()
            weights.append(W)
        lib.nn_write_weights_to_host(nn)                        # the host mirrors equal the device weights
        for i, (W, b) in enumerate(ls):
            assert np.ctypeslib.as_array(nn.contents.layers[i].weights, (W.size,)).tobytes() == W.tobytes()
    for i, a in enumerate(weights):                             # no two equal-shaped layers share a draw
        assert not any(np.array_equal(np.abs(a), np.abs(b)) for b in weights[i + 1:])
    same, other = make(11), make(12)
    assert bits(same) == bits(ppo) != bits(other)
    for bad in [(None, 1, 1.0, 1.0, 1.0)] + [(ppo, 1) + tuple(g if k == j else 1.0 for k in range(3))
                                             for j in range(3) for g in (0.0, -1.0, float("nan"), float("inf"))]:
        assert lib.ppo_init_orthogonal(*bad) == -1
    assert bits(same) == bits(ppo)
    lib.ppo_fill_synthetic(ppo, 4, 64, 3, 1.0 / 500)
    lib.ppo_update(ppo, 0.99, 64, 1, 1, 1, 7)
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    after = bits(ppo)
    assert after != bits(same) and np.isfinite(np.frombuffer(after, F32)).all()
    assert lib.ppo_init_orthogonal(ppo, 11, *gains) == -1 and bits(ppo) == after
    for p in (ppo, plain, same, other):
        lib.free_ppo(p)
