"""A float64 numpy model of an MLP with "elu" (α = 1) / "tanh" / "relu" / "none" layers, on tanh_ref.py and built the
same way: the definitions in float64 from the fp32 values as given, plus the fp32 statement of the one expression
whose order the kernels fix (csrc/dev.h ppo::elu_bwd): gx = h > 0 ? a : a·(h + 1), two roundings (sum, product), no
fma.  Parameters are packed as in tanh_ref.  Pinned on the CPU in test_elu_cpu.py."""
import numpy as np

import tanh_ref as T
from tanh_ref import F32, F64, unpack  # noqa: F401  (unpack: for the tests)


def elu_bwd_f32(a, h):
    """The device expression, operation for operation.  NaN in h fails the comparison and gives a·NaN."""
    a, h = np.asarray(a, F32), np.asarray(h, F32)
    with np.errstate(all="ignore"):
        return np.where(h > 0, a, (a * (h + F32(1)).astype(F32)).astype(F32))


def act_f(z, act):
    if act != "elu":
        return T.act_f(z, act)
    with np.errstate(all="ignore"):
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


def act_bwd(g, h, act):             # g ⊙ act′ through the POST-activation h, float64
    return np.where(h > 0, g, g * (h + 1.0)) if act == "elu" else T.act_bwd(g, h, act)


def layer_forward(W, b, x, act):    # (pre-activation z, post-activation h) of one layer, float64
    z = np.asarray(x, F64) @ np.asarray(W, F64).T + np.asarray(b, F64)
    return z, act_f(z, act)


def layer_backward(W, g, h_in, act_in):
    """Layer with input h_in (the post-activation of a layer of kind act_in; "none" for layer 0) and upstream gradient
    g: (grad_x — below an ELU layer the fp32 statement on the float64 product rounded to fp32 — the float64 product
    acc = g·W, grad_W, grad_b)."""
    g, h_in, W = np.asarray(g, F64), np.asarray(h_in, F64), np.asarray(W, F64)
    acc = g @ W
    gx = elu_bwd_f32(acc.astype(F32), h_in.astype(F32)).astype(F64) if act_in == "elu" else act_bwd(acc, h_in, act_in)
    return gx, acc, g.T @ h_in, g.sum(axis=0)


def grads(sizes, acts, params, x, gout_of):
    """Packed float64 gradients of the network at input x, gout_of(output) being the gradient at its output (the
    output layer is "none" in every use); float64 throughout."""
    layers = unpack(sizes, params)
    hs = [np.asarray(x, F64)]
    for (W, b), act in zip(layers, acts):
        hs.append(layer_forward(W, b, hs[-1], act)[1])
    g, out = np.asarray(gout_of(hs[-1]), F64), []
    for i in range(len(layers) - 1, -1, -1):
        out.insert(0, np.concatenate([(g.T @ hs[i]).ravel(), g.sum(axis=0)]))
        g = act_bwd(g @ layers[i][0], hs[i], acts[i - 1] if i > 0 else "none")
    return np.concatenate(out)
