"""A float64 numpy model of an MLP with "relu" / "tanh" / "none" layers — the reference of the tanh tests.

The oracle (oracle/ref_cpu.c, like the reference) maps every name but "relu" to the identity, so it cannot
judge a tanh network; this model is used the way policy_head_ref.py is: the definition in float64 from the
fp32 inputs as given, plus the fp32 statement of the one expression whose order the kernels fix,

    tanh′ through the post-activation h:   gx = acc − (acc·h)·h        (three fp32 roundings, no fma)

(csrc/dev.h ppo::tanh_bwd).  Parameters are packed [W0, b0, W1, b1, …] with W [out, in], the reference's order
(helpers.nn_params_packed).  Pinned on the CPU in test_tanh_cpu.py."""
import numpy as np

F32 = np.float32
F64 = np.float64


# ------------------------------------------------------------------------------------------ tanh′, both precisions
def tanh_bwd_f32(acc, h):
    """The device expression, operation for operation: fp32 arrays in, every product and the difference rounded
    to fp32 in this order."""
    acc, h = np.asarray(acc, F32), np.asarray(h, F32)
    with np.errstate(all="ignore"):
        t = (acc * h).astype(F32)
        t = (t * h).astype(F32)
        return (acc - t).astype(F32)


def tanh_bwd_f64(acc, h):
    """acc·(1 − h²) in float64 from the fp32 values as given."""
    acc, h = np.asarray(acc, F64), np.asarray(h, F64)
    with np.errstate(all="ignore"):
        return acc * (1.0 - h * h)


# ------------------------------------------------------------------------------------------ the network
def num_params(sizes):
    return sum(sizes[i] * sizes[i + 1] + sizes[i + 1] for i in range(len(sizes) - 1))


def unpack(sizes, params):
    """[(W [out, in], b [out])] in float64 from the packed parameters."""
    params = np.asarray(params, F64)
    out, off = [], 0
    for i in range(len(sizes) - 1):
        n, l = sizes[i], sizes[i + 1]
        W = params[off:off + n * l].reshape(l, n)
        off += n * l
        out.append((W, params[off:off + l]))
        off += l
    assert off == params.size
    return out


def act_f(z, act):
    if act == "tanh":
        return np.tanh(z)
    if act == "relu":
        return np.where(z > 0, z, 0.0)
    return z


def act_bwd(g, h, act):
    """g ⊙ act′ through the POST-activation h."""
    if act == "tanh":
        return g * (1.0 - h * h)
    if act == "relu":
        return np.where(h > 0, g, 0.0)
    return g


def layer_forward(W, b, x, act):
    """(pre-activation z, post-activation h) of one layer, float64."""
    z = np.asarray(x, F64) @ np.asarray(W, F64).T + np.asarray(b, F64)
    return z, act_f(z, act)


def forward(sizes, acts, params, x):
    """hs[i] = the input of layer i (hs[0] = x, hs[L] = the output), zs[i] = layer i's pre-activation."""
    hs, zs = [np.asarray(x, F64)], []
    for (W, b), act in zip(unpack(sizes, params), acts):
        z, h = layer_forward(W, b, hs[-1], act)
        zs.append(z)
        hs.append(h)
    return hs, zs


def layer_backward(W, g, x, act_in):
    """Layer with input x (the post-activation of a layer of kind act_in; "none" for layer 0) and upstream
    gradient g at its pre-activation: (grad_x with act_in's derivative applied, the raw product g·W, grad_W,
    grad_b)."""
    g, x, W = np.asarray(g, F64), np.asarray(x, F64), np.asarray(W, F64)
    acc = g @ W
    return act_bwd(acc, x, act_in), acc, g.T @ x, g.sum(axis=0)


def backward(sizes, acts, params, hs, gout):
    """Packed float64 gradients from the gradient at the network's output (after the output activation)."""
    layers = unpack(sizes, params)
    L = len(layers)
    g = act_bwd(np.asarray(gout, F64), hs[L], acts[L - 1])
    grads = [None] * L
    for i in range(L - 1, -1, -1):
        gx, _, gW, gb = layer_backward(layers[i][0], g, hs[i], acts[i - 1] if i > 0 else "none")
        grads[i] = np.concatenate([gW.ravel(), gb])
        g = gx
    return np.concatenate(grads), g


# ------------------------------------------------------------------------------------------ the update's heads
def value_grads(sizes, acts, params, x, tgt):
    """MSE value step (loss.cu: Σ(t − y)²/m, g = 2(y − t)/m): (packed gradients, y)."""
    hs, _ = forward(sizes, acts, params, x)
    y = hs[-1][:, 0]
    g = 2.0 * (y - np.asarray(tgt, F64)) / y.size
    return backward(sizes, acts, params, hs, g[:, None])[0], y


def gaussian_log_prob(mu, log_std, action):
    mu, ls, a = (np.asarray(v, F64) for v in (mu, log_std, action))
    z = (a - mu) / np.exp(ls)
    return -0.5 * mu.shape[1] * np.log(2 * np.pi) - (ls + 0.5 * z * z).sum(axis=1)


def policy_grads(sizes, acts, params, log_std, x, action, adv, old_lp, eps, ent_coeff):
    """Clipped-surrogate policy step through policy_head_ref.policy_head_f64: (packed μ gradients, ∂/∂log σ, μ)."""
    from policy_head_ref import policy_head_f64

    hs, _ = forward(sizes, acts, params, x)
    head = policy_head_f64(hs[-1], log_std, action, adv, old_lp, eps, ent_coeff)
    return backward(sizes, acts, params, hs, head["grad_mu"])[0], head["gls"], hs[-1]
