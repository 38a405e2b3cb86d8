"""A float64 numpy model of layer normalisation without scale or shift between a hidden layer's GEMM and its activation
(csrc/layernorm.hip, csrc/dev.h ln_*), on elu_ref.py's activations, plus worst-case fp32 error bounds.

    mean = Σ z_j / l,  d_j = z_j − mean,  var = Σ d_j² / l,  r = 1/sqrt(var + eps),  ẑ_j = d_j·r,  h_j = act(ẑ_j)
    a_j = act′·g_j,  s1 = Σ a_j / l,  s2 = Σ a_j·ẑ_j / l,  ∂loss/∂z_j = r·((a_j − s1) − ẑ_j·s2)

Bounds, with u = 2⁻²⁴ and E = (l + 8)·u — the l·u bound of an fp32 sum of l terms in ANY order, carried through the
expressions, plus eight roundings of slack for the divisions, the square root and the products; r, ẑ, a, dz from this
model, c = r·max_k|z_k| (how much of z cancels in z − mean), A1 = mean|a|, A2 = mean|a·ẑ|:
    |mean err| <= E·max|z|      |r err| <= E·r      tol_fwd_j = E·(c + |ẑ_j|)
    tol_bwd_j = E·r·(|a_j| + A1 + (c + |ẑ_j|)·A2 + |ẑ_j|·(2·A2 + c·A1)) + E·|dz_j|
They are not fitted to any kernel (test_layernorm_cpu.py pins them against an fp32 restatement in two sum orders).
The bound on r needs the corrected two-pass variance, Σ d²/l − (Σ d/l)² (zero correction in exact arithmetic, so not
in this model): without it the fp32 mean's own error enters var squared, 100× over E·r on the cancellation row.
In a network the upper gradient g is itself a GEMM's output with |δg| <= G = helpers.gemm_tol; act′ <= 1 carries it to
|δa| <= G, and the same expression gives tol_bwd_gemm_j = r·G·(2 + |ẑ_j|·mean|ẑ|)."""
import numpy as np

import elu_ref as E_

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
ACT_KINDS = {"none": 0, "relu": 1, "tanh": 2, "elu": 3}


def forward(z, eps, act):
    """(h, mean [m], r [m], ẑ) in float64 from the fp32 z as given."""
    z = np.asarray(z, F64)
    mean = z.mean(axis=1)
    d = z - mean[:, None]
    r = 1.0 / np.sqrt((d * d).mean(axis=1) + eps)
    zh = d * r[:, None]
    return E_.act_f(zh, act), mean, r, zh


def backward(g, z, h, eps, act):
    """(∂loss/∂z, a, ẑ, r); act′ through the post-activation h as given — the GPU's stored h when teacher-forced, so
    a ReLU unit whose ẑ rounds across 0 is taken on the side the GPU took."""
    _, _, r, zh = forward(z, eps, act)
    a = E_.act_bwd(np.asarray(g, F64), np.asarray(h, F64), act)
    s1, s2 = a.mean(axis=1, keepdims=True), (a * zh).mean(axis=1, keepdims=True)
    return r[:, None] * ((a - s1) - zh * s2), a, zh, r


def tol_fwd(z, eps):
    """(tol_fwd [m, l], the bound on mean [m], the bound on r [m])"""
    z = np.asarray(z, F64)
    _, _, r, zh = forward(z, eps, "none")
    E, zmax = (z.shape[1] + 8) * U, np.abs(z).max(axis=1)
    return E * ((r * zmax)[:, None] + np.abs(zh)), E * zmax, E * r


def tol_bwd(g, z, h, eps, act, gemm=0.0):
    z = np.asarray(z, F64)
    dz, a, zh, r = backward(g, z, h, eps, act)
    E, c = (z.shape[1] + 8) * U, (r * np.abs(z).max(axis=1))[:, None]
    A1, A2 = np.abs(a).mean(axis=1, keepdims=True), np.abs(a * zh).mean(axis=1, keepdims=True)
    az, r = np.abs(zh), r[:, None]
    return (E * r * (np.abs(a) + A1 + (c + az) * A2 + az * (2 * A2 + c * A1)) + E * np.abs(dz) +
            r * gemm * (2 + az * az.mean(axis=1, keepdims=True)))


def f32_model(z, g, eps, act, pairwise):
    """The stated arithmetic in numpy float32, one rounding per operation, sums sequential or pairwise:
    (h, mean, r, ∂loss/∂z).  act′ from its own ẑ / h."""
    def total(v):
        if pairwise:
            return np.add.reduce(v, axis=1, dtype=F32)          # numpy's pairwise tree
        s = np.zeros(v.shape[0], F32)
        for j in range(v.shape[1]):
            s = (s + v[:, j]).astype(F32)
        return s
    z, g, l, eps = np.asarray(z, F32), np.asarray(g, F32), F32(z.shape[1]), F32(eps)
    mean = total(z) / l
    d = z - mean[:, None]
    c = total(d) / l                                            # the corrected two-pass variance (dev.h ln_rstd)
    r = F32(1) / np.sqrt(np.maximum(total(d * d) / l - c * c, F32(0)) + eps)
    zh = d * r[:, None]
    h = E_.act_f(zh.astype(F64), act).astype(F32)
    a = E_.act_bwd(g.astype(F64), h.astype(F64), act).astype(F32)
    s1, s2 = total(a) / l, total(a * zh) / l
    dz = r[:, None] * ((a - s1[:, None]) - zh * s2[:, None])
    assert all(v.dtype == F32 for v in (h, mean, r, dz))
    return h, mean, r, dz


def crafted(m, l, seed):
    """The kernel tests' inputs: z [m, l] — row 0 scaled ×50, row 1 = 1000 + 1e-3·N(0, 1) (cancellation), row 2 constant
    0.37, row 3 scaled 3e-3 (var ≈ eps), row 4 one-hot, the rest N(0, 1) — and g ~ U(−1, 1)."""
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(m, l))
    z[0] *= 50
    if m > 4:
        z[1] = 1000 + 1e-3 * z[1]
        z[2] = 0.37
        z[3] *= 3e-3
        z[4] = 0
        z[4, l // 2] = 1
    return z.astype(F32), rng.uniform(-1, 1, (m, l)).astype(F32)


def grads(sizes, acts, params, x, gout_of, eps):
    """Packed float64 gradients of the network with every hidden layer normalised, in the shape of elu_ref.grads."""
    layers = E_.unpack(sizes, params)
    L = len(layers)
    hs, zs = [np.asarray(x, F64)], []
    for i, ((W, b), act) in enumerate(zip(layers, acts)):
        z = hs[-1] @ W.T + b
        zs.append(z)
        hs.append(forward(z, eps, act)[0] if i < L - 1 else E_.act_f(z, act))
    g, out = np.asarray(gout_of(hs[-1]), F64), []
    for i in range(L - 1, -1, -1):
        if i < L - 1:
            g = backward(g, zs[i], hs[i + 1], eps, acts[i])[0]
        out.insert(0, np.concatenate([(g.T @ hs[i]).ravel(), g.sum(axis=0)]))
        g = g @ layers[i][0]
    return np.concatenate(out)
