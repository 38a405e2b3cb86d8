"""The multi-discrete policy (csrc/ppo_math.h md_* on the cat_* atoms, csrc/discrete.hip), restated
independently of the kernels, segment by segment on categorical_ref's definitions:

  * head_f64      the definition in float64: D softmaxes side by side, joint lp and H, one surrogate on the joint
                  ratio, each logit's entropy term with its own component's H_d (row_H=True makes the mistake of
                  taking the row's H there: the tests show that the bounds tell the two apart);
  * head_f32      the fp32 mirror in the stated order (k ascending inside a component, d ascending across them);
  * head_bounds   categorical_ref.Err propagated per component exactly as categorical_ref.head_bounds does, plus the
                  D − 1 roundings of each of the two d-sums, plus the gradient with H_d — nothing is taken from a
                  run of the kernels; the mirror has to stay inside them on the CPU (test_multidiscrete_cpu.py);
  * sample_u / sample_f32   the sampler's stream and mirror.

The stream (csrc/rng.h's table): component d of row i reads u01 of word d & 3 of philox(i | (d >> 2) << 32, offset,
key), key and offset the categorical sampler's at each call site."""
import functools

import numpy as np

import categorical_ref as cr
import rng_ref
from categorical_ref import ENT, EPS, F32, F64, U, Err

MD_MAX_D = 256


def offsets(nvec):
    return np.concatenate([[0], np.cumsum(np.asarray(nvec, np.int64))])


def indices(action, nvec):
    """the stored indices [m, D], clamped as cat_index clamps them"""
    a = np.asarray(action)[:, :len(nvec)].astype(np.int64)
    return np.clip(a, 0, np.asarray(nvec, np.int64)[None, :] - 1)


# ------------------------------------------------------------------------------------------------- the head
def head_f64(z, action, adv, old_lp, eps, ent_coeff, nvec, row_H=False):
    """Everything in float64.  Returns per row lp, H, ratio, clipped, dlp, loss_terms; per (row, component) lp_d,
    H_d [m, D]; grad and p [m, A]; and loss."""
    z, adv, old = (np.asarray(v, F64) for v in (z, adv, old_lp))
    m, A = z.shape
    off, a = offsets(nvec), indices(action, nvec)
    assert off[-1] == A
    D = len(nvec)
    zero = np.zeros(m)
    comps = [cr.head_f64(z[:, off[d]:off[d + 1]], a[:, d:d + 1], zero, zero, eps, 0.0) for d in range(D)]
    lp_d = np.stack([c["lp"] for c in comps], axis=1)
    H_d = np.stack([c["H"] for c in comps], axis=1)
    lp, H = lp_d.sum(axis=1), H_d.sum(axis=1)
    with np.errstate(all="ignore"):
        ratio = np.exp(lp - old)
        pos = adv > 0
        clipped = np.where(pos, ratio > 1 + eps, ratio < 1 - eps)
        dlp = np.where(clipped, 0.0, -adv * ratio / m)
        sur = adv * np.where(clipped, np.where(pos, 1 + eps, 1 - eps), ratio)
        grad, p = np.empty((m, A)), np.empty((m, A))
        for d, c in enumerate(comps):
            seg = z[:, off[d]:off[d + 1]]
            zc = seg - seg.max(axis=1, keepdims=True)
            ls = np.log(np.exp(zc).sum(axis=1))
            onehot = np.zeros(seg.shape)
            onehot[np.arange(m), a[:, d]] = 1.0
            Hk = H if row_H else H_d[:, d]
            grad[:, off[d]:off[d + 1]] = (dlp[:, None] * (onehot - c["p"])
                                          + (ent_coeff / m) * c["p"] * ((zc - ls[:, None]) + Hk[:, None]))
            p[:, off[d]:off[d + 1]] = c["p"]
    loss_terms = -sur / m
    return dict(lp=lp, H=H, lp_d=lp_d, H_d=H_d, ratio=ratio, clipped=clipped, dlp=dlp, grad=grad,
                loss_terms=loss_terms, p=p, loss=loss_terms.sum() - ent_coeff * H.sum() / m)


def loss_of(z, action, adv, old_lp, eps, ent_coeff, nvec):
    return head_f64(z, action, adv, old_lp, eps, ent_coeff, nvec)["loss"]


def head_f32(z, action, adv, old_lp, eps, ent_coeff, nvec):
    """The fp32 mirror: per component categorical_ref's order, lp and H summed d ascending, one surrogate."""
    z, adv, old = (np.ascontiguousarray(v, F32) for v in (z, adv, old_lp))
    m, A = z.shape
    off, a = offsets(nvec), indices(action, nvec)
    rows = np.arange(m)
    parts = []
    lp = H = None
    for d in range(len(nvec)):
        seg = np.ascontiguousarray(z[:, off[d]:off[d + 1]])
        M, e, c, t = cr.row_stats_f32(seg)
        s = c[:, -1]
        ls = cr._map("logf", s)
        lpd = (seg[rows, a[:, d]] - M) - ls
        Hd = ls - t / s
        lp = lpd if d == 0 else lp + lpd
        H = Hd if d == 0 else H + Hd
        parts.append((seg, M, e, s, ls, Hd))
    ratio, dlp, sur, clipped = cr.surrogate_f32(adv, lp, old, eps, m)
    cm = F32(ent_coeff) / F32(m)
    grad = np.empty((m, A), F32)
    for d, (seg, M, e, s, ls, Hd) in enumerate(parts):
        p = e / s[:, None]
        onehot = np.zeros(seg.shape, F32)
        onehot[rows, a[:, d]] = 1
        grad[:, off[d]:off[d + 1]] = (dlp[:, None] * (onehot - p)
                                      + cm * p * (((seg - M[:, None]) - ls[:, None]) + Hd[:, None]))
    out = dict(lp=lp, H=H, ratio=ratio, dlp=dlp, sur=sur, grad=grad, clipped=clipped)
    assert all(v.dtype == F32 for n, v in out.items() if n != "clipped")
    return out


def head_bounds(z, action, adv, old_lp, eps, ent_coeff, nvec):
    """Absolute bounds on |device − float64 model| of lp [m], H [m], grad [m, A]; s_rel [m, D] the relative bound of
    a component's s and cumulative sums; ratio_rel [m].  Per component the operations of categorical_ref.head_bounds
    (sums in any order: every partition a kernel may use is covered); the two d-sums as D − 1 fp32 additions each
    (Err.__add__ adds one rounding per addition); the surrogate on the joint lp; the gradient with H_d."""
    z64 = np.asarray(z, F64)
    m, A = z64.shape
    off, a = offsets(nvec), indices(action, nvec)
    rows = np.arange(m)
    col = lambda r: Err(r.v[:, None], r.e[:, None])       # noqa: E731
    parts, s_rel = [], []
    lp = H = None
    for d in range(len(nvec)):
        seg = z64[:, off[d]:off[d + 1]]
        zc = Err.exact(seg) - Err.exact(seg.max(axis=1, keepdims=True))
        e = zc.exp()
        s = e.sum_any_order(axis=1)
        t = (e * zc).sum_any_order(axis=1)
        ls = s.log()
        lpd = Err(zc.v[rows, a[:, d]], zc.e[rows, a[:, d]]) - ls
        Hd = ls - t / s
        lp = lpd if d == 0 else lp + lpd
        H = Hd if d == 0 else H + Hd
        parts.append((zc, e, s, ls, Hd))
        s_rel.append(s.e / s.v)
    x = lp - Err.exact(np.asarray(old_lp, F64))
    rv = np.exp(x.v)
    ratio = Err(rv, rv * np.expm1(x.e) + U * rv + cr.TINY)
    ref = head_f64(z, action, adv, old_lp, eps, ent_coeff, nvec)
    g = (Err.exact(-np.asarray(adv, F64)) * ratio) / Err.exact(F64(m))
    g = Err(np.where(ref["clipped"], 0.0, g.v), np.where(ref["clipped"], 0.0, g.e))
    cm = Err.exact(F64(F32(ent_coeff))) / Err.exact(F64(m))
    grad = np.empty((m, A))
    for d, (zc, e, s, ls, Hd) in enumerate(parts):
        p = e / col(s)
        onehot = np.zeros(zc.v.shape)
        onehot[rows, a[:, d]] = 1.0
        grad[:, off[d]:off[d + 1]] = (col(g) * (Err.exact(onehot) - p) + (cm * p) * ((zc - col(ls)) + col(Hd))).e
    return dict(lp=lp.e, H=H.e, grad=grad, s_rel=np.stack(s_rel, axis=1), ratio_rel=ratio.e / ratio.v)


loss_bound = cr.loss_bound           # the same two cross-row sums over the same per-row terms


# ------------------------------------------------------------------------------------------------- inputs
def mixed_row(nvec):
    """The row that tells H_d from H apart: component 0 flat, component 1 peaked (one logit +15, the others −15) —
    the peaked component's entropy is ≈ 0 while the row's is ≥ ln n_0, and its top logit has p ≈ 1."""
    return 0 if len(nvec) >= 2 else None


@functools.lru_cache(maxsize=None)
def _head_inputs(nvec, m):
    nvec = list(nvec)
    A, D = sum(nvec), len(nvec)
    off = offsets(nvec)
    rng = np.random.default_rng(9500 + 31 * A + D)
    z = (2 * rng.normal(size=(m, A))).astype(F32)
    r = 0
    if D >= 2:                                             # row 0: very different entropies
        z[0, off[0]:off[1]] = F32(0.5)
        z[0, off[1]:off[2]] = F32(-15)
        z[0, off[1] + int(rng.integers(0, nvec[1]))] = F32(15)
        r = 1
    if m > r:                                              # then the ±30 row
        z[r] = rng.permutation(np.linspace(-30, 30, A)).astype(F32)
    if m > r + 1:                                          # then the flat row
        z[r + 1] = F32(0.75)
    act = np.zeros((m, A), F32)
    act[:, :D] = rng.integers(0, np.asarray(nvec)[None, :], (m, D))
    if D >= 2:
        act[0, 1] = np.argmax(z[0, off[1]:off[2]])         # the chosen index of the peaked component is its top
    lp = head_f64(z, act, np.zeros(m), np.zeros(m), EPS, 0.0, nvec)["lp"]

    def draw(n):
        return rng.uniform(0.05, 0.5, n) * rng.choice([-1.0, 1.0], n)

    old = (lp - draw(m)).astype(F32)
    for _ in range(50):
        bad = cr.near_clip(np.exp(lp - old.astype(F64)))
        if not bad.any():
            break
        old[bad] = (lp[bad] - draw(int(bad.sum()))).astype(F32)
    assert not cr.near_clip(np.exp(lp - old.astype(F64))).any()
    adv = rng.normal(size=m).astype(F32)
    adv[5::17] = F32(0.0)
    adv[7::19] = F32(-0.0)
    out = dict(z=z, act=act, adv=adv, old=old)
    for v in out.values():
        v.setflags(write=False)
    return out


def head_inputs(nvec, m=257):
    """As categorical_ref.head_inputs — logits 2·N(0, 1), a ±30 row, a flat row, actions uniform per component,
    adv ~ N(0, 1) with ±0 entries, old_lp = lp − x redrawn until no ratio is within 1e-4 of 1 ± EPS (asserted) — and,
    for D >= 2, row 0 is mixed_row's.  Read-only, shared; fewer rows: the leading ones (rows_of)."""
    return _head_inputs(tuple(int(n) for n in nvec), m)


rows_of = cr.rows_of

# the nvec the GPU tests run, with their row counts
HEAD_NVEC = [[2], [2, 2], [3, 5, 2], [2] * 16, [2] * 17, [11] * 8, [7] * 17, [33, 2], [65, 3, 64]]
HEAD_M = [1, 63, 64, 257]
HEAD_NVEC_WIDE = [[2] * 256, [4096], [2048, 2048], [4094, 2]]
SAMPLE_NVEC = [3, 4, 2, 5, 3, 2, 4, 3, 2]


# ---------------------------------------------------------------------------------------------- the sampler
def sample_u(m, D, key, offset):
    """[m, D] fp32: u01 of word d & 3 of philox(i | (d >> 2) << 32, offset, key)."""
    u = np.empty((m, D), F32)
    rows = np.arange(m, dtype=np.uint64)
    for hi in range((D + 3) // 4):
        w = rng_ref.philox4x32_10(rows | (np.uint64(hi) << np.uint64(32)), offset, key)
        for q in range(4):
            d = 4 * hi + q
            if d < D:
                u[:, d] = rng_ref.u01(w[q] if isinstance(w, tuple) else w[..., q])
    return u


def sample_f32(z, u, nvec):
    """The mirror: indices [m, D], the joint log-prob (d ascending) and margin [m, D] as categorical_ref.sample_f32."""
    z = np.ascontiguousarray(z, F32)
    off = offsets(nvec)
    a, margin, lp = [], [], None
    for d in range(len(nvec)):
        ad, lpd, mg = cr.sample_f32(np.ascontiguousarray(z[:, off[d]:off[d + 1]]), u[:, d])
        a.append(ad)
        margin.append(mg)
        lp = lpd if d == 0 else lp + lpd
    return np.stack(a, axis=1), lp, np.stack(margin, axis=1)


def near_boundary(margin, nvec):
    """rows × components whose threshold is within the bound of a cumulative boundary (categorical_ref's rule, with
    each component's own width)"""
    n = np.asarray(nvec, F64)[None, :]
    return margin <= 2 * (n + 70) * U + 2 * U


def action_rows(a, A):
    act = np.zeros((a.shape[0], A), F32)
    act[:, :a.shape[1]] = a
    return act


@functools.lru_cache(maxsize=None)
def _sample_inputs(nvec, m, shared_row):
    A = sum(nvec)
    rng = np.random.default_rng(9700 + A)
    z = (1.5 * rng.normal(size=(1 if shared_row else m, A))).astype(F32)
    z = np.ascontiguousarray(np.broadcast_to(z, (m, A)))
    z.setflags(write=False)
    return z


def sample_inputs(nvec, m=65536, shared_row=False):
    return _sample_inputs(tuple(nvec), m, shared_row)


# ------------------------------------------------------------------------------- the synthetic environment
def synth_centres(idx, nvec):
    """c_d = 2·a_d/(n_d − 1) − 1 in fp32, [..., D]"""
    n = np.asarray(nvec, F32)
    c = F32(2) * idx.astype(F32) / (n - F32(1)) - F32(1)
    assert c.dtype == F32
    return c
