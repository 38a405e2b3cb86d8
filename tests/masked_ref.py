"""Invalid-action masking (csrc/ppo_math.h "Action masking", csrc/discrete.hip), restated independently of the kernels
on multidiscrete_ref's and categorical_ref's definitions:

  * pack / unpack / effective   the storage (W = (A + 31) // 32 words a row, bit k & 31 of word k >> 5 = column k
                  allowed) and the effective mask of a component: its stored bits; none set = all allowed; where a
                  chosen action exists, its column OR-ed in;
  * head_f64      the definition in float64: every component's softmax over its allowed columns only, masked columns
                  never read (zero_p=True makes the mistake of an unmasked softmax whose p is zeroed afterwards: the
                  tests show that the bounds tell the two apart);
  * head_f32      the fp32 mirror in the stated order (k ascending over the allowed columns, d ascending);
  * head_bounds   categorical_ref.Err propagated exactly as multidiscrete_ref.head_bounds does, the two sums of a
                  component over its allowed columns (n_allowed − 1 roundings) — nothing is taken from a run of the
                  kernels; the mirror has to stay inside them on the CPU (test_masked_cpu.py); with a full mask they
                  are multidiscrete_ref's;
  * sample_f32 / argmax   the sampler's mirror (the stream is multidiscrete_ref.sample_u's) and the greedy action;
  * make_mask / head_inputs   the mask generator with its pinned edge rows, and the head's input sets, whose masked
                  logit columns hold a rotating pattern of NaN, +inf, −inf, 1e30 and ordinary values."""
import functools

import numpy as np

import categorical_ref as cr
import multidiscrete_ref as md
from categorical_ref import EPS, F32, F64, U, Err

offsets, indices, loss_bound, near_boundary, sample_u, rows_of = (md.offsets, md.indices, md.loss_bound,
                                                                   md.near_boundary, md.sample_u, md.rows_of)


# ------------------------------------------------------------------------------------------------ the storage
def words(A):
    return (A + 31) // 32


def pack(allowed):
    """bool [m, A] → uint32 [m, W]"""
    allowed = np.asarray(allowed, bool)
    m, A = allowed.shape
    bits = np.zeros((m, words(A) * 32), np.uint64)
    bits[:, :A] = allowed
    w = (bits.reshape(m, -1, 32) << np.arange(32, dtype=np.uint64)[None, None, :]).sum(axis=2)
    return np.ascontiguousarray(w.astype(np.uint32))


def unpack(mask, A):
    """uint32 [m, W] → bool [m, A]; bits at k >= A are ignored"""
    mask = np.asarray(mask, np.uint32)
    k = np.arange(A)
    return ((mask[:, k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(bool)


def effective(stored, nvec, a=None):
    """The effective mask [m, A] of the stored bits [m, A] (bool): per component rule 2 (none set: all allowed), then
    rule 3 (a [m, D] the chosen indices, or None: no action exists)."""
    eff = np.array(stored, bool)
    off = offsets(nvec)
    rows = np.arange(eff.shape[0])
    for d in range(len(nvec)):
        seg = eff[:, off[d]:off[d + 1]]
        seg[~seg.any(axis=1)] = True
        if a is not None:
            seg[rows, a[:, d]] = True
    return eff


# ------------------------------------------------------------------------------------------------- the head
def head_f64(z, action, adv, old_lp, eps, ent_coeff, nvec, stored, zero_p=False):
    """Everything in float64, multidiscrete_ref.head_f64's expressions over the allowed columns.  Returns what it
    returns, plus eff [m, A].  A masked column's logit is replaced before anything reads it."""
    adv, old = (np.asarray(v, F64) for v in (adv, old_lp))
    m, A = np.shape(z)
    off, a = offsets(nvec), indices(action, nvec)
    assert off[-1] == A
    D = len(nvec)
    eff = effective(stored, nvec, a)
    soft = np.ones_like(eff) if zero_p else eff          # the columns the softmax runs over
    z = np.where(soft, np.asarray(z, F64), 0.0)
    rows = np.arange(m)
    comps = []
    with np.errstate(all="ignore"):
        for d in range(D):
            seg, ok = z[:, off[d]:off[d + 1]], soft[:, off[d]:off[d + 1]]
            M = np.where(ok, seg, -np.inf).max(axis=1, keepdims=True)
            zc = np.where(ok, seg - M, 0.0)
            e = np.where(ok, np.exp(zc), 0.0)
            s = e.sum(axis=1)
            ls = np.log(s)
            comps.append(dict(zc=zc, e=e, s=s, ls=ls, lp=zc[rows, a[:, d]] - ls, p=e / s[:, None],
                              H=ls - (e * zc).sum(axis=1) / s))
        lp_d = np.stack([c["lp"] for c in comps], axis=1)
        H_d = np.stack([c["H"] for c in comps], axis=1)
        lp, H = lp_d.sum(axis=1), H_d.sum(axis=1)
        ratio = np.exp(lp - old)
        pos = adv > 0
        clipped = np.where(pos, ratio > 1 + eps, ratio < 1 - eps)
        dlp = np.where(clipped, 0.0, -adv * ratio / m)
        sur = adv * np.where(clipped, np.where(pos, 1 + eps, 1 - eps), ratio)
        grad, p = np.empty((m, A)), np.empty((m, A))
        for d, c in enumerate(comps):
            onehot = np.zeros(c["zc"].shape)
            onehot[rows, a[:, d]] = 1.0
            g = (dlp[:, None] * (onehot - c["p"])
                 + (ent_coeff / m) * c["p"] * ((c["zc"] - c["ls"][:, None]) + H_d[:, d][:, None]))
            grad[:, off[d]:off[d + 1]] = np.where(eff[:, off[d]:off[d + 1]], g, 0.0)
            p[:, off[d]:off[d + 1]] = np.where(eff[:, off[d]:off[d + 1]], c["p"], 0.0)
    loss_terms = -sur / m
    return dict(lp=lp, H=H, lp_d=lp_d, H_d=H_d, ratio=ratio, clipped=clipped, dlp=dlp, grad=grad,
                loss_terms=loss_terms, p=p, eff=eff, loss=loss_terms.sum() - ent_coeff * H.sum() / m)


def loss_of(z, action, adv, old_lp, eps, ent_coeff, nvec, stored):
    return head_f64(z, action, adv, old_lp, eps, ent_coeff, nvec, stored)["loss"]


def row_stats_f32(z, ok):
    """categorical_ref.row_stats_f32 over the allowed columns ok [m, n]: M, e, the cumulative sums c (a masked column
    repeats its predecessor's), t — k ascending, fp32.  z is already free of masked values."""
    z = np.ascontiguousarray(z, F32)
    m, n = z.shape
    M = np.where(ok, z, F32(-np.inf)).max(axis=1).astype(F32)
    e = cr._map("expf", np.where(ok, z - M[:, None], F32(0)))
    c = np.empty((m, n), F32)
    s, t = np.zeros(m, F32), np.zeros(m, F32)
    for k in range(n):
        s = np.where(ok[:, k], s + e[:, k], s)
        c[:, k] = s
        t = np.where(ok[:, k], t + e[:, k] * (z[:, k] - M), t)
    return M, e, c, t


def head_f32(z, action, adv, old_lp, eps, ent_coeff, nvec, stored):
    """The fp32 mirror: multidiscrete_ref.head_f32 over the allowed columns; masked gradient elements are +0."""
    adv, old = (np.ascontiguousarray(v, F32) for v in (adv, old_lp))
    m, A = np.shape(z)
    off, a = offsets(nvec), indices(action, nvec)
    eff = effective(stored, nvec, a)
    z = np.where(eff, np.asarray(z, F32), F32(0))
    rows = np.arange(m)
    parts = []
    lp = H = None
    for d in range(len(nvec)):
        seg, ok = np.ascontiguousarray(z[:, off[d]:off[d + 1]]), eff[:, off[d]:off[d + 1]]
        M, e, c, t = row_stats_f32(seg, ok)
        s = c[:, -1]
        ls = cr._map("logf", s)
        lpd = (seg[rows, a[:, d]] - M) - ls
        Hd = ls - t / s
        lp = lpd if d == 0 else lp + lpd
        H = Hd if d == 0 else H + Hd
        parts.append((seg, ok, M, e, s, ls, Hd))
    ratio, dlp, sur, clipped = cr.surrogate_f32(adv, lp, old, eps, m)
    cm = F32(ent_coeff) / F32(m)
    grad = np.empty((m, A), F32)
    for d, (seg, ok, M, e, s, ls, Hd) in enumerate(parts):
        p = e / s[:, None]
        onehot = np.zeros(seg.shape, F32)
        onehot[rows, a[:, d]] = 1
        g = dlp[:, None] * (onehot - p) + cm * p * (((seg - M[:, None]) - ls[:, None]) + Hd[:, None])
        grad[:, off[d]:off[d + 1]] = np.where(ok, g, F32(0))
    out = dict(lp=lp, H=H, ratio=ratio, dlp=dlp, sur=sur, grad=grad, clipped=clipped)
    assert all(v.dtype == F32 for n, v in out.items() if n != "clipped")
    return out


def _sum_allowed(x, ok):
    """Err.sum_any_order over the allowed terms of each row: n_allowed − 1 roundings of partial sums"""
    n = ok.sum(axis=1)
    v, e = np.where(ok, x.v, 0.0), np.where(ok, x.e, 0.0)
    mag = (np.abs(v) + e).sum(axis=1)
    return Err(v.sum(axis=1), e.sum(axis=1) + (n - 1) * U * mag + cr.TINY)


def head_bounds(z, action, adv, old_lp, eps, ent_coeff, nvec, stored):
    """multidiscrete_ref.head_bounds with every component's operations over its allowed columns: absolute bounds on
    |device − float64 model| of lp [m], H [m], grad [m, A] (0 on masked columns: those are +0 exactly), s_rel [m, D],
    ratio_rel [m]."""
    m, A = np.shape(z)
    off, a = offsets(nvec), indices(action, nvec)
    eff = effective(stored, nvec, a)
    z64 = np.where(eff, np.asarray(z, F64), 0.0)
    rows = np.arange(m)
    col = lambda r: Err(r.v[:, None], r.e[:, None])       # noqa: E731
    parts, s_rel = [], []
    lp = H = None
    for d in range(len(nvec)):
        seg, ok = z64[:, off[d]:off[d + 1]], eff[:, off[d]:off[d + 1]]
        zc = Err.exact(seg) - Err.exact(np.where(ok, seg, -np.inf).max(axis=1, keepdims=True))
        zc = Err(np.where(ok, zc.v, 0.0), np.where(ok, zc.e, 0.0))
        e = zc.exp()
        s = _sum_allowed(e, ok)
        t = _sum_allowed(e * zc, ok)
        ls = s.log()
        lpd = Err(zc.v[rows, a[:, d]], zc.e[rows, a[:, d]]) - ls
        Hd = ls - t / s
        lp = lpd if d == 0 else lp + lpd
        H = Hd if d == 0 else H + Hd
        parts.append((zc, e, s, ls, Hd, ok))
        s_rel.append(s.e / s.v)
    x = lp - Err.exact(np.asarray(old_lp, F64))
    rv = np.exp(x.v)
    ratio = Err(rv, rv * np.expm1(x.e) + U * rv + cr.TINY)
    ref = head_f64(z, action, adv, old_lp, eps, ent_coeff, nvec, stored)
    g = (Err.exact(-np.asarray(adv, F64)) * ratio) / Err.exact(F64(m))
    g = Err(np.where(ref["clipped"], 0.0, g.v), np.where(ref["clipped"], 0.0, g.e))
    cm = Err.exact(F64(F32(ent_coeff))) / Err.exact(F64(m))
    grad = np.empty((m, A))
    for d, (zc, e, s, ls, Hd, ok) in enumerate(parts):
        p = e / col(s)
        onehot = np.zeros(zc.v.shape)
        onehot[rows, a[:, d]] = 1.0
        b = (col(g) * (Err.exact(onehot) - p) + (cm * p) * ((zc - col(ls)) + col(Hd))).e
        grad[:, off[d]:off[d + 1]] = np.where(ok, b, 0.0)
    return dict(lp=lp.e, H=H.e, grad=grad, s_rel=np.stack(s_rel, axis=1), ratio_rel=ratio.e / ratio.v)


# ------------------------------------------------------------------------------------------------- inputs
JUNK = (np.nan, np.inf, -np.inf, 1e30)                 # then an ordinary value: the pattern rotates over 5


def poison(z, eff):
    """z with the masked columns holding NaN, +inf, −inf, 1e30, (left as it is), rotating with row + column"""
    z = np.array(z, F32)
    r, k = np.indices(z.shape)
    which = (r + k) % 5
    for j, v in enumerate(JUNK):
        z[~eff & (which == j)] = F32(v)
    return z


def straddle_row(A):
    """the pinned row whose only stored bits are columns 31 and 32 (A > 32), else None"""
    return 4 if A > 32 else None


def make_mask(nvec, idx, rng):
    """Stored bits [m, A] for the chosen indices idx [m, D]: every bit allowed with p = 0.5, then at least one
    allowed bit per component and the chosen bit forced on; then the pinned rows (those m has):
      row 0: component 0 has exactly one allowed column (the chosen one): H_0 = 0, its gradient exactly 0;
      row 1: the last component's stored bits are all zero: read as full;
      row 2: component 0's chosen bit is off (another one is on): OR-ed in;
      row 3: a full mask;
      row 4, A > 32: the only stored bits are columns 31 and 32, on either side of a word boundary."""
    m, D = idx.shape
    A = int(sum(nvec))
    off = offsets(nvec)
    rows = np.arange(m)
    st = rng.random((m, A)) < 0.5
    for d in range(D):
        seg = st[:, off[d]:off[d + 1]]
        none = ~seg.any(axis=1)
        seg[none, rng.integers(0, nvec[d], int(none.sum()))] = True
        seg[rows, idx[:, d]] = True
    st[0, off[0]:off[1]] = False
    st[0, off[0] + idx[0, 0]] = True
    if m > 1:
        st[1, off[D - 1]:off[D]] = False
    if m > 2:
        st[2, off[0]:off[1]] = False
        st[2, off[0] + (idx[2, 0] + 1) % nvec[0]] = True
    if m > 3:
        st[3] = True
    if m > 4 and straddle_row(A) is not None:
        st[4] = False
        st[4, 31:33] = True
    return st


@functools.lru_cache(maxsize=None)
def _head_inputs(nvec, m):
    nvec = list(nvec)
    A, D = sum(nvec), len(nvec)
    base = md.head_inputs(nvec, m)
    rng = np.random.default_rng(9900 + 31 * A + D)
    act = base["act"].copy()
    clean = base["z"].copy()
    if D == 1:             # row 0 is multidiscrete_ref's ±30 row there: p of its top logit is 1 masked or not, which
        if m > 5:          # pins nothing — it moves to row 5, and row 0 takes ordinary logits
            clean[5] = clean[0]
        clean[0] = (2 * rng.normal(size=A)).astype(F32)
    stored = make_mask(nvec, indices(act, nvec), rng)
    eff = effective(stored, nvec, indices(act, nvec))
    z = poison(clean, eff)
    lp = head_f64(z, act, np.zeros(m), np.zeros(m), EPS, 0.0, nvec, stored)["lp"]

    def draw(n):
        return rng.uniform(0.05, 0.5, n) * rng.choice([-1.0, 1.0], n)

    old = (lp - draw(m)).astype(F32)
    for _ in range(50):
        bad = cr.near_clip(np.exp(lp - old.astype(F64)))
        if not bad.any():
            break
        old[bad] = (lp[bad] - draw(int(bad.sum()))).astype(F32)
    assert not cr.near_clip(np.exp(lp - old.astype(F64))).any()
    out = dict(z=z, act=act, adv=base["adv"], old=old, stored=stored, mask=pack(stored), z_clean=clean)
    for v in out.values():
        v.setflags(write=False)
    return out


def head_inputs(nvec, m=257):
    """multidiscrete_ref.head_inputs' logits, actions and advantages under make_mask's masks: the masked columns of z
    poisoned (z_clean keeps the ordinary values), old_lp = masked lp − x redrawn until no ratio is within 1e-4 of
    1 ± EPS (asserted).  stored [m, A] bool, mask [m, W] uint32.  Read-only, shared; fewer rows: rows_of."""
    return _head_inputs(tuple(int(n) for n in nvec), m)


def head_args(i, nvec, eps=EPS, ent=cr.ENT):
    return (i["z"], i["act"], i["adv"], i["old"], eps, ent, nvec, i["stored"])


# the nvec the GPU tests run, with their row counts
HEAD_NVEC = [[2], [3, 5, 2], [2] * 17, [7] * 17, [33, 2], [65, 3, 64]]
HEAD_M = [1, 63, 64, 257]
HEAD_NVEC_WIDE = [[2] * 256, [4096], [4094, 2]]
SAMPLE_NVEC = md.SAMPLE_NVEC


# ---------------------------------------------------------------------------------------------- the sampler
def sample_f32(z, u, nvec, stored):
    """The mirror: per component the CDF over the allowed columns (rules 1 and 2; no action exists yet) — the first
    allowed k with u·s <= c_k, the fallback the last allowed k — indices [m, D], the joint log-prob (d ascending) and
    margin [m, D]: the distance of the threshold to the nearest cumulative boundary among the allowed columns but
    the last, relative to s (categorical_ref.sample_f32's, 1 where a single column is allowed)."""
    m, A = np.shape(z)
    off = offsets(nvec)
    eff = effective(stored, nvec)
    z = np.where(eff, np.asarray(z, F32), F32(0))
    rows = np.arange(m)
    a, margin, lp = [], [], None
    for d in range(len(nvec)):
        seg, ok = np.ascontiguousarray(z[:, off[d]:off[d + 1]]), eff[:, off[d]:off[d + 1]]
        n = seg.shape[1]
        M, e, c, t = row_stats_f32(seg, ok)
        s = c[:, -1]
        thr = np.asarray(u[:, d], F32) * s
        hit = (thr[:, None] <= c) & ok
        last = n - 1 - ok[:, ::-1].argmax(axis=1)
        ad = np.where(hit.any(axis=1), hit.argmax(axis=1), last)
        lpd = (seg[rows, ad] - M) - cr._map("logf", s)
        inner = ok.copy()
        inner[rows, last] = False
        dist = np.where(inner, np.abs(thr[:, None].astype(F64) - c.astype(F64)), np.inf).min(axis=1) / s.astype(F64)
        a.append(ad)
        margin.append(np.where(inner.any(axis=1), dist, 1.0))
        lp = lpd if d == 0 else lp + lpd
    return np.stack(a, axis=1), lp, np.stack(margin, axis=1)


def argmax(z, nvec, stored):
    """per component the lowest allowed index holding the maximum over the allowed columns, [m, D]"""
    off = offsets(nvec)
    eff = effective(stored, nvec)
    zz = np.where(eff, np.asarray(z, F64), -np.inf)
    return np.stack([zz[:, off[d]:off[d + 1]].argmax(axis=1) for d in range(len(nvec))], axis=1)


def random_masks(nvec, m, seed, p=0.5):
    """stored bits [m, A], each allowed with probability p, at least one per component"""
    rng = np.random.default_rng(seed)
    off = offsets(nvec)
    st = rng.random((m, int(sum(nvec)))) < p
    for d in range(len(nvec)):
        seg = st[:, off[d]:off[d + 1]]
        none = ~seg.any(axis=1)
        seg[none, rng.integers(0, nvec[d], int(none.sum()))] = True
    return st
