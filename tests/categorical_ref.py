"""The categorical policy (csrc/ppo_math.h cat_* atoms + surrogate, csrc/categorical.hip's head, csrc/discrete.hip's
sampler at D = 1, and CartPole-v1 of csrc/rollout.hip), restated independently of the kernels:

  * head_f64        the definition in float64, from the fp32 inputs as given;
  * head_f32        an fp32 numpy mirror in the stated order (k ascending, libm's expf / logf);
  * head_bounds     the rounding bounds the GPU tests hold the kernels to, derived by propagating, operation by
                    operation, the rounding of every fp32 operation the header lists (class Err below) — nothing is
                    taken from a run of the kernels; the mirror has to stay inside them on the CPU
                    (test_categorical_cpu.py), or they are not valid;
  * sample_f32      the inverse-CDF sampler's mirror and the rows whose threshold lies within the bound of a
                    cumulative boundary;
  * cartpole_f64 / cartpole_f32 / cartpole_bounds   one CartPole-v1 step, likewise.

The streams of csrc/rng.h's table that the categorical sampler reads (restated here, not in rng_ref.py):
    ppo_fill_synthetic(seed)          key splitmix64(seed) ^ 5             counter i (row)  offset 0            .x
    ppo_rollout_device / ppo_eval_device
                                      key splitmix64(seed ^ 0x524F4C4C)    counter e        offset (1 << 40) + g  .x
    ppo_categorical_sample_device     key, offset as given                 counter i (row)                       .x
    CartPole-v1 resets                first: key splitmix64(seed), offset (3 << 40) − 1; later: the rollout key,
                                      offset (3 << 40) + g; counter e; .x .y .z .w → x, ẋ, θ, θ̇ = −0.05 + 0.1·u01
"""
import ctypes as C
import ctypes.util
import functools

import numpy as np

import rng_ref

F32 = np.float32
F64 = np.float64
EPS, ENT = 0.2, 0.01
U = 2.0 ** -24                                   # half an fp32 ulp, relative
TINY = 2.0 ** -126                               # an underflowing result: absolute, whatever the denormal mode
K_NOISE, K_RESET = 1 << 40, 3 << 40
LIBM = 4 * U                                     # a library function's result: 2 ulp

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("expf", "logf", "sinf", "cosf"):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float]


def _map(name, x):
    f = getattr(_libm, name)
    x = np.asarray(x, F32)
    return np.array([f(float(v)) for v in x.ravel()], F32).reshape(x.shape)


# ------------------------------------------------------------------------------------------- error propagation
class Err:
    """A float64 value v (the exact result from the fp32 inputs) with a bound e on |computed fp32 − v|.  Every
    operation adds the operands' propagated error and the half-ulp rounding U·|result| of one fp32 operation
    (LIBM = 4·U for the library functions: expf, logf, sinf, cosf are taken as accurate to 2 ulp, which covers
    glibc's (under 1 ulp) and the 1 – 2 ulp the HIP math library documents for them).  The propagation is
    first order with the denominators and exponents widened by the operands' own bounds, so it stays an upper
    bound wherever e is small against v — which the tests' inputs guarantee and the CPU test checks."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, F64)
        self.e = np.broadcast_to(np.asarray(e, F64), self.v.shape) if np.ndim(e) == 0 else np.asarray(e, F64)

    @staticmethod
    def exact(x):
        return Err(np.asarray(x, F64), 0.0)

    @staticmethod
    def const(c):
        """a literal written in decimal: rounded to fp32 once"""
        return Err(F64(c), U * abs(c))

    def _r(self, v, e):
        return Err(v, e + U * np.abs(v) + TINY)

    def __add__(self, o):
        return self._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return self._r(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return self._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        v = self.v / o.v
        den = np.maximum(np.abs(o.v) - o.e, 1e-300)
        return self._r(v, (self.e + np.abs(v) * o.e) / den)

    def exp(self):
        v = np.exp(self.v)
        return Err(v, v * np.expm1(self.e) + LIBM * v + TINY)

    def log(self):
        v = np.log(self.v)
        return Err(v, self.e / np.maximum(self.v - self.e, 1e-300) + LIBM * np.abs(v) + TINY)

    def sin(self):
        v = np.sin(self.v)
        return Err(v, self.e + LIBM * np.abs(v) + TINY)

    def cos(self):
        v = np.cos(self.v)
        return Err(v, self.e + LIBM * np.abs(v) + TINY)

    def sum_any_order(self, axis=-1):
        """n terms added in any order: the terms' own bounds plus (n − 1) roundings of partial sums, each at most
        the sum of the terms' magnitudes (widened by their bounds)"""
        n = self.v.shape[axis]
        mag = (np.abs(self.v) + self.e).sum(axis=axis)
        return Err(self.v.sum(axis=axis), self.e.sum(axis=axis) + (n - 1) * U * mag + TINY)


# ------------------------------------------------------------------------------------------------- the head
def head_f64(z, action, adv, old_lp, eps, ent_coeff):
    """Everything in float64.  action: [m, A] with the index in column 0.  Returns per row lp, H, ratio, clipped,
    dlp (∂loss/∂lp), grad [m, A], loss_terms [m] (−surrogate/m), p [m, A]; and loss."""
    z, adv, old = (np.asarray(v, F64) for v in (z, adv, old_lp))
    m, A = z.shape
    a = np.asarray(action)[:, 0].astype(np.int64)
    eps = float(eps)
    with np.errstate(all="ignore"):
        M = z.max(axis=1, keepdims=True)
        zc = z - M
        e = np.exp(zc)
        s = e.sum(axis=1)
        ls = np.log(s)
        lp = zc[np.arange(m), a] - ls
        p = e / s[:, None]
        H = ls - (e * zc).sum(axis=1) / s
        ratio = np.exp(lp - old)
        pos = adv > 0
        clipped = np.where(pos, ratio > 1 + eps, ratio < 1 - eps)
        dlp = np.where(clipped, 0.0, -adv * ratio / m)
        sur = adv * np.where(clipped, np.where(pos, 1 + eps, 1 - eps), ratio)
        onehot = np.zeros((m, A))
        onehot[np.arange(m), a] = 1.0
        grad = dlp[:, None] * (onehot - p) + (ent_coeff / m) * p * ((zc - ls[:, None]) + H[:, None])
    loss_terms = -sur / m
    return dict(lp=lp, H=H, ratio=ratio, clipped=clipped, dlp=dlp, grad=grad, loss_terms=loss_terms, p=p,
                loss=loss_terms.sum() - ent_coeff * H.sum() / m)


def loss_of(z, action, adv, old_lp, eps, ent_coeff):
    return head_f64(z, action, adv, old_lp, eps, ent_coeff)["loss"]


def surrogate_f32(adv, lp, old, eps, m):
    """ppo_math.h surrogate, operation for operation (as policy_head_ref.policy_head_f32 states it)."""
    eps, mf = F32(eps), F32(m)
    with np.errstate(all="ignore"):
        ratio = np.exp((lp - old).astype(F64)).astype(F32)
        adv_pos = adv > 0
        ratio_pos, ratio_neg = ratio > F32(1) + eps, ratio < F32(1) - eps
        k = (adv_pos & ~ratio_pos) | (~adv_pos & ~ratio_neg)
        dlp = np.where(k, F32(-1), F32(0)) * adv * ratio / mf
        f = lambda b: b.astype(F32)                                   # noqa: E731
        sur = adv * (f(adv_pos) * (f(ratio_pos) * (F32(1) + eps) + f(~ratio_pos) * ratio)
                     + f(~adv_pos) * (f(ratio_neg) * (F32(1) - eps) + f(~ratio_neg) * ratio))
    return ratio, dlp, sur, ~k


def row_stats_f32(z):
    """M, the cumulative sums c [m, A] (k ascending, fp32), t (k ascending), e — the stated order."""
    z = np.ascontiguousarray(z, F32)
    m, A = z.shape
    M = z.max(axis=1)
    e = _map("expf", z - M[:, None])
    c = np.empty((m, A), F32)
    s, t = np.zeros(m, F32), np.zeros(m, F32)
    for k in range(A):
        s = s + e[:, k]
        c[:, k] = s
        t = t + e[:, k] * (z[:, k] - M)
    return M, e, c, t


def head_f32(z, action, adv, old_lp, eps, ent_coeff):
    """The fp32 mirror in the header's order: s and t summed k ascending, libm's expf / logf."""
    z, adv, old = (np.ascontiguousarray(v, F32) for v in (z, adv, old_lp))
    m, A = z.shape
    a = np.asarray(action)[:, 0].astype(np.int64)
    M, e, c, t = row_stats_f32(z)
    s = c[:, -1]
    ls = _map("logf", s)
    lp = (z[np.arange(m), a] - M) - ls
    H = ls - t / s
    ratio, dlp, sur, clipped = surrogate_f32(adv, lp, old, eps, m)
    cm = F32(ent_coeff) / F32(m)
    p = e / s[:, None]
    onehot = np.zeros((m, A), F32)
    onehot[np.arange(m), a] = 1
    grad = dlp[:, None] * (onehot - p) + cm * p * (((z - M[:, None]) - ls[:, None]) + H[:, None])
    out = dict(lp=lp, H=H, ratio=ratio, dlp=dlp, sur=sur, grad=grad, clipped=clipped)
    assert all(v.dtype == F32 for n, v in out.items() if n != "clipped")
    return out


def head_bounds(z, action, adv, old_lp, eps, ent_coeff):
    """Absolute bounds on |device − float64 model| of lp [m], H [m] and grad [m, A] for rows whose clip branch the
    device and the model agree on (the others are left out by the guard band), and `s_rel` [m], the relative
    bound of a row's s and of every cumulative sum.  Derived by Err from the operations of the header: the max is
    exact; z − M, expf, the two sums in any order (so every partition of them a kernel may use is covered), logf,
    the divisions, the surrogate (the fp32 difference lp − old_lp, exp in double — exact at this level — its
    rounding to fp32, the product with adv and the division by m), and the two-term gradient."""
    z64 = np.asarray(z, F64)
    m, A = z64.shape
    a = np.asarray(action)[:, 0].astype(np.int64)
    zE = Err.exact(z64)
    M = Err.exact(z64.max(axis=1, keepdims=True))
    zc = zE - M
    e = zc.exp()
    s = e.sum_any_order(axis=1)
    t = (e * zc).sum_any_order(axis=1)
    ls = s.log()
    zca = Err(zc.v[np.arange(m), a], zc.e[np.arange(m), a])
    lp = zca - ls
    H = ls - t / s
    x = lp - Err.exact(np.asarray(old_lp, F64))
    rv = np.exp(x.v)                                      # exp itself runs in double: one rounding to fp32, no libm
    ratio = Err(rv, rv * np.expm1(x.e) + U * rv + TINY)
    ref = head_f64(z, action, adv, old_lp, eps, ent_coeff)
    g = (Err.exact(-np.asarray(adv, F64)) * ratio) / Err.exact(F64(m))
    g = Err(np.where(ref["clipped"], 0.0, g.v), np.where(ref["clipped"], 0.0, g.e))
    col = lambda r: Err(r.v[:, None], r.e[:, None])       # noqa: E731
    p = e / col(s)
    onehot = np.zeros((m, A))
    onehot[np.arange(m), a] = 1.0
    cm = Err.exact(F64(F32(ent_coeff))) / Err.exact(F64(m))
    grad = col(g) * (Err.exact(onehot) - p) + (cm * p) * ((zc - col(ls)) + col(H))
    return dict(lp=lp.e, H=H.e, grad=grad.e, s_rel=s.e / s.v, ratio_rel=ratio.e / ratio.v)


def loss_bound(ref, b, m, ent_coeff):
    """|loss − model| for the rows summed in any order: (terms + 4)·U·Σ|term| for the partial sums and the four
    operations that combine the two words, plus the per-row bounds: a row's −surrogate/m carries the ratio's relative
    bound plus four roundings, its −ent_coeff·H/m the bound of H."""
    terms = np.abs(ref["loss_terms"]).sum() + abs(ent_coeff) * np.abs(ref["H"]).sum() / m
    return ((2 * m + 4) * U * terms + (np.abs(ref["loss_terms"]) * (b["ratio_rel"] + 4 * U)).sum()
            + abs(ent_coeff) * b["H"].sum() / m)


GUARD = 1e-4


def near_clip(ratio, eps=EPS):
    return (np.abs(ratio - (1 + eps)) < GUARD) | (np.abs(ratio - (1 - eps)) < GUARD)


@functools.lru_cache(maxsize=None)
def head_inputs(A, m=257):
    """logits 2·N(0, 1); row 0 spreads over ±30 (its small e_k underflow against the largest), row 1 (m > 1) holds
    equal logits; actions uniform over the A indices, stored as (index, 0, …, 0); adv ~ N(0, 1) with entries ±0;
    old_lp = lp − x, |x| ∈ [0.05, 0.5] with random sign — both clip sides and the unclipped side occur — redrawn
    until no row's ratio is within 1e-4 of 1 ± EPS (asserted).  Read-only, shared; a shape with fewer rows takes
    the leading rows."""
    rng = np.random.default_rng(9100 + A)
    z = (2 * rng.normal(size=(m, A))).astype(F32)
    z[0] = rng.permutation(np.linspace(-30, 30, A)).astype(F32)
    if m > 1:
        z[1] = F32(0.75)
    a = rng.integers(0, A, m)
    act = np.zeros((m, A), F32)
    act[:, 0] = a
    lp = head_f64(z, act, np.zeros(m), np.zeros(m), EPS, 0.0)["lp"]

    def draw(n):
        return rng.uniform(0.05, 0.5, n) * rng.choice([-1.0, 1.0], n)

    old = (lp - draw(m)).astype(F32)
    for _ in range(50):
        bad = near_clip(np.exp(lp - old.astype(F64)))
        if not bad.any():
            break
        old[bad] = (lp[bad] - draw(int(bad.sum()))).astype(F32)
    assert not near_clip(np.exp(lp - old.astype(F64))).any()
    adv = rng.normal(size=m).astype(F32)
    adv[5::17] = F32(0.0)
    adv[7::19] = F32(-0.0)
    out = dict(z=z, act=act, adv=adv, old=old)
    for v in out.values():
        v.setflags(write=False)
    return out


def rows_of(inp, m):
    return {k: v[:m] for k, v in inp.items()}


# ---------------------------------------------------------------------------------------------- the sampler
def sample_u(m, key, offset):
    """u01 of the .x word of philox(i, offset, key), fp32."""
    w = rng_ref.philox4x32_10(np.arange(m, dtype=np.uint64), offset, key)
    return rng_ref.u01(w[0] if isinstance(w, tuple) else w[..., 0]).astype(F32)


def sample_f32(z, u):
    """The mirror: index a = min{k : u·c_{A−1} <= c_k} (clamped), its log-prob, and `margin` [m]: the distance of
    thr to the nearest cumulative boundary relative to s — a row is decided unambiguously when margin exceeds
    2·s_rel + 2·U (thr's and c_k's bounds)."""
    z = np.ascontiguousarray(z, F32)
    m, A = z.shape
    M, e, c, t = row_stats_f32(z)
    s = c[:, -1]
    thr = np.asarray(u, F32) * s
    hit = thr[:, None] <= c
    a = np.where(hit.any(axis=1), hit.argmax(axis=1), A - 1)
    lp = (z[np.arange(m), a] - M) - _map("logf", s)
    margin = (np.abs(thr[:, None].astype(F64) - c[:, :-1].astype(F64)).min(axis=1) / s.astype(F64)
              if A > 1 else np.ones(m))
    return a, lp, margin


@functools.lru_cache(maxsize=None)
def sample_inputs(A, m=65536, shared_row=False):
    """logits 1.5·N(0, 1) per row — or, shared_row, one row repeated (the frequency check: every row draws from
    the same p)."""
    rng = np.random.default_rng(9300 + A)
    z = (1.5 * rng.normal(size=(1 if shared_row else m, A))).astype(F32)
    z = np.ascontiguousarray(np.broadcast_to(z, (m, A)))
    z.setflags(write=False)
    return z


SAMPLE_KEY, SAMPLE_OFFSET = 0x5EEDC0DE12345678, 77


# ------------------------------------------------------------------------------------------------ CartPole-v1
X_LIMIT, TH_LIMIT = 2.4, 12 * 2 * np.pi / 360


def cartpole_f64(state, a):
    """One step of gymnasium's CartPole-v1 (explicit Euler) in float64: state [n, 4], a [n] ∈ {0, 1} → next [n, 4],
    terminated [n]."""
    s = np.asarray(state, F64)
    x, xd, th, thd = s.T
    force = np.where(np.asarray(a) == 1, 10.0, -10.0)
    ct, sn = np.cos(th), np.sin(th)
    temp = (force + 0.05 * thd * thd * sn) / 1.1
    thacc = (9.8 * sn - ct * temp) / (0.5 * (4.0 / 3.0 - 0.1 * ct * ct / 1.1))
    xacc = temp - 0.05 * thacc * ct / 1.1
    nxt = np.stack([x + 0.02 * xd, xd + 0.02 * xacc, th + 0.02 * thd, thd + 0.02 * thacc], axis=1)
    term = (np.abs(nxt[:, 0]) > X_LIMIT) | (np.abs(nxt[:, 2]) > TH_LIMIT)
    return nxt, term


def cartpole_f32(state, a):
    """csrc/rollout.hip cartpole_advance, operation for operation in fp32 (libm's sinf / cosf)."""
    s = np.ascontiguousarray(state, F32)
    x, xd, th, thd = (np.ascontiguousarray(v) for v in s.T)
    f = F32
    force = np.where(np.asarray(a) == 1, f(10), f(-10)).astype(F32)
    ct, sn = _map("cosf", th), _map("sinf", th)
    temp = (force + f(0.05) * (thd * thd) * sn) / f(1.1)
    thacc = (f(9.8) * sn - ct * temp) / (f(0.5) * (f(4) / f(3) - f(0.1) * (ct * ct) / f(1.1)))
    xacc = temp - f(0.05) * thacc * ct / f(1.1)
    nxt = np.stack([x + f(0.02) * xd, xd + f(0.02) * xacc, th + f(0.02) * thd, thd + f(0.02) * thacc], axis=1)
    assert nxt.dtype == F32
    th_lim = f(12) * f(2) * f(np.pi) / f(360)
    term = (np.abs(nxt[:, 0]) > f(2.4)) | (np.abs(nxt[:, 2]) > th_lim)
    return nxt, term


def cartpole_bounds(state, a):
    """Absolute bounds [n, 4] on |device next_state − cartpole_f64|, by Err over cartpole_advance's operations (its
    ≈ 30 fp32 operations, the decimal literals rounded to fp32 once each, sinf / cosf to 2 ulp)."""
    s = np.asarray(state, F64)
    x, xd, th, thd = (Err.exact(v) for v in s.T)
    k = Err.const
    force = Err.exact(np.where(np.asarray(a) == 1, 10.0, -10.0))
    ct, sn = th.cos(), th.sin()
    temp = (force + k(0.05) * (thd * thd) * sn) / k(1.1)
    thacc = (k(9.8) * sn - ct * temp) / (Err.exact(0.5) * (Err.exact(4.0) / Err.exact(3.0) - k(0.1) * (ct * ct) / k(1.1)))
    xacc = temp - k(0.05) * thacc * ct / k(1.1)
    outs = [x + k(0.02) * xd, xd + k(0.02) * xacc, th + k(0.02) * thd, thd + k(0.02) * thacc]
    return np.stack([np.broadcast_to(o.e, s.shape[:1]) for o in outs], axis=1)


# the thresholds as the device forms them (fp32) differ from the float64 ones by at most this
LIMIT_SLACK = np.array([U * X_LIMIT, 4 * U * TH_LIMIT])
