"""The clipped-surrogate / Gaussian policy head (csrc/ppo_math.h log_prob_row + surrogate, which every form of the
head in csrc calls): the definition in float64, an fp32 model that mirrors the device functions operation for
operation (np.float32 arrays only, the double temporaries of the log-prob sum kept, so it is bit-comparable with
the kernels, which are built with -ffp-contract=off), the rounding bound the GPU tests hold every form to, and the
inputs those tests run on.  Pinned on the CPU in test_policy_head_cpu.py."""
import ctypes as C
import ctypes.util
import functools

import numpy as np

F32 = np.float32
F64 = np.float64
EPS, ENT = 0.2, 0.01
U = 2.0 ** -24                                   # half an fp32 ulp, relative

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = _libm.logf.restype = C.c_float
_libm.expf.argtypes = _libm.logf.argtypes = [C.c_float]


def expf(x):
    """libm's expf, element by element (log σ has A entries: nothing here is per row)."""
    return np.array([_libm.expf(float(v)) for v in np.asarray(x, F32).ravel()], F32).reshape(np.shape(x))


def entropy_f64(log_std):
    ls = np.asarray(log_std, F64)
    return ls.size * 0.5 * (1 + np.log(2 * np.pi)) + ls.sum()


def policy_head_f64(mu, log_std, action, adv, old_lp, eps, ent_coeff):
    """Everything in float64, from the fp32 inputs as given.  Per row: lp, ratio, clipped (the branch: the row's
    surrogate is the clipped constant and its gradient zero), dlp = ∂L/∂lp, grad_mu [m, A], gls_terms [m, A] (the
    row's terms of ∂L/∂log σ), loss_terms [m] (−surrogate/m); and the sums gls [A] (with −ent_coeff per column,
    D4), gb [A] = Σ_i grad_mu, loss (with −ent_coeff·entropy once, D5).  A tie ratio == 1 ± eps is unclipped,
    as in the code (strict comparisons)."""
    mu, ls, a, adv, old = (np.asarray(v, F64) for v in (mu, log_std, action, adv, old_lp))
    m, A = mu.shape
    eps = float(eps)
    with np.errstate(all="ignore"):
        z = (a - mu) / np.exp(ls)
        lp = -0.5 * A * np.log(2 * np.pi) - (ls + 0.5 * z * z).sum(axis=1)
        ratio = np.exp(lp - old)
        pos = adv > 0
        clipped = np.where(pos, ratio > 1 + eps, ratio < 1 - eps)
        dlp = np.where(clipped, 0.0, -adv * ratio / m)
        sur = adv * np.where(clipped, np.where(pos, 1 + eps, 1 - eps), ratio)
        d, e2 = a - mu, np.exp(-2 * ls)
        grad_mu = d * e2 * dlp[:, None]
        gls_terms = (-1 + d * d * e2) * dlp[:, None]
    loss_terms = -sur / m
    return dict(lp=lp, ratio=ratio, clipped=clipped, dlp=dlp, grad_mu=grad_mu, gls_terms=gls_terms,
                loss_terms=loss_terms, gls=gls_terms.sum(axis=0) - ent_coeff, gb=grad_mu.sum(axis=0),
                loss=loss_terms.sum() - ent_coeff * entropy_f64(ls))


def policy_head_f32(mu, log_std, action, adv, old_lp, eps, ent_coeff=0.0, es=None, e2=None):
    """ppo_math.h log_prob_row + surrogate + the grad_μ / ∂log σ expressions, operation for operation in fp32
    (the log-prob sum through its double temporaries, 1 + eps formed in fp32, the int × float products as the
    device writes them).  es / e2: expf(log σ) / expf(−2 log σ) per column (default: libm's).  Returns lp, ratio,
    dlp, sur (the row's surrogate), grad_mu, gls_terms — all fp32, no sums (their order is the kernel's own)."""
    mu, ls, a, adv, old = (np.ascontiguousarray(v, F32) for v in (mu, log_std, action, adv, old_lp))
    m, A = mu.shape
    eps, mf = F32(eps), F32(m)
    es = expf(ls) if es is None else np.asarray(es, F32)
    e2 = expf(F32(-2) * ls) if e2 is None else np.asarray(e2, F32)
    c = F32(-0.5 * A * F64(_libm.logf(float(F32(2 * np.pi)))))
    with np.errstate(all="ignore"):
        lp = np.full(m, c, F32)
        for j in range(A):
            z = (a[:, j] - mu[:, j]) / es[j]
            lp = (lp.astype(F64) - (F64(ls[j]) + 0.5 * (z * z).astype(F64))).astype(F32)
        ratio = np.exp((lp - old).astype(F64)).astype(F32)
        adv_pos = adv > 0
        ratio_pos, ratio_neg = ratio > F32(1) + eps, ratio < F32(1) - eps
        k = (adv_pos & ~ratio_pos) | (~adv_pos & ~ratio_neg)
        dlp = np.where(k, F32(-1), F32(0)) * adv * ratio / mf        # -(int) is an int: 0 stays +0
        f = lambda b: b.astype(F32)                                   # noqa: E731  (float)(int)
        sur = adv * (f(adv_pos) * (f(ratio_pos) * (F32(1) + eps) + f(~ratio_pos) * ratio)
                     + f(~adv_pos) * (f(ratio_neg) * (F32(1) - eps) + f(~ratio_neg) * ratio))
        d = a - mu
        grad_mu = d * e2 * dlp[:, None]
        gls_terms = (F32(-1) + d * d * e2) * dlp[:, None]
    out = dict(lp=lp, ratio=ratio, dlp=dlp, sur=sur, grad_mu=grad_mu, gls_terms=gls_terms, clipped=~k)
    assert all(v.dtype == F32 for n, v in out.items() if n != "clipped")
    return out


def lp_bound(mu, log_std, action):
    """δlp per row, in float64: 2⁻²⁴·(8·Σ_j z_j² + (A + 1)·max_j |partial sum_j|), z_j = (a_j − μ_j)/σ_j and the
    partial sum the running log-prob after column j.  The first term covers a 2-ulp expf(log σ), the correctly
    rounded fp32 division and the fp32 square of z; the second the A + 1 roundings of the running sum to fp32."""
    mu, ls, a = (np.asarray(v, F64) for v in (mu, log_std, action))
    A = mu.shape[1]
    with np.errstate(all="ignore"):
        z = (a - mu) / np.exp(ls)
        part = -0.5 * A * np.log(2 * np.pi) - np.cumsum(ls + 0.5 * z * z, axis=1)
        return U * (8 * (z * z).sum(axis=1) + (A + 1) * np.abs(part).max(axis=1))


def row_rel_bound(mu, log_std, action):
    """The relative bound of everything that is a product with the row's ratio (∂L/∂lp, grad_μ, the unclipped
    surrogate): δlp — the ratio's relative error to first order — plus 8·2⁻²⁴ for the ratio's own rounding and
    the four fp32 operations after it."""
    return lp_bound(mu, log_std, action) + 8 * U


# ---------------------------------------------------------------------------------------------------- inputs
# rows of the largest set per action size; every shape of test_gpu_policy_head.py is its leading rows
ROWS = {1: 70001, 6: 70001, 17: 135168, 300: 257}
SIZES_A = [1, 2, 3, 6, 17, 31, 32, 33, 64, 100, 300]
# (A, mode): "uniform" log σ ∈ [−0.7, 0.2]; "mixed" log σ ∈ {−3, 0, 1.5} over the columns; "zero" log σ = 0 (σ = 1
# exactly: no expf between the model and the device)
INPUT_SETS = [(A, "uniform") for A in SIZES_A] + [(A, md) for md in ("mixed", "zero") for A in (1, 6, 17, 33)]


def set_rows(A, mode):
    return ROWS.get(A, 4097) if mode == "uniform" else 1000


@functools.lru_cache(maxsize=None)
def head_inputs(A, mode="uniform"):
    """μ ~ N(0, 1), log σ by mode, action = μ + σ·N(0, 1), old_lp = lp − x with |x| ∈ [0.05, 0.5] and random
    sign, redrawn until no row's ratio is within 1e-4 of 1 ± EPS (asserted: zero rows in the guard band), adv ~
    N(0, 1) with every 17th entry +0.0 and every 19th −0.0.  Read-only arrays, shared by the tests."""
    m = set_rows(A, mode)
    rng = np.random.default_rng(7000 + 10 * A + ("uniform", "mixed", "zero").index(mode))
    mu = rng.normal(size=(m, A)).astype(F32)
    if mode == "uniform":
        ls = rng.uniform(-0.7, 0.2, A).astype(F32)
    elif mode == "mixed":
        ls = np.array([-3.0, 0.0, 1.5], F32)[(np.arange(A) + A) % 3]
    else:
        ls = np.zeros(A, F32)
    act = (mu + rng.normal(size=(m, A)).astype(F32) * np.exp(ls)).astype(F32)
    lp = policy_head_f64(mu, ls, act, np.zeros(m), np.zeros(m), EPS, 0.0)["lp"]

    def draw(n):
        return rng.uniform(0.05, 0.5, n) * rng.choice([-1.0, 1.0], n)

    def near(old):
        r = np.exp(lp - old.astype(F64))
        return (np.abs(r - (1 + EPS)) < 1e-4) | (np.abs(r - (1 - EPS)) < 1e-4)

    old = (lp - draw(m)).astype(F32)
    for _ in range(50):
        bad = near(old)
        if not bad.any():
            break
        old[bad] = (lp[bad] - draw(int(bad.sum()))).astype(F32)
    assert not near(old).any(), "rows left in the guard band of the clip boundary"
    adv = rng.normal(size=m).astype(F32)
    adv[::17] = F32(0.0)
    adv[::19] = F32(-0.0)
    out = dict(mu=mu, ls=ls, act=act, adv=adv, old=old)
    for v in out.values():
        v.setflags(write=False)
    return out


def rows_of(inp, m):
    """The leading m rows of an input set."""
    return dict(mu=inp["mu"][:m], ls=inp["ls"], act=inp["act"][:m], adv=inp["adv"][:m], old=inp["old"][:m])
