"""Episode-return statistics (ppo_ext.h ppo_episode_scan_device, csrc/episode.hip): a numpy restatement.

Written from the comment in ppo_ext.h alone.  Every operation is an IEEE double +, −, ×, ÷ or sqrt in the order
the comment gives, so the restatement is bit-comparable with the kernels (built with -ffp-contract=off):
  * the end rule and the per-environment walk {ret, disc, w, len} in row order (`scan`),
  * the aggregate {n, mean, M2, min, max, Σlen, mean disc} and its combine ⊕ (`merge`),
  * the reduce order: per-environment aggregates, 256 contiguous runs of ⌈E/256⌉ environments, a pairwise tree
    (`fold`),
  * the eight reported values of an aggregate (`report`).
"""
import math

import numpy as np

F32 = np.float32
NBATCH = 7            # ppo_ext.h PPO_EP_NBATCH
FOLD = 256            # partials of the fold


def fresh(E):
    s = np.zeros((E, 4))
    s[:, 2] = 1.0
    return s


def zero():
    return np.zeros(NBATCH)


def episode(ret, disc, length):
    return np.array([1.0, ret, 0.0, ret, ret, length, disc])


def merge(a, b):
    """a ⊕ b; an empty side returns the other unchanged."""
    if not b[0] > 0:
        return a.copy()
    if not a[0] > 0:
        return b.copy()
    na, nb = float(a[0]), float(b[0])
    n = na + nb
    f = nb / n
    delta = float(b[1]) - float(a[1])
    out = np.empty(NBATCH)
    out[0] = n
    out[1] = float(a[1]) + delta * f
    out[2] = (float(a[2]) + float(b[2])) + (delta * delta) * (na * f)
    out[3] = b[3] if b[3] < a[3] else a[3]
    out[4] = b[4] if b[4] > a[4] else a[4]
    out[5] = float(a[5]) + float(b[5])
    out[6] = float(a[6]) + (float(b[6]) - float(a[6])) * f
    return out


def ends(term, trunc, cont, E, T):
    """[E, T] bool: terminated || (truncated && (t < T−1 || cont is None || !cont[e]))."""
    term = np.asarray(term).reshape(E, T).astype(bool)
    trunc = np.asarray(trunc).reshape(E, T).astype(bool)
    counts = np.ones((E, T), bool)
    if cont is not None:
        counts[:, T - 1] = ~np.asarray(cont).astype(bool)
    return term | (trunc & counts)


def fold(parts):
    """The batch aggregate of per-environment aggregates parts [E, 7] in the documented order."""
    E = len(parts)
    per = -(-E // FOLD)
    q = []
    for i in range(FOLD):
        a = zero()
        for k in range(i * per, min(E, (i + 1) * per)):
            a = merge(a, parts[k])
        q.append(a)
    stride = 1
    while stride < FOLD:
        for i in range(0, FOLD, 2 * stride):
            q[i] = merge(q[i], q[i + stride])
        stride *= 2
    return q[0]


def scan(reward, term, trunc, cont, E, T, gamma, state=None):
    """One scan.  Returns dict(row_ret [E, T], row_disc [E, T], state [E, 4], parts [E, 7], agg [7], open,
    episodes): `episodes` lists (e, t, ret, disc, len) of every emitted episode, `open` counts the environments
    left mid-episode (len > 0)."""
    r = np.asarray(reward, F32).reshape(E, T).astype(np.float64)
    end = ends(term, trunc, cont, E, T)
    g = float(np.float64(F32(gamma)))
    st = fresh(E) if state is None else np.array(state, np.float64).reshape(E, 4)
    ret, disc, w, ln = st[:, 0].copy(), st[:, 1].copy(), st[:, 2].copy(), st[:, 3].copy()
    row_ret, row_disc = np.empty((E, T)), np.empty((E, T))
    parts = [zero() for _ in range(E)]
    episodes = []
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(T):                      # element-wise over the environments: each walks in row order
            ret = ret + r[:, t]
            disc = disc + w * r[:, t]           # the product rounds, then the sum
            w = w * g
            ln = ln + 1.0
            row_ret[:, t], row_disc[:, t] = ret, disc
            for e in np.nonzero(end[:, t])[0]:
                parts[e] = merge(parts[e], episode(ret[e], disc[e], ln[e]))
                episodes.append((int(e), t, float(ret[e]), float(disc[e]), float(ln[e])))
                ret[e], disc[e], w[e], ln[e] = 0.0, 0.0, 1.0, 0.0
    parts = np.array(parts).reshape(E, NBATCH)
    return dict(row_ret=row_ret, row_disc=row_disc, state=np.stack([ret, disc, w, ln], 1), parts=parts,
                agg=fold(parts), open=int((ln > 0).sum()), episodes=episodes)


def report(agg):
    """{episodes, mean return, population std, min, max, mean length, mean discounted return, M2}; zeros if empty."""
    v = np.zeros(8)
    if agg[0] > 0:
        v[:] = [agg[0], agg[1], math.sqrt(agg[2] / agg[0]), agg[3], agg[4], agg[5] / agg[0], agg[6], agg[2]]
    return v


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)
