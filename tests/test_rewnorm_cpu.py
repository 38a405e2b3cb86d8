"""tests/rewnorm_ref.py pinned on the CPU: hand-worked cases, the kernel's algorithm class (a chunked float64
tree composition of the affine maps) inside the accuracy bound the GPU test uses, and the SB3 identity — one long
stream equals its E × T segments with the carry chained through carry_out → carry_in."""
import numpy as np

from rewnorm_ref import F32, bound, chan, returns64, scale_f32, scale_of, triple64


def rewards(rng, n):
    """10^U(−3, 3) · N(0, 1), the GPU test's rewards."""
    return (10.0 ** rng.uniform(-3, 3, n) * rng.normal(size=n)).astype(F32)


def flags(rng, n, rate=1 / 50):
    end = rng.random(n) < rate
    term = end & (rng.random(n) < 0.5)
    return term, end & ~term


def test_hand_worked():
    z = np.zeros(3, bool)
    mid = np.array([False, True, False])
    # three rows, an end flag in the middle: the third restarts
    R, _ = returns64([1.0, 2.0, 4.0], mid, z, 0.5)
    assert R.tolist() == [1.0, 2.5, 4.0]
    R, _ = returns64([1.0, 2.0, 4.0], z, mid, 0.5)
    assert R.tolist() == [1.0, 2.5, 4.0]
    R, _ = returns64([1.0, 2.0, 4.0], z, z, 0.5)
    assert R.tolist() == [1.0, 2.5, 5.25]
    # γ = 0: the rewards themselves; γ = 1: running sums inside an episode
    R, _ = returns64([1.0, 2.0, 4.0], z, z, 0.0)
    assert R.tolist() == [1.0, 2.0, 4.0]
    R, _ = returns64([1.0, 2.0, 4.0], mid, z, 1.0)
    assert R.tolist() == [1.0, 3.0, 4.0]
    # g is the fp32 gamma widened, not the decimal
    R, _ = returns64([0.0, 1.0, 0.0], z, z, 0.99)
    assert R[2] == float(np.float64(F32(0.99)))
    # segments: row e·T takes g·carry_in[e] whatever row e·T − 1 says, carry_out follows cont
    last = np.array([False, True, False, True])
    R, co = returns64([1.0, 2.0, 4.0, 8.0], np.zeros(4, bool), last, 0.5, 2, [10.0, 100.0], [1, 0])
    assert R.tolist() == [6.0, 5.0, 54.0, 35.0] and co.tolist() == [5.0, 0.0]
    R, co = returns64([1.0, 2.0, 4.0, 8.0], np.zeros(4, bool), np.zeros(4, bool), 0.5, 2, [10.0, 100.0], [0, 1])
    assert R.tolist() == [6.0, 5.0, 56.5, 36.25] and co.tolist() == [0.0, 36.25]
    # the triple, the scale and the scaling of a known case
    t = triple64([1.0, 2.0, 3.0, 6.0])
    assert t.tolist() == [4.0, 3.0, 14.0]
    assert scale_of(t) == F32(1.0 / np.sqrt(3.5 + 1e-8)) and scale_of(np.zeros(3)) == 1.0
    y, cl = scale_f32(np.array([1.0, -1.0, 0.5, np.nan, 3.0], F32), F32(0.5), 0.5)
    assert y[:3].tolist() == [0.5, -0.5, 0.25] and np.isnan(y[3]) and y[4] == 0.5
    assert cl.tolist() == [False, False, False, False, True]


def tree64(r, term, trunc, g, chunk, seg_len=0, carry_in=None):
    """The kernel's algorithm class in float64: per-row maps (a, d), a pairwise tree inside each chunk (up-sweep
    of aggregates, down-sweep of prefixes), the chunks' aggregates applied left to right."""
    r = np.asarray(r, F32).astype(np.float64)
    end = np.asarray(term, bool) | np.asarray(trunc, bool)
    n = r.size
    g = float(np.float64(F32(g)))
    a = np.where(np.concatenate([[True], end[:-1]]), 0.0, g)
    d = r.copy()
    if seg_len:
        d[::seg_len] = d[::seg_len] + g * np.asarray(carry_in, np.float64)
    R = np.empty(n)
    x = 0.0
    for c0 in range(0, n, chunk):
        A, D = a[c0:c0 + chunk].copy(), d[c0:c0 + chunk].copy()
        m = A.size
        o = 1
        while o < m:                      # Hillis–Steele inclusive scan: element i ← i after (i − o)
            A2, D2 = A.copy(), D.copy()
            A2[o:] = A[o:] * A[:-o]
            D2[o:] = D[o:] + A[o:] * D[:-o]
            A, D = A2, D2
            o *= 2
        R[c0:c0 + m] = D + A * x
        x = R[c0 + m - 1]
    return R


def test_tree_composition_stays_inside_the_bound():
    rng = np.random.default_rng(11)
    worst = 0.0
    for n, gamma, rate, seg in [(1, 0.99, 0.02, 0), (4099, 0.99, 0.02, 0), (4099, 1.0, 0.0, 0), (4096, 0.99, 0.02, 64),
                                (6161, 0.0, 0.02, 0), (5000, 1.0, 1.0, 0)]:
        r = rewards(rng, n)
        term, trunc = flags(rng, n, rate)
        ci = rewards(rng, n // seg).astype(np.float64) if seg else None
        ref, _ = returns64(r, term, trunc, gamma, seg, ci, None)
        b = bound(r, term, trunc, gamma, seg, ci)
        for chunk in (7, 64, 2048):
            got = tree64(r, term, trunc, gamma, chunk, seg, ci)
            err = np.abs(got - ref)
            assert (err <= b).all(), (n, gamma, chunk, float((err / np.maximum(b, 1e-300)).max()))
            worst = max(worst, float((err[b > 0] / b[b > 0]).max(initial=0.0)))
    print(f"float64 tree composition vs sequential: worst err / bound {worst:.3g}")
    assert worst < 1.0


def test_one_stream_equals_chained_segments():
    """SB3's running return never restarts at a rollout boundary.  E environments, K rollouts of T steps: rollout j
    holds rows [jT, (j+1)T) of each environment's stream, its last row forced to truncated = 1 as
    ppo_rollout_device does, cont = the stream did not end there, carry_out chained into the next carry_in."""
    rng = np.random.default_rng(12)
    E, T, K, gamma = 5, 7, 6, 0.99
    r = rewards(rng, E * T * K).reshape(E, K * T)
    term, trunc = (f.reshape(E, K * T) for f in flags(rng, E * T * K, 0.25))
    whole = np.stack([returns64(r[e], term[e], trunc[e], gamma)[0] for e in range(E)])
    carry = np.zeros(E)
    saw_cont = saw_stop = False
    for j in range(K):
        sl = slice(j * T, (j + 1) * T)
        tr = trunc[:, sl].copy()
        cont = ~(term[:, sl][:, -1] | tr[:, -1])
        tr[:, -1] |= ~term[:, sl][:, -1]
        R, carry_out = returns64(r[:, sl].ravel(), term[:, sl].ravel(), tr.ravel(), gamma, T, carry, cont)
        np.testing.assert_allclose(R.reshape(E, T), whole[:, sl], rtol=1e-13, atol=0)
        # without the carry the segments do not add up to the stream
        if j > 0 and carry.any():
            R0, _ = returns64(r[:, sl].ravel(), term[:, sl].ravel(), tr.ravel(), gamma, T, np.zeros(E), cont)
            assert np.abs(R0.reshape(E, T) - whole[:, sl]).max() > 1e-6
        assert (carry_out[~cont] == 0).all()
        saw_cont |= bool(cont.any())
        saw_stop |= bool((~cont).any())
        carry = carry_out
    assert saw_cont and saw_stop
    # the fold of per-rollout triples is the triple of all returns
    acc = np.zeros(3)
    for j in range(K):
        acc = chan(acc, triple64(whole[:, j * T:(j + 1) * T].ravel()))
    ref = triple64(whole.ravel())
    assert acc[0] == ref[0]
    np.testing.assert_allclose(acc[1:], ref[1:], rtol=1e-12)


NEW_EXPORTS = ["ppo_set_reward_norm", "ppo_get_reward_norm", "ppo_reward_norm_freeze", "ppo_reward_norm_get_state",
               "ppo_reward_norm_set_state", "ppo_reward_norm_scale", "ppo_reward_returns_device"]


def test_new_functions_are_exported(lib_built):
    import subprocess

    import ppo_ffi
    out = subprocess.run(["nm", "-D", "--defined-only", ppo_ffi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    missing = [n for n in NEW_EXPORTS if n not in exported]
    assert not missing, f"not exported: {missing}"
    for n in NEW_EXPORTS:
        assert getattr(lib_built, n).argtypes is not None, n
