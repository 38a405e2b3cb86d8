"""tests/obsnorm_ref.py pinned on the CPU, the statistics cases and bounds the GPU test shares, and the export
check of the observation-normalisation entry points (ppo_ext.h ppo_set_obs_norm …).

Bounds of the statistics (ISSUE: n·2^-53·sqrt(1 + mean²/var) with n <= 7e4, about 10× margin): a column with
|mean| <= 10·std has its mean within 1e-10·std and M2 within rtol 1e-10; the offset column (mean 1e4, std 0.1:
kappa = 1e5) has M2 within rtol 1e-5 — a shifted form errs at 8e-7 there, a sum-of-squares form at about 3e-4 —
and, by the same expression, its mean within 1e-5·std; a constant column has M2 == 0 and its mean exactly."""
import functools
import subprocess

import numpy as np

import ppo_ffi
from obsnorm_ref import F32, affine, chan, normalize_f32, stats64

STATS_SHAPES = [(1, 3), (7, 5), (4099, 376), (70001, 17)]
NEW_EXPORTS = ["ppo_set_obs_norm", "ppo_get_obs_norm", "ppo_obs_norm_freeze", "ppo_obs_norm_fold_buffer",
               "ppo_obs_norm_get_state", "ppo_obs_norm_set_state", "ppo_obs_norm_affine", "ppo_obs_normalize_device",
               "ppo_obs_stats_device"]


@functools.lru_cache(maxsize=None)
def stats_case(n, S):
    """(x [n, S] fp32, kinds [S], exact triple): column j is N(0, 1), U(−1, 1), a constant or the offset column
    (mean 1e4, std 0.1) for j % 4 = 0, 1, 2, 3."""
    rng = np.random.default_rng(1000 * S + n % 997)
    kinds = np.arange(S) % 4
    x = np.empty((n, S), F32)
    for j in range(S):
        k = kinds[j]
        x[:, j] = (rng.normal(size=n) if k == 0 else rng.uniform(-1, 1, n) if k == 1 else np.full(n, 0.75 + j)
                   if k == 2 else 1e4 + 0.1 * rng.normal(size=n)).astype(F32)
    x.setflags(write=False)
    ref = stats64(x)
    ref.setflags(write=False)
    return x, kinds, ref


def check_triple(got, ref, kinds, what):
    """`got` against the exact triple `ref` within the module's bounds; returns the worst ratios (for printing)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    S = kinds.size
    assert got.shape == ref.shape == (1 + 2 * S,) and got[0] == ref[0], what
    n = ref[0]
    mean, M2, mean_r, M2_r = got[1:1 + S], got[1 + S:], ref[1:1 + S], ref[1 + S:]
    std = np.sqrt(M2_r / n)
    worst = {}
    for j in range(S):
        if kinds[j] == 2:
            assert M2[j] == 0.0 and mean[j] == mean_r[j], f"{what}: constant column {j}: {mean[j]!r}, {M2[j]!r}"
            continue
        offset = kinds[j] == 3
        assert offset or abs(mean_r[j]) <= 10 * std[j] or n < 8, f"{what}: column {j} is not ordinary"
        b_mean, b_m2 = (1e-5, 1e-5) if offset else (1e-10, 1e-10)
        e_mean = abs(mean[j] - mean_r[j])
        e_m2 = abs(M2[j] - M2_r[j])
        assert e_mean <= b_mean * std[j], f"{what}: column {j} mean err {e_mean:.3g} > {b_mean:g}·std {std[j]:.3g}"
        assert e_m2 <= b_m2 * M2_r[j], f"{what}: column {j} M2 rel err {e_m2 / max(M2_r[j], 1e-300):.3g} > {b_m2:g}"
        key = "offset" if offset else "ordinary"
        if std[j] > 0:
            w = worst.setdefault(key, [0.0, 0.0])
            w[0], w[1] = max(w[0], e_mean / std[j]), max(w[1], e_m2 / M2_r[j])
    return worst


def chunked64(x, chunk):
    """Per-chunk two-pass statistics in float64 (numpy sums), folded by chan in chunk order: the device's
    algorithm class (per-workgroup partials, fixed-order combine)."""
    S = x.shape[1]
    acc = np.zeros(1 + 2 * S)
    for r0 in range(0, x.shape[0], chunk):
        blk = np.asarray(x[r0:r0 + chunk], np.float64)
        mean = blk.mean(axis=0)
        acc = chan(acc, np.concatenate([[blk.shape[0]], mean, ((blk - mean) ** 2).sum(axis=0)]))
    return acc


def test_chan_over_chunks_equals_whole():
    for n, S in STATS_SHAPES:
        x, kinds, ref = stats_case(n, S)
        for chunk in (1, 5, 64, 1000):
            if chunk == 1 and n > 5000:
                continue
            if n <= 7 or n <= 10 * chunk:       # exact per-chunk triples: chan itself is what is checked
                acc = np.zeros(1 + 2 * S)
                for r0 in range(0, n, chunk):
                    acc = chan(acc, stats64(x[r0:r0 + chunk]))
                check_triple(acc, ref, kinds, f"chan of exact chunks of {chunk} rows, {n} x {S}")
            worst = check_triple(chunked64(x, chunk), ref, kinds, f"float64 chunks of {chunk} rows, {n} x {S}")
            print(f"{n} x {S}, chunks of {chunk}: worst (mean err / std, M2 rel err) {worst}")
    # an empty side is the identity, on either side
    _, _, ref = stats_case(7, 5)
    zero = np.zeros_like(ref)
    np.testing.assert_array_equal(chan(zero, ref), ref)
    np.testing.assert_array_equal(chan(ref, zero), ref)


def test_sum_of_squares_form_would_fail():
    """The bound of the offset column separates the algorithm classes: float64 Σx² − (Σx)²/n misses it."""
    x, kinds, ref = stats_case(70001, 17)
    j = int(np.nonzero(kinds == 3)[0][0])
    col = x[:, j].astype(np.float64)
    # cumsum adds one element after another, as a thread's running sum does (np.sum adds pairwise)
    naive = float((col * col).cumsum()[-1] - col.cumsum()[-1] ** 2 / col.size)
    rel = abs(naive - ref[1 + 17 + j]) / ref[1 + 17 + j]
    print(f"sum-of-squares M2 of the offset column: rel err {rel:.3g}")
    assert rel > 1e-5


def test_normalize_f32_against_f64():
    """The fp32 model against a float64 evaluation of the same fp32 operands, on every element away from the
    clamp boundary, within 1.5 ulp of the result.  The issue names 1 ulp; two fp32 roundings cannot meet that:
    d = fl(x − m) is correctly rounded whether or not it cancels, a relative error of at most 2^-24, which the
    product carries into y as |y|·2^-24 < 1 ulp(y), and the product's own rounding adds at most ½ ulp(y) — up to
    1.5 ulp in all, and errors above 1 ulp do occur on this data (printed).  ulp is that of the larger of the two
    results, so the bound holds across a binade boundary too."""
    rng = np.random.default_rng(7)
    n, S, c = 3000, 17, 2.0
    scale, shift = 10.0 ** rng.uniform(-2, 3, S), rng.normal(size=S) * 10.0 ** rng.uniform(-1, 2, S)
    x = (rng.normal(size=(n, S)) * scale + shift).astype(F32)
    m, r = affine(stats64(x))
    y, clamped = normalize_f32(x, m, r, c)
    assert y.dtype == F32 and 0.01 < clamped.mean() < 0.2
    t64 = (x.astype(np.float64) - m.astype(np.float64)) * r.astype(np.float64)
    away = np.abs(np.abs(t64) - c) > 1e-3
    y64 = np.clip(t64, -c, c)
    np.testing.assert_array_equal(clamped[away], (np.abs(t64) > c)[away])
    ulp = np.spacing(np.maximum(np.abs(y), np.abs(y64).astype(F32))).astype(np.float64)
    err = (np.abs(y.astype(np.float64) - y64) / ulp)[away]
    print(f"normalize_f32 vs float64: worst {err.max():.3f} ulp over {err.size} elements, {(err > 1).sum()} above 1 ulp")
    assert (err <= 1.5).all()
    # edge cases: exactly ±c is not clamped, NaN stays NaN and is not counted, +inf never clamps, n = 0 is the identity
    one, zero = np.ones(4, F32), np.zeros(4, F32)
    y, cl = normalize_f32(np.array([[0.5, -0.5, np.nan, 0.75]], F32), zero, one, 0.5)
    assert y[0, 0] == 0.5 and y[0, 1] == -0.5 and np.isnan(y[0, 2]) and y[0, 3] == 0.5
    assert cl.tolist() == [[False, False, False, True]]
    y, cl = normalize_f32(x, m, r, np.inf)
    assert not cl.any()
    mi, ri = affine(np.zeros(1 + 2 * S))
    y, cl = normalize_f32(x, mi, ri, np.inf)
    np.testing.assert_array_equal(y.view(np.uint32), x.view(np.uint32))


def test_new_functions_are_exported(lib_built):
    out = subprocess.run(["nm", "-D", "--defined-only", ppo_ffi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    missing = [n for n in NEW_EXPORTS if n not in exported]
    assert len(NEW_EXPORTS) == 9 and not missing, f"not exported: {missing}"
    for n in NEW_EXPORTS:
        assert getattr(lib_built, n).argtypes is not None, n
