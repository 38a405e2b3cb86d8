"""Every form of the clipped-surrogate / Gaussian policy head, row by row, against tests/policy_head_ref.py
(pinned on the CPU in test_policy_head_cpu.py), through ppo_policy_head_device:

    form 0 "separate"  log_prob_kernel → policy_loss_kernel → log_prob_bwd_kernel
    form 1 "head"      policy_head_tiled_kernel<64> (A ≤ 32) / policy_head_kernel (A > 32)
    form 2 "out_head"  out_head_kernel<NPL, A, 1, 1, float>          A ∈ {1, 6}, n ∈ {64, 128, 256, 512}
    form 3 "wide"      out_bwd_wide_kernel<17, NPT, 8, true>         A = 17, n ∈ {256, 512}
    form 4 "fused"     policy_out_fused_kernel<NPT>                  A = 17, n ∈ {256, 512}

Forms 2–4 carry the output layer.  The test's μ is embedded, x = [μ | 0] (m × n), W = [I_A | 0], b = 0, no ReLU
mask: the kernel's μ output must then equal μ bit for bit (one product with 1.0 plus zeros) and columns 0 … A−1
of gx are ∂L/∂μ exactly, the others exactly 0.  That sum starts from +0, so a −0 gradient arrives as +0: where
forms are compared bit for bit, form 0's zeros are canonicalised the same way (x + 0) and nothing else is.

(a) every form against the float64 model: the branch of every row (read off the device's grad_μ), grad_μ within
    |ref|·(δlp + 8·2⁻²⁴), form 0's lp within δlp (policy_head_ref.lp_bound / row_rel_bound; validated on the CPU);
(b) grad_μ of forms 1–4 has the bits of form 0's; form 0's lp has the bits of the fp32 mirror's, run with the
    device's own expf(log σ) per column (found by one probe launch; with log σ = 0 no expf is involved);
(c) one-hot advantages: every sum is then exact in any order, so a dropped, doubled or misplaced row fails;
(d) the dense sums within the any-order summation bound;
(e) non-finite rows stay in their row; (f) the entry's argument contract.

Zero signs: `adv > 0` decides nothing but the sign of a zero gradient at adv = ±0, which forms 0 and 1 show (and
(b) compares) and forms 2–4 cannot show in any output.

Largest observed error / bound of (a) on the MI355X over all shapes, grad_μ: separate 0.462, head 0.462,
out_head 0.447, wide 0.325, fused 0.274; form 0's lp 0.637 of δlp.  Every bit-for-bit comparison of (b) held,
and the device's expf(log σ) equalled libm's in every column probed.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import F32, dev, empty
from policy_head_ref import ENT, EPS, F64, U, entropy_f64, expf, head_inputs, lp_bound, policy_head_f32, \
    policy_head_f64, row_rel_bound, rows_of

pytestmark = pytest.mark.gpu

EPS64 = float(F32(EPS))
NAMES = ["separate", "head", "out_head", "wide", "fused"]
WORST = {}                                       # form name -> largest error / bound seen in (a)


def run(lib, form, i, n=0, ent=ENT, expect=0):
    """One call of the entry on the input rows i (a dict of mu, ls, act, adv, old).  Returns lp (form 0), mu_out
    and gx, gW, gb (forms 2–4), grad_mu [m, A] (every form: forms 2–4 columns 0 … A−1 of gx), gls, loss."""
    m, A = i["mu"].shape
    net = form >= 2
    d = {k: dev(lib, i[k]) for k in ("ls", "act", "adv", "old")}
    out = {}
    try:
        d["gls"] = empty(lib, A)
        if net:
            x = np.zeros((m, n), F32)
            x[:, :A] = i["mu"]
            W = np.zeros((A, n), F32)
            W[np.arange(A), np.arange(A)] = 1
            d["x"], d["W"], d["b"] = dev(lib, x), dev(lib, W), dev(lib, np.zeros(A, F32))
            d["mu"] = dev(lib, i["mu"]) if form == 3 else dev(lib, np.full((m, A), np.nan, F32))
            d["gx"], d["gW"] = dev(lib, np.full((m, n), np.nan, F32)), dev(lib, np.full(A * n + A, np.nan, F32))
        else:
            d["mu"], d["gmu"], d["lp"] = dev(lib, i["mu"]), dev(lib, np.full((m, A), np.nan, F32)), empty(lib, m)
        loss = C.c_double(np.nan)
        p = lambda k: d[k].ptr if k in d else None          # noqa: E731
        rc = lib.ppo_policy_head_device(form, m, A, n, 0, EPS, ent, p("ls"), p("act"), p("adv"), p("old"), p("mu"),
                                        p("x"), p("W"), p("b"), p("lp"), p("gmu"), p("gx"), p("gW"), p("gls"),
                                        C.byref(loss))
        assert rc == expect, f"form {form} m {m} A {A} n {n}: returned {rc}"
        assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
        if rc != 0:
            return None
        out["gls"], out["loss"] = d["gls"].to_numpy(F32, A), loss.value
        if net:
            out["mu_out"] = d["mu"].to_numpy(F32, m * A).reshape(m, A)
            out["gx"] = d["gx"].to_numpy(F32, m * n).reshape(m, n)
            g = d["gW"].to_numpy(F32, A * n + A)
            out["gW"], out["gb"] = g[:A * n].reshape(A, n), g[A * n:]
            out["grad_mu"] = out["gx"][:, :A]
        else:
            out["grad_mu"] = d["gmu"].to_numpy(F32, m * A).reshape(m, A)
            out["gb"] = None
            if form == 0:
                out["lp"] = d["lp"].to_numpy(F32, m)
    finally:
        for a in d.values():
            a.free()
    return out


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_rows(form, i, got, g0=None, n=0):
    """(a) for one launch, and (b) against form 0's grad_μ g0 when given."""
    m, A = i["mu"].shape
    what = f"{NAMES[form]} m {m} A {A} n {n}"
    ref = policy_head_f64(i["mu"], i["ls"], i["act"], i["adv"], i["old"], EPS64, 0.0)
    gm = got["grad_mu"]
    if form >= 2:
        if form != 3:
            np.testing.assert_array_equal(bits(got["mu_out"]), bits(i["mu"]), err_msg=f"{what}: μ output")
        assert not got["gx"][:, A:].any() and not np.signbit(got["gx"][:, A:]).any(), f"{what}: gx beyond column A"
    # branches: a clipped row's gradient is zero; an unclipped one's is not unless adv = ±0 (or a − μ = 0)
    zero_adv = i["adv"] == 0
    dev_clipped = ~gm.any(axis=1)
    live = ~zero_adv & (i["act"] != i["mu"]).any(axis=1)
    np.testing.assert_array_equal(dev_clipped[live], ref["clipped"][live], err_msg=f"{what}: clip branch")
    assert (gm[zero_adv] == 0).all(), f"{what}: adv = ±0 rows"
    assert (gm[ref["clipped"]] == 0).all(), f"{what}: clipped rows"
    # grad_μ, every element
    rel = row_rel_bound(i["mu"], i["ls"], i["act"])
    err, bound = np.abs(gm - ref["grad_mu"]), np.abs(ref["grad_mu"]) * rel[:, None]
    ratio = float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))
    WORST[NAMES[form]] = max(WORST.get(NAMES[form], 0.0), ratio)
    print(f"{what}: grad_mu error / bound {ratio:.3f}, clipped {int(dev_clipped.sum())}")
    assert (err <= bound).all(), f"{what}: grad_mu {ratio:.3g} of the bound"
    if form == 0:
        e, b = np.abs(got["lp"] - ref["lp"]), lp_bound(i["mu"], i["ls"], i["act"])
        r = float((e / b).max())
        WORST["separate lp"] = max(WORST.get("separate lp", 0.0), r)
        assert (e <= b).all(), f"{what}: lp {r:.3g} of the bound"
    if g0 is not None:                                    # (b): + 0 maps −0 to +0, as the embedding does
        want = g0 + F32(0) if form >= 2 else g0
        np.testing.assert_array_equal(bits(gm), bits(want), err_msg=f"{what}: grad_mu bits vs the separate form")
    return ref


def check_sums(form, i, got, ref, ent):
    """(d): grad_log_σ, gb and the loss against the model within the any-order summation bound
    (terms − 1)·2⁻²⁴·Σ|t| plus the per-row bounds summed.  The −ent_coeff of a column and the entropy term of the
    loss count as one more term each (the entropy's own A + 1 fp32 additions and its product: (A + 3)·2⁻²⁴)."""
    m, A = i["mu"].shape
    what = f"{NAMES[form]} m {m} A {A}"
    rel = row_rel_bound(i["mu"], i["ls"], i["act"])
    ls, mu, act = (i[k].astype(F64) for k in ("ls", "mu", "act"))
    d2 = (act - mu) ** 2 * np.exp(-2 * ls)
    # a row's ∂log σ term is (−1 + d²e2)·dlp: its error scales with the addends, not with their difference
    t_b = ((1 + d2) * np.abs(ref["dlp"])[:, None] * rel[:, None]).sum(axis=0)
    ent_col = 0.0 if form == 0 else ent                   # form 0's kernels leave −ent_coeff to the host
    want = ref["gls_terms"].sum(axis=0) - ent_col
    bound = m * U * (np.abs(ref["gls_terms"]).sum(axis=0) + ent_col) + t_b
    assert (np.abs(got["gls"] - want) <= bound).all(), f"{what}: grad_log_std {got['gls']} vs {want} ± {bound}"
    H = entropy_f64(ls)
    want = ref["loss_terms"].sum() - ent * H
    bound = (m * U * (np.abs(ref["loss_terms"]).sum() + abs(ent * H)) + (np.abs(ref["loss_terms"]) * rel).sum()
             + (A + 3) * U * ent * (A * 1.42 + np.abs(ls).sum()))
    assert abs(got["loss"] - want) <= bound, f"{what}: loss {got['loss']} vs {want} ± {bound}"
    if got["gb"] is not None:
        want = ref["grad_mu"].sum(axis=0)
        bound = (m - 1) * U * np.abs(ref["grad_mu"]).sum(axis=0) + (np.abs(ref["grad_mu"]) * rel[:, None]).sum(axis=0)
        assert (np.abs(got["gb"] - want) <= bound).all(), f"{what}: gb"
        assert not got["gW"][:, i["mu"].shape[1]:].any(), f"{what}: gW beyond column A"


def both(lib, form, A, m, n=0, mode="uniform"):
    """(a), (b) and (d) at one shape: the form and the separate form on the same rows."""
    i = rows_of(head_inputs(A, mode), m)
    g0 = run(lib, 0, i)
    ref = check_rows(0, i, g0)
    check_sums(0, i, g0, ref, ENT)
    got = run(lib, form, i, n)
    check_rows(form, i, got, g0["grad_mu"], n)
    check_sums(form, i, got, ref, ENT)
    return i, g0


def report():
    print("largest error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


# ----------------------------------------------------------------------------- (a), (b), (d)
MS01 = [1, 63, 64, 65, 255, 256, 257, 1000, 4097]


@pytest.mark.parametrize("A", [1, 2, 3, 6, 17, 31, 32, 33, 64, 100, 300])
def test_separate_and_head(lib, A):
    """Forms 0 and 1: 64 rows per workgroup tiled (A ≤ 32), 256 generic (A > 32), the 8·A ≤ 256 thread edge at
    A = 32, the j += TPB loops at A = 300."""
    for m in ([1, 65, 257] if A == 300 else MS01):
        both(lib, 1, A, m)
    report()


@pytest.mark.parametrize("A,mode", [(A, md) for md in ("mixed", "zero") for A in (1, 6, 17, 33)])
def test_separate_and_head_other_log_std(lib, A, mode):
    both(lib, 1, A, 1000, mode=mode)
    report()


@pytest.mark.parametrize("n", [64, 128, 256, 512])
@pytest.mark.parametrize("A", [1, 6])
def test_out_head(lib, A, n):
    """Form 2: m below the four-row prefetch ring, m no multiple of the row slots, and (n = 64) the
    1024-workgroup grid cap at m = 70 001."""
    for m in [1, 3, 4, 5, 63, 65, 1000] + ([70001] if n == 64 else []):
        both(lib, 2, A, m, n)
    both(lib, 2, A, 1000, n, mode="mixed")
    report()


@pytest.mark.parametrize("n", [256, 512])
def test_wide(lib, n):
    """Form 3; m = 135 168 at n = 256 is 264 rows per workgroup: the second trip of the row loop."""
    for m in [1, 15, 16, 17, 100, 1000, 8200] + ([135168] if n == 256 else []):
        both(lib, 3, 17, m, n)
    both(lib, 3, 17, 1000, n, mode="mixed")
    report()


def test_wide_declines_past_its_rows(lib):
    """512 workgroups of at most 312 rows (a multiple of 8 whose μ, action, g rows and ∂L/∂lp fit 64 KiB of LDS:
    4·rows·(3·17 + 1) ≤ 65536 → rows ≤ 315): m = 512·312 is taken by the predicate, one row more is not, and
    the entry returns 1 there."""
    m = 512 * 312
    i = rows_of(head_inputs(17), 16)
    big = {k: (np.resize(v, (m + 1,) + v.shape[1:]) if k != "ls" else v) for k, v in i.items()}
    assert run(lib, 3, big, 256, expect=1) is None


@pytest.mark.parametrize("n", [256, 512])
def test_fused(lib, n):
    """Form 4; m = 8209 at n = 256 is 514 blocks over 512 workgroups: the grid-stride loop and its prefetch."""
    for m in [1, 15, 16, 17, 31, 33, 1000] + ([8209] if n == 256 else []):
        both(lib, 4, 17, m, n)
    both(lib, 4, 17, 1000, n, mode="mixed")
    report()


# ----------------------------------------------------------------------------- (b) lp against the fp32 mirror
def device_expf(lib, ls):
    """The device's expf(log σ[j]) per column, by one probe launch of the separate form: 64 rows per column j
    whose action equals μ in every other column (z = 0 there whatever expf gives) — the candidate among libm's
    value ± 2 ulp under which the mirror reproduces all 64 log-probs bit for bit."""
    A, R = ls.size, 64
    rng = np.random.default_rng(5)
    mu = rng.normal(size=(A * R, A)).astype(F32)
    act = mu.copy()
    for j in range(A):
        act[j * R:(j + 1) * R, j] += (rng.uniform(8, 64, R) * np.exp(ls[j])).astype(F32)
    z = np.zeros(A * R, F32)
    lp = run(lib, 0, dict(mu=mu, ls=ls, act=act, adv=z, old=z))["lp"]
    es = expf(ls)
    found = es.copy()
    for j in range(A):
        rows = slice(j * R, (j + 1) * R)
        ok = []
        for k in range(-2, 3):
            cand = es.copy()
            cand[j] = (es[j:j + 1].view(np.int32) + k).view(F32)[0]
            mine = policy_head_f32(mu[rows], ls, act[rows], z[rows], z[rows], EPS, es=cand)["lp"]
            if np.array_equal(bits(mine), bits(lp[rows])):
                ok.append((k, cand[j]))
        assert len(ok) == 1, f"column {j}: candidates {ok}"
        found[j] = ok[0][1]
    return found, int((found != es).sum())


@pytest.mark.parametrize("A", [1, 6, 17])
def test_lp_bits_against_the_mirror(lib, A):
    """Form 0's lp has the bits of policy_head_f32's: with log σ = 0 (σ = 1 exactly) outright; otherwise with
    the device's expf(log σ) per column in place of libm's wherever the two differ."""
    i = rows_of(head_inputs(A, "zero"), 1000)
    got = run(lib, 0, i)
    mine = policy_head_f32(i["mu"], i["ls"], i["act"], i["adv"], i["old"], EPS)
    np.testing.assert_array_equal(bits(got["lp"]), bits(mine["lp"]))
    np.testing.assert_array_equal(bits(got["grad_mu"]), bits(mine["grad_mu"]))      # e2 = expf(−0) = 1 too
    for mode, m in (("uniform", 4097), ("mixed", 1000)):
        i = rows_of(head_inputs(A, mode), m)
        es, differ = device_expf(lib, i["ls"])
        print(f"A {A} {mode}: the device's expf differs from libm's in {differ} of {A} columns")
        got = run(lib, 0, i)
        mine = policy_head_f32(i["mu"], i["ls"], i["act"], i["adv"], i["old"], EPS, es=es)
        np.testing.assert_array_equal(bits(got["lp"]), bits(mine["lp"]))


@pytest.mark.parametrize("form,A,n", [(0, 6, 0), (1, 6, 0), (2, 6, 64), (3, 17, 256), (4, 17, 256)])
def test_exact_ties_are_unclipped(lib, form, A, n):
    """Rows whose fp32 ratio EQUALS 1 + eps (advantage > 0) or 1 − eps (advantage < 0): the comparisons are strict,
    so the row is unclipped and has a gradient.  With log σ = 0 the device's lp is the mirror's bit for bit
    (test_lp_bits_against_the_mirror), so old_lp can be searched on the CPU, a few ulps round lp − log(1 ± eps),
    for values at which the ratio rounds onto the boundary.  lp − old_lp moves on the grid of lp's ulp, so which
    boundary can be hit depends on the set: these reach 1 + eps on nearly every even row and 1 − eps on none (at
    least 50 ties are required, whichever side).  Every form's grad_μ must have the mirror's bits."""
    src = rows_of(head_inputs(A, "zero"), 1000)
    lp = policy_head_f32(src["mu"], src["ls"], src["act"], src["adv"], src["old"], EPS)["lp"]
    up = np.arange(1000) % 2 == 0
    target = np.where(up, F32(1) + F32(EPS), F32(1) - F32(EPS)).astype(F32)
    base = (lp - np.log(target.astype(F64))).astype(F32)
    old, hit = src["old"].copy(), np.zeros(1000, bool)
    for k in range(-4, 5):
        cand = (base.view(np.int32) + k).view(F32)
        r = np.exp((lp - cand).astype(F64)).astype(F32)
        new = (r == target) & ~hit
        old[new], hit = cand[new], hit | new
    assert hit.sum() >= 50, (int((hit & up).sum()), int((hit & ~up).sum()))
    adv = np.where(up, 1, -1).astype(F32) * (np.abs(src["adv"]) + F32(0.5))
    i = dict(src, old=old, adv=adv)
    mine = policy_head_f32(i["mu"], i["ls"], i["act"], adv, old, EPS)
    assert (mine["ratio"][hit] == target[hit]).all() and not mine["clipped"][hit].any()
    got = run(lib, form, i, n)
    assert got["grad_mu"][hit].all(axis=1).all(), f"{NAMES[form]}: a tie row was clipped"
    want = mine["grad_mu"] + F32(0) if form >= 2 else mine["grad_mu"]
    np.testing.assert_array_equal(bits(got["grad_mu"]), bits(want))


# ----------------------------------------------------------------------------- (c) one-hot advantages
ONE_HOT = [(0, 6, 257, 0), (1, 6, 257, 0), (1, 33, 257, 0), (2, 6, 257, 64), (2, 1, 257, 256), (3, 17, 1000, 256),
           (4, 17, 33, 256), (4, 17, 1000, 512)]


@pytest.mark.parametrize("form,A,m,n", ONE_HOT)
def test_one_hot_rows(lib, form, A, m, n):
    """adv = 0 except at row i (ent_coeff = 0): every other row's terms are exactly 0, so grad_log_σ is row i's
    own term, gb its grad_μ, gW its outer product with x and the loss −(its surrogate)/m, exact in any order.
    Row i's advantage takes the sign under which the row is unclipped."""
    src = rows_of(head_inputs(A), m)
    pos = {0, 1, 15, 16, 63, 64, 255, 256, m - 1} | {(m - 1) // T * T for T in (4, 16, 64, 256)}
    rel = row_rel_bound(src["mu"], src["ls"], src["act"])
    lp = policy_head_f64(src["mu"], src["ls"], src["act"], src["adv"], src["old"], EPS64, 0.0)
    for r in sorted(p for p in pos if 0 <= p < m):
        adv = np.zeros(m, F32)
        adv[r] = 1.5 if lp["ratio"][r] < 1 else -1.5
        i = dict(src, adv=adv)
        got = run(lib, form, i, n, ent=0.0)
        ref = policy_head_f64(i["mu"], i["ls"], i["act"], adv, i["old"], EPS64, 0.0)
        what = f"{NAMES[form]} m {m} A {A} row {r}"
        assert not ref["clipped"][r]
        gm = got["grad_mu"]
        others = np.arange(m) != r
        assert (gm[others] == 0).all() and gm[r].all(), what
        assert (np.abs(gm[r] - ref["grad_mu"][r]) <= np.abs(ref["grad_mu"][r]) * rel[r]).all(), what
        d2 = (i["act"][r].astype(F64) - i["mu"][r]) ** 2 * np.exp(-2.0 * i["ls"])
        t_b = (1 + d2) * abs(ref["dlp"][r]) * rel[r]
        assert (np.abs(got["gls"] - ref["gls_terms"][r]) <= t_b).all(), f"{what}: grad_log_std"
        assert abs(got["loss"] - ref["loss_terms"][r]) <= abs(ref["loss_terms"][r]) * rel[r], f"{what}: loss"
        if form >= 2:
            np.testing.assert_array_equal(got["gb"], gm[r], err_msg=f"{what}: gb")
            np.testing.assert_array_equal(got["gW"][:, :A], gm[r][:, None] * i["mu"][r][None, :], err_msg=f"{what}: gW")
            assert not got["gW"][:, A:].any() and not got["gx"][:, A:].any(), what


# ----------------------------------------------------------------------------- (e) non-finite rows
POISON = [(0, 6, 257, 0), (1, 6, 65, 0), (1, 33, 257, 0), (2, 6, 65, 64), (3, 17, 17, 256), (4, 17, 17, 256)]


@pytest.mark.parametrize("form,A,m,n", POISON)
def test_non_finite_rows_stay_in_their_row(lib, form, A, m, n):
    """Each form at its smallest shape of more than one workgroup.  Three poisoned rows: old_lp = lp − 100 (ratio
    +inf; its advantage made positive, so the row is clipped and its gradient 0·adv·inf = NaN — with a negative
    advantage it would be +inf), old_lp = lp + 200 (ratio 0) and a NaN action.  This pins the reference's
    behaviour (the oracle's sums are NaN too); it does not change it."""
    src = rows_of(head_inputs(A), m)
    clean = run(lib, form, src, n)
    lp = policy_head_f32(src["mu"], src["ls"], src["act"], src["adv"], src["old"], EPS)["lp"]
    r_inf, r_zero, r_nan = 1, m // 2, m - 1
    old, act, adv = src["old"].copy(), src["act"].copy(), src["adv"].copy()
    old[r_inf], old[r_zero] = lp[r_inf] - F32(100), lp[r_zero] + F32(200)
    adv[r_inf] = abs(adv[r_inf]) + F32(0.5)
    adv[r_zero] = abs(adv[r_zero]) + F32(0.5)             # unclipped: the gradient is −adv·0/m
    act[r_nan, A // 2] = np.nan
    i = dict(src, old=old, act=act, adv=adv)
    got = run(lib, form, i, n)
    what = f"{NAMES[form]} m {m} A {A}"
    key = "gx" if form >= 2 else "grad_mu"
    others = np.ones(m, bool)
    others[[r_inf, r_zero, r_nan]] = False
    np.testing.assert_array_equal(bits(got[key][others]), bits(clean[key][others]), err_msg=f"{what}: other rows")
    assert np.isfinite(got[key][others]).all()
    assert np.isnan(got["grad_mu"][r_inf]).all() and np.isnan(got["grad_mu"][r_nan]).all(), what
    # the ratio-0 row: finite, the mirror's values and the model's (exp(−200)·adv/m is below fp32's smallest
    # normal number 2⁻¹²⁶: the fp32 result is a zero)
    ref = policy_head_f64(i["mu"], i["ls"], act, adv, old, EPS64, 0.0)
    mine = policy_head_f32(i["mu"], i["ls"], act, adv, old, EPS)
    assert np.isfinite(got[key][r_zero]).all() and not ref["clipped"][r_zero]
    np.testing.assert_array_equal(got["grad_mu"][r_zero], mine["grad_mu"][r_zero])
    assert (np.abs(got["grad_mu"][r_zero] - ref["grad_mu"][r_zero]) <= 2.0 ** -126).all()
    # the sums are NaN, as the oracle's are: a change that silently drops such rows is noticed
    assert np.isnan(got["gls"]).all() and np.isnan(got["loss"]), what
    if form >= 2:
        assert np.isnan(got["gb"]).all() and np.isnan(got["gW"]).all(), what


# ----------------------------------------------------------------------------- (f) the entry's arguments
def test_arguments(lib):
    i = rows_of(head_inputs(6), 64)
    d = dev(lib, np.zeros(64 * 512, F32))
    out = C.c_double(0)
    p = d.ptr

    def call(form, m=64, A=6, n=64, eps=EPS, null=(), shift=()):
        a = [p] * 13
        for k in null:
            a[k] = None
        for k in shift:
            a[k] = p + 4
        return lib.ppo_policy_head_device(form, m, A, n, 0, eps, ENT, *a, C.byref(out))

    LS, ACT, ADV, OLD, MU, X, W, B, LP, GMU, GX, GW, GLS = range(13)
    try:
        for form in range(5):                             # bad arguments: −1, nothing recorded
            assert call(form, m=0) == -1 and call(form, m=-3) == -1 and call(form, A=0) == -1
            assert call(form, eps=float("nan")) == -1
            for k in (LS, ACT, ADV, OLD, MU, GLS):
                assert call(form, null=(k,)) == -1
        assert call(-1) == -1 and call(5) == -1
        assert lib.ppo_policy_head_device(1, 64, 6, 0, 0, EPS, ENT, *([p] * 13), None) == -1
        assert call(0, null=(LP,)) == -1 and call(0, null=(GMU,)) == -1 and call(1, null=(GMU,)) == -1
        for form in (2, 3, 4):
            A = 6 if form == 2 else 17
            assert call(form, A=A, n=0) == -1
            for k in (X, W, GX, GW) + ((B,) if form != 3 else ()):
                assert call(form, A=A, n=256, null=(k,)) == -1
            for k in (X, W, GX, GW):
                assert call(form, A=A, n=256, shift=(k,)) == -1
        # shapes a form does not take: 1, nothing launched
        assert call(1, A=4097) == 1 and call(0, A=16385) == 1
        for A, n in ((2, 64), (17, 256), (6, 96), (6, 1024), (1, 32)):
            assert call(2, A=A, n=n) == 1
        for form in (3, 4):
            for A, n in ((16, 256), (6, 256), (17, 128), (17, 1024), (17, 384)):
                assert call(form, A=A, n=n) == 1
        # arrays a form does not use may be NULL
        assert call(1, null=(X, W, B, LP, GX, GW)) == 0
        assert call(0, null=(X, W, B, GX, GW)) == 0
        assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    finally:
        d.free()
    assert run(lib, 1, i) is not None
