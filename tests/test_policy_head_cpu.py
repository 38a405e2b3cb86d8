"""tests/policy_head_ref.py pinned on the CPU: the float64 model against torch autograd, the fp32 mirror against
the oracle's log_prob / policy_loss_and_grad / log_prob_backwards bit for bit, the input sets of
test_gpu_policy_head.py (no row in the guard band of the clip boundary, for every set used), and the rounding
bound itself: the fp32 mirror with expf(log σ) and expf(−2 log σ) moved by ±2 ulp per column stays inside it."""
import numpy as np
import pytest
import torch

from policy_head_ref import ENT, EPS, F32, F64, INPUT_SETS, U, entropy_f64, expf, head_inputs, lp_bound, \
    policy_head_f32, policy_head_f64, row_rel_bound, rows_of, set_rows


def test_f64_against_torch_autograd():
    """loss = −mean(min(r·A, clamp(r, 1−ε, 1+ε)·A)) − c_ent·H.  The inputs keep their guard band round the clip
    boundaries: autograd splits the gradient at an exact tie and the code does not."""
    for A in (1, 6, 17):
        i = rows_of(head_inputs(A), 1000)
        ref = policy_head_f64(i["mu"], i["ls"], i["act"], i["adv"], i["old"], EPS, ENT)
        assert (np.abs(ref["ratio"] - (1 + EPS)) >= 1e-4).all() and (np.abs(ref["ratio"] - (1 - EPS)) >= 1e-4).all()
        assert 0.1 < ref["clipped"].mean() < 0.9                      # both branches are exercised
        mu = torch.tensor(i["mu"].astype(F64), requires_grad=True)
        ls = torch.tensor(i["ls"].astype(F64), requires_grad=True)
        act, adv, old = (torch.tensor(i[k].astype(F64)) for k in ("act", "adv", "old"))
        dist = torch.distributions.Normal(mu, ls.exp())
        lp = dist.log_prob(act).sum(dim=1)
        r = (lp - old).exp()
        H = (0.5 * (1 + np.log(2 * np.pi)) + ls).sum()
        loss = -torch.min(r * adv, torch.clamp(r, 1 - EPS, 1 + EPS) * adv).mean() - ENT * H
        loss.backward()
        np.testing.assert_allclose(ref["lp"], lp.detach().numpy(), rtol=1e-13)
        np.testing.assert_allclose(ref["loss"], loss.item(), rtol=1e-12)
        np.testing.assert_allclose(ref["grad_mu"], mu.grad.numpy(), rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(ref["gls"], ls.grad.numpy(), rtol=1e-10)
        np.testing.assert_allclose(entropy_f64(i["ls"]), H.item(), rtol=1e-14)
        assert (ref["grad_mu"][ref["clipped"]] == 0).all() and (ref["dlp"][~ref["clipped"] & (i["adv"] != 0)] != 0).all()


@pytest.mark.parametrize("A", [1, 3, 6, 17, 33])
def test_f32_mirror_against_the_oracle(oracle, A):
    """The oracle is the reference's C arithmetic with libm: the mirror's log-prob, ∂L/∂lp and grad_μ carry its
    bits; its ∂log σ terms and surrogates sum to the oracle's values within fp32 summation."""
    m = 1000
    i = rows_of(head_inputs(A), m)
    got = policy_head_f32(i["mu"], i["ls"], i["act"], i["adv"], i["old"], EPS)
    lp = oracle.log_prob(i["mu"], i["ls"], i["act"])
    np.testing.assert_array_equal(got["lp"].view(np.uint32), lp.view(np.uint32))
    H = oracle.entropy(i["ls"])
    loss, g, ge = oracle.policy_loss_and_grad(i["adv"], lp, i["old"], H, ENT, EPS)
    np.testing.assert_array_equal(got["dlp"].view(np.uint32), g.view(np.uint32))
    gmu, gls = oracle.log_prob_backwards(i["mu"], i["ls"], i["act"], g)
    np.testing.assert_array_equal(got["grad_mu"].view(np.uint32), gmu.view(np.uint32))
    t = got["gls_terms"].astype(F64)
    assert (np.abs(gls - t.sum(axis=0)) <= m * U * np.abs(t).sum(axis=0)).all()
    s = got["sur"].astype(F64)
    assert abs(loss - (-s.sum() / m - ENT * H)) <= (m + 4) * U * (np.abs(s).sum() / m + abs(ENT * H))
    assert ge == F32(-ENT)
    # and the mirror's branches are the float64 model's (no row near a boundary)
    ref = policy_head_f64(i["mu"], i["ls"], i["act"], i["adv"], i["old"], float(F32(EPS)), 0.0)
    np.testing.assert_array_equal(got["clipped"], ref["clipped"])


def test_mirror_edge_cases():
    """The int × float products as the device writes them: a clipped row's gradient is 0·adv·ratio (a NaN when
    the ratio is +inf), adv = ±0 gives zeros, a NaN action a NaN row."""
    mu, ls = np.zeros((5, 2), F32), np.zeros(2, F32)
    act = np.array([[0.5, -0.5]] * 5, F32)
    act[4, 1] = np.nan
    lp = policy_head_f32(mu, ls, act, np.zeros(5, F32), np.zeros(5, F32), EPS)["lp"]
    adv = np.array([1.0, 1.0, 0.0, -0.0, 1.0], F32)
    old = lp - np.array([100.0, -200.0, 0.1, 0.1, 0.0], F32)
    r = policy_head_f32(mu, ls, act, adv, old, EPS)
    assert np.isinf(r["ratio"][0]) and np.isnan(r["grad_mu"][0]).all() and r["sur"][0] != r["sur"][0]
    assert r["ratio"][1] == 0 and (r["grad_mu"][1] == 0).all() and r["sur"][1] == 0
    assert (r["grad_mu"][2:4] == 0).all() and (r["sur"][2:4] == 0).all()
    assert np.isnan(r["grad_mu"][4]).all() and np.isnan(r["lp"][4])


@pytest.mark.parametrize("A,mode", INPUT_SETS)
def test_input_sets_and_the_bound(A, mode):
    """Every input set of the GPU tests: built with zero rows in the guard band (head_inputs asserts it; here
    for the whole set, hence for every leading-rows shape), every 17th / 19th advantage ±0, both branches
    taken — and the bound validated against the reference alone: the fp32 mirror, with libm's expf and with
    expf(log σ), expf(−2 log σ) moved by ±2 ulp per column (every column the same way, and alternating), stays
    within |ref|·(δlp + 8·2⁻²⁴) of the float64 model in grad_μ and within δlp in lp, on every row."""
    inp = head_inputs(A, mode)
    m = set_rows(A, mode)
    assert inp["mu"].shape == (m, A)
    adv = inp["adv"]
    assert (adv[::17] == 0).all() and np.signbit(adv[::19]).all() and (adv[::19] == 0).all()
    eps64 = float(F32(EPS))
    ref = policy_head_f64(inp["mu"], inp["ls"], inp["act"], adv, inp["old"], eps64, 0.0)
    assert (np.abs(ref["ratio"] - (1 + EPS)) >= 1e-4).all() and (np.abs(ref["ratio"] - (1 - EPS)) >= 1e-4).all()
    assert 0.1 < ref["clipped"].mean() < 0.9
    dlp_b, rel = lp_bound(inp["mu"], inp["ls"], inp["act"]), row_rel_bound(inp["mu"], inp["ls"], inp["act"])
    es, e2 = expf(inp["ls"]), expf(F32(-2) * inp["ls"])

    def ulps(x, k):
        return (x.view(np.int32) + np.asarray(k, np.int32)).view(F32)

    alt = np.where(np.arange(A) % 2 == 0, 2, -2)
    worst = 0.0
    for k1, k2 in [(0, 0), (2, 2), (-2, -2), (2, -2), (-2, 2), (alt, -alt), (alt, alt)]:
        got = policy_head_f32(inp["mu"], inp["ls"], inp["act"], adv, inp["old"], EPS, es=ulps(es, k1), e2=ulps(e2, k2))
        np.testing.assert_array_equal(got["clipped"], ref["clipped"])
        assert (np.abs(got["lp"] - ref["lp"]) <= dlp_b).all()
        err = np.abs(got["grad_mu"] - ref["grad_mu"])
        bound = np.abs(ref["grad_mu"]) * rel[:, None]
        assert (err <= bound).all(), f"es {k1} e2 {k2}: {float((err / np.maximum(bound, 1e-300)).max()):.3g} of the bound"
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print(f"A {A} {mode}: worst error / bound under ±2 ulp expf {worst:.3f}")
