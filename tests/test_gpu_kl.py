"""Target-KL early stopping and the KL / clip-fraction statistics of the device PPO update
(ppo_set_target_kl, csrc/kl.hip).

The oracle has no such feature: the reference KL sequence is built from it step by step — for each k the
oracle's update truncated at k policy steps gives the parameters step k saw, mlp_forward + log_prob on
minibatch k (feistel_perm) give its log-probs, and kl_ref.py (pinned against torch in test_kl_cpu.py) the
statistic.  A stopped update must equal the oracle's update truncated at the stop step.

Shape of the update tests (test_gpu_clip.py's): 17 → 2×64 → 6, N = 1024, B = 256 (four minibatches per
epoch), device shuffle, ppo_fill_synthetic, ent_coeff = 0.01; one value epoch and four policy epochs (16
policy steps).  Both sides draw the value epoch's shuffle key first, so the oracle runs with the same epoch
counts and a value-step cap of zero where only the policy matters.  lr_policy = 3e-3 (ten times create_ppo's),
chosen on the CPU with the oracle on a buffer of the same distribution: the KL then reaches 0.04–0.1 within
the 16 steps, grows visibly from step to step, and offers a stop step with a ≥ 20 % gap.
"""
import ctypes as C

import numpy as np
import pytest

import ppo_ffi
from clip_ref import clip_grad_norm
from helpers import F32, assert_gemm_close, gpu_relu_masks, nn_grads_packed, nn_params_packed
from kl_ref import approx_kl, clip_fraction
from bf16_ref import bf16
from test_gpu_production import RELU, device_buffer, ref_policy_grads
from test_gpu_update import make_ppo, policy_state

pytestmark = pytest.mark.gpu

SIZES, N, B, A = [17, 64, 64, 6], 1024, 256, 6
NB = N // B
LR_V, LR_P, ENT, SEED, EPS = 3e-4, 3e-3, 0.01, 4321, 0.2
NPE, NVE = 4, 1                     # policy / value epochs
STEPS = NPE * NB
# Largest relative deviation of the GPU's per-step KL from the oracle-built sequence, steps 1..15 (step 0's KL
# is ≈ 0 on both sides and is bounded absolutely).  The bound is 4× the value measured on the MI355X (2.4e-6:
# test_monitor_mode's docstring) and must stay under a tenth of the stop test's threshold gap.
KL_SEQ_RTOL = 4 * 2.4e-6
M64 = 2**64 - 1


def _packed_from_span(lib, nn_ptr, d_span):
    """A flat per-network device array (Adam's m / v: the parameters' layout, padding included) in the
    oracle's packed order."""
    nn = nn_ptr.contents
    base = C.cast(nn.d_params, C.c_void_p).value
    flat = ppo_ffi.d2h(lib, d_span, F32, nn.num_params)
    out = []
    for i in range(nn.num_layers - 1):
        ly = nn.layers[i]
        for ptr, n in ((ly.d_weights, ly.input_size * ly.output_size), (ly.d_biases, ly.output_size)):
            off = (C.cast(ptr, C.c_void_p).value - base) // 4
            out.append(flat[off:off + n])
    return np.concatenate(out)


def run_update(lib, oracle, target_kl, *, max_norm=None, dtype=0, max_p=-1, prof=False, unset=False, masks=False):
    """A fresh PPO from fixed seeds, one update (1 value + 4 policy epochs) and everything the tests read."""
    ppo = make_ppo(lib, oracle, SIZES, N, seed=1234, init_std=0.7, ent_coeff=ENT)
    ppo.contents.lr_policy = LR_P
    assert lib.ppo_set_compute_dtype(ppo, dtype) == 0
    lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 500)
    lib.ppo_synchronize()
    pol = ppo.contents.policy.contents
    mu0, ls0 = policy_state(lib, ppo)
    out = dict(mu0=mu0, ls0=ls0, v0=nn_params_packed(lib, ppo.contents.V), buf=device_buffer(lib, ppo, N, SIZES[0], A))
    if target_kl is not None:
        assert lib.ppo_set_target_kl(ppo, target_kl) == 0
    if unset:
        assert lib.ppo_set_target_kl(ppo, 0.0) == 0
    if max_norm is not None:
        assert lib.ppo_set_max_grad_norm(ppo, max_norm) == 0
    lib.ppo_set_step_limit(ppo, -1, max_p)
    lib.ppo_reset_stats(ppo)
    if prof:
        lib.ppo_prof_enable(1)
        lib.ppo_prof_reset()
    lib.ppo_update(ppo, 0.99, B, NPE, NVE, 1, SEED)
    lib.ppo_synchronize()
    if prof:
        cnt = (C.c_long * 7)()
        lib.ppo_prof_counts(cnt)
        lib.ppo_prof_enable(0)
        out["counts"] = list(cnt)
    st = (C.c_double * 17)()
    lib.ppo_read_stats(ppo, st, 17)
    out["st"] = list(st)
    hist = (C.c_double * 64)()
    n = lib.ppo_kl_history(ppo, hist, 64)
    out["hist"] = np.array(hist[:min(n, 64)])
    out["n_hist"] = n
    ap, ae = ppo.contents.adam_policy.contents, ppo.contents.adam_entropy.contents
    out["t"] = (ap.time_step, ae.time_step, ppo.contents.adam_V.contents.time_step)
    out["m_mu"], out["v_mu"] = _packed_from_span(lib, pol.mu, ap.m), _packed_from_span(lib, pol.mu, ap.v)
    out["m_ls"], out["v_ls"] = ppo_ffi.d2h(lib, ae.m, F32, A), ppo_ffi.d2h(lib, ae.v, F32, A)
    out["gmu"] = nn_grads_packed(lib, pol.mu)
    out["gls"] = ppo_ffi.d2h(lib, pol.d_log_std_grad, F32, A)
    out["v1"] = nn_params_packed(lib, ppo.contents.V)
    out["mu1"], out["ls1"] = policy_state(lib, ppo)
    out["bits_m"] = pol.mu.contents.bits_m
    key = oracle.splitmix64(SEED)
    out["perms"] = [oracle.feistel_perm(N, (key + NVE + j) & M64) for j in range(NPE)]
    if masks:
        last = int(st[3]) - 1
        out["mmu"] = gpu_relu_masks(lib, pol.mu, out["buf"]["state"][step_rows(out["perms"], last)])
    if dtype == 1:
        nn = pol.mu.contents
        out["w16"] = ppo_ffi.d2h(lib, nn.d_w16, np.uint16, nn.num_params)
        out["flat"] = ppo_ffi.d2h(lib, nn.d_params, F32, nn.num_params)
    lib.ppo_set_step_limit(ppo, -1, -1)
    lib.free_ppo(ppo)
    return out


def step_rows(perms, k):
    return perms[k // NB][((k % NB) * B + np.arange(B)) % N]


def oracle_update(oracle, r, max_policy_steps, max_value_steps=0):
    return oracle.ppo_update(SIZES, RELU(SIZES), r["mu0"], r["ls0"], r["v0"], r["buf"], batch_size=B,
                             n_epochs_policy=NPE, n_epochs_value=NVE, ent_coeff=ENT, epsilon=EPS, lr_policy=LR_P,
                             lr_v=LR_V, shuffle_mode=1, seed=SEED, max_value_steps=max_value_steps,
                             max_policy_steps=max_policy_steps)


def pick_stop_step(kls):
    """The step s (not at an epoch's first or last position) whose KL stands furthest above every earlier
    step's, past the first epoch where there is one (so the host's epoch-boundary stop differs from the
    device's): (s, max earlier KL, relative width of the open interval between that and k_s)."""
    best = None
    for s in range(1, len(kls) - 1):
        if s % NB in (0, NB - 1):
            continue
        prev = float(max(kls[:s]))
        if prev <= 0 or kls[s] <= prev:
            continue
        gap = (kls[s] - prev) / prev
        cand = (gap >= 0.2, s >= NB, gap, s, prev)
        if best is None or cand[:3] > best[:3]:
            best = cand
    assert best is not None, f"no step rises above its predecessors: {kls}"
    return best[3], best[4], best[2]


def elementwise(got, want, n_steps, lr, what):
    """test_gpu_update.py::test_short_update_elementwise's bounds: max error ≤ 2·lr·steps, ≥ 99 % within 0.1·lr."""
    err = np.abs(np.asarray(got, np.float64) - want)
    q = float((err <= 0.1 * lr).mean())
    print(f"{what}: max err {err.max() / lr:.4f} lr, {100 * q:.3f} % within 0.1 lr")
    assert err.max() <= 2 * lr * max(n_steps, 1), f"{what}: max err {err.max():.3g}"
    assert q >= 0.99, f"{what}: only {100 * q:.2f} % within 0.1·lr"


def moments_close(got, want, rel, what):
    """Adam moments against the oracle's after the same steps: max |err| ≤ rel · max |ref|.  Over the ≤ 14
    steps here the two parameter trajectories stay within 0.1·lr on 99 % of the elements (the short-update
    bound), a tenth of what one Adam step moves a parameter, so each step's gradient differs by a small
    fraction of the change between consecutive steps' gradients; 2 % of the largest moment (4 % for v,
    which squares the gradient) is far above that and five times below what one more Adam step moves
    m by ((1 − β1) = 10 % of a gradient) — the difference the frozen-state checks must see."""
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    top = float(np.abs(want).max())
    print(f"{what}: max err {err / top:.3g} of max |ref|")
    assert err <= rel * top, f"{what}: {err:.3g} > {rel} x {top:.3g}"


# ----------------------------------------------------------------------------- 1. the kernel alone
MS = [1, 3, 255, 256, 257, 4097, 32768]


def kl_inputs(oracle, Ak, seed):
    """μ, log σ, actions and old log-probs for max(MS) rows with |lp − old_lp| ∈ [0.05, 0.5] and no row
    within 1e-4 of the clip boundary (rows that are get a new draw)."""
    rng = np.random.default_rng(seed)
    m = max(MS)
    mu = rng.normal(size=(m, Ak)).astype(F32)
    ls = rng.uniform(-0.7, 0.2, Ak).astype(F32)
    act = (mu + rng.normal(size=(m, Ak)).astype(F32) * np.exp(ls)).astype(F32)
    lp = oracle.log_prob(mu, ls, act)
    assert np.abs(lp).max() <= 64

    def draw(n):
        return rng.uniform(0.05, 0.5, n) * rng.choice([-1.0, 1.0], n)

    def near(old):
        x = lp.astype(np.float64) - old.astype(np.float64)
        return (np.abs(np.abs(np.exp(x) - 1.0) - EPS) < 1e-4) | (np.abs(x) < 0.05) | (np.abs(x) > 0.5)

    old = (lp - draw(m)).astype(F32)
    for _ in range(50):
        bad = near(old)
        if not bad.any():
            break
        old[bad] = (lp[bad] - draw(int(bad.sum()))).astype(F32)
    x = lp.astype(np.float64) - old.astype(np.float64)
    assert not near(old).any()
    assert (np.abs(x) >= 0.05).all() and (np.abs(x) <= 0.5).all()
    assert (np.abs(np.abs(np.exp(x) - 1.0) - EPS) >= 1e-4).all()
    return mu, ls, act, lp, old


@pytest.mark.parametrize("Ak", [1, 6, 17])
def test_kl_kernel_sizes(lib, oracle, Ak):
    """ppo_policy_kl_device against kl_ref on identical inputs, m from one row over the workgroup edges to
    more rows than one pass of the grid covers.  The clip fraction matches exactly (no row is within 1e-4 of
    the boundary; the fp32 log-prob is within ≈ 1e-5).  KL within rtol 1e-3: δx ≲ 1e-5 at |lp| ≤ 64 and the
    relative KL error ≈ 2 δx / |x| ≤ 4e-4 at |x| ≥ 0.05.  Two calls return bit-identical doubles."""
    mu, ls, act, lp, old = kl_inputs(oracle, Ak, 100 + Ak)
    d = [ppo_ffi.DeviceArray.from_numpy(lib, a) for a in (mu, ls, act, old)]
    try:
        for m in MS:
            got, again = (C.c_double * 2)(), (C.c_double * 2)()
            assert lib.ppo_policy_kl_device(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, m, Ak, EPS, got) == 0
            assert lib.ppo_policy_kl_device(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, m, Ak, EPS, again) == 0
            kl, frac = approx_kl(lp[:m], old[:m]), clip_fraction(lp[:m], old[:m], EPS)
            print(f"A {Ak} m {m}: kl {got[0]:.9g} ref {kl:.9g} rel err {abs(got[0] - kl) / kl:.3g}; "
                  f"clip fraction {got[1]:.6f} ref {frac:.6f}")
            assert got[1] == frac
            assert abs(got[0] - kl) <= 1e-3 * kl
            assert bytes(got) == bytes(again)
    finally:
        for a in d:
            a.free()


# ----------------------------------------------------------------------------- 2. setter
def test_setter_semantics(lib, oracle):
    ppo = make_ppo(lib, oracle, SIZES, N)
    assert lib.ppo_get_target_kl(ppo) == 0.0                         # a fresh PPO: off
    assert lib.ppo_set_target_kl(ppo, 0.02) == 0 and lib.ppo_get_target_kl(ppo) == F32(0.02)
    assert lib.ppo_set_target_kl(ppo, float("nan")) == -1 and lib.ppo_get_target_kl(ppo) == F32(0.02)
    for off in (0.0, -1.0, float("-inf")):
        assert lib.ppo_set_target_kl(ppo, 0.25) == 0 and lib.ppo_get_target_kl(ppo) == 0.25
        assert lib.ppo_set_target_kl(ppo, off) == 0 and lib.ppo_get_target_kl(ppo) == 0.0
    assert lib.ppo_set_target_kl(ppo, float("inf")) == 0 and lib.ppo_get_target_kl(ppo) == float("inf")
    lib.free_ppo(ppo)


# ----------------------------------------------------------------------------- 3. off means off
def test_off_means_off(lib, oracle):
    """A PPO whose target_kl was set and unset launches exactly what a fresh one does (every profiling class
    over the 4 + 4 step update), and the four statistics read 0."""
    fresh = run_update(lib, oracle, None, max_p=NB, prof=True)
    unset = run_update(lib, oracle, 0.01, max_p=NB, prof=True, unset=True)
    print(f"launch counts per class: fresh {fresh['counts']}, set-then-unset {unset['counts']}")
    assert fresh["counts"] == unset["counts"]
    for r in (fresh, unset):
        assert r["st"][1] == NB and r["st"][3] == NB
        assert r["st"][13:17] == [0.0, 0.0, 0.0, 0.0]
        assert r["n_hist"] == 0
        assert r["t"] == (NB, NB, NB)


# ----------------------------------------------------------------------------- 4. monitor mode
@pytest.fixture(scope="module")
def monitor(lib, oracle):
    """target_kl = +inf over the whole update, the oracle's update truncated at every k, and the reference KL
    sequence built from them."""
    r = run_update(lib, oracle, float("inf"))
    r["refs"] = [oracle_update(oracle, r, k) for k in range(STEPS + 1)]
    kls, fracs = [], []
    buf = r["buf"]
    for k in range(STEPS):
        rows, ref = step_rows(r["perms"], k), r["refs"][k]
        acts = oracle.mlp_forward(SIZES, RELU(SIZES), ref["mu"], buf["state"][rows])
        mu = oracle.mlp_layer_outputs(SIZES, acts, B)[-1]
        lp = oracle.log_prob(mu, ref["log_std"], buf["action"][rows])
        kls.append(approx_kl(lp, buf["logprob"][rows]))
        fracs.append(clip_fraction(lp, buf["logprob"][rows], EPS))
    r["kl_ref"], r["frac_ref"] = np.array(kls), np.array(fracs)
    r["adv"] = r["refs"][0]["advantage"]
    return r


def test_monitor_mode(lib, oracle, monitor):
    """+inf measures and never stops: 16 KL values against the oracle-built sequence, and the final
    parameters are the oracle's 16-step update's — monitoring changes nothing.

    Step 0 sees the parameters that sampled the buffer: x is fp32 rounding (≲ 1e-5), so its KL ≈ x²/2 is
    bounded absolutely at 1e-8 on both sides (measured: 1.1e-13 GPU, 1.8e-13 oracle).  Steps 1..15
    relatively, KL_SEQ_RTOL = 4 × the largest deviation measured on the MI355X: 2.4e-6 (the fp32 log-prob
    rounding of ≈ 1e-6 against |x| ≈ 0.15–0.4; the two parameter trajectories agreed to 1e-4·lr)."""
    r = monitor
    assert r["n_hist"] == STEPS and r["st"][3] == STEPS
    assert r["st"][15] == STEPS and r["st"][16] == -1
    assert r["t"][:2] == (STEPS, STEPS)
    assert r["bits_m"] == B                       # the multi-launch loop ran
    got, ref = r["hist"], r["kl_ref"]
    print("GPU KL   ", " ".join(f"{x:.4e}" for x in got))
    print("oracle KL", " ".join(f"{x:.4e}" for x in ref))
    assert 0 <= got[0] <= 1e-8 and 0 <= ref[0] <= 1e-8
    dev = np.abs(got[1:] - ref[1:]) / ref[1:]
    print(f"largest relative deviation of the KL sequence, steps 1..{STEPS - 1}: {dev.max():.3g} (bound {KL_SEQ_RTOL:.3g})")
    assert dev.max() <= KL_SEQ_RTOL
    assert abs(r["st"][13] - got[-1]) == 0
    print(f"last step's clip fraction {r['st'][14]:.4f}, oracle-built {r['frac_ref'][-1]:.4f}")
    rows_clipped = r["st"][14] * B                                # a count of rows over B
    assert 0 < rows_clipped <= B and abs(rows_clipped - round(rows_clipped)) <= 1e-3
    full = r["refs"][STEPS]
    elementwise(r["mu1"], full["mu"], STEPS, LR_P, "monitor mu")
    elementwise(r["ls1"], full["log_std"], STEPS, LR_P, "monitor log_std")


# ----------------------------------------------------------------------------- 5. early stop
@pytest.fixture(scope="module")
def plan(monitor):
    """The stop step and threshold, from the ORACLE's sequence: 1.5 · target_kl at the geometric middle of
    the open interval between max(k_0..k_{s−1}) and k_s."""
    s, prev, gap = pick_stop_step(monitor["kl_ref"])
    thr = float(np.sqrt(prev * monitor["kl_ref"][s]))
    print(f"stop step {s}: earlier max {prev:.4e}, k_s {monitor['kl_ref'][s]:.4e}, gap {100 * gap:.1f} %, threshold {thr:.4e}")
    return dict(s=s, prev=prev, gap=gap, target=thr / 1.5)


@pytest.fixture(scope="module")
def stopped(lib, oracle, plan):
    return run_update(lib, oracle, plan["target"], masks=True)


def test_early_stop(lib, oracle, monitor, plan, stopped):
    """The update stops at the oracle's step s on the device, the host stops issuing at the next epoch
    boundary, and the state is the oracle's update truncated at s."""
    s, r = plan["s"], stopped
    assert plan["gap"] >= 0.2 and s % NB not in (0, NB - 1)
    assert KL_SEQ_RTOL <= plan["gap"] / 10
    issued = (s // NB + 1) * NB
    print(f"stats 13..16: {r['st'][13:17]}, issued policy steps {r['st'][3]:.0f}, time steps {r['t']}")
    assert r["st"][16] == s
    assert r["st"][15] == s
    assert r["st"][3] == issued                                   # the host stopped at the epoch boundary
    assert r["st"][1] == NVE * NB                                 # the value loop ran on
    assert r["t"] == (s, s, NVE * NB)
    assert r["n_hist"] == issued
    ref = monitor["refs"][s]
    assert ref["t_mu"] == s and ref["t_ent"] == s
    elementwise(r["mu1"], ref["mu"], s, LR_P, "stopped mu")
    elementwise(r["ls1"], ref["log_std"], s, LR_P, "stopped log_std")
    moments_close(r["m_mu"], ref["m_mu"], 2e-2, "stopped mu m")
    moments_close(r["v_mu"], ref["v_mu"], 4e-2, "stopped mu v")
    moments_close(r["m_ls"], ref["m_ent"], 2e-2, "stopped log_std m")
    moments_close(r["v_ls"], ref["v_ent"], 4e-2, "stopped log_std v")
    # one more step moves the parameters by about lr each: the next truncation must fail the same criterion
    nxt = monitor["refs"][s + 1]
    assert (np.abs(r["mu1"].astype(np.float64) - nxt["mu"]) <= 0.1 * LR_P).mean() < 0.99
    # V: the whole value loop
    vfull = oracle_update(oracle, r, 0, max_value_steps=-1)
    elementwise(r["v1"], vfull["v"], NVE * NB, LR_V, "stopped V")
    # the gradient left behind is the last issued minibatch's alone, at the frozen parameters: a skipped
    # Adam that forgot to clear would leave the sum over the skipped steps
    rows, buf = step_rows(r["perms"], issued - 1), r["buf"]
    g_ref, gls_ref = ref_policy_grads(oracle, SIZES, r["mu1"], r["ls1"], buf["state"][rows], buf["action"][rows],
                                      monitor["adv"][rows], buf["logprob"][rows], r["mmu"], "stopped policy",
                                      ent_coeff=ENT)
    assert np.abs(g_ref).max() > 0
    assert_gemm_close(r["gmu"], g_ref, B, "stopped policy grads")
    np.testing.assert_allclose(r["gls"], gls_ref, rtol=1e-3, atol=1e-4 * max(1.0, float(np.abs(gls_ref).max())))


# ----------------------------------------------------------------------------- 6. bf16 mode
def test_bf16_mode(lib, oracle):
    """bf16 compute mode: the stop step from the GPU's own monitor run is honoured, the parameters are those
    of a run capped at that step, and the bf16 shadow equals the rounded parameters."""
    mon = run_update(lib, oracle, float("inf"), dtype=1)
    assert mon["n_hist"] == STEPS
    s, prev, gap = pick_stop_step(mon["hist"])
    print(f"bf16 monitor KL {' '.join(f'{x:.4e}' for x in mon['hist'])}; step {s}, gap {100 * gap:.1f} %")
    if gap < 0.2:
        pytest.skip(f"the bf16 monitor run has no gap of at least 20 % (widest {100 * gap:.1f} % at step {s})")
    target = float(np.sqrt(prev * mon["hist"][s])) / 1.5
    r = run_update(lib, oracle, target, dtype=1)
    capped = run_update(lib, oracle, float("inf"), dtype=1, max_p=s)
    assert r["st"][16] == s and r["st"][15] == s and r["st"][3] == (s // NB + 1) * NB
    assert r["t"][:2] == (s, s) and capped["t"][:2] == (s, s)
    elementwise(r["mu1"], capped["mu1"].astype(np.float64), s, LR_P, "bf16 stopped vs capped mu")
    elementwise(r["ls1"], capped["ls1"].astype(np.float64), s, LR_P, "bf16 stopped vs capped log_std")
    moments_close(r["m_mu"], capped["m_mu"].astype(np.float64), 2e-2, "bf16 stopped vs capped m")
    want = (bf16(r["flat"]).view(np.uint32) >> 16).astype(np.uint16)
    np.testing.assert_array_equal(r["w16"], want)


# ----------------------------------------------------------------------------- 7. with clipping on as well
def _clipped_policy_loop(oracle, r, adv, n_steps, max_norm):
    """n_steps policy steps in Python: oracle gradients, float64 clip (clip_ref), oracle Adam."""
    buf = r["buf"]
    mu, ls = r["mu0"].copy(), r["ls0"].copy()
    st = {k: [np.zeros_like(p), np.zeros_like(p), 0] for k, p in (("mu", mu), ("ls", ls))}
    for k in range(n_steps):
        rows = step_rows(r["perms"], k)
        g, gls = ref_policy_grads(oracle, SIZES, mu, ls, buf["state"][rows], buf["action"][rows], adv[rows],
                                  buf["logprob"][rows], None, "ref policy", ent_coeff=ENT)
        coef = clip_grad_norm([g, gls], max_norm)[1]
        for key, p, grad in (("ls", ls, gls), ("mu", mu, g)):       # the entropy Adam, then the policy's
            st[key][2] = oracle.adam_update(p, (grad.astype(np.float64) * coef).astype(F32), st[key][0], st[key][1],
                                            st[key][2], LR_P)
    return mu, ls, st


def test_with_clipping(lib, oracle, monitor):
    """max_grad_norm and target_kl together: the norm launch, then the KL launch, and Adam reads both
    pointers.  Stop step from the GPU's monitor run with the same max_norm; the stopped state equals the
    clipped Python reference loop truncated there."""
    first = run_update(lib, oracle, float("inf"), max_p=1)
    n_p = float(np.sqrt(np.sum(first["gmu"].astype(np.float64) ** 2) + np.sum(first["gls"].astype(np.float64) ** 2)))
    max_norm = 0.5 * n_p
    mon = run_update(lib, oracle, float("inf"), max_norm=max_norm)
    assert mon["n_hist"] == STEPS and mon["st"][12] >= 1           # some policy steps clipped
    s, prev, gap = pick_stop_step(mon["hist"])
    print(f"clipped monitor KL {' '.join(f'{x:.4e}' for x in mon['hist'])}; step {s}, gap {100 * gap:.1f} %")
    assert gap >= 0.2
    r = run_update(lib, oracle, float(np.sqrt(prev * mon["hist"][s])) / 1.5, max_norm=max_norm)
    assert r["st"][16] == s and r["st"][15] == s and r["st"][3] == (s // NB + 1) * NB
    assert r["t"][:2] == (s, s)
    mu, ls, st = _clipped_policy_loop(oracle, r, monitor["adv"], s, max_norm)
    elementwise(r["mu1"], mu, s, LR_P, "clipped + stopped mu")
    elementwise(r["ls1"], ls, s, LR_P, "clipped + stopped log_std")
    moments_close(r["m_mu"], st["mu"][0], 2e-2, "clipped + stopped mu m")


# ----------------------------------------------------------------------------- 8. loopback data parallel
def test_data_parallel_loopback(lib, oracle, plan, stopped, monkeypatch):
    """Two identical in-process ranks (PPO_COMM_LOOPBACK=2): the sums are all-reduced (doubled) and the mean
    runs over 2m rows, so the KL history and the stop step are the one-rank run's."""
    monkeypatch.setenv("PPO_COMM_LOOPBACK", "2")
    assert lib.ppo_comm_init(0, 1, None) == 0, lib.ppo_last_error()
    try:
        assert lib.ppo_comm_world() == 2
        mode = lib.ppo_comm_mode()
        r = run_update(lib, oracle, plan["target"])
        assert lib.ppo_comm_mode() == mode
    finally:
        lib.ppo_comm_finalize()
        monkeypatch.delenv("PPO_COMM_LOOPBACK")
    assert lib.ppo_comm_world() == 1
    s = plan["s"]
    assert r["st"][16] == s and r["st"][15] == s and r["st"][3] == stopped["st"][3]
    assert r["t"][:2] == (s, s)
    assert r["n_hist"] == stopped["n_hist"]
    a, b = r["hist"], stopped["hist"]
    assert 0 <= a[0] <= 1e-8
    dev = np.abs(a[1:] - b[1:]) / b[1:]
    print(f"loopback vs one rank: largest relative KL deviation {dev.max():.3g}")
    assert dev.max() <= KL_SEQ_RTOL
