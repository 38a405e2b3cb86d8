"""Global gradient-norm clipping in the device PPO update (ppo_set_max_grad_norm, csrc/clip.hip).

The oracle has no clipping: the reference here is built from its pieces (mlp_forward / mlp_backward / mse /
log_prob / policy_loss_and_grad / adam_update / feistel_perm) with the float64 numpy clip of clip_ref.py
(pinned against torch in test_clip_cpu.py) between gradient and Adam.

Shape of the update tests: 17 → 2×64 → 6, N = 1024, B = 256 (four minibatches per epoch), device
shuffle, ppo_fill_synthetic, ent_coeff = 0.01 so the log σ gradient carries its entropy term.

Adam's moment constants are the kernel's own: (1 − β) evaluated in fp32, as adam.hip and the
reference do (1 − 0.999f = 0.99998713e-3: the literal 0.001 is 1.3e-5 away, more than the 1e-5 the
moment checks allow).
"""
import ctypes as C

import numpy as np
import pytest

import ppo_ffi
from clip_ref import clip_grad_norm
from helpers import F32, assert_gemm_close, assert_rel_close, gpu_relu_masks, nn_grads_packed, nn_params_packed
from bf16_ref import bf16
from test_gpu_production import RELU, device_buffer, ref_policy_grads, ref_value_grads
from test_gpu_update import make_ppo, policy_state

pytestmark = pytest.mark.gpu

SIZES, N, B, A = [17, 64, 64, 6], 1024, 256, 6
SV = SIZES[:-1] + [1]
LR, ENT, SEED = 3e-4, 0.01, 4321
B1C = float(F32(1) - F32(0.9))            # (1 − β1), (1 − β2) as fp32 arithmetic gives them
B2C = float(F32(1) - F32(0.999))
# PPO_K_ADAM launches of the 4 + 4 step update below with clipping off, read from a run of the commit
# before this feature: one flat Adam per value step, one paired (μ + log σ) Adam per policy step
PARENT_ADAM_LAUNCHES = 8


def norm64(*arrays):
    return float(np.sqrt(sum(float(np.sum(np.asarray(a, np.float64) ** 2)) for a in arrays)))


def _adam_state(lib, adam_ptr):
    """(gradient, m, v) over the Adam's flat span, as the kernels index them."""
    a = adam_ptr.contents
    assert a.flat
    n = a.span
    return tuple(ppo_ffi.d2h(lib, p, F32, n) for p in (a.grad_weights[0], a.m, a.v))


def run_update(lib, oracle, max_norm, nv, npol, dtype=0, masks=False, prof=False):
    """A fresh PPO from fixed seeds, the first nv value and npol policy steps of one update, and
    everything the tests read back."""
    ppo = make_ppo(lib, oracle, SIZES, N, seed=1234, init_std=0.7, ent_coeff=ENT)
    assert lib.ppo_set_compute_dtype(ppo, dtype) == 0
    lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 500)
    lib.ppo_synchronize()
    pol = ppo.contents.policy.contents
    mu0, ls0 = policy_state(lib, ppo)
    out = dict(mu0=mu0, ls0=ls0, v0=nn_params_packed(lib, ppo.contents.V), buf=device_buffer(lib, ppo, N, SIZES[0], A))
    if max_norm is not None:
        assert lib.ppo_set_max_grad_norm(ppo, max_norm) == 0
    lib.ppo_set_step_limit(ppo, nv, npol)
    lib.ppo_reset_stats(ppo)
    if prof:
        lib.ppo_prof_enable(1)
        lib.ppo_prof_reset()
    lib.ppo_update(ppo, 0.99, B, 1, 1, 1, SEED)
    lib.ppo_synchronize()
    if prof:
        cnt = (C.c_long * 7)()
        lib.ppo_prof_counts(cnt)
        lib.ppo_prof_enable(0)
        out["adam_launches"] = cnt[2]                       # PPO_K_ADAM
    st = (C.c_double * 13)()
    lib.ppo_read_stats(ppo, st, 13)
    out["st"] = list(st)
    out["V"] = _adam_state(lib, ppo.contents.adam_V)
    out["mu"] = _adam_state(lib, ppo.contents.adam_policy)
    out["ls"] = _adam_state(lib, ppo.contents.adam_entropy)
    out["gV_packed"], out["gmu_packed"] = nn_grads_packed(lib, ppo.contents.V), nn_grads_packed(lib, pol.mu)
    out["v1"] = nn_params_packed(lib, ppo.contents.V)
    out["mu1"], out["ls1"] = policy_state(lib, ppo)
    out["bits_m"] = (ppo.contents.V.contents.bits_m, pol.mu.contents.bits_m)
    out["hash"] = lib.ppo_param_hash(ppo)
    key = oracle.splitmix64(SEED)
    out["perm_v"] = oracle.feistel_perm(N, key)                          # value epoch 0
    out["perm_p"] = oracle.feistel_perm(N, (key + 1) & (2**64 - 1))      # policy epoch 0
    if masks:
        out["mV"] = gpu_relu_masks(lib, ppo.contents.V, out["buf"]["state"][out["perm_v"][:B]])
        out["mmu"] = gpu_relu_masks(lib, pol.mu, out["buf"]["state"][out["perm_p"][:B]])
    if dtype == 1:
        for name, nn in (("V", ppo.contents.V.contents), ("mu", pol.mu.contents)):
            n = nn.num_params
            out["w16_" + name] = ppo_ffi.d2h(lib, nn.d_w16, np.uint16, n)
            out["flat_" + name] = ppo_ffi.d2h(lib, nn.d_params, F32, n)
    lib.ppo_set_step_limit(ppo, -1, -1)
    lib.free_ppo(ppo)
    return out


def step_norms(r, grad_scale=1.0):
    """(value, policy) norms of the read-back summed gradient buffers, float64; policy: μ and log σ jointly."""
    return grad_scale * norm64(r["V"][0]), grad_scale * norm64(r["mu"][0], r["ls"][0])


def assert_moments(r, max_norm, grad_scale=1.0, what=""):
    """m = (1 − β1)·coef·g and v = (1 − β2)·(coef·g)² after the first Adam step from zero moments, g the
    read-back gradient (× grad_scale), coef from its float64 norm: 1e-5 relative + 1e-12."""
    n_v, n_p = step_norms(r, grad_scale)
    coefs = {"V": min(1.0, max_norm / (n_v + 1e-6))}
    coefs["mu"] = coefs["ls"] = min(1.0, max_norm / (n_p + 1e-6))
    for k in ("V", "mu", "ls"):
        g, m, v = r[k]
        cg = np.asarray(g, np.float64) * (grad_scale * coefs[k])
        print(f"{what} {k}: coef {coefs[k]:.6f}, max |m - ref| / max|ref| "
              f"{np.abs(m - B1C * cg).max() / max(np.abs(B1C * cg).max(), 1e-300):.3g}")
        np.testing.assert_allclose(m, B1C * cg, rtol=1e-5, atol=1e-12, err_msg=f"{what} {k} m")
        np.testing.assert_allclose(v, B2C * cg * cg, rtol=1e-5, atol=1e-12, err_msg=f"{what} {k} v")
    return coefs


@pytest.fixture(scope="module")
def base(lib, oracle):
    """One value and one policy step with clipping off: the first-step norms every other test scales
    max_norm by, and the oracle's GAE of the same buffer."""
    r = run_update(lib, oracle, None, 1, 1)
    ref = oracle.ppo_update(SIZES, RELU(SIZES), r["mu0"], r["ls0"], r["v0"], r["buf"], batch_size=1, n_epochs_policy=0,
                            n_epochs_value=0, max_value_steps=0, max_policy_steps=0)
    r["adv"], r["tgt"] = ref["advantage"], ref["adv_target"]
    r["n_v"], r["n_p"] = step_norms(r)
    print(f"first-step norms: value {r['n_v']:.6g}, policy {r['n_p']:.6g}")
    return r


# ----------------------------------------------------------------------------- the kernel alone
NA = [1, 3, 4, 5, 1023, 1024, 262149, 3 * 2**20 + 1]


@pytest.fixture(scope="module")
def normal_pool(lib):
    rng = np.random.default_rng(11)
    a = rng.standard_normal(max(NA)).astype(F32)
    b = rng.standard_normal(17).astype(F32)
    da, db = ppo_ffi.DeviceArray.from_numpy(lib, a), ppo_ffi.DeviceArray.from_numpy(lib, b)
    yield a, b, da, db
    da.free()
    db.free()


@pytest.mark.parametrize("na", NA)
def test_norm_kernel_sizes(lib, normal_pool, na):
    """ppo_grad_norm_device on N(0,1) data against float64 numpy of the same bits: every tail length,
    a span below one workgroup, grid-stride wrap; with a side span of 0, 1 and 17 floats.  1e-5 relative
    (an fp32 pairwise sum of ≤ 4e6 non-negative terms is within ≈ 1.3e-6, the root halves it; the
    kernel sums in double).  Two calls on the same buffer return identical bits."""
    a, b, da, db = normal_pool
    for nb in (0, 1, 17):
        got = lib.ppo_grad_norm_device(da.ptr, na, db.ptr if nb else None, nb)
        ref = norm64(a[:na], b[:nb])
        print(f"na {na} nb {nb}: rel err {abs(got - ref) / ref:.3g}")
        assert abs(got - ref) <= 1e-5 * ref
        again = lib.ppo_grad_norm_device(da.ptr, na, db.ptr if nb else None, nb)
        assert np.float64(got).tobytes() == np.float64(again).tobytes()


def test_norm_kernel_zero_and_spiky(lib):
    n = 262149
    d = ppo_ffi.DeviceArray.from_numpy(lib, np.zeros(n, F32))
    assert lib.ppo_grad_norm_device(d.ptr, n, d.ptr, 17) == 0.0          # exactly
    spiky = np.full(n, 1e-3, F32)
    spiky[n // 3] = 1e3
    ppo_ffi.h2d(lib, d.ptr, spiky)
    got, ref = lib.ppo_grad_norm_device(d.ptr, n, None, 0), norm64(spiky)
    d.free()
    assert abs(got - ref) <= 1e-5 * ref


# ----------------------------------------------------------------------------- one step, moments
def test_one_step_moments(lib, oracle, base):
    """Clipping off reports zeros in out[9..12]; with max_norm = half the smaller first-step norm both
    steps clip, the reported norms are the read-back gradients', Adam's moments are those of the
    clipped gradient (a parameter check alone would pass unclipped: the first Adam step is ≈ lr·sign g),
    the update ran multi-launch, and the gradients are the oracle's."""
    assert base["st"][9:13] == [0.0, 0.0, 0.0, 0.0]
    assert base["st"][1] == 1 and base["st"][3] == 1
    max_norm = 0.5 * min(base["n_v"], base["n_p"])
    r = run_update(lib, oracle, max_norm, 1, 1, masks=True)
    n_v, n_p = step_norms(r)
    print(f"reported norms {r['st'][9]:.9g} / {r['st'][10]:.9g}, read-back {n_v:.9g} / {n_p:.9g}")
    assert abs(r["st"][9] - n_v) <= 1e-5 * n_v
    assert abs(r["st"][10] - n_p) <= 1e-5 * n_p
    assert r["st"][11] == 1 and r["st"][12] == 1
    coefs = assert_moments(r, max_norm, what="one step")
    assert all(c <= 0.5001 for c in coefs.values())
    assert r["bits_m"] == (B, B)                # the multi-launch loop ran, not a single-workgroup phase
    rows_v, rows_p = r["perm_v"][:B], r["perm_p"][:B]
    buf = r["buf"]
    g_ref, _ = ref_value_grads(oracle, SV, r["v0"], buf["state"][rows_v], base["tgt"][rows_v], r["mV"], "clip value")
    assert_gemm_close(r["gV_packed"], g_ref, B, "clip value grads")
    g_ref, gls_ref = ref_policy_grads(oracle, SIZES, r["mu0"], r["ls0"], buf["state"][rows_p], buf["action"][rows_p],
                                      base["adv"][rows_p], buf["logprob"][rows_p], r["mmu"], "clip policy",
                                      ent_coeff=ENT)
    assert_gemm_close(r["gmu_packed"], g_ref, B, "clip policy grads")
    assert_rel_close(r["ls"][0], gls_ref, 1e-3, 1e-4 * max(1.0, float(np.abs(gls_ref).max())), "clip log_std grad")


# ----------------------------------------------------------------------------- several steps, parameters
def _reference_loop(oracle, base, n_steps, max_norm):
    """n_steps value and policy steps of the update in Python: oracle gradients, float64 clip
    (max_norm None: no clip), oracle Adam."""
    buf, tgt, adv = base["buf"], base["tgt"], base["adv"]
    v, mu, ls = base["v0"].copy(), base["mu0"].copy(), base["ls0"].copy()
    st = {k: [np.zeros_like(p), np.zeros_like(p), 0] for k, p in (("v", v), ("mu", mu), ("ls", ls))}

    def adam(k, p, g):
        st[k][2] = oracle.adam_update(p, g.astype(F32), st[k][0], st[k][1], st[k][2], LR)

    for s in range(n_steps):
        rows = base["perm_v"][(s * B + np.arange(B)) % N]
        g, _ = ref_value_grads(oracle, SV, v, buf["state"][rows], tgt[rows], None, "ref value")
        coef = 1.0 if max_norm is None else clip_grad_norm([g], max_norm)[1]
        adam("v", v, g.astype(np.float64) * coef)
    for s in range(n_steps):
        rows = base["perm_p"][(s * B + np.arange(B)) % N]
        g, gls = ref_policy_grads(oracle, SIZES, mu, ls, buf["state"][rows], buf["action"][rows], adv[rows],
                                  buf["logprob"][rows], None, "ref policy", ent_coeff=ENT)
        coef = 1.0 if max_norm is None else clip_grad_norm([g, gls], max_norm)[1]
        adam("ls", ls, gls.astype(np.float64) * coef)        # the entropy Adam, then the policy's
        adam("mu", mu, g.astype(np.float64) * coef)
    return v, mu, ls


def _elementwise(got, want, n_steps, what):
    """test_short_update_elementwise's bounds: max error ≤ 2·lr·steps and ≥ 99 % within 0.1·lr."""
    err = np.abs(got.astype(np.float64) - want)
    q = float((err <= 0.1 * LR).mean())
    print(f"{what}: max err {err.max() / LR:.4f} lr, {100 * q:.3f} % within 0.1 lr")
    return err.max() <= 2 * LR * n_steps and q >= 0.99


def test_four_steps_parameters(lib, oracle, base):
    """4 value and 4 policy steps (one epoch each) with max_norm = half the smaller first-step norm: V, μ
    and log σ against the Python reference loop, element by element; the same loop without the clip
    must miss the GPU's parameters on at least one tensor."""
    n, max_norm = 4, 0.5 * min(base["n_v"], base["n_p"])
    r = run_update(lib, oracle, max_norm, n, n)
    assert r["st"][1] == n and r["st"][3] == n
    print(f"clipped steps: value {r['st'][11]:.0f}, policy {r['st'][12]:.0f}")
    assert r["st"][11] >= 1 and r["st"][12] >= 1
    got = (r["v1"], r["mu1"], r["ls1"])
    names = ("V", "mu", "log_std")
    clipped = _reference_loop(oracle, base, n, max_norm)
    ok = [_elementwise(g, w, n, f"vs clipped reference, {k}") for g, w, k in zip(got, clipped, names)]
    assert all(ok), dict(zip(names, ok))
    plain = _reference_loop(oracle, base, n, None)
    ok = [_elementwise(g, w, n, f"vs UNCLIPPED reference, {k}") for g, w, k in zip(got, plain, names)]
    assert not all(ok), "the unclipped reference matches too: the test does not discriminate"


# ----------------------------------------------------------------------------- inactive clip
def test_inactive_clip(lib, oracle, base):
    """max_norm far above the norms: nothing clips, the norms are still reported, and the moments are
    bit for bit those of the unscaled gradient (coef = 1 exactly)."""
    r = run_update(lib, oracle, 100.0 * max(base["n_v"], base["n_p"]), 1, 1)
    n_v, n_p = step_norms(r)
    assert r["st"][11] == 0 and r["st"][12] == 0
    assert abs(r["st"][9] - n_v) <= 1e-5 * n_v and abs(r["st"][10] - n_p) <= 1e-5 * n_p
    for k in ("V", "mu", "ls"):
        g, m, _ = r[k]
        np.testing.assert_array_equal(m, (F32(1) - F32(0.9)) * g, err_msg=k)


# ----------------------------------------------------------------------------- data parallel scaling
def test_data_parallel_scale(lib, oracle, base, monkeypatch):
    """Two identical in-process ranks (PPO_COMM_LOOPBACK=2): the gradient buffer holds 2g, the norm is
    the mean gradient's ‖g‖, and Adam's moments are those of coef·g with coef from ‖g‖.  Two identically
    seeded runs: where their gradients agree bit for bit, so must the parameter hashes (the norm adds no
    run-to-run difference).  At this shape they do not agree — the gradient kernels' own atomics reorder
    (observed on the MI355X: the read-back gradients of the two runs differ in their last bits) — so the
    hash assertion has no fixed input and is not made; test_norm_kernel_sizes' two-calls-identical check
    is the determinism evidence."""
    max_norm = 0.5 * min(base["n_v"], base["n_p"])
    monkeypatch.setenv("PPO_COMM_LOOPBACK", "2")
    assert lib.ppo_comm_init(0, 1, None) == 0, lib.ppo_last_error()
    try:
        assert lib.ppo_comm_world() == 2
        runs = [run_update(lib, oracle, max_norm, 1, 1) for _ in range(2)]
    finally:
        lib.ppo_comm_finalize()
        monkeypatch.delenv("PPO_COMM_LOOPBACK")
    assert lib.ppo_comm_world() == 1
    r = runs[0]
    n_v, n_p = step_norms(r, 0.5)
    print(f"loopback: reported {r['st'][9]:.9g} / {r['st'][10]:.9g}, ‖g‖ {n_v:.9g} / {n_p:.9g}")
    assert abs(r["st"][9] - n_v) <= 1e-5 * n_v
    assert abs(r["st"][10] - n_p) <= 1e-5 * n_p
    assert r["st"][11] == 1 and r["st"][12] == 1
    assert_moments(r, max_norm, grad_scale=0.5, what="loopback")
    same = all(np.array_equal(runs[0][k][0], runs[1][k][0]) for k in ("V", "mu", "ls"))
    print(f"loopback: gradients bit-identical between the two runs: {same}; hashes {runs[0]['hash']:#x} "
          f"{runs[1]['hash']:#x}")
    if same:
        assert runs[0]["hash"] == runs[1]["hash"]


# ----------------------------------------------------------------------------- bf16 mode
def test_bf16_mode(lib, oracle, base):
    """bf16 compute mode goes through the same flat Adam kernels: moments of the clipped gradient, and
    the bf16 weight shadow the Adam pass writes equals the rounded fp32 parameters."""
    max_norm = 0.5 * min(base["n_v"], base["n_p"])
    r = run_update(lib, oracle, max_norm, 1, 1, dtype=1)
    assert r["st"][11] == 1 and r["st"][12] == 1
    assert_moments(r, max_norm, what="bf16")
    for name in ("V", "mu"):
        want = (bf16(r["flat_" + name]).view(np.uint32) >> 16).astype(np.uint16)
        np.testing.assert_array_equal(r["w16_" + name], want, err_msg=name)


# ----------------------------------------------------------------------------- launch accounting
def test_launch_accounting(lib, oracle, base):
    """One norm launch per minibatch step in the PPO_K_ADAM class with clipping on; none with it off."""
    n = 4
    off = run_update(lib, oracle, None, n, n, prof=True)
    on = run_update(lib, oracle, 0.5 * min(base["n_v"], base["n_p"]), n, n, prof=True)
    assert off["adam_launches"] == PARENT_ADAM_LAUNCHES
    assert on["adam_launches"] == off["adam_launches"] + 2 * n


# ----------------------------------------------------------------------------- setter
def test_setter_edge_cases(lib, oracle):
    ppo = make_ppo(lib, oracle, SIZES, N)
    assert lib.ppo_get_max_grad_norm(ppo) == 0.0
    assert lib.ppo_set_max_grad_norm(ppo, 0.5) == 0 and lib.ppo_get_max_grad_norm(ppo) == 0.5
    assert lib.ppo_set_max_grad_norm(ppo, float("nan")) == -1 and lib.ppo_get_max_grad_norm(ppo) == 0.5
    for off in (0.0, -1.0, float("inf")):
        assert lib.ppo_set_max_grad_norm(ppo, 0.25) == 0 and lib.ppo_get_max_grad_norm(ppo) == 0.25
        assert lib.ppo_set_max_grad_norm(ppo, off) == 0 and lib.ppo_get_max_grad_norm(ppo) == 0.0
    lib.free_ppo(ppo)
