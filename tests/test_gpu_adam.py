"""Adam on its own, bit for bit against the oracle (csrc/adam.hip, host/adam.c, and the phase
kernels csrc/tiny.hip and csrc/cluster.hip, all on csrc/ppo_math.h adam_elem).

The reference everywhere is oracle.adam_update (oracle/ref_cpu.c, compiled without FMA contraction) on
identical fp32 inputs.  Every comparison views the floats as uint32 and uses assert_array_equal: the
sign of zero counts, two NaNs are equal whatever their payload, and no tolerance appears in this module.

Two seeded input regimes.  normal: p ~ U(−1, 1), g = ±10^U(−12, 6) with about 1 % exact zeros, m and v
warmed by two oracle steps.  edge: g drawn from EDGE (zeros, subnormals, squares that underflow, go
subnormal or straddle overflow, inf, NaN) crossed with the (m, v) states of STATES — where a fast-math
division or square root, denormal flushing or a float ε would show.
"""
import ctypes as C
import struct

import numpy as np
import pytest

import ppo_ffi
from helpers import F32

pytestmark = pytest.mark.gpu

U32 = np.uint32
LR, B1, B2 = 3e-4, 0.9, 0.999
SENT = F32(-12345.678)                     # guard value around and between the caller's tensors
GUARD = 8
EDGE = np.array([0.0, -0.0, 1.401298464e-45, 1e-40, 1e-30, 1e-20, 1.8e19, 2e19, 3e38, np.inf, -np.inf, np.nan],
                F32)
STATES = ["zero", "m_only", "v_only", "warmed"]

LIBC = C.CDLL(None)
LIBC.fopen.restype = C.c_void_p
LIBC.fopen.argtypes = [C.c_char_p, C.c_char_p]
LIBC.fclose.argtypes = [C.c_void_p]


def align4(n):
    return (n + 3) & ~3


def assert_bits(got, want, what):
    """bitwise equality of two fp32 arrays; two NaNs are equal whatever their payload"""
    got, want = np.ascontiguousarray(got, F32).ravel(), np.ascontiguousarray(want, F32).ravel()
    assert got.shape == want.shape, what
    g, w = got.view(U32).copy(), want.view(U32).copy()
    nan = np.isnan(got) & np.isnan(want)
    g[nan] = 0
    w[nan] = 0
    np.testing.assert_array_equal(g, w, err_msg=what)


def normal_grads(rng, n):
    g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-12, 6, n)).astype(F32)
    g[rng.uniform(size=n) < 0.01] = 0
    return g


def edge_grads(rng, n):
    return rng.permutation(np.resize(EDGE, n))


def initial_state(oracle, rng, n, state):
    """(p, m, v) before the compared steps"""
    p = rng.uniform(-1, 1, n).astype(F32)
    m, v = np.zeros(n, F32), np.zeros(n, F32)
    if state == "m_only":
        m[:] = 1e-3
    elif state == "v_only":
        v[:] = 1e-6
    elif state == "warmed":
        t = 0
        for _ in range(2):
            t = oracle.adam_update(p, normal_grads(rng, n), m, v, t, LR)
    else:
        assert state == "zero"
    return p, m, v


def addr(ptr):
    return C.cast(ptr, C.c_void_p).value or 0


# ----------------------------------------------------------------------------- caller tensor lists
class TensorList:
    """Parameter and gradient tensors in caller device allocations, every float that is not a tensor's
    (before, between and GUARD floats after) holding SENT.  The host images are the expected device
    contents: the oracle's results go into them, and check() compares whole allocations.

    layout: "separate" — one allocation per tensor, the tensor `lead` floats in;
            ("gaps", g) — one allocation, g[i % len(g)] floats between tensor i and i + 1, the same
            offsets in the parameter and the gradient allocation;
            "offset" — parameters abut, gradients have gaps: the parameter→gradient offset differs."""

    def __init__(self, lib, lengths, layout, lead=0):
        self.lib, self.lengths, self.n = lib, list(lengths), len(lengths)
        self.size = int(sum(lengths))
        kind, gaps = layout if isinstance(layout, tuple) else (layout, None)
        if kind == "separate":
            self.ploc = [(i, lead) for i in range(self.n)]
            self.gloc = list(self.ploc)
            psizes = gsizes = [lead + ln + GUARD for ln in lengths]
        else:
            pgaps = [0] * self.n if kind == "offset" else [gaps[i % len(gaps)] for i in range(self.n)]
            ggaps = [5 * ((i + 1) % 2) for i in range(self.n)] if kind == "offset" else pgaps
            self.ploc, self.gloc, psizes, gsizes = [], [], [], []
            for loc, gp, sz in ((self.ploc, pgaps, psizes), (self.gloc, ggaps, gsizes)):
                off = lead
                for i, ln in enumerate(lengths):
                    loc.append((0, off))
                    off += ln + (gp[i] if i + 1 < self.n else 0)
                sz.append(off + GUARD)
        self.pb = [np.full(s, SENT, F32) for s in psizes]
        self.gb = [np.full(s, SENT, F32) for s in gsizes]
        self.dp = [ppo_ffi.DeviceArray(lib, 4 * s) for s in psizes]
        self.dg = [ppo_ffi.DeviceArray(lib, 4 * s) for s in gsizes]
        self.wp = (C.c_void_p * self.n)(*[self.dp[b].ptr + 4 * o for b, o in self.ploc])
        self.gp = (C.c_void_p * self.n)(*[self.dg[b].ptr + 4 * o for b, o in self.gloc])
        self.ln = ppo_ffi.c_ints(self.lengths)

    def args(self):
        return self.wp, self.gp, self.ln

    def _scatter(self, bufs, locs, cat):
        off = 0
        for (b, o), ln in zip(locs, self.lengths):
            bufs[b][o:o + ln] = cat[off:off + ln]
            off += ln

    def params(self):
        return np.concatenate([self.pb[b][o:o + ln] for (b, o), ln in zip(self.ploc, self.lengths)] or
                              [np.zeros(0, F32)]).astype(F32)

    def set_params(self, cat, upload=False):
        self._scatter(self.pb, self.ploc, cat)
        if upload:
            for h, d in zip(self.pb, self.dp):
                ppo_ffi.h2d(self.lib, d.ptr, h)

    def set_grads(self, cat):
        self._scatter(self.gb, self.gloc, cat)
        for h, d in zip(self.gb, self.dg):
            ppo_ffi.h2d(self.lib, d.ptr, h)

    def check(self, what):
        """every parameter allocation holds the expected image (the oracle's tensors, the sentinels
        untouched); every gradient allocation is as it was uploaded"""
        for i, (h, d) in enumerate(zip(self.pb, self.dp)):
            assert_bits(d.to_numpy(F32, h.size), h, f"{what}: parameter allocation {i}")
        for i, (h, d) in enumerate(zip(self.gb, self.dg)):
            assert_bits(d.to_numpy(F32, h.size), h, f"{what}: gradient allocation {i}")

    def free(self):
        for d in self.dp + self.dg:
            d.free()


class AdamRun:
    """A device Adam over a TensorList beside the oracle's state (p in the list's images, m, v, t)."""

    def __init__(self, lib, oracle, tl, p, m, v, t0=0):
        self.lib, self.oracle, self.tl = lib, oracle, tl
        tl.set_params(p, upload=True)
        tl.set_grads(np.zeros(tl.size, F32))
        self.m, self.v, self.t = m.copy(), v.copy(), t0
        self.adam = lib.create_adam_cuda(*tl.args(), tl.n, tl.size, B1, B2)
        a = self.adam.contents
        assert a.on_device == 1 and a.size == tl.size and a.num_layers == tl.n and a.time_step == 0
        self.upload_moments()
        a.time_step = t0

    def _index(self):
        """device position in adam.m / adam.v of every packed element"""
        a = self.adam.contents
        if not a.flat:
            return np.arange(self.tl.size)
        base = self.tl.ploc[0][1]
        return np.concatenate([np.arange(ln) + (o - base) for (_, o), ln in zip(self.tl.ploc, self.tl.lengths)])

    def upload_moments(self):
        a = self.adam.contents
        idx = self._index()
        for dst, src in ((a.m, self.m), (a.v, self.v)):
            img = np.zeros(align4(a.span), F32)
            img[idx] = src
            ppo_ffi.h2d(self.lib, dst, img)

    def step(self, g, scale=None):
        a = self.adam.contents
        if scale is not None:
            a.grad_scale = scale
        self.tl.set_grads(g)
        self.lib.adam_update_cuda(self.adam, LR)
        g_eff = g if scale is None else g * F32(a.grad_scale)          # fl32(g · scale), one rounding
        assert g_eff.dtype == F32
        p = self.tl.params()
        self.t = self.oracle.adam_update(p, g_eff, self.m, self.v, self.t, LR)
        self.tl.set_params(p)

    def check(self, what):
        a = self.adam.contents
        self.tl.check(what)
        assert a.time_step == self.t, what
        idx = self._index()
        rest = np.ones(align4(a.span), bool)
        rest[idx] = False
        for name, ptr, want in (("m", a.m, self.m), ("v", a.v, self.v)):
            img = ppo_ffi.d2h(self.lib, ptr, F32, align4(a.span))
            assert_bits(img[idx], want, f"{what}: {name}")
            assert not img[rest].view(U32).any(), f"{what}: {name} outside the tensors is no longer 0"

    def free(self):
        self.lib.free_adam_cuda(self.adam)
        self.tl.free()


def drive(lib, oracle, lengths, layout, *, lead=0, regime="normal", state="warmed", t0=0, steps=3, scales=None,
          flat=None, seed=0, what=""):
    rng = np.random.default_rng([seed, sum(lengths), len(lengths)])
    tl = TensorList(lib, lengths, layout, lead=lead)
    run = AdamRun(lib, oracle, tl, *initial_state(oracle, rng, tl.size, state), t0=t0)
    try:
        if flat is not None:
            assert run.adam.contents.flat == flat, f"{what}: flat = {run.adam.contents.flat}"
        if flat == 1:
            assert run.adam.contents.span == tl.size
        for k in range(steps):
            g = (edge_grads if regime == "edge" else normal_grads)(rng, tl.size)
            run.step(g, None if scales is None else scales[k])
            run.check(f"{what} step {k + 1} (t = {run.t})")
        assert run.t == t0 + steps
    finally:
        run.free()


# ----------------------------------------------------------------------------- A. flat, vectorised
NA = [1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1027, 2098179]


@pytest.mark.parametrize("t0", [0, 9997])
@pytest.mark.parametrize("n", NA)
def test_flat_vec_normal(lib, oracle, n, t0):
    """One tensor at the start of a device allocation (16-B aligned: adam_flat_vec_kernel), every n & 3,
    either side of one workgroup, and 2 098 179 > 2048·256·4: the grid-stride loop wraps and leaves a
    3-element tail.  Steps 1–3 and 9 998–10 000 (bias corrections near 1)."""
    drive(lib, oracle, [n], "separate", t0=t0, flat=1, what=f"vec n={n}")


@pytest.mark.parametrize("t0", [0, 9997])
@pytest.mark.parametrize("state", STATES)
def test_flat_vec_edge(lib, oracle, state, t0):
    drive(lib, oracle, [1027], "separate", regime="edge", state=state, t0=t0, flat=1, what=f"vec edge {state}")


def test_flat_vec_grad_scale(lib, oracle):
    """grad_scale through the struct field: the oracle is fed fl32(g · scale)"""
    drive(lib, oracle, [1027], "separate", flat=1, scales=[0.25, 1.0 / 3.0, 1.0 / 3.0], what="vec grad_scale")


# ----------------------------------------------------------------------------- B. flat, scalar
@pytest.mark.parametrize("t0", [0, 9997])
@pytest.mark.parametrize("n", [1, 6, 1027, 530001])
def test_flat_scalar_unaligned(lib, oracle, n, t0):
    """p and g one float into their allocations: adam_flat_kernel; 530 001 > 2048·256 threads, so its
    stride loop runs.  The float before and the 8 after are untouched."""
    drive(lib, oracle, [n], "separate", lead=1, t0=t0, flat=1, what=f"scalar n={n}")


@pytest.mark.parametrize("state", STATES)
def test_flat_scalar_edge(lib, oracle, state):
    drive(lib, oracle, [1027], "separate", lead=1, regime="edge", state=state, flat=1, what=f"scalar edge {state}")


# ----------------------------------------------------------------------------- C. multi-tensor
LMIX = [3, 0, 64, 1, 1000]


def mixed_lengths(count):
    lengths = [LMIX[i % len(LMIX)] for i in range(count)]
    if count == 25:
        lengths[24] = 530000          # the second chunk alone exceeds the grid; its m / v start at `base`
    return lengths


@pytest.mark.parametrize("layout", ["separate", ("gaps", (4, 5, 9)), "offset"], ids=["separate", "gaps", "offset"])
@pytest.mark.parametrize("count", [1, 2, 24, 25, 49])
def test_multi_tensor(lib, oracle, count, layout):
    """Lists flat_span must reject → adam_multi_kernel: its search over start[], the chunks of 24
    tensors and the base offset into m / v.  Parameters against the oracle run on the concatenation,
    m / v packed in tensor order, sentinels between and after the tensors unchanged.  (A list of one
    tensor is one span whatever its allocation: flat, and the same results are asserted.)"""
    lengths = mixed_lengths(count) if count > 1 else [1000]
    drive(lib, oracle, lengths, layout, flat=0 if count > 1 else 1, what=f"multi {count} {layout}")


def test_multi_tensor_edge(lib, oracle):
    drive(lib, oracle, [3, 1000, 0, 24], ("gaps", (4,)), regime="edge", state="zero", flat=0, what="multi edge")


# ----------------------------------------------------------------------------- D. gaps of 1–3 floats
D_CASES = [([5, 64], (1,)), ([5, 64], (2,)), ([6, 64], (3,)), ([3, 1000, 1, 64, 7], (1, 2, 3))]


@pytest.mark.parametrize("lengths,gaps", D_CASES, ids=["2x-gap1", "2x-gap2", "2x-gap3", "5x-gaps123"])
def test_gapped_list_is_not_one_span(lib, oracle, lengths, gaps):
    """Tensors carved from one parameter and one gradient allocation with 1–3 floats between them, the
    gap floats nonzero in both: they are the caller's.  A span kernel would read the gradient gaps as
    gradients and write the parameter gaps; the list must take the multi-tensor path."""
    drive(lib, oracle, lengths, ("gaps", gaps), flat=0, what=f"gapped {lengths} {gaps}")


def test_abutting_list_is_one_span(lib, oracle):
    drive(lib, oracle, [8, 1000, 4, 64], ("gaps", (0,)), flat=1, what="abutting")
    drive(lib, oracle, [5, 1000, 3, 64], ("gaps", (0,)), flat=1, what="abutting, odd lengths")


@pytest.mark.parametrize("sizes", [[3, 64, 64, 1], [17, 256, 256, 6]])
def test_network_adam_keeps_padded_span(lib, sizes):
    """create_adam_from_nn_cuda owns the ≤ 3 floats of padding after each tensor: still one span"""
    acts = ["relu"] * (len(sizes) - 2) + ["none"]
    nn = lib.create_neural_network(ppo_ffi.c_ints(sizes), ppo_ffi.c_strings(acts), len(sizes))
    adam = lib.create_adam_from_nn_cuda(nn, B1, B2)
    off = size = 0
    for n_in, n_out in zip(sizes[:-1], sizes[1:]):
        last = off + align4(n_in * n_out) + n_out
        off += align4(n_in * n_out) + align4(n_out)
        size += n_in * n_out + n_out
    a = adam.contents
    got = (a.flat, a.span, a.size, a.num_layers)
    lib.free_adam_cuda(adam)
    lib.free_neural_network(nn)
    assert got == (1, last, size, 2 * (len(sizes) - 1))


# ----------------------------------------------------------------------------- E. host API, checkpoints
def test_host_pointer_update(lib, oracle):
    """create_adam / adam_update on host tensors (staged through HBM): two steps"""
    rng = np.random.default_rng(5)
    lengths = [5, 1000, 17]
    n = sum(lengths)
    ps = [rng.uniform(-1, 1, ln).astype(F32) for ln in lengths]
    gs = [np.zeros(ln, F32) for ln in lengths]
    wp = (C.c_void_p * 3)(*[p.ctypes.data for p in ps])
    gp = (C.c_void_p * 3)(*[g.ctypes.data for g in gs])
    adam = lib.create_adam(wp, gp, ppo_ffi.c_ints(lengths), 3, n, B1, B2)
    a = adam.contents
    assert a.on_device == 0
    p_ref, m_ref, v_ref, t = np.concatenate(ps), np.zeros(n, F32), np.zeros(n, F32), 0
    for k in range(2):
        g = normal_grads(rng, n)
        for dst, src in zip(gs, np.split(g, np.cumsum(lengths)[:-1])):
            dst[:] = src
        lib.adam_update(adam, LR)
        t = oracle.adam_update(p_ref, g, m_ref, v_ref, t, LR)
        assert_bits(np.concatenate(ps), p_ref, f"host p step {k + 1}")
        assert_bits(np.concatenate(gs), g, f"host g step {k + 1}")
        assert_bits(np.ctypeslib.as_array(a.m, shape=(n,)), m_ref, f"host m step {k + 1}")
        assert_bits(np.ctypeslib.as_array(a.v, shape=(n,)), v_ref, f"host v step {k + 1}")
    assert a.time_step == t == 2
    lib.free_adam(adam)


@pytest.mark.parametrize("lengths,layout,flat", [(mixed_lengths(25)[:24] + [4000], "separate", 0),
                                                 ([8, 1000, 3, 64], ("gaps", (0,)), 1),
                                                 ([3, 1000, 1, 64, 7], ("gaps", (1, 2, 3)), 0)],
                         ids=["non-flat", "abutting", "gapped"])
def test_checkpoint_round_trip(lib, oracle, tmp_path, lengths, layout, flat):
    """save_adam after two steps writes the reference layout (size, t, β1, β2, count, packed m, packed v);
    load_adam(cuda) and one further step is the third step of the uninterrupted (oracle) run."""
    rng = np.random.default_rng(9)
    tl = TensorList(lib, lengths, layout)
    run = AdamRun(lib, oracle, tl, *initial_state(oracle, rng, tl.size, "zero"))
    try:
        assert run.adam.contents.flat == flat
        for k in range(2):
            run.step(normal_grads(rng, tl.size))
        run.check("before save")
        path = str(tmp_path / "adam.bin").encode()
        f = LIBC.fopen(path, b"wb")
        assert f
        lib.save_adam(run.adam, f, True)
        LIBC.fclose(f)
        want = struct.pack("<2i2fi", tl.size, 2, B1, B2, tl.n) + run.m.astype("<f4").tobytes() + \
            run.v.astype("<f4").tobytes()
        with open(path, "rb") as fh:
            assert fh.read() == want
        lib.free_adam_cuda(run.adam)
        f = LIBC.fopen(path, b"rb")
        assert f
        run.adam = lib.load_adam(f, *tl.args(), True)
        LIBC.fclose(f)
        a = run.adam.contents
        assert (a.flat, a.time_step, a.size, a.num_layers, a.on_device) == (flat, 2, tl.size, tl.n, 1)
        run.check("after load")
        run.step(normal_grads(rng, tl.size))
        run.check("third step from the loaded Adam")
    finally:
        run.free()


# ----------------------------------------------------------------------------- F. inside ppo_update
K1 = F32(1) - F32(B1)                      # (1 − β) as fp32 arithmetic gives them
K2 = F32(1) - F32(B2)
SEED = 4321
ENVS = ("PPO_NO_TINY", "PPO_NO_CLUSTER", "PPO_GRAPH", "PPO_GRAPH_STEPS", "PPO_SERIAL")
PATHS = {
    # the multi-launch loop: value step adam_flat_vec_kernel, policy step the pair kernel (log σ beside μ)
    "multi": dict(sizes=[17, 64, 64, 6], N=1024, B=256, env={"PPO_NO_TINY": "1"}, dtype=0),
    # bf16 compute, fp32 master parameters (the Adam kernels also write the bf16 shadow)
    "bf16": dict(sizes=[17, 64, 64, 6], N=1024, B=256, env={"PPO_NO_TINY": "1"}, dtype=1),
    # graph replay of steps 1 … n−2 (adam_flat_tab_kernel)
    "graph": dict(sizes=[17, 256, 256, 6], N=1024, B=64,
                  env={"PPO_NO_CLUSTER": "1", "PPO_GRAPH": "1", "PPO_GRAPH_STEPS": "16"}, dtype=0),
    "eager64": dict(sizes=[17, 256, 256, 6], N=1024, B=64, env={"PPO_NO_CLUSTER": "1"}, dtype=0),
    # the single-workgroup phases (tiny.hip, calling ppo_math.h adam_elem)
    "tiny": dict(sizes=[3, 64, 64, 1], N=1024, B=64, env={}, dtype=0),
    # the multi-workgroup phases at B = 64 (cluster.hip, the same adam_elem)
    "cluster": dict(sizes=[17, 256, 256, 6], N=1024, B=64, env={}, dtype=0),
}


def adam_span(lib, adam_ptr):
    """p, g, m, v of a flat device Adam's tensors (the padding between them left out), and its step"""
    a = adam_ptr.contents
    assert a.flat and a.on_device
    base = addr(a.weights[0])
    idx = np.concatenate([np.arange(a.lengths[i]) + (addr(a.weights[i]) - base) // 4 for i in range(a.num_layers)])
    out = {k: ppo_ffi.d2h(lib, ptr, F32, a.span)[idx]
           for k, ptr in (("p", a.weights[0]), ("g", a.grad_weights[0]), ("m", a.m), ("v", a.v))}
    out["t"] = a.time_step
    return out


def ppo_run(lib, oracle, monkeypatch, path, limit):
    """A fresh PPO from fixed seeds on a synthetic rollout, the first `limit` value and policy steps of
    one update; the three Adams' state before and after."""
    cfg = PATHS[path]
    for k in ENVS:
        monkeypatch.delenv(k, raising=False)
    for k, val in cfg["env"].items():
        monkeypatch.setenv(k, val)
    sizes, N, B = cfg["sizes"], cfg["N"], cfg["B"]
    oracle.srand(1234)
    acts = ["relu"] * (len(sizes) - 2) + ["none"]
    ppo = lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), N, LR, LR, 0.95, 0.2, 0.01,
                         0.7, True)
    try:
        assert lib.ppo_set_compute_dtype(ppo, cfg["dtype"]) == 0
        lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 500)
        lib.ppo_synchronize()
        c = ppo.contents
        adams = (("V", c.adam_V), ("mu", c.adam_policy), ("ls", c.adam_entropy))
        out = {"before": {k: adam_span(lib, a) for k, a in adams}}
        lib.ppo_set_step_limit(ppo, limit, limit)
        lib.ppo_reset_stats(ppo)
        lib.ppo_update(ppo, 0.99, B, 1, 1, 1, SEED)
        lib.ppo_synchronize()
        assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
        st = (C.c_double * 9)()
        lib.ppo_read_stats(ppo, st, 9)
        out["after"] = {k: adam_span(lib, a) for k, a in adams}
        out["graph_steps"] = st[8]
        out["steps"] = (st[1], st[3])
        out["bits_m"] = (c.V.contents.bits_m, c.policy.contents.mu.contents.bits_m)
        out["dtype"] = (c.V.contents.dtype, c.policy.contents.mu.contents.dtype)
        lib.ppo_set_step_limit(ppo, -1, -1)
    finally:
        lib.free_ppo(ppo)
        for k in cfg["env"]:
            monkeypatch.delenv(k, raising=False)
    return out


def assert_path(r, path, limit):
    """the intended path ran (as the tiny / cluster / graph tests tell: bits_m and stats out[8])"""
    B = PATHS[path]["B"]
    multi = (B, B)
    assert r["steps"] == (limit, limit)
    if path in ("tiny", "cluster"):
        assert r["bits_m"][0] != B and r["bits_m"][1] != B, f"{path}: the multi-launch loop ran"
    else:
        assert r["bits_m"] == multi, f"{path}: bits_m {r['bits_m']}"
    assert r["graph_steps"] == (2 * (limit - 2) if path == "graph" else 0)
    assert r["dtype"] == (PATHS[path]["dtype"],) * 2
    for k in ("V", "mu", "ls"):
        assert r["before"][k]["t"] == 0 and r["after"][k]["t"] == limit


def assert_param_line(oracle, p_prev, now, what):
    """p == ref_adam_apply(p_prev, m, v, t): the parameter line given the kernel's own moments — no
    gradient enters, so none of the GEMM rounding does"""
    want = p_prev.copy()
    oracle.adam_apply(want, now["m"], now["v"], now["t"], LR)
    assert_bits(now["p"], want, f"{what}: parameters vs ref_adam_apply at t = {now['t']}")
    assert (now["p"].view(U32) != p_prev.view(U32)).mean() > 0.5, f"{what}: parameters did not move"


def assert_first_moments(now, what):
    """After the first step from zero moments m = fl((1−β1)·g) and v = fl((1−β2)·fl(g·g)) for ONE fp32 g.
    g is within 2 ulp of fl(m / (1−β1)) (two roundings, each ≤ 2⁻²⁴ relative): some candidate among
    those five floats must reproduce both m and v bitwise.  m = 0 exactly is checked like any other value
    (the candidate 0 must give v = +0): whole rows of a weight gradient are exact zeros where a ReLU unit
    is inactive over the minibatch (36 % of the 3 → 64 → 64 → 1 value network at B = 64, measured).  Only
    0 < |m| < 2⁻¹⁰⁰ is left out (at most 1 % of a tensor, asserted): there the quotient's ulp argument
    meets the subnormals."""
    m, v = now["m"], now["v"]
    use = (np.abs(m) >= F32(2.0 ** -100)) | (m == 0)
    left_out = 1.0 - use.mean()
    print(f"{what}: {m.size} elements, {100 * (m == 0).mean():.3f} % exact zeros, "
          f"{100 * left_out:.3f} % left out (0 < |m| < 2^-100)")
    assert left_out <= 0.01, f"{what}: {100 * left_out:.2f} % of the tensor has 0 < |m| < 2^-100"
    assert (m != 0).mean() > 0.5, f"{what}: most first moments are zero"
    m, v = m[use], v[use]
    c0 = m / K1
    assert c0.dtype == F32
    lo = np.nextafter(np.nextafter(c0, F32(-np.inf)), F32(-np.inf))
    ok = np.zeros(m.size, bool)
    c = lo
    for _ in range(5):
        ok |= ((K1 * c).view(U32) == m.view(U32)) & ((K2 * (c * c)).view(U32) == v.view(U32))
        c = np.nextafter(c, F32(np.inf))
    assert ok.all(), f"{what}: {int((~ok).sum())}/{ok.size} (m, v) pairs come from no single fp32 gradient"


def assert_moment_recurrence(prev, now, what):
    """m = fl(fl(β1·m′) + fl((1−β1)·g)), v = fl(fl(β2·v′) + fl((1−β2)·fl(g·g))) with g the gradient the
    last step of the run left in the buffer (the loop does not clear it after its last step)"""
    g = now["g"]
    assert np.abs(g).max() > 0
    assert_bits(now["m"], F32(B1) * prev["m"] + K1 * g, f"{what}: m at t = {now['t']}")
    assert_bits(now["v"], F32(B2) * prev["v"] + K2 * (g * g), f"{what}: v at t = {now['t']}")


@pytest.mark.parametrize("path", ["multi", "bf16", "tiny", "cluster"])
def test_update_first_step(lib, oracle, monkeypatch, path):
    """One value and one policy step (ppo_set_step_limit(1, 1)) from fresh Adam state on each path that
    carries its own copy or form of the arithmetic; V, μ and log σ."""
    r = ppo_run(lib, oracle, monkeypatch, path, 1)
    assert_path(r, path, 1)
    for k in ("V", "mu", "ls"):
        assert not r["before"][k]["m"].any() and not r["before"][k]["v"].any()
        assert_param_line(oracle, r["before"][k]["p"], r["after"][k], f"{path} {k}")
        assert_first_moments(r["after"][k], f"{path} {k}")


@pytest.fixture
def deterministic_gemms(lib):
    lib.ppo_gemm_tune(-1, 1)               # split-K target 1: gradient sums without atomics
    yield
    lib.ppo_gemm_tune(-1, 0)


def same_state(a, b):
    return all(a[k].view(U32).tobytes() == b[k].view(U32).tobytes() for k in ("p", "m", "v"))


@pytest.mark.parametrize("path,nets", [("multi", ("V",)), ("tiny", ("V", "mu", "ls")), ("cluster", ("V", "mu", "ls"))],
                         ids=["multi", "tiny", "cluster"])
def test_update_third_step(lib, oracle, monkeypatch, deterministic_gemms, path, nets):
    """The parameter line and the moments at t = 3 (warm moments, a later step's bias corrections) under
    deterministic GEMMs: two runs capped at two steps are bit-identical (asserted first), so the run
    capped at three went through their state, and its last step left its gradient in the buffer:
    p₃ = ref_adam_apply(p₂, m₃, v₃) and m₃, v₃ are the fp32 recurrences from (m₂, v₂, g₃), bitwise.
    The single-workgroup and cluster phases reproduce their own capped runs bit for bit (V, μ and log σ;
    measured on the MI355X) and write their last gradients back, so they are included.  In the
    multi-launch loop only the value network is: at B = 256 its policy step sums the log σ gradient with
    fp32 atomics across workgroups, two runs capped at two differed in log σ (measured), and μ's later
    gradients depend on log σ — the policy there stays at step 1 (test_update_first_step)."""
    a = ppo_run(lib, oracle, monkeypatch, path, 2)
    b = ppo_run(lib, oracle, monkeypatch, path, 2)
    assert_path(a, path, 2)
    c = ppo_run(lib, oracle, monkeypatch, path, 3)
    assert_path(c, path, 3)
    for k in nets:
        assert same_state(a["after"][k], b["after"][k]), f"{path} {k}: two runs capped at two steps differ"
        assert_param_line(oracle, a["after"][k]["p"], c["after"][k], f"{path} {k}")
        assert_moment_recurrence(a["after"][k], c["after"][k], f"{path} {k}")


def test_update_graph_replay(lib, oracle, monkeypatch):
    """Graph replay (adam_flat_tab_kernel: step size and bias correction from the device step table).
    A phase replays steps 1 … n−2, so the smallest run with a replayed step is capped at three: step 0
    eager, step 1 replayed, step 2 eager.  Replay needs the fused heads, which the deterministic-GEMM
    switch turns off, so the GEMMs are as tuned; at B = 64 the value network is reproducible all the same
    (one workgroup per sum; asserted: two eager runs capped at two are bit-identical, as
    test_graph_replay_matches_eager finds over whole updates).  The state after the replayed step must be
    the eager run's capped at two, and the third step continue from exactly that:
    p₃ = ref_adam_apply(p₂, m₃, v₃) and the moment recurrences from (m₂, v₂) with the last step's
    gradient, all bitwise.  The policy is checked for its step counts only: its replayed step cannot be
    separated from the eager third without a reproducible log σ gradient; its table kernel is the value
    network's, reading the table's other column."""
    e1 = ppo_run(lib, oracle, monkeypatch, "eager64", 1)
    e2 = ppo_run(lib, oracle, monkeypatch, "eager64", 2)
    e2b = ppo_run(lib, oracle, monkeypatch, "eager64", 2)
    assert_path(e2, "eager64", 2)
    assert same_state(e2["after"]["V"], e2b["after"]["V"]), "two eager runs capped at two steps differ"
    assert_param_line(oracle, e1["after"]["V"]["p"], e2["after"]["V"], "eager B=64 V")
    assert_moment_recurrence(e1["after"]["V"], e2["after"]["V"], "eager B=64 V")
    g3 = ppo_run(lib, oracle, monkeypatch, "graph", 3)
    assert_path(g3, "graph", 3)
    assert_param_line(oracle, e2["after"]["V"]["p"], g3["after"]["V"], "graph V")
    assert_moment_recurrence(e2["after"]["V"], g3["after"]["V"], "graph V")
