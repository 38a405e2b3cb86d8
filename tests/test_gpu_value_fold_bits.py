"""The value-head fold without its fp32 activation (DESIGN.md §4 "value-head fold"; csrc/gemm_x3.hip FOLD 2,
fold_finish_kernel; host/neural_network.c nn_value_fold_step): the fold forward writes the last hidden layer's
ReLU′ mask words and partial dots but no activation, the fold grad_W stages its mask operand from those words and
leaves P = maskᵀ·diag(g)·x and q = maskᵀ·g unscaled, and the finishing launch forms the output layer's gradient
gW_out(c) = ⟨W(c,:), P(c,:)⟩ + b(c)·q(c) (= Σ_rows g·h(·,c), h never read) and scales P, q by the output weights.

Shapes: the smallest at which these kernels can still go wrong — hidden widths 96 and 160 (no multiple of the
128-unit tile, 3 and 5 mask words per row, the tile's last word group absent), input width 40, batch rows 257 and
1000 (ragged against the 16-row k-tile and the 128-row tiles).  The engine gives a split at least 8 k-tiles per
k-group (256 rows), so 257 rows run as ONE split (plain stores) and 1000 rows as 3 splits in the slab form (both
deterministic: the two stagings must agree bit for bit there); 2100 rows at a split target of 2 take the
f32-atomic form of split-K that C4 runs.  The whole value step needs more than 1024 rows for the x3 engine (and so
for the fold) to take it: 1100 rows, ragged against every tile, are the smallest used there.  ppo_update keeps the
store of the activation on the last step of its value loop, so a capped one-step update would run the storing
forward: the whole-step case turns that off (ppo_value_fold_keep_h) and checks that the block was not written.

The GAE's value forwards are not covered here: they run the plain forward and the output layer's own kernel, not
the fold's partial dots, and stay as they were.
"""
import ctypes as C

import numpy as np
import pytest

import ppo_ffi
from helpers import F32, assert_gemm_close, dev, empty, gemm_tol, nn_grads_packed, nn_params_packed

pytestmark = pytest.mark.gpu

LIBC = C.CDLL("libc.so.6")
N_IN = 40
WIDTHS = (96, 160)
# rows: (m, split-K workgroup target; 0 = automatic), the form of split-K it takes
ROWS = {"one_split": (257, 0), "slab": (1000, 0), "atomics": (2100, 2)}


def layer_inputs(m, l, seed, bias=None):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (m, N_IN)).astype(F32)
    W = rng.uniform(-0.3, 0.3, (l, N_IN)).astype(F32)
    b = rng.uniform(-0.2, 0.2, l).astype(F32) if bias is None else bias
    w = rng.uniform(-0.5, 0.5, l).astype(F32)
    g = rng.uniform(-1, 1, m).astype(F32)
    return x, W, b, w, g


def unpack_bits(words, l):
    c = np.arange(l)
    return ((words[:, c // 32] >> (c % 32).astype(np.uint32)) & 1).astype(bool)


class Layer:
    """One folded layer on the device: the storing forward's h, bits and ypart, and both grad_W forms."""

    def __init__(self, lib, x, W, b, w, g, target=0):
        self.lib, self.m, self.l, self.n = lib, x.shape[0], W.shape[0], x.shape[1]
        self.target = target
        self.wpr = (self.l + 31) // 32
        self.d = {k: dev(lib, v) for k, v in dict(x=x, W=W, b=b, w=w, g=g, ones=np.ones(self.l, F32)).items()}
        self.slots_max = 2 * ((self.l + 63) // 64)
        self.arrays = list(self.d.values())

    def buf(self, count, fill=None, dtype=F32):
        a = dev(self.lib, np.full(count, fill, dtype)) if fill is not None else empty(self.lib, count, dtype)
        self.arrays.append(a)
        return a

    def forward(self, nostore):
        m, l = self.m, self.l
        h = self.buf(m * l, fill=np.float32(-7.0))
        bits = self.buf(m * self.wpr, fill=np.uint32(0xA5A5A5A5), dtype=np.uint32)
        yp = self.buf(self.slots_max * m, fill=np.float32(0.0))
        d = self.d
        slots = self.lib.ppo_x3_fold_forward(h.ptr, d["x"].ptr, d["W"].ptr, d["b"].ptr, m, self.n, l, bits.ptr, d["w"].ptr,
                                             yp.ptr, int(nostore))
        assert 0 < slots <= self.slots_max
        return h, bits, yp, slots

    def grad_w(self, h=None, bits=None, w="ones"):
        """(gW, gb, gw_out) of one form: the fp32 form with w = 1 leaves P and q themselves."""
        l, n, d = self.l, self.n, self.d
        gW, gb, gwo = self.buf(l * n, fill=np.float32(3.0)), self.buf(l, fill=np.float32(3.0)), self.buf(l)
        self.lib.ppo_gemm_x3_tune(-1, self.target)
        try:
            rc = self.lib.ppo_x3_fold_grad_w(gW.ptr, gb.ptr, h.ptr if h else None, bits.ptr if bits else None, d["g"].ptr,
                                             d[w].ptr, gwo.ptr, d["x"].ptr, self.m, n, l)
        finally:
            self.lib.ppo_gemm_x3_tune(-1, 0)
        assert rc == 0
        return gW, gb, gwo

    def finish(self, gW, gb):
        d = self.d
        gwo = self.buf(self.l, fill=np.float32(9.0))
        self.lib.ppo_x3_fold_finish(gW.ptr, gb.ptr, d["W"].ptr, d["b"].ptr, d["w"].ptr, gwo.ptr, self.n, self.l)
        return gwo

    def free(self):
        self.lib.ppo_synchronize()
        assert self.lib.ppo_last_error() in (b"", None), self.lib.ppo_last_error()
        for a in self.arrays:
            a.free()


def model64(x, W, b, w, g, mask):
    """float64 model of the layer's fold gradients given the GPU's own mask."""
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    P = (mask * g64[:, None]).T @ x64                             # [l, n]
    q = (mask * g64[:, None]).sum(axis=0)                         # [l]
    z = x64 @ W.astype(np.float64).T + b.astype(np.float64)
    gw_out = ((mask * z) * g64[:, None]).sum(axis=0)              # Σ_rows g·h
    return P, q, gw_out


@pytest.mark.parametrize("rows", sorted(ROWS))
@pytest.mark.parametrize("l", WIDTHS)
def test_fold_grad_w_from_bits_matches_fp32_h(lib, l, rows):
    """Case 1: the same g and x through the fp32-h staging (the retained storing forward) and the mask-word
    staging (the no-store forward): P, q element by element, both against a float64 model; bit for bit where
    split-K is deterministic; then the finishing launch's three outputs against the model and the fp32 form."""
    m, target = ROWS[rows]
    x, W, b, w, g = layer_inputs(m, l, 100 + l + m)
    L = Layer(lib, x, W, b, w, g, target)
    h_d, bits_d, yp_d, slots = L.forward(nostore=False)
    h2_d, bits2_d, yp2_d, slots2 = L.forward(nostore=True)
    h = h_d.to_numpy(F32, m * l).reshape(m, l)
    words = bits_d.to_numpy(np.uint32, m * L.wpr).reshape(m, L.wpr)
    # the no-store forward: the activation untouched, the same words and partial dots
    np.testing.assert_array_equal(h2_d.to_numpy(F32, m * l), np.full(m * l, -7.0, F32))
    np.testing.assert_array_equal(bits2_d.to_numpy(np.uint32, m * L.wpr).reshape(m, L.wpr), words)
    assert slots2 == slots
    np.testing.assert_array_equal(yp2_d.to_numpy(F32, slots * m), yp_d.to_numpy(F32, slots * m))
    mask = unpack_bits(words, l)
    np.testing.assert_array_equal(mask, h > 0)
    assert 0.2 < mask.mean() < 0.8

    P64, q64, gwo64 = model64(x, W, b, w, g, mask)
    Pa_d, qa_d, gwa_d = L.grad_w(h=h_d)                        # fp32 h, w = 1: P, q and Σ g·h
    Pb_d, qb_d, _ = L.grad_w(bits=bits2_d)                     # the mask words of the no-store forward
    Pa, qa = Pa_d.to_numpy(F32, l * N_IN).reshape(l, N_IN), qa_d.to_numpy(F32, l)
    Pb, qb = Pb_d.to_numpy(F32, l * N_IN).reshape(l, N_IN), qb_d.to_numpy(F32, l)
    gw_old = gwa_d.to_numpy(F32, l)
    for got, what in ((Pa, "fp32 h"), (Pb, "mask words")):
        assert_gemm_close(got, P64, m, f"P from {what} vs float64 ({rows}, l={l})")
    for got, what in ((qa, "fp32 h"), (qb, "mask words")):
        assert_gemm_close(got, q64, m, f"q from {what} vs float64 ({rows}, l={l})")
    assert_gemm_close(Pb, Pa, m, "P: mask words vs fp32 h")
    assert_gemm_close(qb, qa, m, "q: mask words vs fp32 h")
    if rows != "atomics":            # one split, or slabs summed in a fixed order: the same products, the same bits
        np.testing.assert_array_equal(Pb, Pa)
    if rows == "one_split":
        np.testing.assert_array_equal(qb, qa)

    gwo_d = L.finish(Pb_d, qb_d)
    gW, gb, gwo = Pb_d.to_numpy(F32, l * N_IN).reshape(l, N_IN), qb_d.to_numpy(F32, l), gwo_d.to_numpy(F32, l)
    np.testing.assert_array_equal(gW, w[:, None] * Pb)          # one fp32 product per element
    np.testing.assert_array_equal(gb, w * qb)
    e_new, e_old = np.abs(gwo - gwo64).max(), np.abs(gw_old - gwo64).max()
    print(f"{rows} l={l} m={m}: gW_out max err vs float64: from P, q {e_new:.3g}, from fp32 h {e_old:.3g}, "
          f"bound {gemm_tol(gwo64, m):.3g} (max |gW_out| {np.abs(gwo64).max():.3g})")
    assert_gemm_close(gwo, gwo64, m, f"gW_out from P and q vs float64 ({rows}, l={l})")
    assert_gemm_close(gw_old, gwo64, m, f"gW_out from fp32 h vs float64 ({rows}, l={l})")
    L.free()


def mask_case(kind, m, l, seed):
    """(x, W, b, want): a layer whose mask is known exactly, every |z| ≥ 0.09 away from 0.
    single: unit u(k) = (7k + 3) mod l reads input k alone (W(u(k), k) = 1, 7 and l coprime: 40 distinct units
    spread over every mask word) with bias −0.5; every other unit has W = 0 and bias −10 and never fires.  Row i
    holds a value in [1, 2] at input i mod 40 and values ≤ 0.41 elsewhere, so exactly one unit of the row is
    positive, u(i mod 40): the bias places it, and the column varies with the row."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (m, N_IN))
    if kind == "single":
        x = np.minimum(x, 0.4)
        x[np.arange(m), np.arange(m) % N_IN] = rng.uniform(1.0, 2.0, m)
        units = (7 * np.arange(N_IN) + 3) % l
        assert np.unique(units).size == N_IN
        W = np.zeros((l, N_IN), F32)
        W[units, np.arange(N_IN)] = 1.0
        b = np.full(l, -10.0, F32)
        b[units] = -0.5
        want = np.zeros((m, l), bool)
        want[np.arange(m), units[np.arange(m) % N_IN]] = True
    else:
        W = rng.uniform(-0.3, 0.3, (l, N_IN)).astype(F32)
        b = np.full(l, 13.0 if kind == "all" else -13.0, F32)      # |x·Wᵀ| ≤ 40·0.3·1 = 12: the bias decides
        want = np.full((m, l), kind == "all")
    xq = (np.round(x * 64) / 64).astype(F32)      # 6 fraction bits
    return xq, W, b, want


@pytest.mark.parametrize("kind", ["single", "all", "none"])
@pytest.mark.parametrize("l", WIDTHS)
def test_mask_layout(lib, l, kind):
    """Case 2: masks whose product is known exactly — one positive unit per row at a varying column (placed by
    the bias), every unit, no unit.  With g ∈ {±2^-k} and x on a coarse binary grid every product and sum of
    P = maskᵀ·diag(g)·x is exact in fp32, so P must equal the sum of the rows of diag(g)·x it selects bit for
    bit (1000 rows: three splits in the slab form, ragged against the k-tile)."""
    m = 1000
    xq, W, b, want = mask_case(kind, m, l, 7 + l)
    rng = np.random.default_rng(3)
    # g·x is a multiple of 2^-9 below 2 in size: any sum of 1000 of them, in any order, is exact in fp32
    g = (rng.choice([-1.0, 1.0], m) * 2.0 ** -rng.integers(0, 4, m).astype(np.float64)).astype(F32)
    w = rng.uniform(-0.5, 0.5, l).astype(F32)
    L = Layer(lib, xq, W, b, w, g)
    z = xq.astype(np.float64) @ W.astype(np.float64).T + b
    np.testing.assert_array_equal(z > 0, want)               # the construction itself (margins ≥ 0.1: no rounding doubt)
    _, bits_d, _, _ = L.forward(nostore=True)
    mask = unpack_bits(bits_d.to_numpy(np.uint32, m * L.wpr).reshape(m, L.wpr), l)
    np.testing.assert_array_equal(mask, want)
    P_d, q_d, _ = L.grad_w(bits=bits_d)
    P, q = P_d.to_numpy(F32, l * N_IN).reshape(l, N_IN), q_d.to_numpy(F32, l)
    gx = g[:, None].astype(np.float64) * xq
    P_want = np.stack([gx[want[:, c]].sum(axis=0) for c in range(l)])
    q_want = np.array([g[want[:, c]].astype(np.float64).sum() for c in range(l)])
    np.testing.assert_array_equal(P, P_want.astype(F32))
    np.testing.assert_array_equal(q, q_want.astype(F32))
    assert (P_want.astype(F32) == P_want).all() and (q_want.astype(F32) == q_want).all()     # exact in fp32
    if kind == "none":
        assert not P.any() and not q.any()
    if kind == "single":
        assert (want.sum(axis=1) == 1).all() and np.unique(np.argmax(want, axis=1)).size == N_IN
    L.free()


STEP_FEATURES = {
    "plain": dict(),
    "value_clip": dict(vclip=0.2),
    "grad_clip": dict(max_norm=0.5),
}


def value_step(lib, sizes, N, B, fold, monkeypatch, vclip=0.0, max_norm=0.0, keep_h=1, steps=1, seed=31):
    """One capped update (steps value minibatch steps, no policy step) from the seeded state.  keep_h = 0
    (ppo_value_fold_keep_h): the capped loop's last step does not store the last hidden activation either — the
    one step then runs the form that every step but the last of a full update runs."""
    monkeypatch.setenv("PPO_VALUE_FOLD", "1" if fold else "0")
    monkeypatch.setenv("PPO_NO_TINY", "1")
    LIBC.srand(seed)
    acts = ["relu"] * (len(sizes) - 2) + ["none"]
    ppo = lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), N, 3e-4, 3e-4, 0.95, 0.2, 0.0,
                         1.0, True)
    lib.ppo_fill_synthetic(ppo, 8, N // 8, 5, 1.0 / 200)
    if vclip > 0:
        assert lib.ppo_set_value_clip(ppo, vclip) == 0
    if max_norm > 0:
        assert lib.ppo_set_max_grad_norm(ppo, max_norm) == 0
    assert lib.ppo_value_fold_keep_h(ppo, keep_h) == 1 and lib.ppo_value_fold_keep_h(ppo, -1) == keep_h
    lib.ppo_set_step_limit(ppo, steps, 0)
    lib.ppo_reset_stats(ppo)
    v0 = nn_params_packed(lib, ppo.contents.V)
    lib.ppo_prof_enable(1)
    lib.ppo_prof_reset()
    lib.ppo_update(ppo, 0.99, B, 0, 1, 1, 11)
    lib.ppo_synchronize()
    counts = (C.c_long * 7)()
    lib.ppo_prof_counts(counts)
    lib.ppo_prof_enable(0)
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
    st = (C.c_double * 4)()
    lib.ppo_read_stats(ppo, st, 4)
    V = ppo.contents.V.contents
    L = V.num_layers - 1
    out = dict(g=nn_grads_packed(lib, ppo.contents.V), v=nn_params_packed(lib, ppo.contents.V), v0=v0,
               y=ppo_ffi.d2h(lib, V.d_output, F32, B), loss=st[0], steps=st[1], launches=list(counts),
               h=ppo_ffi.d2h(lib, V.layers[L - 1].d_input, F32, B * sizes[-2]),     # the last hidden activation block
               h_prev=ppo_ffi.d2h(lib, V.layers[L - 2].d_input, F32, B * sizes[-3]))
    lib.ppo_set_step_limit(ppo, -1, -1)
    lib.free_ppo(ppo)
    return out


def assert_block_untouched(got, left, B):
    """The block equals what the GAE left, bit for bit.  The GAE's last forward covers the few rows whose next
    state is not the next row (episode ends), compacted to the block's first rows in an order its atomic counter
    decides per run: those leading rows must be the same rows in some order, every other row the same row."""
    got, left = got.reshape(B, -1), left.reshape(B, -1)
    bad = np.flatnonzero((got != left).any(axis=1))
    lead = int(bad[-1]) + 1 if bad.size else 0
    assert lead <= B // 20, f"{bad.size} rows of the block differ, up to row {lead - 1}: the step wrote it"
    key = lambda r: sorted(x.tobytes() for x in r[:lead])
    assert key(got) == key(left), "the block's leading rows are not the GAE's own-row forward"


@pytest.fixture(scope="module")
def gae_only(lib):
    """The activation blocks as the update's GAE forwards leave them, before any value step (step limit 0, 0), per
    hidden pair: the forwards have no atomics, so from the same seeded state they repeat bit for bit."""
    cache = {}

    def get(hidden, monkeypatch):
        if hidden not in cache:
            cache[hidden] = value_step(lib, [N_IN, hidden[0], hidden[1], 6], 2200, 1100, True, monkeypatch, steps=0)
        return cache[hidden]
    return get


@pytest.mark.parametrize("feature", sorted(STEP_FEATURES))
@pytest.mark.parametrize("hidden", [(96, 160), (160, 96)])
def test_whole_value_step(lib, hidden, feature, monkeypatch, gae_only):
    """Case 3: one whole value minibatch step through the NO-STORE forward (ppo_value_fold_keep_h(0): the form of
    every step of a full update but its last), the mask-word grad_W and the finishing launch, against the fused
    output-head pass from identical state (PPO_VALUE_FOLD=0: the comparison and the bounds of
    test_gpu_value_fold.py), plain, with value-loss clipping and with gradient clipping.  The last hidden
    activation block must be untouched by the step — bit for bit what the update's GAE forwards left in it — while
    the block below it holds the minibatch's rows; with the store kept (the default) the block is the minibatch's.
    The fold is taken under each feature, never a fallback: its launches differ from the out_head step's and
    include the finishing launch (class PPO_K_HEAD)."""
    sizes = [N_IN, hidden[0], hidden[1], 6]
    N, B = 2200, 1100
    kw = STEP_FEATURES[feature]
    a = value_step(lib, sizes, N, B, True, monkeypatch, keep_h=0, **kw)
    b = value_step(lib, sizes, N, B, False, monkeypatch, **kw)
    gae = gae_only(hidden, monkeypatch)
    assert a["steps"] == b["steps"] == 1 and gae["steps"] == 0
    np.testing.assert_array_equal(a["v0"], b["v0"])
    np.testing.assert_array_equal(a["v0"], gae["v0"])
    # no store: the block is the GAE's; the layer below was written by the step (and differs from the GAE's rows)
    assert_block_untouched(a["h"], gae["h"], B)
    assert (a["h_prev"] != gae["h_prev"]).mean() > 0.1
    if feature == "plain":
        c = value_step(lib, sizes, N, B, True, monkeypatch, keep_h=1, **kw)      # the default: the last step stores
        assert (c["h"] != gae["h"]).mean() > 0.1
        np.testing.assert_array_equal(c["h_prev"], a["h_prev"])
        np.testing.assert_array_equal(c["y"], a["y"])            # y comes from the partial dots, store or not
    print(f"{hidden} {feature}: launches per class, fold {a['launches']}, out_head {b['launches']}")
    assert a["launches"] != b["launches"], "PPO_VALUE_FOLD=1 did not change the step's launches: the fold was not taken"
    assert a["launches"][4] >= 1, "no launch of class PPO_K_HEAD: the finishing launch did not run"
    assert_gemm_close(a["y"], b["y"], sizes[-2], f"{feature}: value output y (fold vs out_head)")
    assert_gemm_close(a["g"], b["g"], B, f"{feature}: value gradients (fold vs out_head)")
    np.testing.assert_allclose(a["loss"], b["loss"], rtol=1e-5)
    err = np.abs(a["v"] - b["v"])
    assert err.max() <= 2 * 3e-4 * 1.0001, err.max()
    assert (err > 1e-6).mean() < 0.01, (err > 1e-6).mean()
    print(f"{hidden} {feature}: fold vs out_head max |Δgrad| {np.abs(a['g'] - b['g']).max():.3g} "
          f"(max |grad| {np.abs(b['g']).max():.3g}), max |Δy| {np.abs(a['y'] - b['y']).max():.3g}")
