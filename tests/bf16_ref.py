"""bf16 compute mode (csrc/gemm16.hip): the rounding model, the per-kernel checker and the inputs of the
kernel tests, in one place.  Pinned on the CPU in test_bf16_ref_cpu.py; used on the GPU by test_gpu_bf16.py,
test_gpu_bf16_kernels.py and test_gpu_production.py.

* bf16 / unpack / emulate / emu_forward / emu_backward: what the kernels round (layer inputs and the weight
  shadow on the way into the MFMA, hidden activations and hidden gradients in storage), end to end, float64 sums.
* check_bf16_readback: every launch of one forward + backward checked on its own from the operands the GPU
  itself stored (teacher forcing), so a rounding flip upstream never enters a comparison.  The bounds:
    forward, bf16 out   |h − want| ≤ 2^-8·|want| + 2^-15·Σ|terms|      (half a bf16 ulp + the fp32 sum)
    forward, fp32 out   |y − want| ≤ 2^-15·Σ|terms| + 2^-23·|want|     and ≤ 1e-5·max|want| (the older bar)
    ReLU′ bits          word block == pack(stored h > 0) bit for bit, pad bits of the last word zero
    grad_W, bias grad   |gW − want| ≤ 2^-15·Σ|g·h| + 1e-9,  |gb − want| ≤ 2^-15·Σ|g| + 1e-9
    grad_x, bf16 out    the forward's bf16 bound on where(stored h > 0, g·bf16(W), 0)
    grad_x, fp32 out    (layer 0, unmasked) the forward's fp32 bound
  Σ|terms| is the same product on absolute values (|h|·|bf16(W)|ᵀ + |b|, |g|ᵀ·|h|, |g|·|bf16(W)|).  2^-15 is
  ≈ 256 chained fp32 additions of unit roundoff 2^-24 — the kernels' chains (k-tiles, split-K partials, atomics)
  are shorter; 2^-8 is half a bf16 ulp relative, 2^-23 one fp32 rounding of the sum plus one of the bias add.
  Every check prints its worst err / bound per product and returns it.
* check_bf16_layers: reads those operands back from a bf16-mode NeuralNetwork and runs the checker.
* gemm_f32_model / model_run: a numpy fp32 model of the kernels' accumulation (fp32 partial sums per BK-wide
  k-tile, chained; split-K partials added in fp32; stored outputs rounded to bf16) with one injectable defect —
  what test_bf16_ref_cpu.py uses to show that the bounds admit a valid fp32 evaluation and reject each defect.
* NETWORKS / BATCHES / make_case: the shapes and inputs of the kernel tests (why each: test_gpu_bf16_kernels.py).
"""
import ctypes as C

import numpy as np

F32 = np.float32
F64 = np.float64
ULP = 2.0 ** -8          # bf16 round-to-nearest: relative error ≤ 2^-8 (8 significant bits)
ACC = 2.0 ** -15         # fp32 accumulation: ≈ 256 chained additions of unit roundoff 2^-24


def bf16(a):
    """round-to-nearest-even to bf16, returned as float32 (NaN-free inputs)"""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F32)


def bf16_trunc(a):
    """fp32 → bf16 by dropping the low 16 bits (what a kernel must NOT do), as float32"""
    return (np.ascontiguousarray(a, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def num_params(sizes):
    return sum(a * b + b for a, b in zip(sizes[:-1], sizes[1:]))


def unpack(sizes, params):
    out, off = [], 0
    for i in range(len(sizes) - 1):
        nw = sizes[i] * sizes[i + 1]
        W = params[off:off + nw].reshape(sizes[i + 1], sizes[i])
        off += nw
        b = params[off:off + sizes[i + 1]]
        off += sizes[i + 1]
        out.append((W, b))
    return out


def emu_forward(sizes, params, x):
    """bf16-mode forward as the kernels compute it, end to end (float64 accumulation)."""
    layers = unpack(sizes, params)
    hs = [bf16(x)]                                      # layer inputs as the MFMA sees them
    for i, (W, b) in enumerate(layers):
        z = hs[-1].astype(np.float64) @ bf16(W).astype(np.float64).T + b
        if i < len(layers) - 1:
            hs.append(bf16(np.maximum(z, 0.0).astype(F32)))
        else:
            y = z.astype(F32)
    return hs, y


def emu_backward(sizes, params, hs, gout):
    layers = unpack(sizes, params)
    grads = [None] * len(layers)
    g = gout.astype(F32)                                # fp32 from the heads, rounded in the loader
    for i in range(len(layers) - 1, -1, -1):
        W, _ = layers[i]
        gb16 = bf16(g).astype(np.float64)
        grads[i] = ((gb16.T @ hs[i].astype(np.float64)).astype(F32).ravel(), gb16.sum(axis=0).astype(F32))
        if i > 0:
            gx = np.where(hs[i] > 0, gb16 @ bf16(W).astype(np.float64), 0.0)
            g = bf16(gx.astype(F32))                    # hidden gradients stored bf16
    return np.concatenate([np.concatenate([gw, gb]) for gw, gb in grads])


def emulate(sizes, params, x, gout):
    """bf16-mode forward + backward as the kernels compute it (float64 accumulation)."""
    hs, y = emu_forward(sizes, params, x)
    return y, emu_backward(sizes, params, hs, gout)


# ----------------------------------------------------------------------------- the checker
def _finite(a, what):
    assert np.isfinite(a).all(), f"{what}: {int((~np.isfinite(a)).sum())} NaN/Inf elements"


def assert_bf16_rounding(got, want, sum_abs, what):
    """got (bf16 storage) is the bf16 rounding of an fp32 accumulation of want (float64): within half
    a bf16 ulp of want, plus the fp32 accumulation bound 2^-15·Σ|terms| (sum_abs).  Returns the worst
    err / bound."""
    _finite(got, what)
    tol = ULP * np.abs(want) + ACC * sum_abs + 1e-12
    err = np.abs(got - want)
    ratio = float((err / tol).max(initial=0.0))
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off by more than a bf16 rounding, worst " \
                          f"{float(err[bad].max()):.3g} (err / bound {ratio:.3g})"
    return ratio


def assert_f32_sum(got, want, sum_abs, what):
    """got (fp32 storage) is an fp32 accumulation of want (float64): 2^-15·Σ|terms| + 2^-23·|want|."""
    _finite(got, what)
    tol = ACC * sum_abs + 2.0 ** -23 * np.abs(want) + 1e-30
    err = np.abs(got - want)
    ratio = float((err / tol).max(initial=0.0))
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond the fp32 summation bound, worst " \
                          f"{float(err[bad].max()):.3g} (err / bound {ratio:.3g})"
    return ratio


def pack_bits(mask):
    """[m, n] bool → [m, ⌈n/32⌉] uint32, bit c % 32 of word c / 32 (NeuralNetwork.d_act_bits), pad bits zero"""
    m, n = mask.shape
    wpr = (n + 31) // 32
    padded = np.zeros((m, wpr * 32), bool)
    padded[:, :n] = mask
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").astype(np.uint32)


def unpack_bits(words, n):
    cols = np.arange(n)
    return ((words[:, cols // 32] >> (cols % 32).astype(np.uint32)) & 1).astype(bool)


def check_bf16_readback(sizes, params, x, gtop, top_rounded, rb, what):
    """The per-kernel check (module docstring) of one forward + backward over x's rows.  rb holds what the
    kernels stored: h[i] / gx[i] (i = 1 … L−1: stored bf16 hidden activations / gradients, as float32),
    bits[i] (i = 1 … L−1: uint32 [m, ⌈w/32⌉], or bits = None where there is nothing to read), y (fp32
    [m, out]), grads (packed fp32), gx[0] (fp32 layer-0 grad_x, or None where it was not asked for).
    gtop: the gradient at the network output; top_rounded: it enters its products rounded to bf16.
    Returns the worst err / bound per product."""
    L, m = len(sizes) - 1, x.shape[0]
    layers = unpack(sizes, params)
    hs = [bf16(x)] + [np.asarray(rb["h"][i], F32) for i in range(1, L)]
    worst = dict(fwd_bf16=0.0, fwd_f32=0.0, grad_W=0.0, bias=0.0, grad_x=0.0, grad_x0=0.0)

    def up(key, ratio):
        worst[key] = max(worst[key], ratio)

    for i in range(L - 1):                                  # hidden layers: bf16(relu(x·Wᵀ + b))
        W, b = layers[i]
        assert hs[i + 1].shape == (m, sizes[i + 1])
        z = hs[i].astype(F64) @ bf16(W).astype(F64).T + b
        sa = np.abs(hs[i]).astype(F64) @ np.abs(bf16(W)).astype(F64).T + np.abs(b)
        up("fwd_bf16", assert_bf16_rounding(hs[i + 1], np.maximum(z, 0.0), sa, f"{what} forward layer {i}"))
    W, b = layers[L - 1]
    y = np.asarray(rb["y"], F32).reshape(m, sizes[L])
    z = hs[L - 1].astype(F64) @ bf16(W).astype(F64).T + b
    sa = np.abs(hs[L - 1]).astype(F64) @ np.abs(bf16(W)).astype(F64).T + np.abs(b)
    up("fwd_f32", assert_f32_sum(y, z, sa, f"{what} forward layer {L - 1} (fp32 out)"))
    err = float(np.abs(y - z).max())
    tol = 1e-5 * float(np.abs(z).max()) + 1e-6
    assert err <= tol, f"{what} output layer (fp32 out): max |err| {err:.3g} > {tol:.3g}"

    if rb.get("bits") is not None:                          # ReLU′ bits: the stored, rounded value > 0
        for i in range(1, L):
            got = np.asarray(rb["bits"][i], np.uint32)
            want = pack_bits(hs[i] > 0)
            assert got.shape == want.shape, f"{what} ReLU′ bits layer {i}: shape {got.shape} vs {want.shape}"
            bad = got != want
            if bad.any():
                r, w = np.argwhere(bad)[0]
                pad = sizes[i] % 32 and bool(((got ^ want)[:, -1] >> np.uint32(sizes[i] % 32)).any())
                raise AssertionError(f"{what} ReLU′ bits layer {i}: {int(bad.sum())} words differ"
                                     f"{' (pad bits set)' if pad else ''}, first row {r} word {w}: "
                                     f"{int(got[r, w]):#010x} vs {int(want[r, w]):#010x}")

    grads = np.asarray(rb["grads"], F32)
    _finite(grads, f"{what} packed gradients")
    off = 0
    for i in range(L):
        W, b = layers[i]
        nw = W.size
        if i == L - 1:
            g = (bf16(gtop) if top_rounded else np.asarray(gtop)).astype(F64).reshape(m, sizes[L])
        else:
            g = np.asarray(rb["gx"][i + 1], F32).astype(F64)
        gW = g.T @ hs[i].astype(F64)
        # fp32 sums over the batch (split-K partials, wave-level chains, f32 atomics): bounded by the fp32
        # summation error of those terms, c·Σ|g·h| with c = 2^-15, not by max|gW|: the MSE / surrogate
        # gradients change sign row to row, so |Σ g·h| ≪ Σ|g·h|
        sum_abs = np.abs(g).T @ np.abs(hs[i]).astype(F64)
        err = np.abs(grads[off:off + nw].reshape(W.shape) - gW)
        up("grad_W", float((err / (ACC * sum_abs + 1e-9)).max()))
        assert (err <= ACC * sum_abs + 1e-9).all(), f"{what} grad_W layer {i}: worst err / Σ|g·h| " \
            f"{float((err / np.maximum(sum_abs, 1e-30)).max()):.3g}"
        errb = np.abs(grads[off + nw:off + nw + b.size] - g.sum(axis=0))
        tolb = ACC * np.abs(g).sum(axis=0) + 1e-9
        up("bias", float((errb / tolb).max()))
        assert (errb <= tolb).all(), f"{what} bias grad layer {i}: worst err / Σ|g| " \
            f"{float((errb / np.maximum(np.abs(g).sum(axis=0), 1e-30)).max()):.3g}"
        off += nw + b.size
        if i > 0:
            gx = np.where(hs[i] > 0, g @ bf16(W).astype(F64), 0.0)
            sa = np.abs(g) @ np.abs(bf16(W)).astype(F64)
            up("grad_x", assert_bf16_rounding(np.asarray(rb["gx"][i], F32), gx, sa, f"{what} grad_x layer {i}"))
        elif rb["gx"][0] is not None:                       # layer 0: fp32, no mask
            gx = g @ bf16(W).astype(F64)
            sa = np.abs(g) @ np.abs(bf16(W)).astype(F64)
            up("grad_x0", assert_f32_sum(np.asarray(rb["gx"][0], F32), gx, sa, f"{what} grad_x layer 0 (fp32 out)"))
    print(f"{what}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


def _bf16_dev(lib, ptr, rows, width):
    import ppo_ffi
    u = ppo_ffi.d2h(lib, ptr, np.uint16, rows * width).reshape(rows, width)
    return (u.astype(np.uint32) << 16).view(F32)


def read_bf16_layers(lib, nn_ptr, sizes, m, grad_x0=False):
    """Everything the bf16 kernels stored for the last forward + backward of m rows (check_bf16_readback's rb)."""
    import ppo_ffi
    from helpers import nn_grads_packed
    nn = nn_ptr.contents
    L = len(sizes) - 1
    assert nn.dtype == 1 and nn.bits_m == m and nn.act_cap_m >= m
    cap = nn.act_cap_m
    wpr = [(s + 31) // 32 for s in sizes]
    base = C.cast(nn.d_act_bits, C.c_void_p).value
    bits, off = [None] * L, 0
    for i in range(L):                                      # one [cap, ⌈w/32⌉] block per layer input: its first m rows
        if i > 0:
            bits[i] = ppo_ffi.d2h(lib, C.c_void_p(base + 4 * off), np.uint32, m * wpr[i]).reshape(m, wpr[i])
        off += cap * wpr[i]
    return dict(h=[None] + [_bf16_dev(lib, nn.layers[i].d_input, m, sizes[i]) for i in range(1, L)],
                y=ppo_ffi.d2h(lib, nn.d_output, F32, m * sizes[L]).reshape(m, sizes[L]),
                bits=bits, grads=nn_grads_packed(lib, nn_ptr),
                gx=[ppo_ffi.d2h(lib, nn.layers[0].d_grad_x, F32, m * sizes[0]).reshape(m, sizes[0]) if grad_x0 else None]
                + [_bf16_dev(lib, nn.layers[i].d_grad_x, m, sizes[i]) for i in range(1, L)])


def check_bf16_layers(lib, nn_ptr, sizes, params, x, gtop, top_rounded, what, grad_x0=False):
    """Teacher-forced check of every bf16 kernel of one minibatch: each layer's forward from the GPU's own
    bf16 input activation, its ReLU′ bits from the activation it stored, each layer's grad_W / bias sums /
    grad_x from the GPU's own stored bf16 gradient (layers[i+1].d_grad_x) — so a bf16 rounding-boundary
    flip upstream (inherent to bf16 storage: the flip rate compounds with depth, ≈ 7e-3 of the last hidden
    layer's elements at C5) does not propagate into the comparison, and every kernel is pinned to fp32
    accumulation accuracy.  top_rounded: the output layer's gradient enters its products rounded to
    bf16 (both the separate bf16 launches and the fused bf16 value head, out_head.hip, round it as
    they stage it).  grad_x0: layer 0's fp32 grad_x was produced (backward_propagation_cuda) and is checked.
    Returns the packed gradients."""
    rb = read_bf16_layers(lib, nn_ptr, sizes, x.shape[0], grad_x0)
    check_bf16_readback(sizes, params, x, gtop, top_rounded, rb, what)
    return rb["grads"]


# ----------------------------------------------------------------------------- shapes and inputs of the kernel tests
NETWORKS = [[3, 33, 65, 1], [17, 40, 72, 6], [130, 264, 136, 17], [64, 128, 256, 8], [40, 24], [256, 256, 256, 8],
            [64, 40, 33, 8]]
BATCHES = [1, 33, 300, 576]


def make_case(sizes, m):
    """Parameters uniform(−1, 1)/√max(sizes), inputs and the output gradient uniform(−1, 1); returns (params, x,
    gout).  Two adjustments keep every defect of test_bf16_ref_cpu.py visible: the hidden layers' biases are moved
    up by half such a unit, so that more than half of every hidden layer is live; and each hidden layer's LAST
    unit gets the bias that centres it on the batch (minus the median of its pre-bias sum), so that the last
    column — the one a tail bug touches — is live in half of the rows and dead in the others (live, with one row)."""
    rng = np.random.default_rng(1000 * sum(sizes) + m)
    scale = 1.0 / np.sqrt(max(sizes))
    params = (rng.uniform(-1, 1, num_params(sizes)) * scale).astype(F32)
    x = rng.uniform(-1, 1, (m, sizes[0])).astype(F32)
    gout = rng.uniform(-1, 1, (m, sizes[-1])).astype(F32)
    h = bf16(x).astype(F64)
    for W, b in unpack(sizes, params)[:-1]:                 # views into params
        b += F32(0.5 * scale)
        w16 = bf16(W).astype(F64)
        b[-1] = F32(-np.median(h @ w16[-1])) + (F32(0.5 * scale) if m == 1 else F32(0))   # one row: live
        h = bf16(np.maximum(h @ w16.T + b, 0.0).astype(F32)).astype(F64)
    return params, x, gout


# ----------------------------------------------------------------------------- fp32 model of the kernels
def gemm_f32_model(A, B, bk=32, splits=1, reverse=False, drop_last_tile=False):
    """C = A·B (A [M, K], B [K, N], bf16-valued) as the kernels accumulate it: each split of K chains its
    BK-wide k-tiles' partial sums in float32 (ascending, or descending with `reverse`), the splits' partials
    are added in float32 (in order, or reversed).  The split ranges are phip_linear16_bwd_w's: kchunk =
    ⌈⌈K/splits⌉/BK⌉·BK.  drop_last_tile: the defect "the last split loses its last k-tile"."""
    M, K = A.shape
    if K == 0:
        return np.zeros((M, B.shape[1]), F32)
    kchunk = -(-(-(-K // splits)) // bk) * bk
    parts = []
    for lo in range(0, K, kchunk):
        hi = min(K, lo + kchunk)
        tiles = list(range(lo, hi, bk))
        if drop_last_tile and hi == K:
            tiles = tiles[:-1]
        if reverse:
            tiles.reverse()
        acc = np.zeros((M, B.shape[1]), F32)
        for k0 in tiles:
            k1 = min(k0 + bk, hi)
            acc = acc + (A[:, k0:k1].astype(F64) @ B[k0:k1].astype(F64)).astype(F32)
        parts.append(acc)
    if reverse:
        parts.reverse()
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


MUTANTS = ("fwd_drop_last_k", "fwd_drop_last_row", "fwd_trunc_one", "bits_clear_last_valid", "bits_set_pad",
           "gw_drop_last_row", "gw_drop_last_tile", "bias_drop_last_row", "gx_drop_last_k", "gx_unmask_last_col",
           "gx_mask_next_row", "gx_trunc_one")


def _trunc_one(v32, sum_abs):
    """v32 (fp32, before storage) rounded to bf16 to nearest even, except ONE element truncated: the one where
    the truncation error is largest against 2^-8·|value| + 2^-15·Σ|terms| (a truncation errs by up to one bf16
    ulp; the bound grants half an ulp of the VALUE, so it is visible where the mantissa sits low in its binade
    and the dropped bits are large — and the sum's own slack is small)."""
    out = bf16(v32)
    tr = bf16_trunc(v32)
    score = np.where(tr != out, np.abs(tr.astype(F64) - v32) / (ULP * np.abs(v32.astype(F64)) + ACC * sum_abs + 1e-30),
                     0.0)
    at = np.unravel_index(int(np.argmax(score)), score.shape)
    out[at] = tr[at]
    return out


def model_run(sizes, params, x, gout, bk=32, splits=1, reverse=False, mutant=None, layer=None):
    """One forward + backward of m rows as the bf16 kernels run it, in the fp32 model above: returns
    (rb, changed) — rb as check_bf16_readback reads it; changed: the injected defect (`mutant` at `layer`:
    the layer whose launch is defective; later launches consume what it stored, as on the GPU) altered the
    defective launch's output."""
    L, m = len(sizes) - 1, x.shape[0]
    layers = unpack(sizes, params)
    kw = dict(bk=bk, splits=splits, reverse=reverse)
    changed = False

    def hit(name, i):
        return mutant == name and layer == i

    h = [bf16(x)] + [None] * (L - 1)
    bits = [None] * L
    y = None
    for i, (W, b) in enumerate(layers):
        a, w16 = h[i], bf16(W).T                            # [m, n], [n, l]
        if hit("fwd_drop_last_k", i):
            a, w16 = a[:, :-1], w16[:-1]
        v = gemm_f32_model(a, w16, **kw) + b.astype(F32)    # fp32 bias add in the epilogue
        clean = gemm_f32_model(h[i], bf16(W).T, **kw) + b.astype(F32) if mutant and layer == i else v
        if i < L - 1:
            v, clean = np.maximum(v, F32(0)), np.maximum(clean, F32(0))
            out = bf16(v)
            if hit("fwd_trunc_one", i):
                out = _trunc_one(v, np.abs(h[i]).astype(F64) @ np.abs(bf16(W)).astype(F64).T + np.abs(b))
            if hit("fwd_drop_last_row", i):
                out[m - 1] = 0
            live = out > 0
            if hit("bits_clear_last_valid", i):
                changed |= bool(live[:, -1].any())
                live = live.copy()
                live[:, -1] = False
            words = pack_bits(live)
            if hit("bits_set_pad", i) and sizes[i + 1] % 32:
                words[:, -1] |= np.uint32(1) << np.uint32(sizes[i + 1] % 32)
                changed = True
            if mutant in ("fwd_drop_last_k", "fwd_drop_last_row", "fwd_trunc_one") and layer == i:
                changed |= bool((out != bf16(clean)).any())
            h[i + 1], bits[i + 1] = out, words
        else:
            y = v.astype(F32)
            if hit("fwd_drop_last_row", i):
                y[m - 1] = 0
            if mutant in ("fwd_drop_last_k", "fwd_drop_last_row") and layer == i:
                changed |= bool((y != clean).any())
    grads = [None] * L
    gx = [None] * L
    g = bf16(gout)                                          # fp32 from the heads, rounded in the loader
    for i in range(L - 1, -1, -1):
        W, _ = layers[i]
        rows = m - 1 if hit("gw_drop_last_row", i) else m
        gW = gemm_f32_model(np.ascontiguousarray(g[:rows].T), h[i][:rows], drop_last_tile=hit("gw_drop_last_tile", i),
                            **kw) if rows else np.zeros(W.shape, F32)
        rows = m - 1 if hit("bias_drop_last_row", i) else m
        gb = gemm_f32_model(np.ascontiguousarray(g[:rows].T), np.ones((rows, 1), F32), **kw).ravel() if rows \
            else np.zeros(sizes[i + 1], F32)
        if mutant in ("gw_drop_last_row", "gw_drop_last_tile", "bias_drop_last_row") and layer == i:
            changed |= bool((gW != gemm_f32_model(np.ascontiguousarray(g.T), h[i], **kw)).any() or
                            (gb != gemm_f32_model(np.ascontiguousarray(g.T), np.ones((m, 1), F32), **kw).ravel()).any())
        grads[i] = (gW.ravel(), gb)
        ga, w16 = g, bf16(W)                                # [m, l], [l, n]
        if hit("gx_drop_last_k", i):
            ga, w16 = ga[:, :-1], w16[:-1]
        v = gemm_f32_model(ga, w16, **kw)
        if i == 0:
            gx[0] = v
            if hit("gx_drop_last_k", i):
                changed |= bool((v != gemm_f32_model(g, bf16(W), **kw)).any())
            break
        keep = unpack_bits(bits[i], sizes[i])               # the kernel reads the bits, not the activation
        clean = bf16(np.where(keep, gemm_f32_model(g, bf16(W), **kw), F32(0))) if mutant and layer == i else None
        if hit("gx_mask_next_row", i):
            keep = keep[np.minimum(np.arange(m) + 1, m - 1)]
        if hit("gx_unmask_last_col", i):
            keep = keep.copy()
            keep[:, -1] = True
        v = np.where(keep, v, F32(0))
        out = bf16(v)
        if hit("gx_trunc_one", i):
            out = _trunc_one(v, np.where(keep, np.abs(g).astype(F64) @ np.abs(bf16(W)).astype(F64), 0.0))
        if mutant and mutant.startswith("gx_") and layer == i:
            changed |= bool((out != clean).any())
        gx[i] = out
        g = out
    rb = dict(h=h, y=y, bits=bits, gx=gx,
              grads=np.concatenate([np.concatenate([gw, gb]) for gw, gb in grads]).astype(F32))
    return rb, changed
