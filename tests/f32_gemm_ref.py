"""fp32 mode's two GEMM engines (csrc/gemm.hip: the exact fp32 MFMA; csrc/gemm_x3.hip: three bf16 planes), one
linear layer's three launches in float64 with a bound of its own for every output element.  Pinned on the CPU in
test_f32_gemm_ref_cpu.py; used on the GPU by test_gpu_f32_kernels.py.  pack_bits / unpack_bits are bf16_ref's.

The float64 model of a layer (h its input, W [l, n], b, g the gradient at its output, all as the GPU stored them):
    forward   z = h·Wᵀ + b, relu(z) for a hidden layer      Σ|terms| = |h|·|W|ᵀ + |b|
    ReLU′     word block == pack_bits(stored output > 0) bit for bit, pad bits of the last word zero
    grad_x    where(stored h > 0, g·W, 0) (layer 0: g·W)    Σ|terms| = |g|·|W|
    grad_W    gᵀ·h,  bias gradient Σ_rows g                  Σ|terms| = |g|ᵀ·|h|,  Σ_rows |g|

(a) The bound, for every element:  |got − want| ≤ c·2^-24·Σ|terms| + 2^-24·|want|.
c is the longest chain of fp32 roundings the engine can put on one output: a term that passes through d rounded
operations carries a relative error ≤ d·2^-24 (to first order), so the sum errs by ≤ max d·2^-24·Σ|terms|; the
last 2^-24·|want| is the rounding of the stored value itself.  Where Σ|terms| = 0 the bound is 0: a zero stays zero.
Neither MFMA's internal order is documented, so every k of an MFMA counts as one addition of the chain (the worst
any fp32 evaluation of that dot product can do).

  chain_exact(K, partials) = K + 2 + partials          csrc/gemm.hip
    gemm_tile compute() (lines 285-299): one v_mfma_f32_32x32x2_f32 per pair of k (one k from each lane half) into
      the same accumulator: K additions over [kbeg, kend) (237-238), + 1 for the rounding of the product itself;
    split-K (bwd_w_args 751-759): `splits` atomicAdds onto a zeroed output (402);
    small-M kernels (474-526, 547): eight waves' chains of ≤ ⌈K/8⌉ k, then 8 additions through LDS;
    forward bias add (392, 551): + 1;
    bias gradient: rowsum per k-tile (277), a shuffle tree (331), split atomics (334); small-M 522, 534: ≤ K + 16.
    partials = max(16, number of splits) covers each of them.
  chain_x3(K, partials) = 1.01·6·K + 4 + partials    csrc/gemm_x3.hip
    mm() (613-622): six plane products per k-tile of 16 k (cfg 6: 32 k, two MFMA k-steps), each a
      v_mfma_f32_32x32x16_bf16 into the same accumulator.  A product of two bf16 values is exact in fp32 (8 + 8
      significant bits), so only the additions round: 6·KB per k-tile, ⌈K/KB⌉ k-tiles (626-628); the partial
      last tile is padded with zeros, whose additions are exact: 6·K.  (Weighting the planes by their magnitude
      does not shorten the chain: every addition rounds the whole accumulator, however small the term it adds);
    the planes' |a_p|·|b_q| sum to ≤ (1 + 2^-8)²·|a|·|b| ≤ 1.01·|a·b| (|a_0| ≤ (1 + 2^-8)|a|, |a_1| ≤ 2^-9|a|);
    two k-groups (cfg 3 of grad_W) add their accumulators through LDS (863): + 1;
    split-K: slabs summed by slab_reduce_kernel<4> / <16> (1013, 1019), by the next grad_x launch
      (x3_slab_reduce_block 114, 121) or f32 atomics (923): ≤ `splits` additions;
    the dropped plane products (1,2), (2,1), (2,2): ≤ (2·2^-27 + 2^-36)·|a·b| < 2^-24·|a·b|: + 1;
    forward bias add (445): + 1;
    bias gradient: per-thread sums over the split's k (665), NV + S additions through LDS (810, 815), atomics (818):
      under the same count.
  partials: splits ≤ m/128 in both engines (≥ 8 k-tiles of ≥ 16 per split: gemm.hip 753, gemm_x3.hip 1252).

acc_exact / acc_x3 are fp32 models of the two accumulations (x3 with the round-to-nearest three-plane split of
split4, gemm_x3.hip 149-157) in forward, reverse and split orders; the CPU test shows them inside the bound at every
network and batch of the GPU test.

(b) One-term probes.  Operands with full 24-bit mantissas and exponents in 2^-6 … 2^6 arranged so that most outputs
are ONE product a·b (W with one nonzero per row at column π(j) = j mod n, zero biases; the top gradient with one
nonzero row per unit).  check_f32_readback(probe=…) counts the nonzero terms of every output from the GPU's own
operands: none — the output is 0; one — on the exact engine it equals float32(float64(a)·float64(b)) bit for bit
(one correctly rounded product added to zero), on x3 it is within 2^-21·|a·b| (x3_product_model: over 2 000 000
random pairs and all 720 orders of the six kept products the worst relative error is 2^-21.72, and dropping any one
kept product puts most elements beyond 2^-21); more than one — bound (a).

(c) Integer probes.  Integer operands small enough that Σ|terms| < 2^24 and every operand < 2^16 (so x3's third
plane is zero and no product is dropped): every partial sum in any order is an integer below 2^24, both engines,
every configuration and every split-K mode equal int64 arithmetic exactly (check_f32_readback(exact=True)).  The
network input, layer 0's weights, the top gradient and all biases are integers in [−8, 8]; the upper layers' weights
are −1 / 0 / 1 (a quarter nonzero), which keeps the activations they pass on small (int_premise asserts it).
"""
import ctypes as C
import itertools
import math

import numpy as np

from bf16_ref import bf16, num_params, pack_bits, unpack, unpack_bits

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24
X3_ONE_TERM = 2.0 ** -21

# the shapes of test_gpu_f32_kernels.py (why each: its docstring)
EXACT_NETWORKS = [[3, 33, 65, 1], [17, 40, 72, 6], [130, 264, 136, 17], [64, 128, 256, 8], [40, 24]]
EXACT_BATCHES = [1, 33, 200, 300, 1100]
X3_NETWORKS = [[36, 68, 132, 260, 4], [64, 128, 256, 8]]
X3_BATCHES = [1025, 1100]
SPLIT_TARGET = 4096      # exact engine: as many splits as 8 k-tiles each allow — a partial last one at m = 300, 1100
# x3 grad_W, (m, n, l, cfg, split target, reduce deferred to grad_x) → the mode test_gpu_f32_kernels.py reaches with it
X3_GRADW_MODES = {(1100, 36, 68, 3, 1, True): "one", (1100, 36, 68, 3, 0, True): "carried",
                  (1100, 36, 68, 3, 0, False): "reduce4", (18145, 36, 68, 3, 0, False): "reduce16",
                  (2340, 36, 68, 3, 2, False): "atomics"}


def chain_exact(K, partials=16):
    return K + 2 + max(16, partials)


def chain_x3(K, partials=16):
    return math.ceil(1.01 * 6 * K) + 4 + max(16, partials)


def max_splits(m):
    return max(16, m // 128 + 1)


# ----------------------------------------------------------------------------- host arithmetic, restated
EXACT_CFGS = [(128, 128, 16), (128, 128, 32), (128, 32, 16), (32, 128, 16), (64, 64, 16), (128, 64, 16),
              (256, 128, 16), (128, 128, 16), (128, 64, 16), (64, 64, 32), (128, 32, 32)]      # gemm.hip kCfgs
X3_CFGS = [(256, 256, 1, 1, 16), (128, 128, 1, 2, 16), (128, 128, 1, 1, 16), (128, 128, 2, 1, 16),
           (64, 64, 1, 4, 16), (256, 128, 1, 1, 16), (64, 64, 1, 2, 32)]                       # gemm_x3.hip kCfgX3


def _divup(a, b):
    return -(-a // b)


def exact_pick_cfg(op, M, N):
    """gemm.hip pick_cfg → (cfg, split-K target); op 0 forward, 1 grad_x, 2 grad_W"""
    target = 1024
    if N <= 32 and M > 32:
        return (10 if op == 0 else 2), target
    if M <= 32 and N > 32:
        return 3, target
    if M <= 64 or N <= 64:
        return 4, target
    tiles = _divup(M, 128) * _divup(N, 128)
    if op == 2:
        big = tiles >= 16 and N % 128 == 0
        return (0 if big else 4), (512 if big else 2048)
    return (5 if tiles < 512 else 0), target


def exact_use_smallm(m, K, N):
    """gemm.hip use_smallm (forward: K = n, N = l; grad_x: K = l, N = n)"""
    return m <= 1024 and K >= 64 and _divup(m, 128) * _divup(N, 64) < 64


def exact_use_smallm_w(m, n, l):
    return 128 < m <= 256 and _divup(l, 32) * _divup(n, 32) >= 16


def exact_gradw_splits(m, n, l, cfg=-1, target_override=0):
    """gemm.hip bwd_w / bwd_w_args → (cfg, kchunk, splits); cfg −1: automatic (small-M grad_W: splits 0)"""
    if cfg < 0 and exact_use_smallm_w(m, n, l):
        return -1, m, 0
    if cfg < 0 and m <= 128 and l > 32 and n > 32:
        cfg = 4
    target = 1024
    if cfg < 0:
        cfg, target = exact_pick_cfg(2, l, n)
    if target_override > 0:
        target = target_override
    bm, bn, bk = EXACT_CFGS[cfg]
    tiles = _divup(l, bm) * _divup(n, bn)
    splits = max(1, min(target // tiles, max(1, m // (8 * bk))))
    kchunk = _divup(_divup(m, splits), bk) * bk
    return cfg, kchunk, _divup(m, kchunk)


def x3_pick(M, N, op, force=-1):
    """gemm_x3.hip pick_x3 (M, N the output's extents; grad_W: M = l, N = n)"""
    if force >= 0:
        return force
    if op == 2:
        return 3
    if _divup(M, 256) * _divup(N, 256) >= 256:
        return 0
    if _divup(M, 128) * _divup(N, 128) >= 256:
        return 2
    return 4


def x3_gradw_mode(m, n, l, cfg=-1, target=0, defer=False):
    """phip_x3_bwd_w_vhead's split arithmetic (gemm_x3.hip 1243-1256, 1298) → (kchunk, splits, mode); mode: "one",
    "carried" (slabs, the reduce rides on the next grad_x), "reduce4" / "reduce16" (slabs + slab_reduce_kernel<Q>),
    "atomics"."""
    c = x3_pick(l, n, 2, cfg)
    bm, bn, kg, slots, kb = X3_CFGS[c]
    tiles = _divup(l, bm) * _divup(n, bn)
    kq = kb * kg
    tgt = target if target > 0 else 256 * slots
    splits = max(1, min(tgt // tiles, max(1, m // (8 * kq))))
    kchunk = _divup(_divup(m, splits), kq) * kq
    splits = _divup(m, kchunk)
    if splits == 1:
        return kchunk, 1, "one"
    if kchunk > 1024:
        return kchunk, splits, "atomics"
    if defer and splits < 64:
        return kchunk, splits, "carried"
    return kchunk, splits, "reduce16" if splits >= 64 else "reduce4"


def x3_layer(engine, m, n, l):
    """neural_network.c use_x3_layer + phip_x3_supported: the MLP route gives this layer to x3"""
    return engine == 1 and m > 1024 and n > 32 and l > 32 and n % 4 == 0 and l % 4 == 0


def x3_product(engine, m, n, l):
    """neural_network.c lin_fwd / lin_bwd_*: the reference-API products' route (any width)"""
    return engine == 1 and m > 1024 and n % 4 == 0 and l % 4 == 0


# ----------------------------------------------------------------------------- fp32 models of the accumulations
def acc_exact(A, B, order="forward", splits=1, drop=None):
    """C = A·B (A [M, K], B [K, N] float32) as the exact engine accumulates: one rounded product and one rounded
    addition per k (float32 numpy arithmetic), k ascending, descending ("reverse") or in `splits` ranges whose
    partials are added in float32 ("split")."""
    M, K = A.shape
    ks = list(range(K))
    if order == "reverse":
        ks.reverse()
    parts = [ks] if order != "split" or splits <= 1 else [list(c) for c in np.array_split(ks, splits) if len(c)]
    out = None
    for part in parts:
        acc = np.zeros((M, B.shape[1]), F32)
        for k in part:
            acc += A[:, k:k + 1] * B[k:k + 1, :]
        out = acc if out is None else out + acc
    return out if out is not None else np.zeros((M, B.shape[1]), F32)


def split3(a):
    """the round-to-nearest three-plane split of gemm_x3.hip split4: a = a0 + a1 + a2 exactly, each a bf16"""
    a = np.ascontiguousarray(a, F32)
    a0 = bf16(a)
    r = a - a0
    a1 = bf16(r)
    return a0, a1, bf16(r - a1)


X3_KEPT = ((2, 0), (0, 0), (1, 0), (0, 2), (0, 1), (1, 1))          # mm()'s order within a k-tile


def acc_x3(A, B, order="forward", splits=1, kb=16, kept=X3_KEPT):
    """C = A·B as the x3 engine accumulates: per k-tile of kb the kept plane products, each one MFMA dot product
    (taken exactly, in float64, then rounded once) added to the float32 accumulator; tiles ascending, descending
    or in `splits` ranges of whole tiles."""
    M, K = A.shape
    pa, pb = split3(A), split3(B)
    tiles = list(range(0, K, kb))
    if order == "reverse":
        tiles.reverse()
    parts = [tiles] if order != "split" or splits <= 1 else [list(c) for c in np.array_split(tiles, splits) if len(c)]
    out = None
    for part in parts:
        acc = np.zeros((M, B.shape[1]), F32)
        for k0 in part:
            for p, q in kept:
                acc += (pa[p][:, k0:k0 + kb].astype(F64) @ pb[q][k0:k0 + kb].astype(F64)).astype(F32)
        out = acc if out is None else out + acc
    return out if out is not None else np.zeros((M, B.shape[1]), F32)


def x3_product_model(a, b, kept=X3_KEPT, orders=None):
    """One product a·b per element as x3 forms it: the kept plane products (exact in fp32) added to a zero float32
    accumulator in every order of `orders` (default: all permutations).  Returns the worst |got − a·b| / |a·b| per
    element over the orders."""
    pa, pb = split3(a), split3(b)
    prods = [pa[p] * pb[q] for p, q in kept]                            # exact: 8 × 8 significant bits
    want = a.astype(F64) * b.astype(F64)
    lo, hi = np.full(a.shape, np.inf, F32), np.full(a.shape, -np.inf, F32)
    if orders is not None:
        for perm in orders:
            acc = np.zeros(a.shape, F32)
            for i in perm:
                acc = acc + prods[i]
            np.minimum(lo, acc, out=lo)
            np.maximum(hi, acc, out=hi)
    else:                                                               # all orders, shared prefixes
        def walk(acc, left):
            if not left:
                np.minimum(lo, acc, out=lo)
                np.maximum(hi, acc, out=hi)
            for i in left:
                walk(acc + prods[i], [j for j in left if j != i])
        walk(np.zeros(a.shape, F32), list(range(len(kept))))
    return np.maximum(np.abs(lo.astype(F64) - want), np.abs(hi.astype(F64) - want)) / np.abs(want)


def full_mantissa(rng, shape):
    """float32 values with all 24 mantissa bits in use (the lowest bit set), exponents 2^-6 … 2^6, positive"""
    mant = (rng.integers(1 << 23, 1 << 24, shape, dtype=np.int64) | 1).astype(F64) / (1 << 23)     # [1, 2), odd
    return (mant * 2.0 ** rng.integers(-6, 7, shape)).astype(F32)


# ----------------------------------------------------------------------------- inputs
def make_case(sizes, m):
    """Random inputs with small outputs next to large ones: the rows of x and of the top gradient, and the rows
    of every W with their biases, are scaled by powers of two from 2^-6 … 2^6 (row 0 / unit 0 by 2^6, the last
    row / last unit by 2^-6: the tails are the small ones).  One row of x is zero and units 1 and 2 of every hidden
    layer have zero bias, so some pre-activations are exactly 0 (mask bit clear).  Returns (params, x, gout)."""
    rng = np.random.default_rng(7000 * sum(sizes) + m)
    L = len(sizes) - 1
    params = np.empty(num_params(sizes), F32)
    for i, (W, b) in enumerate(unpack(sizes, params)):
        l, n = W.shape
        t = 2.0 ** rng.integers(-6, 7, l)
        t[0], t[-1] = 2.0 ** 6, 2.0 ** -6
        W[:] = rng.uniform(-1, 1, (l, n)) / np.sqrt(n) * t[:, None]
        b[:] = rng.uniform(-0.5, 0.5, l) * t
        if i < L - 1:
            b[1:3] = 0
    s = 2.0 ** rng.integers(-6, 7, m)
    s[0], s[-1] = 2.0 ** 6, 2.0 ** -6
    x = (rng.uniform(-1, 1, (m, sizes[0])) * s[:, None]).astype(F32)
    if m >= 3:
        x[m // 2] = 0
    s = 2.0 ** rng.integers(-6, 7, m)
    s[0], s[-1] = 2.0 ** 6, 2.0 ** -6
    gout = (rng.uniform(-1, 1, (m, sizes[-1])) * s[:, None]).astype(F32)
    return params, x, gout


def probe_rows(m, kchunks=()):
    """rows a grad_W probe must touch: 0, m − 1 and the first and last row of every split of every kchunk given"""
    rows = {0, m - 1}
    for kc in kchunks:
        for lo in range(0, m, kc):
            rows.update((lo, min(m, lo + kc) - 1))
    return sorted(rows)


def make_oneterm_case(sizes, m, rows, rep=0):
    """(b): W[j, j mod n] = ±w_j (an eighth of the units negative: dead, their outputs exact zeros), zero biases,
    x dense; the top gradient has one nonzero per unit j, in row rows[(j + rep·out) mod len(rows)]."""
    rng = np.random.default_rng(9000 * sum(sizes) + m)
    params = np.zeros(num_params(sizes), F32)
    for W, _ in unpack(sizes, params):
        l, n = W.shape
        w = full_mantissa(rng, l)
        w[rng.random(l) < 0.125] *= -1
        W[np.arange(l), np.arange(l) % n] = w
    x = full_mantissa(rng, (m, sizes[0]))
    out = sizes[-1]
    gout = np.zeros((m, out), F32)
    j = np.arange(out)
    gout[np.asarray(rows)[(j + rep * out) % len(rows)], j] = full_mantissa(rng, out) * np.where(j % 2, -1, 1)
    return params, x, gout


def make_int_case(sizes, m):
    """(c): integers.  x, W0, biases and the top gradient in [−8, 8]; the upper layers' weights −1 / 0 / 1."""
    rng = np.random.default_rng(11000 * sum(sizes) + m)
    params = np.empty(num_params(sizes), F32)
    for i, (W, b) in enumerate(unpack(sizes, params)):
        if i == 0:
            W[:] = rng.integers(-8, 9, W.shape)
        else:
            W[:] = rng.integers(-1, 2, W.shape) * (rng.random(W.shape) < 0.375)
        b[:] = rng.integers(-8, 9, b.shape)
    x = rng.integers(-8, 9, (m, sizes[0])).astype(F32)
    gout = rng.integers(-8, 9, (m, sizes[-1])).astype(F32)
    return params, x, gout


# ----------------------------------------------------------------------------- the float64 model of one layer
def layer_forward(h, W, b, relu):
    z = h.astype(F64) @ W.astype(F64).T + (0 if b is None else b.astype(F64))
    sa = np.abs(h).astype(F64) @ np.abs(W).astype(F64).T + (0 if b is None else np.abs(b).astype(F64))
    return (np.maximum(z, 0.0) if relu else z), sa


def layer_grad_x(g, W, mask):
    gx = g.astype(F64) @ W.astype(F64)
    sa = np.abs(g).astype(F64) @ np.abs(W).astype(F64)
    if mask is not None:
        gx, sa = np.where(mask, gx, 0.0), np.where(mask, sa, 0.0)
    return gx, sa


def layer_grad_w(g, h):
    g64, h64 = g.astype(F64), h.astype(F64)
    return g64.T @ h64, np.abs(g64).T @ np.abs(h64), g64.sum(axis=0), np.abs(g64).sum(axis=0)


def _terms(A, B):
    """number of nonzero terms of every element of A·B"""
    return (A != 0).astype(F64) @ (B != 0).astype(F64)


def check_elements(got, want, sum_abs, c, what, terms=None, one_term=None, exact=False, extra=0.0):
    """(a) for every element; with `terms` (the nonzero-term counts) the probe rules of (b): no term — zero; one
    term — `one_term` = 0: bit for bit float32(want), else within one_term·|want|.  exact: (c), array equality.
    extra: further roundings on top of c (the fold's scale multiplications).  Returns (worst err / bound,
    Σ (err / Σ|terms|)², count) — the last two over the elements with Σ|terms| > 0."""
    got = np.asarray(got, F32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} NaN/Inf elements"
    if exact:
        np.testing.assert_array_equal(got, want.astype(F32), err_msg=f"{what}: integer probe")   # −0 == 0
    err = np.abs(got.astype(F64) - want)
    tol = (c + extra) * U * sum_abs + U * np.abs(want)
    if terms is not None:
        one = terms == 1
        if one_term:
            tol = np.where(one, one_term * np.abs(want), tol)
        else:
            bad = one & (got != want.astype(F32))
            assert not bad.any(), f"{what}: {int(bad.sum())} one-term outputs are not the correctly rounded product, " \
                                  f"first at {tuple(np.argwhere(bad)[0])}"
        nz = (terms == 0) & (got != 0)
        assert not nz.any(), f"{what}: {int(nz.sum())} outputs without a term are not zero"
    bad = err > tol
    live = sum_abs > 0
    ratio = float((err[live] / tol[live]).max(initial=0.0))
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond their bound, first at " \
                          f"{tuple(np.argwhere(bad)[0])}: err {float(err[bad].max()):.3g} (worst err / bound {ratio:.3g})"
    rel = err[live] / sum_abs[live]
    return ratio, float((rel * rel).sum()), int(live.sum())


def check_bits(got, h, what):
    """the ReLU′ words equal pack_bits(stored h > 0) bit for bit (so the pad bits are zero)"""
    got = np.asarray(got, np.uint32)
    want = pack_bits(h > 0)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = got != want
    if bad.any():
        r, w = np.argwhere(bad)[0]
        n = h.shape[1]
        pad = n % 32 and bool(((got ^ want)[:, -1] >> np.uint32(n % 32)).any())
        raise AssertionError(f"{what}: {int(bad.sum())} words differ{' (pad bits set)' if pad else ''}, first row {r} "
                             f"word {w}: {int(got[r, w]):#010x} vs {int(want[r, w]):#010x}")


PRODUCTS = ("forward", "grad_x", "grad_W", "bias")


class Tally:
    """worst err / bound and the RMS of err / Σ|terms| per product"""

    def __init__(self):
        self.worst = dict.fromkeys(PRODUCTS, 0.0)
        self.sq = dict.fromkeys(PRODUCTS, 0.0)
        self.n = dict.fromkeys(PRODUCTS, 0)

    def add(self, key, res):
        self.worst[key] = max(self.worst[key], res[0])
        self.sq[key] += res[1]
        self.n[key] += res[2]

    def merge(self, other):
        for k in PRODUCTS:
            self.add(k, (other.worst[k], other.sq[k], other.n[k]))

    def rms(self, key):
        return math.sqrt(self.sq[key] / self.n[key]) if self.n[key] else 0.0

    def line(self):
        return ", ".join(f"{k} {self.worst[k]:.4f}" for k in PRODUCTS)


def check_f32_readback(sizes, params, x, gtop, rb, chains, what, probe=None, exact=False, engine_of=None):
    """Every launch of one forward + backward over x's rows against the model, from the operands the GPU itself
    stored (teacher forcing).  rb: h[i] (i = 1 … L−1, stored activations), y, bits[i] (i = 1 … L−1), gx[i]
    (i = 0 … L−1; None: not produced), grads (packed).  chains(i, op, K) → c of layer i's launch (op 0 forward, 1
    grad_x, 2 grad_W and its bias sums).  probe: None, or the one-term bound of the engine of layer i as
    probe(i) → 0 (bit for bit) / 2^-21.  exact: the integer probes.  Returns a Tally; with engine_of(i) → name its
    .by holds one Tally per engine name (the x3 setting leaves narrow layers to the exact kernels)."""
    L, m = len(sizes) - 1, x.shape[0]
    layers = unpack(sizes, params)
    hs = [np.asarray(x, F32)] + [np.asarray(rb["h"][i], F32) for i in range(1, L)]
    t = Tally()
    t.by = {}
    kw = dict(exact=exact)

    def add(i, key, res):
        t.add(key, res)
        if engine_of:
            t.by.setdefault(engine_of(i), Tally()).add(key, res)
    for i, (W, b) in enumerate(layers):
        n, l = sizes[i], sizes[i + 1]
        got = rb["y"] if i == L - 1 else hs[i + 1]
        want, sa = layer_forward(hs[i], W, b, i < L - 1)
        pk = {}
        if probe:
            terms = _terms(hs[i], W.T) + (b != 0)
            pk = dict(terms=terms, one_term=probe(i))
            if i < L - 1:                                   # a negative single product: relu → an exact zero
                pk["terms"] = np.where(want > 0, terms, np.where(terms == 1, 0, terms))
        add(i, "forward", check_elements(np.asarray(got, F32).reshape(m, l), want, sa, chains(i, 0, n),
                                        f"{what} forward layer {i}", **pk, **kw))
        if i < L - 1:
            check_bits(rb["bits"][i + 1], hs[i + 1], f"{what} ReLU′ bits of layer {i}")
    grads = np.asarray(rb["grads"], F32)
    off = 0
    for i, (W, b) in enumerate(layers):
        n, l = sizes[i], sizes[i + 1]
        g = np.asarray(gtop if i == L - 1 else rb["gx"][i + 1], F32).reshape(m, l)
        gW, saW, gb, sab = layer_grad_w(g, hs[i])
        c = chains(i, 2, m)
        pk = dict(terms=_terms(g.T, hs[i]), one_term=probe(i)) if probe else {}
        add(i, "grad_W", check_elements(grads[off:off + l * n].reshape(l, n), gW, saW, c, f"{what} grad_W layer {i}",
                                       **pk, **kw))
        pk = dict(terms=(g != 0).sum(axis=0).astype(F64), one_term=0.0) if probe else {}
        add(i, "bias", check_elements(grads[off + l * n:off + l * n + l], gb, sab, c, f"{what} bias gradient layer {i}",
                                     **pk, **kw))
        off += l * n + l
        if rb["gx"][i] is not None:
            mask = hs[i] > 0 if i > 0 else None
            gx, sa = layer_grad_x(g, W, mask)
            pk = {}
            if probe:
                terms = _terms(g, W)
                pk = dict(terms=terms if mask is None else np.where(mask, terms, 0), one_term=probe(i))
            add(i, "grad_x", check_elements(rb["gx"][i], gx, sa, chains(i, 1, l), f"{what} grad_x layer {i}", **pk, **kw))
    print(f"{what}: worst err / bound {t.line()}")
    return t


def check_product(x, W, b, g, y, gx, gW, c_of, what, probe=None, exact=False):
    """the three reference-API products (mat_mul_cuda, mat_mul_backwards_cuda: no activation, no bias gradient)"""
    m, n = x.shape
    l = W.shape[0]
    t = Tally()
    pk = lambda terms: dict(terms=terms, one_term=probe) if probe is not None else {}
    want, sa = layer_forward(x, W, b, False)
    t.add("forward", check_elements(y, want, sa, c_of(0, n), f"{what} forward", exact=exact,
                                    **pk(_terms(x, W.T) + (b != 0))))
    want, sa = layer_grad_x(g, W, None)
    t.add("grad_x", check_elements(gx, want, sa, c_of(1, l), f"{what} grad_x", exact=exact, **pk(_terms(g, W))))
    want, sa, _, _ = layer_grad_w(g, x)
    t.add("grad_W", check_elements(gW, want, sa, c_of(2, m), f"{what} grad_W", exact=exact, **pk(_terms(g.T, x))))
    print(f"{what}: worst err / bound {t.line()}")
    return t


def int_premise(sizes, params, x, gout):
    """(c)'s premise on the int64 model of the whole pass: returns (largest Σ|terms| of any output of any launch,
    largest |operand| of any launch)."""
    L = len(sizes) - 1
    layers = unpack(sizes, params)
    hs, big, op = [x.astype(F64)], 0.0, float(np.abs(x).max(initial=0))
    for i, (W, b) in enumerate(layers):
        z, sa = layer_forward(hs[i], W, b, i < L - 1)
        big, op = max(big, sa.max()), max(op, np.abs(W).max(), np.abs(z).max())
        hs.append(z)
    g = gout.astype(F64)
    for i in range(L - 1, -1, -1):
        W = layers[i][0]
        _, saW, _, sab = layer_grad_w(g, hs[i])
        gx, sa = layer_grad_x(g, W, hs[i] > 0 if i > 0 else None)
        big, op = max(big, saW.max(), sab.max(), sa.max()), max(op, np.abs(g).max())
        g = gx
    return big, op


# ----------------------------------------------------------------------------- a model run with injectable defects
DEFECTS = ("lost_last_row", "lost_last_k", "lost_last_k_tile", "lost_row_in_last_split", "split_boundary_off_by_a_tile",
           "cleared_mask_bit", "set_pad_bit")


def _mm(A, B, engine, order, splits):
    if engine == "exact":
        return acc_exact(A, B, order, splits)
    if engine == "x3":
        return acc_x3(A, B, order, splits)
    return (A.astype(F64) @ B.astype(F64)).astype(F32)          # "ideal": the correctly rounded result


def model_run(sizes, params, x, gout, engine="ideal", order="forward", splits=1, defect=None, layer=None, kchunk=None):
    """One forward + backward of m rows in a model of the kernels (engine "ideal" — float64 rounded once —,
    "exact" or "x3"), each launch consuming what the one before stored, as on the GPU: rb as check_f32_readback
    reads it.  defect at `layer` (DEFECTS; kchunk: the split length of grad_W the split defects refer to):
      lost_last_row                 grad_W and the bias sum lose the last batch row
      lost_last_k                   the last row's forward dot products stop one k early (a row-tail × k-tail path)
      lost_last_k_tile              grad_W and the bias sum lose the last 16 batch rows
      lost_row_in_last_split        … the first row of the last split
      split_boundary_off_by_a_tile  … the 16 rows before the last split's first
      cleared_mask_bit              the forward clears the bit of one live element of the last row
      set_pad_bit                   the forward sets the first pad bit of the last row's last word"""
    L, m = len(sizes) - 1, x.shape[0]
    layers = unpack(sizes, params)
    h = [np.asarray(x, F32)] + [None] * (L - 1)
    bits, y = [None] * L, None
    hit = lambda name, i: defect == name and layer == i
    for i, (W, b) in enumerate(layers):
        v = _mm(h[i], np.ascontiguousarray(W.T), engine, order, splits) + b
        if hit("lost_last_k", i):
            v[m - 1] = _mm(h[i][m - 1:, :-1], np.ascontiguousarray(W[:, :-1].T), engine, order, splits)[0] + b
        if i < L - 1:
            v = np.maximum(v, F32(0))
        if i == L - 1:
            y = v
            break
        words = pack_bits(v > 0)
        if hit("cleared_mask_bit", i):
            col = int(np.flatnonzero(v[m - 1] > 0)[-1])
            words[m - 1, col // 32] &= ~(np.uint32(1) << np.uint32(col % 32))
        if hit("set_pad_bit", i):
            assert sizes[i + 1] % 32, "no pad bits at this width"
            words[m - 1, -1] |= np.uint32(1) << np.uint32(sizes[i + 1] % 32)
        h[i + 1], bits[i + 1] = v, words
    grads, gx = [None] * L, [None] * L
    g = np.asarray(gout, F32)
    for i in range(L - 1, -1, -1):
        W = layers[i][0]
        keep = np.ones(m, bool)
        last0 = ((m - 1) // kchunk) * kchunk if kchunk else 0
        if hit("lost_last_row", i):
            keep[m - 1] = False
        if hit("lost_last_k_tile", i):
            keep[max(0, m - 16):] = False
        if hit("lost_row_in_last_split", i):
            keep[last0] = False
        if hit("split_boundary_off_by_a_tile", i):
            keep[max(0, last0 - 16):last0] = False
        gk, hk = g[keep], h[i][keep]
        gW = _mm(np.ascontiguousarray(gk.T), hk, engine, order, splits)
        gb = _mm(np.ascontiguousarray(gk.T), np.ones((len(gk), 1), F32), engine, order, splits).ravel()
        grads[i] = np.concatenate([gW.ravel(), gb])
        v = _mm(g, W, engine, order, splits)
        gx[i] = v if i == 0 else np.where(unpack_bits(bits[i], sizes[i]), v, F32(0))   # the kernel reads the bits
        g = gx[i]
    return dict(h=h, y=y, bits=bits, gx=gx, grads=np.concatenate(grads).astype(F32))


# ----------------------------------------------------------------------------- reading a network back
def read_f32_layers(lib, nn_ptr, sizes, m):
    """Everything the fp32 kernels stored for the last forward + backward of m rows (check_f32_readback's rb)."""
    import ppo_ffi
    from helpers import nn_grads_packed
    nn = nn_ptr.contents
    L = len(sizes) - 1
    assert nn.dtype == 0 and nn.bits_m == m and nn.act_cap_m >= m
    cap = nn.act_cap_m
    wpr = [(s + 31) // 32 for s in sizes]
    base = C.cast(nn.d_act_bits, C.c_void_p).value
    bits, off = [None] * L, 0
    for i in range(L):                                      # one [cap, ⌈w/32⌉] block per layer input: its first m rows
        if i > 0:
            bits[i] = ppo_ffi.d2h(lib, C.c_void_p(base + 4 * off), np.uint32, m * wpr[i]).reshape(m, wpr[i])
        off += cap * wpr[i]
    rd = lambda p, w: ppo_ffi.d2h(lib, p, F32, m * w).reshape(m, w)
    return dict(h=[None] + [rd(nn.layers[i].d_input, sizes[i]) for i in range(1, L)], y=rd(nn.d_output, sizes[L]),
                bits=bits, grads=nn_grads_packed(lib, nn_ptr), gx=[rd(nn.layers[i].d_grad_x, sizes[i]) for i in range(L)])
