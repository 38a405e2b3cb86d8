"""Both fp32 GEMM engines (csrc/gemm.hip, csrc/gemm_x3.hip) launch by launch and element by element, at the smallest
shapes that have every kind of tail — f32_gemm_ref.check_f32_readback (the bounds, the chain lengths c and the probes
are in f32_gemm_ref.py; test_f32_gemm_ref_cpu.py shows on the CPU that they admit both engines' fp32 accumulations
and reject each tail defect).

Each network is built with create_neural_network and runs forward_propagation_cuda + backward_propagation_cuda
under every forced tile configuration, the automatic choice and several split-K targets; after each pass everything
the launches stored is read back (every activation, the ReLU′ words, every layer's grad_x, the packed gradients)
and every launch is checked from the GPU's own operands: random inputs scaled by 2^-6 … 2^6 per row and per unit
(bound (a)), the one-term probes (b) and the integer probes (c).

Exact engine (ppo_gemm_f32_engine(0)), networks × batches 1, 33, 200, 300, 1100:
  [3, 33, 65, 1]       nothing a multiple of 4: scalar loaders; one past the 32- and 64-wide tiles and bit words
  [17, 40, 72, 6]      layer 0 scalar; 40 and 72 vector widths with a k tail inside a k-tile and partial bit words
  [130, 264, 136, 17]  264 = 256 + 8 and 136 = 128 + 8: a vector column tail past the widest tiles; 130 scalar
  [64, 128, 256, 8]    everything aligned
  [40, 24]             one layer: unmasked grad_x, no hidden activation
  cfg 0–10 forced      every launch on gemm_f32_kernel at that cfg's tile (kCfgs), VEC where n, l % 4 = 0, else scalar;
                       grad_W with the default split target (1024): 1 split up to m = 255, 2 at m = 300, up to 8 at 1100
  automatic            pick_cfg: 10 / 2 for the ≤ 32-wide outputs, 3 for M ≤ 32, 4 where an extent ≤ 64, else 5; the
                       small-M forward / grad_x kernel where m ≤ 1024 and K ≥ 64 (use_smallm: all of [64, 128, 256, 8],
                       layers 1, 2 of [17, …], layers 0–2 of [130, …], layers 1, 2 of [3, …] at every m but 1100); the
                       small-M grad_W kernel at m = 200 where ⌈l/32⌉·⌈n/32⌉ ≥ 16 (use_smallm_w: the hidden layers of
                       [130, …] and [64, …]); m ≤ 128 grad_W on cfg 4 without a split
  split targets        default; 1 (the deterministic request: one split); 4096 with the automatic choice and cfg 0
                       and 4: as many splits as 8 k-tiles each allow — 2 at m = 300 (160 + 140 rows), 8 at m = 1100
                       (7 × 144 + 92), the last one partial (f32 atomics)
x3 engine (ppo_gemm_f32_engine(1)), batches 1025 and 1100 (a one-row and a 76-row tail past 1024):
  [36, 68, 132, 260, 4]  each hidden width one float4 past a 64-, 128-, 256-wide tile; every bit word partial; the
                         4-wide output layer runs the exact engine (use_x3_layer: widths > 32)
  [64, 128, 256, 8]      aligned
  cfg 0–6 forced       launch_tile_x3: 0 256×256, 1 128×128 (4 waves), 2 128×128 (8 waves), 3 128×128 — grad_W with
                       two k-groups —, 4 64×64, 5 256×128, 6 64×64 with 32-k tiles; forward with bias + ReLU + bits,
                       grad_x with the mask words, grad_W with the bias sums
  automatic            pick_x3: cfg 4 for forward and grad_x (fewer than 256 tiles of 128×128), cfg 3 for grad_W
  grad_W modes         (X3_GRADW_MODES, checked against the host's arithmetic on the CPU) MLP backward, default target:
                       4 or 8 slabs, the reduce carried by the following grad_x; target 1: one split; through
                       mat_mul_backwards_cuda (no grad_x to ride on): (1100, 36, 68) 4 slabs + slab_reduce_kernel<4>,
                       (18145, 36, 68) 64 slabs with a one-row last split + slab_reduce_kernel<16>, (2340, 36, 68)
                       with target 2: two splits of 1184 > 1024 rows, f32 atomics
  narrow products      mat_mul_cuda / mat_mul_backwards_cuda at (1025, 4, 8) and (1025, 36, 4): x3 at widths ≤ 32
x3 against the exact engine: test_x3_rms_against_exact.

Value-head fold (test_value_fold_every_cfg): one value step of ppo_update, N = B = 1100, value network
  [36, 68, 132, 1]: layer 1's forward on the FOLD forward kernels (the partial dots of h·w in the epilogue), the head
  carried by its grad_W launch (y, g), its grad_W / bias gradient / the output layer's gW on the FOLD grad_W kernels
  (the 0/1 mask as the A operand, 4 or 8 slabs, the reduce carried by grad_x), its grad_x on the FOLD grad_x kernels
  (A from the mask words, W scaled by w as it is staged); layer 0 on the plain x3 kernels with the fused gather.

Measured on an MI355X (worst err / bound per product, tallied by the engine that ran the launch — under the x3
setting the 4- and 8-wide output layers run the exact kernels and count there; printed at the end of the run):
  exact           forward 0.107   grad_x 0.199   grad_W 0.174   bias gradient 0.048
  x3              forward 0.074   grad_x 0.088   grad_W 0.002   bias gradient 0.0003
  x3 value fold   forward 0.022   grad_x 0.003   grad_W 0.0004  bias gradient 0.0002   (g: within 6·2^-24·|g|)
(x3's largest figures come from the narrow products at K = 4 and 8, where c is smallest.  c counts every k of an MFMA
as one rounding, so a correct kernel uses a fifth of the exact bound and a tenth or less of x3's; the probes, not
the bound, are what sees one lost plane product.)
RMS of err / Σ|terms|, x3 (each forced cfg) over the exact engine, at the hidden layers' shapes with m = 1100 — the
asserted ratios (grad_W at equal chain length: 144 rows per accumulator for cfg 0–5, 288 for cfg 6):
  cfg 0, 1, 2, 4, 5   forward 0.922   grad_x 0.899   grad_W 0.837
  cfg 3               forward 0.922   grad_x 0.899   grad_W 0.828
  cfg 6               forward 0.949   grad_x 0.920   grad_W 0.810
cfg 6's grad_W against the exact engine's default 144-row chains: 1.108–1.117 over two runs (split-K atomics make
the exact figure vary), above 1.1 — its own chains are twice as long; not asserted, printed by the test.
"""
import numpy as np
import pytest

import f32_gemm_ref as R
import ppo_ffi
from helpers import F32, dev, empty, nn_set_params_packed

pytestmark = pytest.mark.gpu
ids = lambda s: "-".join(map(str, s)) if isinstance(s, list) else str(s)
FILE_WORST = {}


@pytest.fixture(scope="module")
def engines(lib):
    """(exact cfgs, x3 cfgs); every setter restored"""
    old = lib.ppo_gemm_f32_engine(-1)
    flags = lib.ppo_gemm_flags(-1)
    n0, n1 = lib.ppo_gemm_tune(-1, 0), lib.ppo_gemm_x3_tune(-1, 0)
    yield n0, n1
    lib.ppo_gemm_tune(-1, 0)
    lib.ppo_gemm_x3_tune(-1, 0)
    lib.ppo_gemm_flags(flags)
    lib.ppo_gemm_f32_engine(old)
    for eng, t in FILE_WORST.items():
        print(f"\nfp32 kernels, {eng}: worst err / bound over the file: {t.line()}")


def _tally(engine, t):
    FILE_WORST.setdefault(engine, R.Tally()).merge(t)


def _mlp_runs(lib, sizes, m, engine, runs, tune):
    """every run of `runs` (cfg, split target) on the scaled random inputs, the one-term probes and the integer
    probes; each launch checked from the GPU's own operands"""
    L = len(sizes) - 1
    x3 = [R.x3_layer(engine, m, sizes[i], sizes[i + 1]) for i in range(L)]
    parts = R.max_splits(m)
    chains = lambda i, op, K: (R.chain_x3 if x3[i] else R.chain_exact)(K, parts)
    probe = lambda i: R.X3_ONE_TERM if x3[i] else 0.0
    kchunks = {R.exact_gradw_splits(m, n, l, -1, t)[1] for n, l in zip(sizes[:-1], sizes[1:]) for t in (0, R.SPLIT_TARGET)}
    kchunks |= {R.x3_gradw_mode(m, n, l, c, 0)[0] for n, l in zip(sizes[:-1], sizes[1:]) for c in (3, 4)}
    rows = R.probe_rows(m, sorted(kchunks))
    reps = min(4, -(-len(rows) // sizes[-1]))
    cases = [("random", R.make_case(sizes, m), {})]
    cases += [(f"one-term {r}", R.make_oneterm_case(sizes, m, rows, r), dict(probe=probe)) for r in range(reps)]
    cases += [("integer", R.make_int_case(sizes, m), dict(exact=True))]
    nn = lib.create_neural_network(ppo_ffi.c_ints(sizes), ppo_ffi.c_strings(["relu"] * (L - 1) + ["none"]), len(sizes))
    name = "x3" if engine else "exact"
    worst = R.Tally()
    old = lib.ppo_gemm_f32_engine(engine)
    try:
        for kind, (params, x, gout), kw in cases:
            nn_set_params_packed(lib, nn, params)
            dx, dgo = dev(lib, x), dev(lib, gout)
            try:
                for c, target in runs:
                    tune(c, target)
                    lib.forward_propagation_cuda(nn, dx.ptr, m)
                    lib.backward_propagation_cuda(nn, dgo.ptr, m)
                    rb = R.read_f32_layers(lib, nn, sizes, m)
                    t = R.check_f32_readback(sizes, params, x, gout, rb, chains,
                                             f"{name} {sizes} m={m} cfg {c} target {target} {kind}",
                                             engine_of=lambda i: "x3" if x3[i] else "exact", **kw)
                    if kind == "random":
                        worst.merge(t)
                        for eng, te in t.by.items():
                            _tally(eng, te)
            finally:
                dx.free()
                dgo.free()
    finally:
        tune(-1, 0)
        lib.ppo_gemm_f32_engine(old)
        lib.free_neural_network(nn)
    print(f"WORST {name} {sizes} m={m}: {worst.line()}")


@pytest.mark.parametrize("m", R.EXACT_BATCHES)
@pytest.mark.parametrize("sizes", R.EXACT_NETWORKS, ids=ids)
def test_exact_kernels_every_cfg(lib, engines, sizes, m):
    runs = [(c, 0) for c in range(engines[0])] + [(-1, 0), (-1, 1), (-1, R.SPLIT_TARGET), (0, R.SPLIT_TARGET),
                                                  (4, R.SPLIT_TARGET)]
    _mlp_runs(lib, sizes, m, 0, runs, lib.ppo_gemm_tune)


@pytest.mark.parametrize("m", R.X3_BATCHES)
@pytest.mark.parametrize("sizes", R.X3_NETWORKS, ids=ids)
def test_x3_kernels_every_cfg(lib, engines, sizes, m):
    runs = [(c, 0) for c in range(-1, engines[1])] + [(-1, 1), (3, 1), (3, 2)]
    _mlp_runs(lib, sizes, m, 1, runs, lib.ppo_gemm_x3_tune)


# ----------------------------------------------------------------------------- the reference-API products
def _product_cases(m, n, l, rows):
    rng = np.random.default_rng(m + 13 * n + 29 * l)
    sc = lambda k: 2.0 ** rng.integers(-6, 7, k)
    out = []
    sx, sg, sw = sc(m), sc(m), sc(l)
    sx[-1] = sg[-1] = sw[-1] = 2.0 ** -6
    out.append(("random", ((rng.uniform(-1, 1, (m, n)) * sx[:, None]).astype(F32),
                           (rng.uniform(-1, 1, (l, n)) / np.sqrt(n) * sw[:, None]).astype(F32),
                           (rng.uniform(-0.5, 0.5, l) * sw).astype(F32),
                           (rng.uniform(-1, 1, (m, l)) * sg[:, None]).astype(F32)), {}))
    W = np.zeros((l, n), F32)
    W[np.arange(l), np.arange(l) % n] = R.full_mantissa(rng, l) * np.where(np.arange(l) % 3, 1, -1)
    for rep in range(-(-len(rows) // l)):
        g = np.zeros((m, l), F32)
        g[np.asarray(rows)[(np.arange(l) + rep * l) % len(rows)], np.arange(l)] = R.full_mantissa(rng, l)
        out.append((f"one-term {rep}", (R.full_mantissa(rng, (m, n)), W, np.zeros(l, F32), g), "probe"))
    ints = lambda shape: rng.integers(-8, 9, shape).astype(F32)
    out.append(("integer", (ints((m, n)), ints((l, n)), ints(l), ints((m, l))), dict(exact=True)))
    return out


def _products(lib, x, W, b, g):
    m, n = x.shape
    l = W.shape[0]
    dx, dW, db, dg = dev(lib, x), dev(lib, W), dev(lib, b), dev(lib, g)
    dy, dgx, dgW = empty(lib, m * l), empty(lib, m * n), empty(lib, l * n)
    try:
        lib.mat_mul_cuda(None, dy.ptr, dx.ptr, dW.ptr, db.ptr, m, n, l)
        lib.mat_mul_backwards_cuda(None, dgx.ptr, dgW.ptr, dg.ptr, dx.ptr, dW.ptr, m, n, l)
        return (dy.to_numpy(F32, m * l).reshape(m, l), dgx.to_numpy(F32, m * n).reshape(m, n),
                dgW.to_numpy(F32, l * n).reshape(l, n))
    finally:
        for d in (dx, dW, db, dg, dy, dgx, dgW):
            d.free()


X3_PRODUCTS = [(1100, 36, 68, [(3, 0)]), (18145, 36, 68, [(3, 0)]), (2340, 36, 68, [(3, 2)]),
               (1025, 4, 8, None), (1025, 36, 4, None)]


@pytest.mark.parametrize("m,n,l,runs", X3_PRODUCTS, ids=lambda v: str(v) if isinstance(v, int) else "")
def test_x3_products(lib, engines, m, n, l, runs):
    """mat_mul_cuda / mat_mul_backwards_cuda on x3: grad_W's standalone reduces and atomics (runs given: the cfg and
    split target of X3_GRADW_MODES) and the widths ≤ 32 the MLP route never gives x3 (every cfg and the automatic)"""
    assert R.x3_product(1, m, n, l)
    if runs is None:
        runs = [(c, 0) for c in range(-1, engines[1])]
    kchunks = {R.x3_gradw_mode(m, n, l, c, t)[0] for c, t in runs}
    c_of = lambda op, K: R.chain_x3(K, R.max_splits(m))
    worst = R.Tally()
    old = lib.ppo_gemm_f32_engine(1)
    try:
        for kind, (x, W, b, g), kw in _product_cases(m, n, l, R.probe_rows(m, sorted(kchunks))):
            for c, target in runs:
                lib.ppo_gemm_x3_tune(c, target)
                y, gx, gW = _products(lib, x, W, b, g)
                kw_ = dict(probe=R.X3_ONE_TERM) if kw == "probe" else kw
                t = R.check_product(x, W, b, g, y, gx, gW, c_of, f"x3 product ({m}, {n}, {l}) cfg {c} target {target} {kind}",
                                    **kw_)
                if kind == "random":
                    worst.merge(t)
    finally:
        lib.ppo_gemm_x3_tune(-1, 0)
        lib.ppo_gemm_f32_engine(old)
    _tally("x3", worst)


RMS_SHAPES = [(1100, 36, 68), (1100, 68, 132), (1100, 132, 260), (1100, 64, 128), (1100, 128, 256)]


def test_x3_rms_against_exact(lib, engines):
    """On the same scaled random inputs, the RMS of err / Σ|terms| of every x3 configuration may not exceed the
    exact engine's by more than 10 % (the margin of test_x3_as_accurate_as_exact_fp32), per product, over the hidden
    layers' shapes at m = 1100.  Forward and grad_x: against the exact engine's automatic choice.  grad_W: against
    the exact engine splitting the batch into ranges as long as the x3 configuration gives one accumulator (its
    kchunk over its k-groups) — cfg 0–5 sum 144 rows per accumulator, which is also the exact engine's default at
    m = 1100; cfg 6 (32-k tiles, one k-group, never the automatic choice for grad_W) sums 288, and against the
    exact engine's 144-row chains its ratio is 1.108: twice the chain, √2 × 0.83 ≈ 1.17 expected — the effect
    pick_x3's comment records for cfg 2.  At equal chain length the header's statement holds for it as well.
    Measured ratios: the module docstring."""
    cases = [(s, _product_cases(*s, [0])[0][1]) for s in RMS_SHAPES]

    def sweep(what, chain=0):
        t = R.Tally()
        for (m, n, l), (x, W, b, g) in cases:
            target = 0
            if chain:                                       # the exact engine with kchunk = chain
                cfg = R.exact_gradw_splits(m, n, l)[0]
                target = -(-m // chain) * -(-l // R.EXACT_CFGS[cfg][0]) * -(-n // R.EXACT_CFGS[cfg][1])
                assert R.exact_gradw_splits(m, n, l, -1, target)[1] == chain
                lib.ppo_gemm_tune(-1, target)
            y, gx, gW = _products(lib, x, W, b, g)
            c_of = lambda op, K: R.chain_x3(K, R.max_splits(m))
            t.merge(R.check_product(x, W, b, g, y, gx, gW, c_of, f"{what} ({m}, {n}, {l})"))
        return t
    chain_of = lambda c: {R.x3_gradw_mode(m, n, l, c, 0)[0] // R.X3_CFGS[c][2] for m, n, l in RMS_SHAPES}
    old = lib.ppo_gemm_f32_engine(0)
    try:
        lib.ppo_gemm_tune(-1, 0)
        exact = {0: sweep("exact")}
        for c in range(engines[1]):
            (chain,) = chain_of(c)
            if chain not in exact:
                exact[chain] = sweep(f"exact, {chain}-row splits", chain)
        lib.ppo_gemm_tune(-1, 0)
        lib.ppo_gemm_f32_engine(1)
        ratios = {}
        for c in range(engines[1]):
            lib.ppo_gemm_x3_tune(c, 0)
            t = sweep(f"x3 cfg {c}")
            (chain,) = chain_of(c)
            ratios[c] = {k: t.rms(k) / exact[0].rms(k) for k in ("forward", "grad_x")}
            ratios[c]["grad_W"] = t.rms("grad_W") / exact[chain].rms("grad_W")
            print(f"x3 cfg {c} RMS err / Σ|terms| over exact: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios[c].items())
                  + f" (grad_W at {chain}-row chains; over the exact default {t.rms('grad_W') / exact[0].rms('grad_W'):.3f})")
    finally:
        lib.ppo_gemm_tune(-1, 0)
        lib.ppo_gemm_x3_tune(-1, 0)
        lib.ppo_gemm_f32_engine(old)
    for c, r in ratios.items():
        for k, v in r.items():
            assert v <= 1.1, f"x3 cfg {c} {k}: RMS error {v:.3f} of the exact engine's"


# ----------------------------------------------------------------------------- the value-head fold
def _check_value_fold(lib, oracle, ppo, N, B, seed, v0, what):
    """Everything one folded value step stored, element by element from the GPU's own operands (module docstring of
    f32_gemm_ref.py for c; + 2 for the two scale multiplications of the folded products)."""
    import ctypes as C
    from bf16_ref import unpack
    from helpers import nn_grads_packed, nn_input_rows
    F64 = np.float64
    V = ppo.contents.V
    nn = V.contents
    sizes = [36, 68, 132, 1]
    m, parts = B, R.max_splits(B)
    b = ppo.contents.buffer.contents
    rows = oracle.feistel_perm(N, oracle.splitmix64(seed))[:B]
    assert len(set(rows.tolist())) == B
    state = ppo_ffi.d2h(lib, b.d_state_p, F32, N * sizes[0]).reshape(N, sizes[0])
    x = nn_input_rows(lib, V, m)
    np.testing.assert_array_equal(x, state[rows])
    tgt = ppo_ffi.d2h(lib, b.d_adv_target_p, F32, N)[rows].astype(F64)
    assert nn.fold_ws_cap > 0 and nn.bits_m == m, "the value step did not take the fold"
    (W0, b0), (W1, b1), (w, bo) = unpack(sizes, v0)
    rd = lambda p, r, c: ppo_ffi.d2h(lib, p, F32, r * c).reshape(r, c)
    h1, h2 = rd(nn.layers[1].d_input, m, 68), rd(nn.layers[2].d_input, m, 132)
    y = ppo_ffi.d2h(lib, nn.d_output, F32, m)
    mp, slots_max = (m + 3) & ~3, 2 * ((132 + 63) // 64)              # nn_value_fold_step's workspace layout
    g = ppo_ffi.d2h(lib, C.c_void_p(C.cast(nn.d_fold_ws, C.c_void_p).value + 4 * slots_max * mp), F32, m)
    gx1 = rd(nn.layers[1].d_grad_x, m, 68)
    grads = nn_grads_packed(lib, V)
    cap, base = nn.act_cap_m, C.cast(nn.d_act_bits, C.c_void_p).value
    wpr = [(s + 31) // 32 for s in sizes]
    bits1 = ppo_ffi.d2h(lib, C.c_void_p(base + 4 * cap * wpr[0]), np.uint32, m * wpr[1]).reshape(m, wpr[1])
    bits2 = ppo_ffi.d2h(lib, C.c_void_p(base + 4 * cap * (wpr[0] + wpr[1])), np.uint32, m * wpr[2]).reshape(m, wpr[2])
    t = R.Tally()
    cx = lambda K: R.chain_x3(K, parts)
    # forward: layer 0 (x3, fused gather), layer 1 (x3 FOLD forward), the ReLU′ words of both
    want, sa = R.layer_forward(x, W0, b0, True)
    t.add("forward", R.check_elements(h1, want, sa, cx(36), f"{what} forward layer 0"))
    want, sa = R.layer_forward(h1, W1, b1, True)
    t.add("forward", R.check_elements(h2, want, sa, cx(68), f"{what} forward layer 1 (fold)"))
    R.check_bits(bits1, h1, f"{what} ReLU′ bits of layer 0")
    R.check_bits(bits2, h2, f"{what} ReLU′ bits of layer 1")
    # y = h·w + b: each wave's products and sums over its columns, a 32-lane tree, the slots' sum, the bias — under
    # the exact engine's count for K = 132
    want, sa = R.layer_forward(h2, w, bo, False)
    t.add("forward", R.check_elements(y.reshape(m, 1), want, sa, R.chain_exact(132), f"{what} y"))
    # g = 2(y − t)/B from the stored y: one subtraction and one division (≤ 2.5 ulp): 6·2^-24·|g|
    gw_ = 2.0 * (y.astype(F64) - tgt) / B
    err = np.abs(g - gw_)
    assert (err <= 6 * R.U * np.abs(gw_)).all(), f"{what} g: worst err / |g| {float((err / np.abs(gw_)).max()):.3g}"
    mask = (h2 > 0).astype(F64)
    g64, w64 = g.astype(F64), w.astype(F64).ravel()
    off = [0, 36 * 68, 36 * 68 + 68, 36 * 68 + 68 + 68 * 132, 36 * 68 + 68 + 68 * 132 + 132, 36 * 68 + 68 + 68 * 132 + 132 + 132]
    gW0, gb0, gW1, gb1, gWo = (grads[a:z] for a, z in zip(off[:-1], off[1:]))
    gbo = grads[off[-1]:]
    # hidden layer (fold): gW = diag(w)·maskᵀ·diag(g)·h1, gb = diag(w)·maskᵀ·g
    A = mask * g64[:, None]
    want = w64[:, None] * (A.T @ h1.astype(F64))
    sa = np.abs(w64)[:, None] * (np.abs(A).T @ np.abs(h1).astype(F64))
    t.add("grad_W", R.check_elements(gW1.reshape(132, 68), want, sa, cx(m), f"{what} grad_W layer 1 (fold)", extra=2))
    t.add("bias", R.check_elements(gb1, w64 * A.sum(axis=0), np.abs(w64) * np.abs(A).sum(axis=0), cx(m),
                                   f"{what} bias gradient layer 1 (fold)", extra=2))
    # output layer: gW = Σ g·h2 (one product rounding per term), gb = Σ g
    t.add("grad_W", R.check_elements(gWo, g64 @ h2.astype(F64), np.abs(g64) @ np.abs(h2).astype(F64), cx(m),
                                     f"{what} grad_W output layer", extra=2))
    t.add("bias", R.check_elements(gbo, np.array([g64.sum()]), np.array([np.abs(g64).sum()]), cx(m),
                                   f"{what} bias gradient output layer"))
    # hidden grad_x (fold): diag(g)·(mask·diag(w)·W1) ⊙ (h1 > 0)
    want = np.where(h1 > 0, g64[:, None] * ((mask * w64) @ W1.astype(F64)), 0.0)
    sa = np.where(h1 > 0, np.abs(g64)[:, None] * ((mask * np.abs(w64)) @ np.abs(W1).astype(F64)), 0.0)
    t.add("grad_x", R.check_elements(gx1, want, sa, cx(132), f"{what} grad_x layer 1 (fold)", extra=2))
    # layer 0 from the stored grad_x
    gW, saW, gb, sab = R.layer_grad_w(gx1, x)
    t.add("grad_W", R.check_elements(gW0.reshape(68, 36), gW, saW, cx(m), f"{what} grad_W layer 0"))
    t.add("bias", R.check_elements(gb0, gb, sab, cx(m), f"{what} bias gradient layer 0"))
    print(f"{what}: worst err / bound {t.line()}")
    return t


def test_value_fold_every_cfg(lib, oracle, engines, monkeypatch):
    """One value step of ppo_update (N = B = 1100, value network [36, 68, 132, 1], PPO_VALUE_FOLD at its default)
    under every forced x3 configuration and the automatic choice: y, g on the Feistel rows, the hidden layer's
    gW / gb / grad_x through the FOLD kernels, the output layer's gW and gb, layer 0's — every value from the
    GPU's own stored h, mask, y and g."""
    import ctypes as C
    from helpers import nn_params_packed
    monkeypatch.delenv("PPO_VALUE_FOLD", raising=False)
    monkeypatch.setenv("PPO_NO_TINY", "1")                  # the multi-launch loop, whatever the cluster phase takes
    sizes, N, B, seed = [36, 68, 132, 4], 1100, 1100, 11
    worst = R.Tally()
    old = lib.ppo_gemm_f32_engine(1)
    try:
        for c in range(-1, engines[1]):
            C.CDLL("libc.so.6").srand(31)
            ppo = lib.create_ppo(ppo_ffi.c_strings(["relu", "relu", "none"]), ppo_ffi.c_ints(sizes), len(sizes), N, 3e-4,
                                 3e-4, 0.95, 0.2, 0.0, 1.0, True)
            try:
                assert lib.ppo_get_max_grad_norm(ppo) == 0
                lib.ppo_fill_synthetic(ppo, 4, N // 4, 5, 1.0 / 200)
                lib.ppo_set_step_limit(ppo, 1, 0)
                v0 = nn_params_packed(lib, ppo.contents.V)
                lib.ppo_gemm_x3_tune(c, 0)
                lib.ppo_update(ppo, 0.99, B, 0, 1, 1, seed)
                lib.ppo_synchronize()
                assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()
                worst.merge(_check_value_fold(lib, oracle, ppo, N, B, seed, v0, f"value fold cfg {c}"))
            finally:
                lib.ppo_set_step_limit(ppo, -1, -1)
                lib.free_ppo(ppo)
    finally:
        lib.ppo_gemm_x3_tune(-1, 0)
        lib.ppo_gemm_f32_engine(old)
    print(f"WORST value fold: {worst.line()}")
    _tally("x3 value fold", worst)
