"""f32_gemm_ref.py pinned on the CPU: the fp32 models of both engines' accumulations stay inside the per-element
bound at every network and batch of test_gpu_f32_kernels.py; each injected defect is rejected by the bound, the
one-term probes or the integer probes, while the lost-row and lost-k defects pass helpers.gemm_tol (the older
max-norm check) on the same data; the plane-product model behind the x3 one-term bound 2^-21; the premise of the
integer probes; the host arithmetic that picks the GPU test's grad_W modes."""
import numpy as np
import pytest

import f32_gemm_ref as R
from bf16_ref import unpack
from helpers import gemm_tol

F32, F64 = np.float32, np.float64
ids = lambda s: "-".join(map(str, s)) if isinstance(s, list) else str(s)


def _chains(fn):
    return lambda i, op, K: fn(K, 3)


@pytest.mark.parametrize("m", R.EXACT_BATCHES)
@pytest.mark.parametrize("sizes", R.EXACT_NETWORKS, ids=ids)
def test_exact_model_inside_bound(sizes, m):
    params, x, gout = R.make_case(sizes, m)
    for order in ("forward", "reverse", "split"):
        rb = R.model_run(sizes, params, x, gout, engine="exact", order=order, splits=3)
        t = R.check_f32_readback(sizes, params, x, gout, rb, _chains(R.chain_exact), f"exact model {order} {sizes} m={m}")
        assert max(t.worst.values()) <= 1.0


@pytest.mark.parametrize("m", R.X3_BATCHES)
@pytest.mark.parametrize("sizes", R.X3_NETWORKS, ids=ids)
def test_x3_model_inside_bound(sizes, m):
    params, x, gout = R.make_case(sizes, m)
    for order in ("forward", "reverse", "split"):
        rb = R.model_run(sizes, params, x, gout, engine="x3", order=order, splits=3)
        t = R.check_f32_readback(sizes, params, x, gout, rb, _chains(R.chain_x3), f"x3 model {order} {sizes} m={m}")
        assert max(t.worst.values()) <= 1.0


def test_zero_preactivations_exist():
    """the generator's exact zeros: a zero row of x under zero biases clears the bit (mask = z > 0)"""
    sizes, m = [17, 40, 72, 6], 33
    params, x, gout = R.make_case(sizes, m)
    rb = R.model_run(sizes, params, x, gout)
    assert (x[m // 2] == 0).all() and (rb["h"][1][m // 2, 1:3] == 0).all()
    assert not R.unpack_bits(rb["bits"][1], sizes[1])[m // 2, 1:3].any()
    z = x.astype(F64) @ unpack(sizes, params)[0][0].astype(F64).T
    assert (z[m // 2] == 0).all()


# ----------------------------------------------------------------------------- defects
SIZES, M, LAYER = [130, 264, 136, 17], 300, 0
KCHUNK = R.exact_gradw_splits(M, SIZES[LAYER], SIZES[LAYER + 1])[1]


def _rejects(make, defect, chain, **kw):
    params, x, gout = make
    rb = R.model_run(SIZES, params, x, gout, defect=defect, layer=LAYER, kchunk=KCHUNK)
    try:
        R.check_f32_readback(SIZES, params, x, gout, rb, _chains(chain), f"{defect}", **kw)
    except AssertionError:
        return True, rb
    return False, rb


# Which check rejects which defect at this shape.  The probes reject every defect under either engine's rules: the
# integer probes every lost term, the one-term probes every lost term that a probe row carries (probe_rows: the
# last row and the rows around the split boundary); the bit words reject both bit defects on any data.  The bound
# on the scaled random data rejects a defect wherever some output's lost terms are not small next to c·2^-24 of
# its own Σ|terms|: with the exact engine's c (≈ K) all seven; with x3's c (≈ 6·K) not the lost last batch row, whose
# scale is the smallest of the 300 (2^-6: its terms are below 6·300·2^-24 of every Σ|terms|) — on x3 only the probes
# see that one.  (The lost row in the last split has a drawn scale, large enough here for either bound.)
BOUND_MISSES = {"exact": (), "x3": ("lost_last_row",)}


@pytest.mark.parametrize("engine", ["exact", "x3"])
@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defect_rejected(defect, engine):
    assert KCHUNK < M, "the split defects need several splits"
    chain = R.chain_exact if engine == "exact" else R.chain_x3
    one = 0.0 if engine == "exact" else R.X3_ONE_TERM
    rows = R.probe_rows(M, [KCHUNK])
    data = {"bound": (R.make_case(SIZES, M), {}),
            "one_term": (R.make_oneterm_case(SIZES, M, rows), dict(probe=lambda i: one)),
            "integer": (R.make_int_case(SIZES, M), dict(exact=True))}
    got = {}
    for name, (make, kw) in data.items():
        clean, _ = _rejects(make, None, chain, **kw)
        assert not clean, f"{name}: the defect-free model is rejected"
        got[name], rb = _rejects(make, defect, chain, **kw)
        if name == "bound" and defect in ("lost_last_row", "lost_last_k"):
            # the older check on the same data, as the suite applies it: assert_gemm_close on one product's output
            # (forward, grad_W: the reference-API tests) and on the whole packed gradient (the MLP tests, the only
            # place the bias gradient meets it) — both defects pass each; the bias block on its own is printed
            params, x, gout = make
            ref = R.model_run(SIZES, params, x, gout)
            n, l = SIZES[LAYER], SIZES[LAYER + 1]
            off = sum(a * b + b for a, b in zip(SIZES[:LAYER], SIZES[1:LAYER + 1]))
            blocks = ((rb["h"][LAYER + 1], ref["h"][LAYER + 1], n, "forward"),
                      (rb["grads"][off:off + l * n], ref["grads"][off:off + l * n], M, "grad_W"),
                      (rb["grads"], ref["grads"], M, "packed gradient"))
            gb, gb_ref = (r["grads"][off + l * n:off + l * n + l] for r in (rb, ref))
            print(f"{defect} bias block alone (no check of the suite): max-norm err / tol "
                  f"{float(np.abs(gb.astype(F64) - gb_ref).max()) / gemm_tol(gb_ref, M):.3g}")
            changed = False
            for a, b, K, prod in blocks:
                err = float(np.abs(a.astype(F64) - b).max())
                changed |= err > 0
                assert err <= gemm_tol(b, K), f"{defect}: the max-norm check sees it ({err:.3g} vs {gemm_tol(b, K):.3g})"
                print(f"{defect} {prod}: max-norm err / tol {err / gemm_tol(b, K):.3g} (passes)")
            assert changed
    print(f"{defect} under the {engine} rules: rejected by {[k for k, v in got.items() if v]}")
    assert got["one_term"] and got["integer"], f"{defect}: the probes do not reject it"
    assert got["bound"] == (defect not in BOUND_MISSES[engine]), f"{defect}: bound {got['bound']}"


# ----------------------------------------------------------------------------- the x3 plane-product model
def test_x3_plane_product_model():
    """2 000 000 random pairs with full mantissas, the six kept plane products added to zero in all 720 orders:
    no element beyond 2^-21·|a·b| (worst 2^-21.72); with any one kept product dropped most elements are."""
    rng = np.random.default_rng(2)
    a, b = R.full_mantissa(rng, 2_000_000), R.full_mantissa(rng, 2_000_000)
    b *= np.where(rng.random(b.shape) < 0.5, -1, 1).astype(F32)
    for v in (a, b):
        p = R.split3(v)
        assert ((p[0].astype(F64) + p[1] + p[2]) == v).all(), "the three-plane split is not exact"
    rel = R.x3_product_model(a, b)
    worst = float(rel.max())
    print(f"x3 one product, 720 orders: worst relative error 2^{np.log2(worst):.2f}")
    assert (rel <= R.X3_ONE_TERM).all()
    assert 2.0 ** -22.5 < worst < 2.0 ** -21.5
    n = 200_000
    for drop in range(6):
        kept = tuple(k for i, k in enumerate(R.X3_KEPT) if i != drop)
        rel = R.x3_product_model(a[:n], b[:n], kept=kept, orders=[tuple(range(5)), tuple(range(4, -1, -1))])
        frac = float((rel > R.X3_ONE_TERM).mean())
        print(f"without plane product {R.X3_KEPT[drop]}: {100 * frac:.1f} % beyond 2^-21")
        assert frac > 0.7


def test_one_term_probe_on_the_models():
    """the probe rules on both accumulation models: bit for bit on the exact one, 2^-21 on x3; and a doubled
    plane product on x3 is rejected"""
    sizes, m = [36, 68, 132, 4], 40
    make = R.make_oneterm_case(sizes, m, R.probe_rows(m, [16]))
    rb = R.model_run(sizes, *make, engine="exact")
    t = R.check_f32_readback(sizes, *make, rb, _chains(R.chain_exact), "one-term exact", probe=lambda i: 0.0)
    assert t.n["grad_W"] > 0
    rb = R.model_run(sizes, *make, engine="x3", order="reverse")
    R.check_f32_readback(sizes, *make, rb, _chains(R.chain_x3), "one-term x3", probe=lambda i: R.X3_ONE_TERM)
    with pytest.raises(AssertionError):                     # x3 is not bit exact: the exact rule must see that
        R.check_f32_readback(sizes, *make, rb, _chains(R.chain_x3), "one-term x3 as exact", probe=lambda i: 0.0)
    params, x, gout = make
    W0 = unpack(sizes, params)[0][0]
    y = R.acc_x3(x, np.ascontiguousarray(W0.T), kept=R.X3_KEPT + ((1, 1),))
    want, sa = R.layer_forward(x, W0, None, False)
    with pytest.raises(AssertionError):
        R.check_elements(y, want, sa, R.chain_x3(36), "doubled (1,1)", terms=R._terms(x, W0.T), one_term=R.X3_ONE_TERM)


# ----------------------------------------------------------------------------- the integer probes' premise
@pytest.mark.parametrize("sizes,m", [(s, m) for s in R.EXACT_NETWORKS for m in R.EXACT_BATCHES] +
                         [(s, m) for s in R.X3_NETWORKS for m in R.X3_BATCHES], ids=ids)
def test_integer_premise(sizes, m):
    params, x, gout = R.make_int_case(sizes, m)
    assert np.abs(x).max() <= 8 and np.abs(gout).max() <= 8 and np.abs(unpack(sizes, params)[0][0]).max() <= 8
    big, op = R.int_premise(sizes, params, x, gout)
    print(f"{sizes} m={m}: largest Σ|terms| 2^{np.log2(max(big, 1)):.1f}, largest operand 2^{np.log2(max(op, 1)):.1f}")
    assert big < 2 ** 24 and op < 2 ** 16


def test_integer_models_exact():
    sizes, m = [36, 68, 132, 260, 4], 70
    make = R.make_int_case(sizes, m)
    for engine in ("exact", "x3"):
        for order in ("forward", "reverse", "split"):
            rb = R.model_run(sizes, *make, engine=engine, order=order, splits=3)
            R.check_f32_readback(sizes, *make, rb, _chains(R.chain_x3), f"integer {engine} {order}", exact=True)


# ----------------------------------------------------------------------------- grad_W modes of the GPU test
def test_gradw_modes_reached():
    """the (m, n, l, cfg, split target) the GPU test uses for each x3 grad_W mode, from the host's arithmetic"""
    G = R
    seen = set()
    for (m, n, l, cfg, target, defer), mode in G.X3_GRADW_MODES.items():
        kchunk, splits, got = R.x3_gradw_mode(m, n, l, cfg, target, defer)
        assert got == mode, f"m={m} n={n} l={l} cfg {cfg} target {target}: {got}, wanted {mode}"
        seen.add(mode)
    assert seen == {"one", "carried", "reduce4", "reduce16", "atomics"}
    # the host caps the splits at m / (8 k-tiles of 32): 64 splits are reached from m = 16384 on, and m = 18145 leaves the last one one row
    kchunk, splits, mode = R.x3_gradw_mode(18145, 36, 68, 3, 0)
    assert (splits, 18145 - (splits - 1) * kchunk, mode) == (64, 1, "reduce16")
    # the exact engine: the split target that gives several splits with a partial last one at m = 300 and 1100
    for m in (300, 1100):
        for sizes in R.EXACT_NETWORKS:
            for n, l in zip(sizes[:-1], sizes[1:]):
                cfg, kchunk, splits = R.exact_gradw_splits(m, n, l, 4, G.SPLIT_TARGET)
                assert splits >= 2 and m % kchunk, (m, n, l, kchunk, splits)
    assert R.exact_gradw_splits(200, 264, 130)[2] == 0 and R.exact_use_smallm(200, 264, 136)
