"""bf16_ref.py on the CPU: the rounding model against an independent one, and the per-kernel checker against
a numpy fp32 model of the kernels' accumulation (bf16_ref.gemm_f32_model / model_run: fp32 partial sums per
BK-wide k-tile, chained; split-K partials added in fp32; stored outputs rounded to bf16) at every (network,
batch) of test_gpu_bf16_kernels.py:

* the clean model is inside every bound for BK ∈ {32, 64}, 1–4 splits and both tile orders — the bounds are not
  so tight that a valid fp32 evaluation fails them (its worst err / bound is asserted ≤ 0.25: the model chains
  at most 18 k-tiles + 4 splits, ≈ 22·2^-24 of a 2^-15 = 512·2^-24 bound; the half-ulp term carries the rest);
* every injected defect (bf16_ref.MUTANTS, at every layer it applies to) is rejected by the check of the launch
  that carries it, wherever it changes what that launch stores;
* no case leans on a dead layer: in every hidden layer more than half of the units are live, and every row has
  a live unit (asserted on the clean model's stored activations).

One truncated element is visible to the 2^-8·|want| bound only where the value's mantissa sits low in its binade
(the truncation error, up to one bf16 ulp, then exceeds half an ulp of the VALUE); model_run truncates the
element where that is most so.  No GPU is used."""
import numpy as np
import pytest
import torch

import bf16_ref as R
from bf16_ref import F32

CASES = [(s, m) for s in R.NETWORKS for m in R.BATCHES]
IDS = ["-".join(map(str, s)) + f"_m{m}" for s, m in CASES]

# the check that must reject each defect (a fragment of its message)
CAUGHT_BY = dict(fwd_drop_last_k="forward layer {i}", fwd_drop_last_row="forward layer {i}",
                 fwd_trunc_one="forward layer {i}", bits_clear_last_valid="bits layer {j}",
                 bits_set_pad="bits layer {j}", gw_drop_last_row="grad_W layer {i}", gw_drop_last_tile="grad_W layer {i}",
                 bias_drop_last_row="bias grad layer {i}", gx_drop_last_k="grad_x layer {i}",
                 gx_unmask_last_col="grad_x layer {i}", gx_mask_next_row="grad_x layer {i}",
                 gx_trunc_one="grad_x layer {i}")


def test_bf16_rounding_against_torch():
    """bf16() against torch's float32 → bfloat16 conversion, bit for bit: exact ties in both directions (the
    kept mantissa even: down; odd: up), one fp32 ulp either side of a tie, ±0, the largest finite bf16 and the
    largest fp32 that still rounds to it, fp32 subnormals (ties included) and a random sweep of bit patterns."""
    keep = np.array([0x3F80, 0x3F81, 0x4049, 0x0001, 0x0000, 0x7F7E, 0x0080, 0x00FF], np.uint32) << 16
    pats = []
    for lo in (0x8000, 0x7FFF, 0x8001, 0x0000, 0x0001, 0xFFFF):
        pats.append(keep | np.uint32(lo))
    pats = np.concatenate(pats)
    pats = pats[(pats >> 23) != 0xFF]                       # finite inputs
    pats = pats[bf_finite(pats)]
    special = np.array([0x00000000, 0x80000000, 0x7F7F0000, 0x7F7F7FFF, 0x00000001, 0x00008000, 0x00018000,
                        0x00007FFF, 0x007FFFFF, 0x00800000], np.uint32)
    rng = np.random.default_rng(5)
    rnd = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    rnd = rnd[((rnd >> 23) & 0xFF) != 0xFF]
    rnd = rnd[bf_finite(rnd)]
    u = np.concatenate([pats, pats | np.uint32(0x80000000), special, rnd])
    x = u.view(F32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    got = R.bf16(x)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # the named edges, spelled out (not only "equal to torch")
    one = lambda bits: np.array([bits], np.uint32).view(F32)          # noqa: E731
    assert R.bf16(one(0x3F808000)).view(np.uint32)[0] == 0x3F800000   # tie, even mantissa: down
    assert R.bf16(one(0x3F818000)).view(np.uint32)[0] == 0x3F820000   # tie, odd mantissa: up
    assert R.bf16(one(0x3F807FFF)).view(np.uint32)[0] == 0x3F800000   # one ulp below the tie
    assert R.bf16(one(0x3F808001)).view(np.uint32)[0] == 0x3F810000   # one ulp above the tie
    assert R.bf16(one(0x80000000)).view(np.uint32)[0] == 0x80000000   # −0 keeps its sign
    assert R.bf16(one(0x7F7F7FFF)).view(np.uint32)[0] == 0x7F7F0000   # the largest value that stays finite
    assert R.bf16(one(0x00008000)).view(np.uint32)[0] == 0x00000000   # subnormal tie: to even (zero)
    assert R.bf16(one(0x00018000)).view(np.uint32)[0] == 0x00020000   # subnormal tie: odd, up


def bf_finite(u):
    """fp32 bit patterns whose bf16 rounding is finite (|x| below the midpoint to 2^128)"""
    return (u & np.uint32(0x7FFFFFFF)) < np.uint32(0x7F7F8000)


def test_pack_bits_round_trip():
    rng = np.random.default_rng(3)
    for n in (1, 31, 32, 33, 40, 65, 264):
        mask = rng.uniform(size=(5, n)) < 0.5
        words = R.pack_bits(mask)
        assert words.shape == (5, (n + 31) // 32) and words.dtype == np.uint32
        np.testing.assert_array_equal(R.unpack_bits(words, n), mask)
        for c in range(n):
            assert ((words[:, c // 32] >> np.uint32(c % 32)) & 1 == mask[:, c]).all()
        if n % 32:
            assert not (words[:, -1] >> np.uint32(n % 32)).any()


def test_gemm_model_split_ranges():
    """The model's split ranges are the kernels': m = 300 at BK = 32 in two splits is 160 + 140 rows, the second
    with a partial last k-tile; its sum equals the float64 product within fp32 chaining."""
    rng = np.random.default_rng(4)
    A, B = R.bf16(rng.uniform(-1, 1, (7, 300))), R.bf16(rng.uniform(-1, 1, (300, 5)))
    ref = A.astype(np.float64) @ B.astype(np.float64)
    sa = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    for bk in (32, 64):
        for splits in (1, 2, 3, 4):
            for rev in (False, True):
                C = R.gemm_f32_model(A, B, bk, splits, rev)
                assert C.dtype == F32 and (np.abs(C - ref) <= 32 * 2.0 ** -24 * sa).all()
    dropped = R.gemm_f32_model(A, B, 32, 2, drop_last_tile=True)       # rows 288..299 lost
    np.testing.assert_allclose(dropped, A[:, :288].astype(np.float64) @ B[:288].astype(np.float64), atol=1e-4)


@pytest.fixture(scope="module")
def clean():
    """The clean model at BK = 32, one split, ascending — per case, computed once."""
    out = {}
    for sizes, m in CASES:
        params, x, gout = R.make_case(sizes, m)
        out[(tuple(sizes), m)] = R.model_run(sizes, params, x, gout)[0]
    return out


@pytest.mark.parametrize("sizes,m", CASES, ids=IDS)
def test_live_unit_cap(clean, sizes, m):
    rb = clean[(tuple(sizes), m)]
    for i in range(1, len(sizes) - 1):
        live = rb["h"][i] > 0
        assert live.mean() > 0.5, f"layer {i}: only {live.mean():.2f} of the units live"
        assert live.any(axis=1).all(), f"layer {i}: a row with no live unit"


@pytest.mark.parametrize("sizes,m", CASES, ids=IDS)
def test_clean_model_inside_bounds(sizes, m):
    params, x, gout = R.make_case(sizes, m)
    for bk in (32, 64):
        for splits in (1, 2, 3, 4):
            for rev in (False, True):
                rb, changed = R.model_run(sizes, params, x, gout, bk, splits, rev)
                assert not changed
                worst = R.check_bf16_readback(sizes, params, x, gout, True, rb, f"model BK{bk} s{splits} r{int(rev)}")
                for k in ("fwd_f32", "grad_W", "bias", "grad_x0"):      # pure fp32 sums: far inside 2^-15
                    assert worst[k] <= 0.25, (k, worst[k])
                assert worst["fwd_bf16"] <= 1.0 and worst["grad_x"] <= 1.0


def _mutant_layers(name, L):
    if name.startswith("fwd_trunc") or name.startswith("bits_"):
        return range(L - 1)                                 # launches with a bf16 output and bits
    if name.startswith("fwd_") or name.startswith("gw_") or name.startswith("bias_"):
        return range(L)
    if name == "gx_drop_last_k":
        return range(L)                                     # layer 0: the fp32 grad_x
    return range(1, L)                                      # masked bf16 grad_x


@pytest.mark.parametrize("sizes,m", CASES, ids=IDS)
def test_every_mutant_is_rejected(sizes, m):
    params, x, gout = R.make_case(sizes, m)
    L = len(sizes) - 1
    bit, skipped = 0, []
    for name in R.MUTANTS:
        for i in _mutant_layers(name, L):
            for bk, splits in ((32, 2), (64, 1)):
                rb, changed = R.model_run(sizes, params, x, gout, bk, splits, False, name, i)
                if not changed:
                    skipped.append((name, i))
                    continue
                frag = CAUGHT_BY[name].format(i=i, j=i + 1)
                with pytest.raises(AssertionError, match=frag):
                    R.check_bf16_readback(sizes, params, x, gout, True, rb, f"mutant {name}@{i}")
                bit += 1
    # what may change nothing: with one row, a neighbour's mask (there is none) and an unmasked last column
    # (make_case keeps it live there); a pad bit where the width is a multiple of 32.  Nothing else.
    for name, i in skipped:
        assert name in ("gx_mask_next_row", "gx_unmask_last_col", "bits_set_pad"), (name, i)
        assert sizes[i + 1] % 32 == 0 if name == "bits_set_pad" else m == 1, (name, i)
    assert bit > 0
