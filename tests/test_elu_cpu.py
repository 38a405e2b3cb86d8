"""The fp32 statement of ELU′ the kernels use, gx = h > 0 ? a : a·(h + 1) (elu_ref.elu_bwd_f32 = csrc/dev.h
ppo::elu_bwd), against the float64 a·(h + 1) (numpy only).  The bound, derived: with u = 2⁻²⁴, s = fl(h + 1) =
(h + 1)(1 + d1) and gx = fl(a·s) = a·(h + 1)(1 + d1)(1 + d2), |d_i| ≤ u, so |gx − a(h + 1)| ≤ |a|·|h + 1|·(2u + u²)
≤ |a|·(2u + u²) for a stored post-activation h ∈ [−1, 0] — two roundings times |a|, relative to the PRODUCT a as the
GEMM bound of the GPU tests is; h > 0 passes a itself.  The forward's saturation: e^z < 2⁻²⁵ (half the spacing of
fp32 just above −1) for z < −17.33, so expm1 of any fp32 z below −17.4 rounds to −1.0f and the unit passes exactly 0."""
import numpy as np

import elu_ref as E

F32, F64 = np.float32, np.float64
U = 2.0 ** -24


def test_elu_bwd_fp32_grid_within_two_roundings():
    rng = np.random.default_rng(5)
    a = np.concatenate([[0.0, 1.0, -3.25, 1e-30, 6.5e4, -1e-3],
                        rng.normal(size=4000) * np.exp(rng.uniform(-20, 20, 4000))]).astype(F32)
    hs = np.concatenate([[-1.0, -0.5, -U, 0.0, U], np.expm1(-rng.exponential(3.0, 400)), rng.uniform(0, 5, 50)])
    for h in hs.astype(F32):
        got = E.elu_bwd_f32(a, np.full_like(a, h))
        ref = a.astype(F64) * (F64(h) + 1.0) if h <= 0 else a.astype(F64)
        assert got.dtype == F32 and (np.abs(got - ref) <= np.abs(a.astype(F64)) * (2 * U + U * U) + 1e-45).all(), h
        assert h != -1 or (got == 0).all()           # a saturated unit passes exactly nothing
        assert h < 0 or (got == a).all()             # h = 0 and h > 0 pass a unchanged
    nan = F32(np.nan)                                # NaN propagates from either operand
    assert np.isnan(E.elu_bwd_f32(a, np.full_like(a, nan))).all()
    assert np.isnan(E.elu_bwd_f32(np.full_like(a, nan), np.full_like(a, -0.5))).all()


def test_expm1_saturates_to_minus_one_below_17_4():
    z = np.concatenate([[np.nextafter(F32(-17.4), F32(-np.inf))], -np.geomspace(17.5, 3e38, 500)]).astype(F32)
    assert (z < F32(-17.4)).all() and (E.act_f(z.astype(F64), "elu").astype(F32) == F32(-1)).all()
    assert E.act_f(np.array([-np.inf, np.inf, 0.0, 2.5]), "elu").tolist() == [-1.0, np.inf, 0.0, 2.5]
    assert np.isnan(E.act_f(np.array([np.nan]), "elu")).all()
