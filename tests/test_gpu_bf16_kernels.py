"""Every bf16 GEMM path of csrc/gemm16.hip, launch by launch and element by element, at the smallest shapes
that have every kind of tail — bf16_ref.check_bf16_readback (the bounds and their reasoning are in bf16_ref.py;
test_bf16_ref_cpu.py shows on the CPU that they admit a valid fp32 evaluation and reject each tail defect).

Each network is built with create_neural_network + nn_set_compute_dtype(nn, 1), runs one forward + backward
(forward_propagation_cuda / backward_propagation_cuda, so layer 0's fp32 grad_x is produced too) under every
forced tile configuration and the automatic choice, and after each pass everything the launches stored is read
back and checked from the GPU's own operands.  Three ReLU layers + an identity output give the type combinations
forward f32→b16, b16→b16, b16→f32; grad_W (f32 g, b16 x), (b16, b16), (b16, f32); grad_x f32→b16, b16→b16, b16→f32;
the one-layer network adds forward f32→f32, grad_W (f32, f32) and grad_x f32→f32.

Networks (bf16_ref.NETWORKS), each width against the loaders' and epilogues' conditions:
  [3, 33, 65, 1]       nothing a multiple of 4: every loader scalar; one past the 32/64 tile and bit-word edges;
                       the output layer takes the N ≤ 32 route (cfg 8 forward, cfg 1 backward when automatic)
  [17, 40, 72, 6]      layer 0 scalar (17); 40 and 72 are multiples of 8, not of 32: the vector path with a k tail
                       inside one BK and a partial bit word; vec on for bf16 g, off for the fp32 g (6 % 4)
  [130, 264, 136, 17]  264 = 256 + 8: a vector-path column tail of 8 past a 256-wide tile (the Rmax − EPL clamp);
                       130 scalar with k tails in BK 32 and 64
  [64, 128, 256, 8]    everything aligned; layer 1's grad_W (l 256, n 128, b16 × b16) takes the DMA TN tile at m 576
  [40, 24]             one layer: the f32→f32 / (f32, f32) instantiations
  [256, 256, 256, 8]   added: the only shape at which grad_x reaches the LDS-DMA kernels (they need N % 256 = 0: layer
                       1's b16→b16 on the 16×16×32 form, layer 0's b16→f32 on the 32×32×16 form) and at which the DMA
                       TN tile can be 256 wide (n % 256 = 0; at n = 128 ppo_gemm16_tn_width(256) falls back to 128)
  [64, 40, 33, 8]      added: a bf16-output forward on the double-buffered kernel WITHOUT the LDS-staged epilogue
                       (layer 1: k = 40 vector path, l = 33 not a multiple of 8, so cvec is off and epilogue256
                       takes its per-element branch with the ballot bit words)
Batches (bf16_ref.BATCHES): 1 (a single row); 33 (one past a 32-row tile); 300 (a row tail in every BM, not a
multiple of 8; grad_W at BK 32 splits in two with kchunk 160: the second split has 140 rows and a partial last
k-tile, bias sums by atomics); 576 (a multiple of 64 for the DMA TN tile: two splits of 320 + 256; at BK 64 two
splits with a remainder, at BK 32 four of 160 with a partial fourth … 96 rows).

Reached kernels (from launch_cfg / launch_dma / launch_dma_tn / pick16; F = forward, X = grad_x, W = grad_W;
"generic" = gemm_bf16_kernel<BM×BN/BK>, "db" = gemm_bf16_db_kernel, "dma32" = gemm_bf16_dma_kernel,
"dma16" = gemm_bf16_dma16_kernel, "tn" = gemm_bf16_dma_tn_kernel):
  cfg 0–8 forced   every launch of every network and m on generic at that cfg's tile (0 128×128/32, 1 128×32/32,
                   2 32×128/32, 3 64×64/32, 4 128×128/64, 5 256×128/64, 6 128×256/64 — grad_W in the 16×16×32 MFMA
                   form —, 7 256×128/32, 8 128×32/64): scalar loaders where an extent is not a multiple of the load
                   width (all of [3, 33, 65, 1]; layer 0 of [17, …] and [130, …]; every launch fed by the 6- and
                   17-wide fp32 g; layer 2 of [64, 40, 33, 8]), vector loaders elsewhere, k tails wherever K is
                   not a multiple of BK (every network but the two 256-aligned ones in F / X; every m in W)
  cfg 9 forced     F / X: dma16 for b16→b16 with K % 64 = 0 (F1 of [64, 128, 256, 8]; F1 and X1 of [256, 256, 256, 8]);
                   dma32 for b16→f32 (F2 of both; X0 of [256, 256, 256, 8]); db where an operand is fp32 or K % 64 ≠ 0
                   or (X) N % 256 ≠ 0 but the vector path holds (F0, X2, X1, X0 of [64, 128, 256, 8]; F0, X2 of
                   [256, …]; F1, F2, X1 of [17, …] and [130, …], with k tails 40 / 72 / 8 / 264 / 136 inside BK 64;
                   F0, X0 of [40, 24]; F0, F1, X0 of [64, 40, 33, 8] — F1 without cvec); cfg 9 WITHOUT the vector
                   path silently falls back to generic 128×256/64 (all of [3, …]; layer 0 and the fp32-g launches of
                   [17, …], [130, …]).  W: cfg 9 is never taken — generic 128×256/64 in the 32×32×16 MFMA form (cfg 6
                   is the same tile in the 16×16×32 form); a forced cfg also switches the DMA TN tile off
  cfg 9, DMA off   (aligned networks) the dma16 / dma32 launches above run on db instead
  automatic        pick16: m = 1 → cfg 2 (3 for narrow N); m = 33 → cfg 3, the N ≤ 32 output layer cfg 8 (F) / 1 (W of
                   layer 0 of the narrow networks) / 2 (W of the output layer: M = l ≤ 32); m ≥ 300 → cfg 0 / 4 (X) for
                   wide N, cfg 6 where N % 256 = 0, cfg 3 where N ≤ 64.  W1 of [64, 128, 256, 8] and [256, 256, 256, 8]
                   at m = 576 → tn (128 wide; 256 wide for [256, …] with ppo_gemm16_tn_width(256)), two splits through
                   the slab reduce; with DMA off → generic.  At m = 1, 33, 300 (m % 64 ≠ 0) the tile declines → generic
So all five kernels run, the generic one with both paths of both loader layouts, with one split and several, and
with full and partial last k-tiles.  The fused in-kernel gather (Stage16::copy_out, S % 4 ≠ 0) and the separate
gather kernel (S % 4 = 0) are reached through ppo_update in test_fused_gather_ragged.

Worst err / bound per product over this file on an MI355X (printed by every check; bounds in bf16_ref.py):
  forward bf16 0.982   forward fp32 0.003   grad_W 0.004   bias gradient 0.001   grad_x (bf16) 0.985   grad_x (fp32) 0.004
The two bf16-output figures sit just under 1 by construction (a correct round-to-nearest errs by up to half an
ulp, which IS the 2^-8·|want| term); the fp32 sums use well under a hundredth of 2^-15·Σ|terms| at these K ≤ 576,
so those checks would also catch an error 100 times smaller than the bound.  The C5 production tests print
the same line (forward fp32 0.005, grad_W 0.006 at K = 16384).  With layer 0's grad_W and bias sum made to lose
the batch's last row in a scratch build, all 28 cases of test_bf16_kernels_every_cfg fail, while
test_gpu_bf16.py::test_bf16_mlp_every_cfg still passes at its three larger shapes.
"""
import numpy as np
import pytest

import ppo_ffi
from bf16_ref import (BATCHES, NETWORKS, _bf16_dev, bf16, check_bf16_layers, check_bf16_readback, make_case,
                      read_bf16_layers)
from helpers import F32, dev, nn_params_packed, nn_set_params_packed

pytestmark = pytest.mark.gpu

DMA_NETS = ([64, 128, 256, 8], [256, 256, 256, 8])          # the shapes that reach the LDS-DMA kernels


@pytest.fixture(scope="module")
def ncfg16(lib):
    n = lib.ppo_gemm16_tune(-1)
    yield n
    lib.ppo_gemm16_tune(-1)


@pytest.fixture(scope="module")
def file_worst():
    """worst err / bound per product over this file's cfg sweep, printed once at the end"""
    worst = {}
    yield worst
    print("\nbf16 kernels, worst err / bound over the file: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("m", BATCHES)
@pytest.mark.parametrize("sizes", NETWORKS, ids=lambda s: "-".join(map(str, s)))
def test_bf16_kernels_every_cfg(lib, ncfg16, file_worst, sizes, m):
    params, x, gout = make_case(sizes, m)
    names = ["relu"] * (len(sizes) - 2) + ["none"]
    nn = lib.create_neural_network(ppo_ffi.c_ints(sizes), ppo_ffi.c_strings(names), len(sizes))
    nn_set_params_packed(lib, nn, params)
    assert lib.nn_set_compute_dtype(nn, 1) == 0
    dx, dgo = dev(lib, x), dev(lib, gout)
    runs = [(c, 1, 128) for c in range(ncfg16)] + [(-1, 1, 128)]
    if sizes in DMA_NETS:
        runs += [(-1, 1, 256), (-1, 0, 128), (9, 0, 128)]
    old_dma, old_w = lib.ppo_gemm16_dma(-1), lib.ppo_gemm16_tn_width(0)
    worst = {}
    try:
        for c, dma, width in runs:
            lib.ppo_gemm16_tune(c)
            lib.ppo_gemm16_dma(dma)
            lib.ppo_gemm16_tn_width(width)
            lib.forward_propagation_cuda(nn, dx.ptr, m)
            lib.backward_propagation_cuda(nn, dgo.ptr, m)
            rb = read_bf16_layers(lib, nn, sizes, m, grad_x0=True)
            w = check_bf16_readback(sizes, params, x, gout, True, rb, f"{sizes} m={m} cfg {c} dma {dma} tn {width}")
            for k, v in w.items():
                worst[k] = max(worst.get(k, 0.0), v)
                file_worst[k] = max(file_worst.get(k, 0.0), v)
    finally:
        lib.ppo_gemm16_tune(-1)
        lib.ppo_gemm16_dma(old_dma)
        lib.ppo_gemm16_tn_width(old_w)
        lib.free_neural_network(nn)
        dx.free()
        dgo.free()
    print(f"WORST {sizes} m={m}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("S", [17, 20])
def test_fused_gather_ragged(lib, oracle, S):
    """One bf16-mode policy step and one value step of ppo_update at B = 300 of N = 1200 rows, layers
    [S, 40, 72, 6] / [S, 40, 72, 1]: S = 17 gathers inside layer 0's GEMM (Stage16::copy_out, the scalar
    stores of a ragged width), S = 20 through the separate gather kernel.  The gathered bf16 copy equals
    bf16(state[rows]) bit for bit, and every launch of both networks passes the per-kernel check (the policy's
    top gradient from the fp32 head on the GPU's own output, the value's 2(y − target)/B)."""
    from test_gpu_production import bench_ppo
    sizes, A, E, T, B = [S, 40, 72, 6], 6, 4, 300, 300
    N = E * T
    ppo = bench_ppo(lib, oracle, sizes, E, T, seed=1700 + S, dtype=1)
    try:
        b = ppo.contents.buffer.contents
        state = ppo_ffi.d2h(lib, b.d_state_p, F32, N * S).reshape(N, S)
        pol, V = ppo.contents.policy.contents, ppo.contents.V
        # ---- policy step
        seed = 59
        mu0 = nn_params_packed(lib, pol.mu)
        ls0 = ppo_ffi.d2h(lib, pol.d_log_std, F32, A)
        lib.ppo_set_step_limit(ppo, 0, 1)
        lib.ppo_update(ppo, 0.99, B, 1, 0, 1, seed)
        lib.ppo_synchronize()
        rows = oracle.feistel_perm(N, oracle.splitmix64(seed))[:B]
        assert len(set(rows.tolist())) == B < N
        x = state[rows]
        assert pol.mu.contents.x0_dtype == 1
        np.testing.assert_array_equal(_bf16_dev(lib, pol.mu.contents.d_x0, B, S).view(np.uint32), bf16(x).view(np.uint32))
        a = ppo_ffi.d2h(lib, b.d_action_p, F32, N * A).reshape(N, A)[rows]
        adv = ppo_ffi.d2h(lib, b.d_advantage_p, F32, N)[rows]
        old = ppo_ffi.d2h(lib, b.d_logprob_p, F32, N)[rows]
        y = ppo_ffi.d2h(lib, pol.mu.contents.d_output, F32, B * A).reshape(B, A)
        lp = oracle.log_prob(y, ls0, a)
        _, glp, _ = oracle.policy_loss_and_grad(adv, lp, old, oracle.entropy(ls0), 0.0, 0.2)
        gtop, _ = oracle.log_prob_backwards(y, ls0, a, glp)
        check_bf16_layers(lib, pol.mu, sizes, mu0, x, gtop, True, f"gather S={S} policy")
        # ---- value step
        seed = 57
        sv = sizes[:-1] + [1]
        v0 = nn_params_packed(lib, V)
        lib.ppo_set_step_limit(ppo, 1, 0)
        lib.ppo_update(ppo, 0.99, B, 0, 1, 1, seed)
        lib.ppo_synchronize()
        rows = oracle.feistel_perm(N, oracle.splitmix64(seed))[:B]
        x = state[rows]
        assert V.contents.x0_dtype == 1
        np.testing.assert_array_equal(_bf16_dev(lib, V.contents.d_x0, B, S).view(np.uint32), bf16(x).view(np.uint32))
        tgt = ppo_ffi.d2h(lib, b.d_adv_target_p, F32, N)[rows]
        y = ppo_ffi.d2h(lib, V.contents.d_output, F32, B)
        gtop = (2 * (y.astype(np.float64) - tgt) / B).reshape(-1, 1)
        check_bf16_layers(lib, V, sv, v0, x, gtop, True, f"gather S={S} value")
    finally:
        lib.ppo_set_step_limit(ppo, -1, -1)
        lib.free_ppo(ppo)
