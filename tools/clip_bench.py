#!/usr/bin/env python3
"""What gradient clipping costs at the bench's C4 configuration (one GPU, one process).

bench.py's C4 update (376 -> 3x512 -> 17, 4096 steps x 256 envs, B = 32768, 10 value + 4 policy epochs,
device shuffle), alternating clipping off and on with max_norm = 0.5 x the smaller first-step gradient
norm, timed over whole updates as bench.py does; then one profiled update of each kind (PPO_SERIAL=1,
events around every launch) for the PPO_K_ADAM class: the Adam kernel's µs per launch from the
clipping-off update, and the norm kernel's from the class's extra time and extra launches with it on.

    python tools/clip_bench.py [--rounds 3] [--updates 2] > profiles/clip_c4.txt
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo.c_amd"))
import ppo_ffi  # noqa: E402

S, H, A, T, E, B = 376, [512, 512, 512], 17, 4096, 256, 32768
K_ADAM = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="off/on alternations")
    ap.add_argument("--updates", type=int, default=2, help="timed updates per measurement")
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    lib = ppo_ffi.load()
    if lib.ppo_device_count() < 1:
        raise RuntimeError("clip_bench: no HIP device visible")
    lib.ppo_set_device(0)
    sizes = [S] + H + [A]
    acts = ["relu"] * len(H) + ["none"]
    C.CDLL("libc.so.6").srand(args.seed)
    ppo = lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), E * T, 3e-4, 3e-4, 0.95, 0.2, 0.0,
                         1.0, True)
    lib.ppo_fill_synthetic(ppo, E, T, args.seed * 1000, 1.0 / 500)

    def update():
        lib.ppo_update(ppo, 0.99, B, 4, 10, 1, args.seed)

    # the first step's norms, from the gradients the first value / policy step leaves behind
    lib.ppo_set_step_limit(ppo, 1, 1)
    update()
    lib.ppo_synchronize()
    pol = ppo.contents.policy.contents
    av, ap_ = ppo.contents.adam_V.contents, ppo.contents.adam_policy.contents
    n_v = lib.ppo_grad_norm_device(C.cast(av.grad_weights[0], C.c_void_p), av.span, None, 0)
    n_p = lib.ppo_grad_norm_device(C.cast(ap_.grad_weights[0], C.c_void_p), ap_.span,
                                   C.cast(pol.d_log_std_grad, C.c_void_p), A)
    max_norm = 0.5 * min(n_v, n_p)
    lib.ppo_set_step_limit(ppo, -1, -1)
    print(f"C4 {sizes}, N = {E * T}, B = {B}, 10 value + 4 policy epochs (448 minibatch steps per update)")
    print(f"first-step norms: value {n_v:.6g} ({av.span} floats), policy {n_p:.6g} ({ap_.span} + {A} floats); "
          f"max_norm = {max_norm:.6g}")
    update()                                              # warm-up
    lib.ppo_synchronize()

    ms = {0: [], 1: []}
    for _ in range(args.rounds):
        for on in (0, 1):
            lib.ppo_set_max_grad_norm(ppo, max_norm if on else 0.0)
            update()                                      # settle into the mode
            lib.ppo_synchronize()
            t0 = time.perf_counter()
            for _ in range(args.updates):
                update()
            lib.ppo_synchronize()
            ms[on].append(1e3 * (time.perf_counter() - t0) / args.updates)
    for on in (0, 1):
        xs = sorted(ms[on])
        print(f"clipping {'on ' if on else 'off'}: {xs[len(xs) // 2]:.2f} ms per update (median of {len(xs)}; "
              + ", ".join(f"{x:.2f}" for x in ms[on]) + ")")

    os.environ["PPO_SERIAL"] = "1"
    prof = {}
    for on in (0, 1):
        lib.ppo_set_max_grad_norm(ppo, max_norm if on else 0.0)
        lib.ppo_reset_stats(ppo)
        lib.ppo_prof_enable(1)
        lib.ppo_prof_reset()
        update()
        t_ms, work, launches = (C.c_double * 7)(), (C.c_double * 7)(), (C.c_long * 7)()
        lib.ppo_prof_read(t_ms, work, launches)
        lib.ppo_prof_enable(0)
        st = (C.c_double * 13)()
        lib.ppo_read_stats(ppo, st, 13)
        prof[on] = (t_ms[K_ADAM], launches[K_ADAM], work[K_ADAM], list(st))
    del os.environ["PPO_SERIAL"]
    (t0_, l0, w0, _), (t1, l1, w1, st) = prof[0], prof[1]
    adam_us = 1e3 * t0_ / max(l0, 1)
    print(f"PPO_K_ADAM, clipping off: {l0} launches, {t0_:.3f} ms: Adam {adam_us:.2f} us per launch "
          f"({w0 / max(l0, 1) / 1e6:.2f} MB each)")
    extra = l1 - l0
    print(f"PPO_K_ADAM, clipping on:  {l1} launches, {t1:.3f} ms: the {extra} norm launches take "
          f"{1e3 * (t1 - t0_) / max(extra, 1):.2f} us each ({(w1 - w0) / max(extra, 1) / 1e6:.2f} MB each; "
          f"the class's extra time over its extra launches)")
    print(f"last norms: value {st[9]:.6g}, policy {st[10]:.6g}; clipped steps: value {st[11]:.0f} of {st[1]:.0f}, "
          f"policy {st[12]:.0f} of {st[3]:.0f}")
    lib.free_ppo(ppo)


if __name__ == "__main__":
    main()
