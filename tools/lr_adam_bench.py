#!/usr/bin/env python3
"""The flat Adam launch with the learning rate by value against the pointer variant (the adaptive schedule's),
at the size of bench.py's C4 value network (376 -> 3x512 -> 1: one 16-B aligned span, adam_flat_vec_kernel<RateValue>
against adam_flat_vec_kernel<RateWord>).

Two Adams over two networks of that shape, gradients of a fixed seed; per round 100 launches of each through
ppo_prof_* (events around every launch, PPO_K_ADAM), alternating by value / pointer; six rounds, the first
discarded.  The pointer variant costs one scalar load and one fp32 division per wave on top of the same 28 B/param.

    python tools/lr_adam_bench.py          (recorded in profiles/lr_schedule.txt, part 2)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo.c_amd"))
import ppo_ffi  # noqa: E402

SIZES = [376, 512, 512, 512, 1]
K_ADAM, LAUNCHES, ROUNDS = 2, 100, 6


def timed(lib, step):
    lib.ppo_synchronize()
    lib.ppo_prof_reset()
    for _ in range(LAUNCHES):
        step()
    ms, work, n = (C.c_double * 7)(), (C.c_double * 7)(), (C.c_long * 7)()
    lib.ppo_prof_read(ms, work, n)
    assert n[K_ADAM] == LAUNCHES, list(n)
    return 1e3 * ms[K_ADAM] / LAUNCHES, work[K_ADAM] / LAUNCHES


def main():
    lib = ppo_ffi.load()
    if lib.ppo_device_count() < 1:
        raise RuntimeError("lr_adam_bench: no HIP device visible")
    lib.ppo_set_device(0)
    acts = ppo_ffi.c_strings(["relu"] * 3 + ["none"])
    rng = np.random.default_rng(7)
    nets, adams = [], []
    for _ in range(2):
        nn = lib.create_neural_network(ppo_ffi.c_ints(SIZES), acts, len(SIZES))
        ad = lib.create_adam_from_nn_cuda(nn, 0.9, 0.999)
        a = ad.contents
        assert a.flat
        ppo_ffi.h2d(lib, a.grad_weights[0], rng.normal(0, 1e-2, a.span).astype(np.float32))
        nets.append(nn)
        adams.append(ad)
    rate = np.array([3e-4], np.float32)
    d_rate = ppo_ffi.DeviceArray.from_numpy(lib, rate)
    span = adams[0].contents.span
    print(f"flat Adam span {span} floats ({28.0 * span / 1e6:.2f} MB per launch), {LAUNCHES} launches per measurement")
    lib.ppo_prof_enable(1)
    steps = {"by value": lambda: lib.adam_update_cuda(adams[0], float(rate[0])),
             "pointer": lambda: lib.ppo_adam_update_lr_device(adams[1], d_rate.ptr)}
    kept = {k: [] for k in steps}
    for r in range(ROUNDS):
        for name, step in steps.items():
            us, work = timed(lib, step)
            print(f"round {r} {name:9s} {us:8.3f} us/launch  {work / us / 1e3:7.1f} GB/s" + ("   (discarded)" if r == 0 else ""))
            if r > 0:
                kept[name].append(us)
    lib.ppo_prof_enable(0)
    bv, pt = (float(np.mean(kept[k])) for k in ("by value", "pointer"))
    print(f"mean of the kept rounds: by value {bv:.3f} us, pointer {pt:.3f} us, ratio {pt / bv:.4f}")
    d_rate.free()
    for ad, nn in zip(adams, nets):
        lib.free_adam_cuda(ad)
        lib.free_neural_network(nn)


if __name__ == "__main__":
    main()
