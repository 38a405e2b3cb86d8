"""Time the multi-discrete head against the categorical head at the same traffic.

Both heads read logits [m, A] once and write their gradient once: 2·m·A·4 bytes.  One process, one device; after
warm-up launches every launch is sampled by ppo_prof_* (class PPO_K_HEAD, events around the launch), one read per
launch, the median over the launches reported with the achieved GB/s on 2·m·A·4 bytes.

    python tools/multidiscrete_head_bench.py [--m 32768] [--n 7] [--D 17] [--launches 30] > profiles/multidiscrete_head.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo.c_amd"))
import ppo_ffi  # noqa: E402

K_HEAD = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=32768)
    ap.add_argument("--n", type=int, default=7)
    ap.add_argument("--D", type=int, default=17)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    lib = ppo_ffi.load()
    if lib.ppo_device_count() < 1:
        raise RuntimeError("no HIP device visible")
    lib.ppo_set_device(0)
    m, nvec = args.m, [args.n] * args.D
    A = sum(nvec)
    rng = np.random.default_rng(0)
    F32 = np.float32
    z = (2 * rng.normal(size=(m, A))).astype(F32)
    act = np.zeros((m, A), F32)
    act[:, :args.D] = rng.integers(0, args.n, (m, args.D))
    adv = rng.normal(size=m).astype(F32)
    old = (-np.log(args.n) * args.D + rng.uniform(-0.3, 0.3, m)).astype(F32)
    d = {k: ppo_ffi.DeviceArray.from_numpy(lib, v) for k, v in dict(z=z, act=act, adv=adv, old=old).items()}
    g, lp, H = (ppo_ffi.DeviceArray(lib, 4 * n) for n in (m * A, m, m))
    loss = C.c_double(0)
    c_nvec = ppo_ffi.c_ints(nvec)

    def md():
        assert lib.ppo_multidiscrete_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, m, A, c_nvec,
                                                 args.D, 0.2, 0.01, g.ptr, lp.ptr, H.ptr, C.byref(loss)) == 0

    def cat():
        assert lib.ppo_categorical_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, m, A, 0.2, 0.01,
                                               g.ptr, lp.ptr, H.ptr, C.byref(loss)) == 0

    ms, work, n = (C.c_double * 7)(), (C.c_double * 7)(), (C.c_long * 7)()
    med = {}
    print(f"m = {m}, A = {A}: multi-discrete nvec = [{args.n}]*{args.D} against categorical A = {A}; "
          f"{2 * m * A * 4 / 1e6:.2f} MB of logits + gradient per launch")
    for name, fn in (("categorical", cat), ("multi-discrete", md), ("categorical (again)", cat)):
        for _ in range(args.warmup):
            fn()
        lib.ppo_prof_enable(1)
        us = []
        for _ in range(args.launches):
            lib.ppo_prof_reset()
            fn()
            lib.ppo_prof_read(ms, work, n)
            assert n[K_HEAD] == 1
            us.append(ms[K_HEAD] * 1e3)
        lib.ppo_prof_enable(0)
        us.sort()
        med[name] = us[len(us) // 2]
        print(f"{name:20s}: median {med[name]:8.2f} us of {len(us)} launches (min {us[0]:.2f}, max {us[-1]:.2f}); "
              f"{2 * m * A * 4 / med[name] / 1e3:7.1f} GB/s")
    base = min(med["categorical"], med["categorical (again)"])
    print(f"multi-discrete / categorical = {med['multi-discrete'] / base:.3f} (target: at most 1.5)")


if __name__ == "__main__":
    main()
