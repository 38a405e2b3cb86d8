#!/usr/bin/env python3
"""Time the state-dependent-σ Gaussian head (csrc/gauss_sd.hip) against the Gaussian head (form 1) at the C4 policy
minibatch's row count, in one process, in alternating rounds.

Both heads run through their test entries under libppo's own per-launch device events (ppo_prof_enable: an event pair
around every launch, attributed to class HEAD), so the figure is the kernel's time on the device and not the entry's
host work.  The new head reads z [m, 2·Aa], the action rows and writes the gradient [m, 2·Aa]: about twice the bytes
of the Gaussian head at A = Aa.

    python tools/gauss_sd_bench.py [--rows 32768] [--aa 17] [--rounds 5] [--iters 50] > profiles/gauss_sd_head.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo.c_amd"))
import ppo_ffi  # noqa: E402

F32 = np.float32
K_HEAD, K_COUNT = 4, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32768, help="the C4 policy minibatch")
    ap.add_argument("--aa", type=int, default=17)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    lib = ppo_ffi.load()
    lib.ppo_set_device(0)
    m, Aa = args.rows, args.aa
    A = 2 * Aa
    rng = np.random.default_rng(0)

    def dev(a):
        return ppo_ffi.DeviceArray.from_numpy(lib, np.ascontiguousarray(a, F32))

    z = rng.normal(size=(m, A)).astype(F32)
    act = np.zeros((m, A), F32)
    act[:, :Aa] = z[:, :Aa] + rng.normal(size=(m, Aa)).astype(F32)
    adv, old = rng.normal(size=m).astype(F32), rng.normal(size=m).astype(F32) - F32(1.4 * Aa)
    d = dict(z=dev(z), act=dev(act), adv=dev(adv), old=dev(old), g=dev(np.zeros((m, A))), lp=dev(np.zeros(m)),
             H=dev(np.zeros(m)), mu=dev(z[:, :Aa]), a1=dev(act[:, :Aa]), ls=dev(np.zeros(Aa)), g1=dev(np.zeros((m, Aa))),
             gls=dev(np.zeros(Aa)))
    loss, cnt = C.c_double(), (C.c_longlong * 2)()

    def sd_head():
        assert lib.ppo_gauss_sd_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, m, A, -20.0, 2.0, 0.2,
                                            0.01, d["g"].ptr, d["lp"].ptr, d["H"].ptr, C.byref(loss), cnt) == 0

    def gauss_head():
        assert lib.ppo_policy_head_device(1, m, Aa, 0, 0, 0.2, 0.01, d["ls"].ptr, d["a1"].ptr, d["adv"].ptr, d["old"].ptr,
                                          d["mu"].ptr, None, None, None, None, d["g1"].ptr, None, None, d["gls"].ptr,
                                          C.byref(loss)) == 0

    def timed(fn):
        t_ms, work, launches = (C.c_double * K_COUNT)(), (C.c_double * K_COUNT)(), (C.c_long * K_COUNT)()
        lib.ppo_prof_enable(1)
        lib.ppo_prof_reset()
        for _ in range(args.iters):
            fn()
        lib.ppo_prof_read(t_ms, work, launches)
        lib.ppo_prof_enable(0)
        return 1e3 * t_ms[K_HEAD] / max(1, launches[K_HEAD])

    for fn in (sd_head, gauss_head):
        for _ in range(5):
            fn()
    sd_us, g_us = [], []
    for r in range(args.rounds):
        g_us.append(timed(gauss_head))
        sd_us.append(timed(sd_head))
        print(f"round {r}: Gaussian head (form 1, A = {Aa}) {g_us[-1]:.2f} us   state-dependent-sigma head "
              f"(A = {A}) {sd_us[-1]:.2f} us   ratio {sd_us[-1] / g_us[-1]:.2f}")
    bytes_sd, bytes_g = 4.0 * m * (3 * A + 2), 4.0 * m * (3 * Aa + 2)
    print(f"rows {m}, Aa {Aa}: bytes moved {bytes_sd / 1e6:.1f} MB vs {bytes_g / 1e6:.1f} MB (ratio {bytes_sd / bytes_g:.2f})")
    print(f"median: Gaussian {np.median(g_us):.2f} us (spread {min(g_us):.2f} .. {max(g_us):.2f}), "
          f"state-dependent-sigma {np.median(sd_us):.2f} us (spread {min(sd_us):.2f} .. {max(sd_us):.2f}), "
          f"ratio {np.median(sd_us) / np.median(g_us):.2f}, {bytes_sd / np.median(sd_us) / 1e3:.0f} GB/s")
    for a in d.values():
        a.free()


if __name__ == "__main__":
    main()
