#!/usr/bin/env python3
"""Time the Beta head (csrc/beta.hip) against the state-dependent-σ Gaussian head (csrc/gauss_sd.hip) at the C4 policy
minibatch's row count and the same row width, in one process, in alternating rounds.

Both heads run through their test entries under libppo's own per-launch device events (ppo_prof_enable: an event pair
around every launch, attributed to class HEAD), so the figure is the kernel's time on the device and not the entry's
host work.  The two heads move the same bytes (z, the action rows, the gradient, 8 bytes a row): what separates them is
the Beta head's three lnΓ, three ψ and three ψ′ per component, in double.

    python tools/beta_bench.py [--rows 32768] [--aa 17] [--rounds 5] [--iters 20] > profiles/beta_head.txt
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
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    lib = ppo_ffi.load()
    lib.ppo_set_device(0)
    m, Aa = args.rows, args.aa
    A = 2 * Aa
    rng = np.random.default_rng(0)

    def dev(a):
        return ppo_ffi.DeviceArray.from_numpy(lib, np.ascontiguousarray(a, F32))

    z = rng.normal(scale=2.0, size=(m, A)).astype(F32)
    x = np.zeros((m, A), F32)
    x[:, :Aa] = np.clip(rng.beta(2.0, 2.0, (m, Aa)), 2.0 ** -24, 1 - 2.0 ** -24)
    adv, old = rng.normal(size=m).astype(F32), rng.normal(size=m).astype(F32)
    d = dict(z=dev(z), x=dev(x), adv=dev(adv), old=dev(old), g=dev(np.zeros((m, A))), lp=dev(np.zeros(m)),
             H=dev(np.zeros(m)))
    loss, cnt = C.c_double(), (C.c_longlong * 2)()

    def beta_head():
        assert lib.ppo_beta_head_device(d["z"].ptr, d["x"].ptr, d["adv"].ptr, d["old"].ptr, m, A, 15.0, 0.2, 0.01,
                                        d["g"].ptr, d["lp"].ptr, d["H"].ptr, C.byref(loss), cnt) == 0

    def sd_head():
        assert lib.ppo_gauss_sd_head_device(d["z"].ptr, d["x"].ptr, d["adv"].ptr, d["old"].ptr, m, A, -20.0, 2.0, 0.2,
                                            0.01, d["g"].ptr, d["lp"].ptr, d["H"].ptr, C.byref(loss), cnt) == 0

    def timed(fn):
        t_ms, work, launches = (C.c_double * K_COUNT)(), (C.c_double * K_COUNT)(), (C.c_long * K_COUNT)()
        lib.ppo_prof_enable(1)
        lib.ppo_prof_reset()
        for _ in range(args.iters):
            fn()
        lib.ppo_prof_read(t_ms, work, launches)
        lib.ppo_prof_enable(0)
        return 1e3 * t_ms[K_HEAD] / max(1, launches[K_HEAD])

    for fn in (beta_head, sd_head):
        for _ in range(5):
            fn()
    b_us, s_us = [], []
    for r in range(args.rounds):
        s_us.append(timed(sd_head))
        b_us.append(timed(beta_head))
        print(f"round {r}: state-dependent-sigma head {s_us[-1]:.2f} us   Beta head {b_us[-1]:.2f} us   "
              f"ratio {b_us[-1] / s_us[-1]:.2f}")
    nbytes = 4.0 * m * (3 * A + 2)
    print(f"rows {m}, Aa {Aa}, A {A}: both heads move {nbytes / 1e6:.1f} MB")
    print(f"median: state-dependent-sigma {np.median(s_us):.2f} us (spread {min(s_us):.2f} .. {max(s_us):.2f}), "
          f"Beta {np.median(b_us):.2f} us (spread {min(b_us):.2f} .. {max(b_us):.2f}), "
          f"ratio {np.median(b_us) / np.median(s_us):.2f}; the Beta head at {nbytes / np.median(b_us) / 1e3:.0f} GB/s and "
          f"{np.median(b_us) * 1e3 / (m * Aa):.2f} ns per component: the special functions, not the bytes, set its time")
    for a in d.values():
        a.free()


if __name__ == "__main__":
    main()
