#!/usr/bin/env python3
"""Time the orthogonal initialisation (csrc/ortho.hip): ppo_init_orthogonal on the C4 networks that bench.py builds
(376 → 3×512 → 17 and → 1: eight matrices, one launch) and ppo_orthogonal_device at the largest supported shape,
4096 × 1024.  Three runs after one warm-up each, under libppo's own device events (ppo_prof_enable: an event pair
around the launch, class OTHER), so the figure is the kernel's time and not the entry's allocations.

    python tools/ortho_bench.py > profiles/ortho_init.txt
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo.c_amd"))
import ppo_ffi  # noqa: E402

K_OTHER, K_COUNT = 6, 7


def main():
    lib = ppo_ffi.load()
    lib.ppo_set_device(0)

    def timed(fn):
        t_ms, work, launches = (C.c_double * K_COUNT)(), (C.c_double * K_COUNT)(), (C.c_long * K_COUNT)()
        lib.ppo_prof_enable(1)
        lib.ppo_prof_reset()
        fn()
        lib.ppo_prof_read(t_ms, work, launches)
        lib.ppo_prof_enable(0)
        assert launches[K_OTHER] == 1, launches[K_OTHER]
        return t_ms[K_OTHER]

    sizes = [376, 512, 512, 512, 17]
    ppo = lib.create_ppo(ppo_ffi.c_strings(["relu"] * 3 + ["none"]), ppo_ffi.c_ints(sizes), len(sizes), 4096, 3e-4, 3e-4,
                         0.95, 0.2, 0.0, 1.0, True)

    def init():
        assert lib.ppo_init_orthogonal(ppo, 1, float(np.sqrt(2)), 0.01, 1.0) == 0

    G = ppo_ffi.DeviceArray.from_numpy(lib, np.random.default_rng(0).standard_normal((4096, 1024)).astype(np.float32))

    def largest():
        assert lib.ppo_orthogonal_device(G.ptr, 4096, 1024, 1.0) == 0

    for name, fn in (("ppo_init_orthogonal, C4 networks (8 matrices)", init), ("ppo_orthogonal_device, 4096 x 1024", largest)):
        fn()
        runs = [timed(fn) for _ in range(3)]
        print(f"{name}: {', '.join(f'{t:.2f}' for t in runs)} ms")
    G.free()
    lib.free_ppo(ppo)


if __name__ == "__main__":
    main()
