"""Time the masked head against the unmasked multi-discrete head of the same build at the same shape (DESIGN.md §4,
"Action masking").

The unmasked head moves 4·(2A + D + 2) bytes per row; the mask adds 4·W, read through a row list — at worst one more
128-byte line per scattered row.  The masks allow each column with p = 0.5 (at least one per component, the chosen one
among them), `rows` is a random permutation of the store's rows.  One process, one device; after warm-up launches
every launch is sampled by ppo_prof_* (class PPO_K_HEAD, events around the launch), one read per launch, the median
over the launches reported with the achieved GB/s on 2·m·A·4 bytes.

    python tools/masked_head_bench.py [--m 32768] [--n 7] [--D 17] [--launches 30] > profiles/masked_head.txt
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


def pack(allowed):
    m, A = allowed.shape
    bits = np.zeros((m, (A + 31) // 32 * 32), np.uint64)
    bits[:, :A] = allowed
    return (bits.reshape(m, -1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


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
    idx = rng.integers(0, args.n, (m, args.D))
    act = np.zeros((m, A), F32)
    act[:, :args.D] = idx
    adv = rng.normal(size=m).astype(F32)
    old = (-np.log(args.n) * args.D + rng.uniform(-0.3, 0.3, m)).astype(F32)
    allowed = rng.random((m, A)) < 0.5
    allowed[np.arange(m)[:, None], np.arange(args.D)[None, :] * args.n + idx] = True
    rows = rng.permutation(m).astype(np.int32)
    store = np.empty((m, (A + 31) // 32), np.uint32)
    store[rows] = pack(allowed)                               # minibatch row i reads store row rows[i]
    full = np.full_like(store, 0xFFFFFFFF)
    d = {k: ppo_ffi.DeviceArray.from_numpy(lib, v)
         for k, v in dict(z=z, act=act, adv=adv, old=old, mask=store, full=full, rows=rows).items()}
    g, lp, H = (ppo_ffi.DeviceArray(lib, 4 * n) for n in (m * A, m, m))
    loss = C.c_double(0)
    c_nvec = ppo_ffi.c_ints(nvec)

    def md():
        assert lib.ppo_multidiscrete_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, m, A, c_nvec,
                                                 args.D, 0.2, 0.01, g.ptr, lp.ptr, H.ptr, C.byref(loss)) == 0

    def masked(mask, rows_ptr):
        assert lib.ppo_masked_head_device(d["z"].ptr, d["act"].ptr, d["adv"].ptr, d["old"].ptr, d[mask].ptr, rows_ptr,
                                          m, A, c_nvec, args.D, 0.2, 0.01, g.ptr, lp.ptr, H.ptr, C.byref(loss)) == 0

    ms, work, n = (C.c_double * 7)(), (C.c_double * 7)(), (C.c_long * 7)()
    med = {}
    print(f"m = {m}, A = {A}: masked head, nvec = [{args.n}]*{args.D}, p = 0.5 masks through a permuted row list, "
          f"against the unmasked multi-discrete head; {2 * m * A * 4 / 1e6:.2f} MB of logits + gradient per launch")
    runs = (("unmasked", md), ("masked p=0.5, permuted rows", lambda: masked("mask", d["rows"].ptr)),
            ("masked full, identity rows", lambda: masked("full", None)), ("unmasked (again)", md))
    for name, fn in runs:
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
        print(f"{name:28s}: median {med[name]:8.2f} us of {len(us)} launches (min {us[0]:.2f}, max {us[-1]:.2f}); "
              f"{2 * m * A * 4 / med[name] / 1e3:7.1f} GB/s")
    base = min(med["unmasked"], med["unmasked (again)"])
    ratio = med["masked p=0.5, permuted rows"] / base
    print(f"masked / unmasked = {ratio:.3f} (target: at most 1.25; byte model 1.12): "
          f"{'met' if ratio <= 1.25 else 'MISSED'}")


if __name__ == "__main__":
    main()
