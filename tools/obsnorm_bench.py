#!/usr/bin/env python3
"""What running observation normalisation (ppo_set_obs_norm, csrc/obsnorm.hip) costs on one GPU.

1. The kernels alone at the bench rollout's shape, 1,048,576 x 376 fp32 (1.58 GB), in one process: the normalise
   launch (read + write, out of place and in place), the statistics launches (read only) and a ppo_d2d of the same
   bytes (read + write) as the yardstick.  Each call synchronises; wall-clock around it, `--warmup` calls
   first, then `--reps` timed ones: median, min and max.  Rates count the bytes each one moves (normalise and the
   copy 2 x 1.58 GB, the statistics 1 x); the goal for the kernels is >= 0.8 of the copy's rate.
2. bench.py's C4 update (376 -> 3x512 -> 17, 4096 steps x 256 envs, B = 32768, 10 value + 4 policy epochs, device
   shuffle) with the feature off and on, alternating, every timed update on a fresh synthetic rollout (outside
   the timed region).
3. With --parent-lib (a libppo.so built from the parent commit): the same update with the parent's library and
   with this build, feature off, each in a process of its own, alternating for --rounds rounds — the parent's
   own run-to-run spread on this machine is the yardstick for "off costs nothing".
Section 1 is followed by the same calls timed on the device (event pairs around every launch), which separates
the statistics' streaming launch from its partials fold and from the synchronise and read-back.

    python tools/obsnorm_bench.py [--reps 10] [--warmup 3] [--updates 5] [--parent-lib PATH --rounds 3] \\
        > profiles/obsnorm_c4.txt
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo.c_amd"))

S, H, A, T, E, B = 376, [512, 512, 512], 17, 4096, 256, 32768
ROWS = 1 << 20


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def update_arm(path, updates):
    """One process, one library (path: another build of libppo with the same C ABI, "" = this build), the
    feature off: two warm-up updates, then `updates` timed ones, each on a fresh synthetic rollout; prints the
    ms as JSON."""
    import ppo_ffi
    if path:
        lib = C.CDLL(path)
        lib.create_ppo.restype = C.c_void_p
        lib.create_ppo.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_float, C.c_float,
                                   C.c_float, C.c_float, C.c_float, C.c_float, C.c_bool]
        lib.ppo_fill_synthetic.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_ulonglong, C.c_float]
        lib.ppo_update.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong]
        lib.free_ppo.argtypes = [C.c_void_p]
    else:
        lib = ppo_ffi.load()
    if lib.ppo_device_count() < 1:
        raise RuntimeError("obsnorm_bench: no HIP device visible")
    lib.ppo_set_device(0)
    sizes = [S] + H + [A]
    C.CDLL("libc.so.6").srand(1)
    ppo = lib.create_ppo(ppo_ffi.c_strings(["relu"] * len(H) + ["none"]), ppo_ffi.c_ints(sizes), len(sizes), E * T,
                         3e-4, 3e-4, 0.95, 0.2, 0.0, 1.0, True)
    ms = []
    for i in range(2 + updates):
        lib.ppo_fill_synthetic(ppo, E, T, 10 + i, 1.0 / 1000)
        lib.ppo_synchronize()
        t0 = time.perf_counter()
        lib.ppo_update(ppo, 0.99, B, 4, 10, 1, 7)
        lib.ppo_synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    lib.free_ppo(ppo)
    print(json.dumps(ms[2:]))


def parent_vs_this(parent_lib, rounds, updates):
    """The parent commit's library against this build with the feature off: each arm in a process of its own,
    alternating, `rounds` times on this machine."""
    arms = {"parent commit": os.path.abspath(parent_lib), "this build, obs-norm off": ""}
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for name, path in arms.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--update-arm", path, "--updates",
                                  str(updates)], capture_output=True, text=True, check=True).stdout
            ms[name].append(statistics.median(json.loads(out.strip().splitlines()[-1])))
    print(f"\nC4 update, parent commit vs this build with the feature off: {rounds} rounds, alternating, a process per "
          f"arm, each figure the median of {updates} updates")
    for name, v in ms.items():
        print(f"  {name:26s}: median {statistics.median(v):8.2f} ms  run to run {min(v):8.2f} - {max(v):8.2f}  "
              f"({', '.join(f'{x:.2f}' for x in v)})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", help="a libppo.so built from the parent commit: adds the parent-vs-this arm")
    ap.add_argument("--update-arm", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.update_arm is not None:
        return update_arm(args.update_arm, args.updates)
    import ppo_ffi
    lib = ppo_ffi.load()
    if lib.ppo_device_count() < 1:
        raise RuntimeError("obsnorm_bench: no HIP device visible")
    lib.ppo_set_device(0)
    print(lib.ppo_build_info().decode())

    sizes = [S] + H + [A]
    acts = ["relu"] * len(H) + ["none"]
    C.CDLL("libc.so.6").srand(1)
    ppo = lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), E * T, 3e-4, 3e-4, 0.95, 0.2, 0.0,
                         1.0, True)
    lib.ppo_fill_synthetic(ppo, E, T, 1, 1.0 / 1000)
    lib.ppo_synchronize()
    buf = ppo.contents.buffer.contents
    nbytes = ROWS * S * 4
    assert E * T == ROWS
    scratch = lib.ppo_dev_alloc(nbytes)
    out = (C.c_double * (1 + 2 * S))()

    # --- 1. the kernels alone
    assert lib.ppo_set_obs_norm(ppo, 10.0) == 0
    assert lib.ppo_obs_norm_fold_buffer(ppo) == 0          # a warmed normaliser: the clamp is live
    lib.ppo_synchronize()
    rows = [
        ("ppo_d2d (yardstick)", 2, lambda: lib.ppo_d2d(scratch, buf.d_state_p, nbytes)),
        ("normalise, out of place", 2, lambda: lib.ppo_obs_normalize_device(ppo, buf.d_state_p, scratch, ROWS)),
        ("normalise, in place", 2, lambda: lib.ppo_obs_normalize_device(ppo, scratch, scratch, ROWS)),
        ("statistics (2 launches + 6 KB read-back)", 1, lambda: lib.ppo_obs_stats_device(buf.d_state_p, ROWS, S, out)),
    ]
    print(f"\nkernels at {ROWS} x {S} fp32 ({nbytes / 1e9:.3f} GB), {args.warmup} warm-up + {args.reps} timed calls")
    print(f"{'':44s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'GB/s':>8s} {'vs copy':>8s}")
    copy_rate = None
    for name, passes, fn in rows:
        med, lo, hi = timed(fn, args.warmup, args.reps)
        rate = passes * nbytes / (med * 1e-3) / 1e9
        copy_rate = copy_rate or rate
        print(f"{name:44s} {med:10.3f} {lo:8.3f} {hi:8.3f} {rate:8.0f} {rate / copy_rate:8.2f}")

    # the same calls by device time: HIP events around every launch (ppo_prof_*), per kernel class — the streaming
    # launches are class "other", the small combines (partials fold, rank fold, affine) class "gae"
    def device_ms(fn):
        ms, work, n = (C.c_double * 7)(), (C.c_double * 7)(), (C.c_long * 7)()
        lib.ppo_prof_enable(1)
        fn()                                               # events allocated
        lib.ppo_prof_reset()
        for _ in range(args.reps):
            fn()
        lib.ppo_prof_read(ms, work, n)
        lib.ppo_prof_enable(0)
        return {k: (ms[i] / n[i], n[i] // args.reps) for k, i in (("other", 6), ("gae", 1)) if n[i]}

    print(f"\ndevice time per launch (event pairs, mean of {args.reps} calls)")
    for name, passes, fn in rows[1:]:
        for cls, (per, count) in device_ms(fn).items():
            what = "streaming launch" if cls == "other" else "partials fold (16 x 16 threads per 16 columns)"
            rate = f"{passes * nbytes / (per * 1e-3) / 1e9:6.0f} GB/s  {passes * nbytes / (per * 1e-3) / 1e9 / copy_rate:4.2f} of the copy" \
                if cls == "other" else ""
            print(f"  {name:44s} {what:48s} {count} x {per * 1e3:8.1f} us  {rate}")
    lib.ppo_dev_free(scratch)

    # --- 2. the whole update, feature off / on, alternating
    def update(on, seed):
        lib.ppo_set_obs_norm(ppo, 10.0 if on else 0.0)
        lib.ppo_fill_synthetic(ppo, E, T, seed, 1.0 / 1000)
        lib.ppo_synchronize()
        t0 = time.perf_counter()
        lib.ppo_update(ppo, 0.99, B, 4, 10, 1, 7)
        lib.ppo_synchronize()
        return (time.perf_counter() - t0) * 1e3

    for on in (0, 1, 0, 1):                                # warm-up: workspaces, the shadow, clocks
        update(on, 2)
    ts = {0: [], 1: []}
    for i in range(args.updates):
        for on in (0, 1):
            ts[on].append(update(on, 10 + i))
    print(f"\nC4 update, B = {B}, 10 value + 4 policy epochs, {args.updates} timed updates each, alternating")
    for on in (0, 1):
        v = ts[on]
        print(f"  obs-norm {'on ' if on else 'off'}: median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  "
              f"max {max(v):8.2f}")
    print(f"  difference of medians: {statistics.median(ts[1]) - statistics.median(ts[0]):+.2f} ms")
    st = (C.c_double * 22)()
    lib.ppo_read_stats(ppo, st, 22)
    print(f"  last update: running count {st[19]:.0f}, clamped {st[20]:.0f} of {st[21]:.0f} elements")
    err = lib.ppo_last_error()
    if err:
        raise RuntimeError(err.decode())
    lib.free_ppo(ppo)
    if args.parent_lib:
        parent_vs_this(args.parent_lib, args.rounds, args.updates)


if __name__ == "__main__":
    main()
