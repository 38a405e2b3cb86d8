#!/usr/bin/env python3
"""What running reward normalisation (ppo_set_reward_norm, csrc/retnorm.hip) costs on one GPU.

1. The return scan at n = 1,048,576 rows (bench.py's C4 rollout: 256 envs x 4096 steps) against GAE's scan at the
   same n in the same process, by device time: event pairs around every launch libppo times (ppo_prof_*, class
   "gae").  Of the return scan those are its two streaming launches, block aggregates and apply (about 6 B read
   per row each; composition in double); its one-wave carry launch and one-workgroup finish launch carry no
   events.  Of compute_gae_cuda under PPO_GAE_FULL=1 (the two value forwards are GEMM class, no next-value map)
   they are the GAE scan's block aggregates (18 B per row) and apply (26 B per row) and the advantage normalisation
   (8 B per row) — three launches, so GAE's figure is an upper bound of its block + apply; its carry and Welford
   combine carry no events either.  The whole synchronised ppo_reward_returns_device call (four launches, no
   returns written, 24-byte read-back) is timed by wall-clock beside it.
2. bench.py's C4 update (376 -> 3x512 -> 17, 4096 steps x 256 envs, B = 32768, 10 value + 4 policy epochs, device
   shuffle) with the feature off and on, alternating, every timed update on a fresh synthetic rollout (outside
   the timed region): median of --updates.
3. With --parent-lib (a libppo.so built from the parent commit): the same update with the parent's library and
   with this build, feature off, each in a process of its own, alternating for --rounds rounds — the parent's
   own run-to-run spread on this machine is the yardstick for "off costs nothing".

    python tools/rewnorm_bench.py [--reps 10] [--warmup 3] [--updates 5] [--parent-lib PATH --rounds 3] \\
        > profiles/rewnorm_c4.txt
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
        raise RuntimeError("rewnorm_bench: no HIP device visible")
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
    arms = {"parent commit": os.path.abspath(parent_lib), "this build, reward-norm off": ""}
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for name, path in arms.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--update-arm", path, "--updates",
                                  str(updates)], capture_output=True, text=True, check=True).stdout
            ms[name].append(statistics.median(json.loads(out.strip().splitlines()[-1])))
    print(f"\nC4 update, parent commit vs this build with the feature off: {rounds} rounds, alternating, a process per "
          f"arm, each figure the median of {updates} updates")
    for name, v in ms.items():
        print(f"  {name:28s}: median {statistics.median(v):8.2f} ms  run to run {min(v):8.2f} - {max(v):8.2f}  "
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
        raise RuntimeError("rewnorm_bench: no HIP device visible")
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
    assert E * T == ROWS
    out3 = (C.c_double * 3)()

    # --- 1. the scans alone
    def ret_scan():
        assert lib.ppo_reward_returns_device(buf.d_reward_p, buf.d_terminated_p, buf.d_truncated_p, ROWS, 0.99, 0,
                                             None, None, None, None, out3) == 0

    def gae_scan():
        lib.compute_gae_cuda(ppo.contents.V, ppo.contents.buffer, 0.99, 0.95, 0)
        lib.ppo_synchronize()

    def device_ms(fn):
        ms, work, n = (C.c_double * 7)(), (C.c_double * 7)(), (C.c_long * 7)()
        lib.ppo_prof_enable(1)
        fn()                                               # events allocated
        lib.ppo_prof_reset()
        for _ in range(args.reps):
            fn()
        lib.ppo_prof_read(ms, work, n)
        lib.ppo_prof_enable(0)
        return ms[1] / args.reps, n[1] // args.reps, work[1] / args.reps

    med, lo, hi = timed(ret_scan, args.warmup, args.reps)
    print(f"\nscans at n = {ROWS} rows, {args.warmup} warm-up + {args.reps} timed calls")
    print(f"  ppo_reward_returns_device, wall-clock of the synchronised call (4 launches, no returns written): "
          f"median {med * 1e3:.1f} us  min {lo * 1e3:.1f}  max {hi * 1e3:.1f}")
    os.environ["PPO_GAE_FULL"] = "1"
    rows = [("return scan: block + apply", ret_scan), ("GAE: block + apply + normalise", gae_scan)]
    print(f"  device time of the timed launches per call (event pairs, mean of {args.reps} calls)")
    for name, fn in rows:
        ms, count, work = device_ms(fn)
        print(f"    {name:34s} {count} launches  {ms * 1e3:8.1f} us  {work / 1e6:7.1f} MB  "
              f"{work / (ms * 1e-3) / 1e9:7.0f} GB/s")
    del os.environ["PPO_GAE_FULL"]

    # --- 2. the whole update, feature off / on, alternating
    def update(on, seed):
        lib.ppo_set_reward_norm(ppo, 10.0 if on else 0.0)
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
        print(f"  reward-norm {'on ' if on else 'off'}: median {statistics.median(v):8.2f} ms  min {min(v):8.2f}  "
              f"max {max(v):8.2f}")
    print(f"  difference of medians: {statistics.median(ts[1]) - statistics.median(ts[0]):+.2f} ms")
    st = (C.c_double * 25)()
    lib.ppo_read_stats(ppo, st, 25)
    print(f"  last update: running count {st[22]:.0f}, clamped {st[23]:.0f} of {st[24]:.0f} rewards, "
          f"scale {lib.ppo_reward_norm_scale(ppo):.6g}")
    err = lib.ppo_last_error()
    if err:
        raise RuntimeError(err.decode())
    lib.free_ppo(ppo)
    if args.parent_lib:
        parent_vs_this(args.parent_lib, args.rounds, args.updates)


if __name__ == "__main__":
    main()
