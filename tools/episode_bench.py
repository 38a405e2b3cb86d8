#!/usr/bin/env python3
"""What the episode statistics (ppo_episode_stats, csrc/episode.hip) cost ppo_rollout_device on one GPU.

1. The scan alone through ppo_episode_scan_device (synchronised wall-clock of the whole call: two launches and a
   56-byte read-back) over a rollout's own rewards and flags, at bench.py's C4 shape (256 environments x 4096
   steps: four single-wave workgroups, the scan's worst case for parallelism) and over the same bytes read as
   4096 environments x 256 steps (64 workgroups).
2. ppo_rollout_device at bench.py's C4 synthetic shape (376 -> 3x512 -> 17, 256 environments x 4096 steps) and at
   Pendulum-v1 (3 -> 2x64 -> 1, 1024 environments x 256 steps): one warm-up rollout, then --rollouts timed ones,
   synchronised wall-clock.
3. With --parent-lib (a libppo.so built from the parent commit): the same rollouts with the parent's library and
   with this build, each in a process of its own, alternating for --rounds rounds — the parent's own run-to-run
   spread on this machine is the yardstick for "the scan costs nothing".

    python tools/episode_bench.py [--reps 20] [--rollouts 5] [--parent-lib PATH --rounds 3] \\
        > profiles/episode_rollout_ab.txt
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

SHAPES = {"synthetic C4": dict(sizes=[376, 512, 512, 512, 17], E=256, T=4096, kind=1),
          "pendulum": dict(sizes=[3, 64, 64, 1], E=1024, T=256, kind=0)}


def open_lib(path):
    """path: another build of libppo with the same C ABI for what is called here, "" = this build."""
    import ppo_ffi
    if not path:
        return ppo_ffi.load()
    lib = C.CDLL(path)
    lib.create_ppo.restype = C.c_void_p
    lib.create_ppo.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_float, C.c_float,
                               C.c_float, C.c_float, C.c_float, C.c_float, C.c_bool]
    lib.ppo_rollout_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_ulonglong]
    lib.free_ppo.argtypes = [C.c_void_p]
    return lib


def make(lib, cfg):
    import ppo_ffi
    sizes = cfg["sizes"]
    C.CDLL("libc.so.6").srand(1)
    return lib.create_ppo(ppo_ffi.c_strings(["relu"] * (len(sizes) - 2) + ["none"]), ppo_ffi.c_ints(sizes), len(sizes),
                          cfg["E"] * cfg["T"], 3e-4, 3e-4, 0.95, 0.2, 0.0, 1.0, True)


def rollout_arm(path, rollouts):
    """One process, one library: per shape one warm-up rollout, then `rollouts` timed ones; prints the ms as JSON."""
    lib = open_lib(path)
    if lib.ppo_device_count() < 1:
        raise RuntimeError("episode_bench: no HIP device visible")
    lib.ppo_set_device(0)
    out = {}
    for name, cfg in SHAPES.items():
        ppo = make(lib, cfg)
        ms = []
        for _ in range(1 + rollouts):
            lib.ppo_synchronize()
            t0 = time.perf_counter()
            lib.ppo_rollout_device(ppo, cfg["E"], cfg["T"], cfg["kind"], 7)
            lib.ppo_synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        lib.free_ppo(ppo)
        out[name] = ms[1:]
    print(json.dumps(out))


def run_arm(path, rollouts):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rollout-arm", path, "--rollouts", str(rollouts)],
                         capture_output=True, text=True, check=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rollouts", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", help="a libppo.so built from the parent commit: adds the parent-vs-this arm")
    ap.add_argument("--rollout-arm", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.rollout_arm is not None:
        return rollout_arm(args.rollout_arm, args.rollouts)
    import ppo_ffi
    lib = ppo_ffi.load()
    if lib.ppo_device_count() < 1:
        raise RuntimeError("episode_bench: no HIP device visible")
    lib.ppo_set_device(0)
    print(lib.ppo_build_info().decode())

    # --- 1. the scan alone, over a rollout's own rewards and flags
    cfg = SHAPES["synthetic C4"]
    ppo = make(lib, cfg)
    lib.ppo_rollout_device(ppo, cfg["E"], cfg["T"], cfg["kind"], 7)
    lib.ppo_synchronize()
    buf = ppo.contents.buffer.contents
    out = (C.c_double * 7)()
    print(f"\nppo_episode_scan_device, synchronised wall-clock of the whole call, {args.reps} timed calls after 3")
    for E, T in ((cfg["E"], cfg["T"]), (cfg["T"], cfg["E"])):
        ts = []
        for i in range(3 + args.reps):
            t0 = time.perf_counter()
            assert lib.ppo_episode_scan_device(buf.d_reward_p, buf.d_terminated_p, buf.d_truncated_p, None, E, T, 0.99,
                                               None, None, None, out) == 0
            ts.append((time.perf_counter() - t0) * 1e6)
        ts = ts[3:]
        print(f"  {E:5d} environments x {T:5d} rows ({6e-6 * E * T:.1f} MB read): median {statistics.median(ts):8.1f} us  "
              f"min {min(ts):8.1f}  max {max(ts):8.1f}   ({out[0]:.0f} episodes)")
    st = (C.c_double * 16)()
    lib.ppo_episode_stats(ppo, st, 16)
    print(f"  the rollout's own tracker: {st[8]:.0f} episodes, mean return {st[9]:.4f}, mean length {st[13]:.1f}")
    lib.free_ppo(ppo)

    # --- 2. / 3. the rollout, this build alone or against the parent's library
    arms = {"this build": ""}
    if args.parent_lib:
        arms = {"parent commit": os.path.abspath(args.parent_lib), "this build": ""}
    rounds = args.rounds if args.parent_lib else 1
    ms = {k: {s: [] for s in SHAPES} for k in arms}
    for _ in range(rounds):
        for name, path in arms.items():
            res = run_arm(path, args.rollouts)
            for s in SHAPES:
                ms[name][s].append(statistics.median(res[s]))
    print(f"\nppo_rollout_device: {rounds} round(s), alternating, a process per arm, each figure the median of "
          f"{args.rollouts} rollouts after one warm-up")
    for s, cfg in SHAPES.items():
        print(f"  {s}: {cfg['sizes'][0]} -> {cfg['sizes'][1:-1]} -> {cfg['sizes'][-1]}, {cfg['E']} environments x "
              f"{cfg['T']} steps")
        for name in arms:
            v = ms[name][s]
            print(f"    {name:14s}: median {statistics.median(v):9.2f} ms  run to run {min(v):9.2f} - {max(v):9.2f}  "
                  f"({', '.join(f'{x:.2f}' for x in v)})")
    err = lib.ppo_last_error()
    if err:
        raise RuntimeError(err.decode())


if __name__ == "__main__":
    main()
