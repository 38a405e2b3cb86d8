#!/usr/bin/env python3
"""What PPO2 value-loss clipping costs at the bench's C4 configuration (one GPU).

bench.py's C4 update (376 -> 3x512 -> 17, 4096 steps x 256 envs, B = 32768, 10 value + 4 policy epochs, device
shuffle) three ways, alternating, each measurement in a process of its own so that two builds of libppo can be
compared on one box:
  (a) the parent commit's library (--parent-lib: a libppo.so built from the parent commit; omitted: arm skipped),
  (b) this build with clipping off,
  (c) this build with clipping on, default old values (the update's own GAE values), eps_v = 0.2.
Every timed update starts from a fresh synthetic rollout (outside the timed region).  Then, in this build, one
profiled update (PPO_SERIAL=1, events around every launch) with clipping off and one with it on: the clipped
fraction per value epoch (one update per epoch count, from ppo_read_stats out[17] / out[18]) and the per-launch
time of the grad_W launch that carries the value head (ppo_prof_shapes, op 2, engine x3, m = 32768, 512 x 512).

    python tools/vclip_bench.py [--parent-lib PATH] [--rounds 3] [--updates 3] > profiles/vclip_c4.txt
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo.c_amd"))

S, H, A, T, E, B = 376, [512, 512, 512], 17, 4096, 256, 32768
NB = E * T // B
EPS_V = 0.2


def load(path):
    import ppo_ffi
    if path:                                   # another build of the library: the same C ABI, fewer exports
        lib = C.CDLL(path)
        lib.create_ppo.restype = C.c_void_p
        lib.create_ppo.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_float, C.c_float,
                                   C.c_float, C.c_float, C.c_float, C.c_float, C.c_bool]
        lib.ppo_fill_synthetic.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_ulonglong, C.c_float]
        lib.ppo_update.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong]
        lib.free_ppo.argtypes = [C.c_void_p]
        return lib, ppo_ffi
    return ppo_ffi.load(), ppo_ffi


def make(lib, ppo_ffi, seed):
    sizes = [S] + H + [A]
    acts = ["relu"] * len(H) + ["none"]
    C.CDLL("libc.so.6").srand(seed)
    return lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), E * T, 3e-4, 3e-4, 0.95, 0.2, 0.0,
                          1.0, True)


def arm(args):
    """One measurement in this process: warm up, then the mean ms of `updates` timed updates, as JSON."""
    lib, ppo_ffi = load(args.lib)
    if lib.ppo_device_count() < 1:
        raise RuntimeError("vclip_bench: no HIP device visible")
    lib.ppo_set_device(0)
    ppo = make(lib, ppo_ffi, args.seed)
    if args.arm == "c":
        assert lib.ppo_set_value_clip(ppo, EPS_V) == 0
    total = 0.0
    for i in range(args.updates + 1):
        lib.ppo_fill_synthetic(ppo, E, T, args.seed * 1000 + i, 1.0 / 500)
        lib.ppo_synchronize()
        t0 = time.perf_counter()
        lib.ppo_update(ppo, 0.99, B, 4, 10, 1, args.seed)
        lib.ppo_synchronize()
        if i > 0:                                 # update 0 warms up
            total += time.perf_counter() - t0
    lib.free_ppo(ppo)
    print(json.dumps({"arm": args.arm, "ms": 1e3 * total / args.updates}))


def profile(args):
    lib, ppo_ffi = load(None)
    lib.ppo_set_device(0)
    ppo = make(lib, ppo_ffi, args.seed)
    st = (C.c_double * 19)()
    # the clipped fraction per value epoch: updates of 1 … 10 value epochs from the same rollout and parameters
    # would retrain; instead one update per epoch count on a fresh PPO, differences of the exact counters
    lib.ppo_set_value_clip(ppo, EPS_V)
    prev, fracs = (0.0, 0.0), []
    for ne in range(1, 11):
        p2 = make(lib, ppo_ffi, args.seed)
        lib.ppo_set_value_clip(p2, EPS_V)
        lib.ppo_fill_synthetic(p2, E, T, args.seed * 1000, 1.0 / 500)
        lib.ppo_reset_stats(p2)
        lib.ppo_update(p2, 0.99, B, 0, ne, 1, args.seed)
        lib.ppo_read_stats(p2, st, 19)
        fracs.append((st[17] - prev[0]) / max(st[18] - prev[1], 1.0))
        prev = (st[17], st[18])
        lib.free_ppo(p2)
    print("clipped fraction per value epoch (eps_v = 0.2, default old values): " + ", ".join(f"{f:.4f}" for f in fracs))
    os.environ["PPO_SERIAL"] = "1"
    for mode, eps in (("off", 0.0), ("on", EPS_V)):
        lib.ppo_set_value_clip(ppo, eps)
        lib.ppo_fill_synthetic(ppo, E, T, args.seed * 1000 + 7, 1.0 / 500)
        lib.ppo_update(ppo, 0.99, B, 4, 10, 1, args.seed)            # settle
        lib.ppo_fill_synthetic(ppo, E, T, args.seed * 1000 + 8, 1.0 / 500)
        lib.ppo_reset_stats(ppo)
        lib.ppo_prof_enable(1)
        lib.ppo_prof_reset()
        lib.ppo_update(ppo, 0.99, B, 4, 10, 1, args.seed)
        keys, ms, n, work = (C.c_longlong * 64)(), (C.c_double * 64)(), (C.c_long * 64)(), (C.c_double * 64)()
        k = lib.ppo_prof_shapes(keys, ms, n, work, 64)
        cnt = (C.c_long * 7)()
        lib.ppo_prof_counts(cnt)
        lib.ppo_prof_enable(0)
        lib.ppo_read_stats(ppo, st, 19)
        # the value network's last hidden layer: grad_W (op 2), x3 engine, m = B, n = l = 512 — with the policy
        # loop's two 512 x 512 hidden layers this shape has 3 launches per step pair; the value loop's carries
        # the head, so the shape's mean moves by a third of what that launch gains
        for i in range(min(k, 64)):
            op, m_, n_, l_ = (keys[i] >> 60) & 0xF, (keys[i] >> 32) & 0xFFFFFF, (keys[i] >> 16) & 0xFFFF, keys[i] & 0xFFFF
            if op == 2 and m_ == B and n_ == 512 and l_ == 512:
                print(f"clipping {mode:3s}: grad_W 32768 x 512 x 512 (x3): {n[i]} launches, {1e3 * ms[i] / max(n[i], 1):.2f} us "
                      f"per launch; all launches {sum(cnt)}; value steps {st[1]:.0f}, clipped rows {st[17]:.0f} of "
                      f"{st[18]:.0f}")
    lib.free_ppo(ppo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libppo.so built from the parent commit (arm a)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--updates", type=int, default=3, help="timed updates per measurement")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--arm", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--profile", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.arm:
        return arm(args)
    if args.profile:
        return profile(args)
    print(f"C4 [{S}, 512, 512, 512, {A}], N = {E * T}, B = {B}, 10 value + 4 policy epochs ({10 * NB} + {4 * NB} "
          f"minibatch steps per update); each figure the mean of {args.updates} updates in a process of its own")
    arms = [("a", args.parent_lib)] if args.parent_lib else []
    arms += [("b", None), ("c", None)]
    ms = {a: [] for a, _ in arms}
    me = [sys.executable, os.path.abspath(__file__), "--updates", str(args.updates), "--seed", str(args.seed)]
    for _ in range(args.rounds):
        for a, path in arms:
            cmd = me + ["--arm", a] + (["--lib", path] if path else [])
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
            ms[a].append(json.loads(out.strip().splitlines()[-1])["ms"])
    names = {"a": "(a) parent commit", "b": "(b) clipping off", "c": f"(c) clipping on, eps_v = {EPS_V}"}
    med = {}
    for a, _ in arms:
        xs = sorted(ms[a])
        med[a] = xs[len(xs) // 2]
        print(f"{names[a]:32s}: {med[a]:.2f} ms per update (median of {len(xs)}; " + ", ".join(f"{x:.2f}" for x in ms[a]) + ")")
    if "a" in med:
        print(f"(b) / (a) = {med['b'] / med['a']:.4f}; (c) / (b) = {med['c'] / med['b']:.4f}")
    else:
        print(f"(c) / (b) = {med['c'] / med['b']:.4f}")
    sys.stdout.flush()
    subprocess.run(me + ["--profile"], check=True, timeout=600)


if __name__ == "__main__":
    main()
