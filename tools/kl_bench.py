#!/usr/bin/env python3
"""What target-KL early stopping costs, and saves, at the bench's C4 configuration (one GPU, one process).

bench.py's C4 update (376 -> 3x512 -> 17, 4096 steps x 256 envs, B = 32768, 10 value + 4 policy epochs,
device shuffle) under three settings, alternating: off, target_kl = +inf (measure only) and a target chosen
from a monitor run's KL history so that the update stops in its second policy epoch.  Every timed update
starts from a fresh synthetic rollout of the current policy (outside the timed region), so its KL starts at
zero as in training.  Then one profiled update of each kind (PPO_SERIAL=1, events around every launch) for
the PPO_K_ADAM class: the Adam kernel's us per launch from the off update, the KL kernel's from the class's
extra time and extra launches in monitor mode, and the class's launches in the stopped update.

    python tools/kl_bench.py [--rounds 3] [--updates 2] > profiles/kl_c4.txt

--estimators times, instead, the same update with the monitor on (target_kl = +inf) under the k3 estimator and under
the closed-form one (ppo_set_kl_estimator), alternating on the same build: the cost of the whole-buffer μ forward at
the head of the update plus the wider per-step KL launch.

    python tools/kl_bench.py --estimators > profiles/kl_exact_c4.txt
"""
import argparse
import ctypes as C
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo.c_amd"))
import ppo_ffi  # noqa: E402

S, H, A, T, E, B = 376, [512, 512, 512], 17, 4096, 256, 32768
NB = E * T // B
K_ADAM = 2
MODES = ("off", "inf", "stop")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="off / +inf / stop alternations")
    ap.add_argument("--updates", type=int, default=2, help="timed updates per measurement")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--estimators", action="store_true", help="time k3 against the closed-form estimator instead")
    args = ap.parse_args()
    lib = ppo_ffi.load()
    if lib.ppo_device_count() < 1:
        raise RuntimeError("kl_bench: no HIP device visible")
    lib.ppo_set_device(0)
    sizes = [S] + H + [A]
    acts = ["relu"] * len(H) + ["none"]
    C.CDLL("libc.so.6").srand(args.seed)
    ppo = lib.create_ppo(ppo_ffi.c_strings(acts), ppo_ffi.c_ints(sizes), len(sizes), E * T, 3e-4, 3e-4, 0.95, 0.2, 0.0,
                         1.0, True)
    fills = [0]

    def rollout():
        fills[0] += 1
        lib.ppo_fill_synthetic(ppo, E, T, args.seed * 1000 + fills[0], 1.0 / 500)
        lib.ppo_synchronize()

    def update():
        lib.ppo_update(ppo, 0.99, B, 4, 10, 1, args.seed)

    def stats():
        st = (C.c_double * 17)()
        lib.ppo_read_stats(ppo, st, 17)
        return list(st)

    print(f"C4 {sizes}, N = {E * T}, B = {B}, 10 value + 4 policy epochs ({10 * NB} + {4 * NB} minibatch steps per update)")
    rollout()
    update()                                              # warm-up
    lib.ppo_synchronize()
    if args.estimators:
        estimators(lib, ppo, args, rollout, update)
        lib.free_ppo(ppo)
        return

    # the target: from a monitor run, the first step of the second policy epoch or later whose KL stands above
    # every earlier step's; 1.5 x target at the geometric middle of that gap
    lib.ppo_set_target_kl(ppo, float("inf"))
    rollout()
    update()
    hist = (C.c_double * (4 * NB))()
    n = lib.ppo_kl_history(ppo, hist, 4 * NB)
    h = list(hist[:n])
    s = next((k for k in range(NB, n) if h[k] > max(h[:k])), None)
    if s is None:
        raise RuntimeError(f"kl_bench: the KL never rises past the first epoch's maximum: {h}")
    target = math.sqrt(max(h[:s]) * h[s]) / 1.5
    print(f"monitor run: KL per step, epoch ends: " + ", ".join(f"{h[k]:.3e}" for k in range(NB - 1, n, NB))
          + f"; step {s} ({h[s]:.3e}) first exceeds the earlier maximum {max(h[:s]):.3e}: target_kl = {target:.4e}")
    setting = {"off": 0.0, "inf": float("inf"), "stop": target}

    ms = {m: [] for m in MODES}
    stops = []
    for _ in range(args.rounds):
        for mode in MODES:
            lib.ppo_set_target_kl(ppo, setting[mode])
            rollout()
            update()                                      # settle into the mode
            lib.ppo_synchronize()
            total = 0.0
            for _ in range(args.updates):
                rollout()
                lib.ppo_reset_stats(ppo)
                t0 = time.perf_counter()
                update()
                lib.ppo_synchronize()
                total += time.perf_counter() - t0
                if mode == "stop":
                    st = stats()
                    stops.append((int(st[16]), int(st[3])))
            ms[mode].append(1e3 * total / args.updates)
    for mode in MODES:
        xs = sorted(ms[mode])
        print(f"target_kl {mode:4s}: {xs[len(xs) // 2]:.2f} ms per update (median of {len(xs)}; "
              + ", ".join(f"{x:.2f}" for x in ms[mode]) + ")")
    print("stopped updates (stop step, policy steps issued of 128): " + ", ".join(f"{a} / {b}" for a, b in stops))

    os.environ["PPO_SERIAL"] = "1"
    prof = {}
    for mode in MODES:
        lib.ppo_set_target_kl(ppo, setting[mode])
        rollout()
        lib.ppo_reset_stats(ppo)
        lib.ppo_prof_enable(1)
        lib.ppo_prof_reset()
        update()
        t_ms, work, launches = (C.c_double * 7)(), (C.c_double * 7)(), (C.c_long * 7)()
        lib.ppo_prof_read(t_ms, work, launches)
        lib.ppo_prof_enable(0)
        prof[mode] = (t_ms[K_ADAM], launches[K_ADAM], work[K_ADAM], sum(t_ms), sum(launches), stats())
    del os.environ["PPO_SERIAL"]
    t0_, l0, w0, all0, n0, _ = prof["off"]
    t1, l1, w1, all1, n1, st1 = prof["inf"]
    t2, l2, _, all2, n2, st2 = prof["stop"]
    print(f"PPO_K_ADAM, off:  {l0} launches, {t0_:.3f} ms: Adam {1e3 * t0_ / max(l0, 1):.2f} us per launch "
          f"({w0 / max(l0, 1) / 1e6:.2f} MB each); all classes {n0} launches, {all0:.2f} ms")
    extra = l1 - l0
    print(f"PPO_K_ADAM, +inf: {l1} launches, {t1:.3f} ms: the {extra} KL launches take "
          f"{1e3 * (t1 - t0_) / max(extra, 1):.2f} us each ({(w1 - w0) / max(extra, 1) / 1e6:.2f} MB each; the class's "
          f"extra time over its extra launches); all classes {n1} launches, {all1:.2f} ms; last KL {st1[13]:.4e}, "
          f"clip fraction {st1[14]:.4f}")
    print(f"PPO_K_ADAM, stop: {l2} launches, {t2:.3f} ms; all classes {n2} launches, {all2:.2f} ms; stop step "
          f"{st2[16]:.0f}, policy steps issued {st2[3]:.0f} of {4 * NB}, applied {st2[15]:.0f}")
    lib.free_ppo(ppo)


def estimators(lib, ppo, args, rollout, update):
    """monitor on (+inf), k3 against the closed-form estimator, alternating; then one profiled update of each"""
    names = {0: "k3", 1: "exact"}
    lib.ppo_set_target_kl(ppo, float("inf"))
    ms = {0: [], 1: []}
    last = {}
    for _ in range(args.rounds):
        for est in (0, 1):
            assert lib.ppo_set_kl_estimator(ppo, est) == 0
            rollout()
            update()                                      # settle into the mode (the store is allocated here)
            lib.ppo_synchronize()
            total = 0.0
            for _ in range(args.updates):
                rollout()
                lib.ppo_reset_stats(ppo)
                t0 = time.perf_counter()
                update()
                lib.ppo_synchronize()
                total += time.perf_counter() - t0
            ms[est].append(1e3 * total / args.updates)
            st = (C.c_double * 34)()
            lib.ppo_read_stats(ppo, st, 34)
            last[est] = (st[13], st[33])
    med = {}
    for est in (0, 1):
        xs = sorted(ms[est])
        med[est] = xs[len(xs) // 2]
        print(f"monitor on, estimator {names[est]:5s}: {med[est]:.2f} ms per update (median of {len(xs)}; "
              + ", ".join(f"{x:.2f}" for x in ms[est]) + f"); last step: deciding KL {last[est][0]:.4e}"
              + (f", k3 beside it {last[est][1]:.4e}" if est else ""))
    print(f"exact − k3: {med[1] - med[0]:+.2f} ms per update ({100 * (med[1] / med[0] - 1):+.2f} %)")
    os.environ["PPO_SERIAL"] = "1"
    prof = {}
    for est in (0, 1):
        lib.ppo_set_kl_estimator(ppo, est)
        rollout()
        lib.ppo_prof_enable(1)
        lib.ppo_prof_reset()
        update()
        t_ms, work, launches = (C.c_double * 7)(), (C.c_double * 7)(), (C.c_long * 7)()
        lib.ppo_prof_read(t_ms, work, launches)
        lib.ppo_prof_enable(0)
        prof[est] = (list(t_ms), list(launches))
    del os.environ["PPO_SERIAL"]
    for est in (0, 1):
        t, n = prof[est]
        print(f"profiled (serial), estimator {names[est]:5s}: all classes {sum(n)} launches, {sum(t):.2f} ms; "
              f"PPO_K_ADAM (Adam + KL) {n[K_ADAM]} launches, {t[K_ADAM]:.3f} ms")
    dn = [a - b for a, b in zip(prof[1][1], prof[0][1])]
    dt = [a - b for a, b in zip(prof[1][0], prof[0][0])]
    print("exact − k3 by class (launches, ms): " + ", ".join(f"[{k}] {dn[k]:+d}, {dt[k]:+.3f}" for k in range(7)))


if __name__ == "__main__":
    main()
