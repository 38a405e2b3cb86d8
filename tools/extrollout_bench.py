#!/usr/bin/env python3
"""What the open rollout (ppo_rollout_begin / _act / _store / _end) costs against ppo_rollout_device on one GPU.

Both arms step the synthetic environment at bench.py's flagship shape (376 -> 3x512 -> 17, 4096 environments x 256
steps): ppo_rollout_device with its built-in kernel, and the open rollout with the same environment driven from
outside through ppo_env_step_device — per step one launch more for the dense copy of the actions, the store in
place of the built-in environment's own writes, and three calls through ctypes instead of none.  Two PPOs from the
same seed, one per arm, in one process; one warm-up rollout each, then --rollouts timed pairs, alternating, each a
synchronised wall-clock of the whole rollout.  Prints env-steps/s of both arms and their ratio.

    python tools/extrollout_bench.py [--rollouts 7] [--envs 4096 --horizon 256]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppo.c_amd"))

SIZES, KIND, SEED = [376, 512, 512, 512, 17], 1, 7


def make(lib, N):
    import ppo_ffi
    C.CDLL("libc.so.6").srand(1)
    return lib.create_ppo(ppo_ffi.c_strings(["relu"] * (len(SIZES) - 2) + ["none"]), ppo_ffi.c_ints(SIZES), len(SIZES),
                          N, 3e-4, 3e-4, 0.95, 0.2, 0.0, 1.0, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollouts", type=int, default=7)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=256)
    args = ap.parse_args()
    import ppo_ffi
    lib = ppo_ffi.load()
    if lib.ppo_device_count() < 1:
        raise RuntimeError("extrollout_bench: no HIP device visible")
    lib.ppo_set_device(0)
    E, T, S, A = args.envs, args.horizon, SIZES[0], SIZES[-1]
    inner, outer = make(lib, E * T), make(lib, E * T)
    alloc = lambda n, size=4: ppo_ffi.DeviceArray(lib, n * size)
    es, obs, act, nxt, after = alloc(E * S), alloc(E * S), alloc(E * A), alloc(E * S), alloc(E * S)
    rew, term, trunc = alloc(E), alloc(E, 1), alloc(E, 1)
    assert lib.ppo_env_reset_device(KIND, es.ptr, obs.ptr, E, S, SEED) == 0

    def internal():
        lib.ppo_rollout_device(inner, E, T, KIND, SEED)

    first = [True]

    def external():
        assert lib.ppo_rollout_begin(outer, E, T, obs.ptr if first[0] else None, SEED) == 0
        first[0] = False
        for _ in range(T):
            step = lib.ppo_rollout_act(outer, act.ptr)
            lib.ppo_env_step_device(KIND, es.ptr, act.ptr, nxt.ptr, after.ptr, rew.ptr, term.ptr, trunc.ptr, E, S, A, 0,
                                    SEED, step)
            lib.ppo_rollout_store(outer, rew.ptr, nxt.ptr, term.ptr, trunc.ptr, after.ptr)
        assert lib.ppo_rollout_end(outer) == 0

    def timed(fn):
        lib.ppo_synchronize()
        t0 = time.perf_counter()
        fn()
        lib.ppo_synchronize()
        return time.perf_counter() - t0

    arms = {"ppo_rollout_device": internal, "open rollout": external}
    secs = {k: [] for k in arms}
    for i in range(1 + args.rollouts):
        for name, fn in arms.items():
            s = timed(fn)
            if i:
                secs[name].append(s)
    # the two arms must have laid the same rollouts: the figures compare the same work
    hashes = []
    for ppo in (inner, outer):
        b = ppo.contents.buffer.contents
        hashes.append(hash(ppo_ffi.d2h(lib, b.d_reward_p, "float32", E * T).tobytes()
                           + ppo_ffi.d2h(lib, b.d_logprob_p, "float32", E * T).tobytes()))
    assert hashes[0] == hashes[1], "the two arms diverged"
    err = lib.ppo_last_error()
    if err:
        raise RuntimeError(err.decode())
    rate = {k: E * T / statistics.median(v) for k, v in secs.items()}
    res = dict(shape=f"{S} -> {SIZES[1:-1]} -> {A}, {E} environments x {T} steps, synthetic environment",
               rollouts=args.rollouts,
               ms={k: [round(1e3 * x, 2) for x in v] for k, v in secs.items()},
               env_steps_per_s={k: round(v) for k, v in rate.items()},
               ratio_open_over_internal=round(rate["open rollout"] / rate["ppo_rollout_device"], 4))
    print(json.dumps(res))
    for ppo in (inner, outer):
        lib.free_ppo(ppo)


if __name__ == "__main__":
    main()
