"""Learning-rate schedules on the CPU (ppo_set_lr_schedule; DESIGN.md §4 "Learning-rate schedules").

The numpy model's own properties (tests/lr_schedule_ref.py: the adaptive rule, the coupling expression, the linear
formula), the new symbols in the headers and the binding, and the checkpoint container's schedule section through the
stand-alone validator build of test_checkpoint_cpu.py (its `dump` fixture: host C compiler, its own main, sanitizers
where they link).  The setter's return codes need a PPO, which needs a device: tests/test_gpu_lr_schedule.py.
"""
import math
import os
import re
import struct

import numpy as np

import checkpoint_ref as ck
import lr_schedule_ref as lr
from test_checkpoint_cpu import dump, small_sections  # noqa: F401  (dump: the validator fixture)

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LRSCHED, F_LRSCHED = 7, 4


# ----------------------------------------------------------------------------- the model
def test_rule_clamps_at_both_ends():
    lo, hi = F32(1e-5), F32(1e-2)
    assert lr.adapt_step(1.2e-5, 1.0, 0.01, lo, hi) == (lo, 0, 1)            # 1.2e-5 / 1.5 < lr_min
    assert lr.adapt_step(lo, 1.0, 0.01, lo, hi) == (lo, 0, 1)                # at the floor: counted, unchanged
    assert lr.adapt_step(8e-3, 1e-4, 0.01, lo, hi) == (hi, 1, 0)             # 8e-3 · 1.5 > lr_max
    assert lr.adapt_step(hi, 1e-4, 0.01, lo, hi) == (hi, 1, 0)
    got = lr.adapt_step(3e-4, 1.0, 0.01, lo, hi)[0]
    assert got.dtype == F32 and got == F32(3e-4) / F32(1.5)
    got = lr.adapt_step(3e-4, 1e-4, 0.01, lo, hi)[0]
    assert got.dtype == F32 and got == F32(3e-4) * F32(1.5)
    assert lr.initial_lr(1.0, lo, hi) == hi and lr.initial_lr(0.0, lo, hi) == lo and lr.initial_lr(3e-4, lo, hi) == F32(3e-4)


def test_rule_edges_of_the_band():
    """strict comparisons against 2·desired and desired/2 in fp32; NaN and zero are inert"""
    want, lo, hi = F32(0.01), F32(1e-6), F32(1.0)
    base = F32(3e-4)
    assert lr.adapt_step(base, F32(2.0) * want, want, lo, hi) == (base, 0, 0)
    assert lr.adapt_step(base, np.nextafter(F32(2.0) * want, F32(1)), want, lo, hi)[2] == 1
    assert lr.adapt_step(base, F32(0.5) * want, want, lo, hi) == (base, 0, 0)
    assert lr.adapt_step(base, np.nextafter(F32(0.5) * want, F32(0)), want, lo, hi)[1] == 1
    assert lr.adapt_step(base, float("nan"), want, lo, hi) == (base, 0, 0)
    assert lr.adapt_step(base, 0.0, want, lo, hi) == (base, 0, 0)            # kl == 0 never raises
    assert lr.adapt_step(base, -0.0, want, lo, hi) == (base, 0, 0)
    assert lr.adapt_step(base, 1e-45, want, lo, hi)[1] == 1                  # the smallest positive kl does
    assert lr.adapt_step(base, float("inf"), want, lo, hi)[2] == 1
    hist, last, up, down = lr.replay(base, [float("nan")] * 5 + [0.0] * 5, want, lo, hi)
    assert (hist == base).all() and last == base and (up, down) == (0, 0)


def test_repeated_lowering_reaches_the_floor_and_stays():
    """from 3e-4 under lr_min = 1e-5: 3e-4 / 1.5^k <= 1e-5 first at k = ceil(log(30) / log(1.5)) = 9"""
    k = math.ceil(math.log(3e-4 / 1e-5) / math.log(1.5))
    assert k == 9 and lr.steps_to_floor(3e-4, 1e-5) == k
    hist, last, up, down = lr.replay(3e-4, [1.0] * 12, 1e-3, 1e-5, 1.0)
    assert hist.dtype == F32 and (hist[:k - 1] > F32(1e-5)).all() and (hist[k - 1:] == F32(1e-5)).all()
    assert np.all(np.diff(hist[:k]) < 0) and last == F32(1e-5) and (up, down) == (0, 12)
    # every step is one fp32 division: the history is the chain of correctly rounded quotients
    x = F32(3e-4)
    for h in hist[:k - 1]:
        x = x / F32(1.5)
        assert h == x


def test_replay_freezes_behind_a_stop():
    kls = [1.0, 1.0, 1e-9, 1.0, 1e-9]
    free = lr.replay(3e-4, kls, 1e-3, 1e-6, 1.0)
    held = lr.replay(3e-4, kls, 1e-3, 1e-6, 1.0, stop_step=1)
    assert (held[0][:2] == free[0][:2]).all() and (held[0][2:] == held[0][1]).all()
    assert held[1] == held[0][1] and held[2:] == (0, 2) and free[2:] == (2, 3)


def test_coupling_expression():
    lo, hi = 1e-5, 1e-2
    assert lr.coupled_value_lr(1e-3, 3e-4, 3e-4, lo, hi) == F32(1e-3)        # ratio exactly 1
    got = lr.coupled_value_lr(1e-3, F32(3e-4) / F32(1.5), 3e-4, lo, hi)
    assert got.dtype == F32 and got == F32(1e-3) * ((F32(3e-4) / F32(1.5)) / F32(3e-4))
    assert lr.coupled_value_lr(1e-3, hi, 1.0, lo, hi) == F32(1e-3)           # the base is the clamped one


def test_linear_endpoints_and_shape():
    for base in (3e-4, 1e-3, 2.5e-4, 0.1):
        for N in (1, 3, 4, 7, 1000):
            for f in (0.0, 0.1, 0.5, 1.0):
                assert lr.linear_lr(base, 0, N, f).tobytes() == F32(base).tobytes()          # u = 0: the base, bit for bit
                end = F32(float(F32(base)) * float(F32(f)))
                for u in (N, N + 1, 10 * N):
                    assert lr.linear_lr(base, u, N, f).tobytes() == end.tobytes(), (base, N, f, u)
                seq = [float(lr.linear_lr(base, u, N, f)) for u in range(N + 2)]
                assert all(a >= b for a, b in zip(seq, seq[1:]))
    assert lr.linear_lr(3e-4, 2, 4, 0.1) == F32(float(F32(3e-4)) * (1.0 - (1.0 - float(F32(0.1))) * 0.5))


# ----------------------------------------------------------------------------- headers and binding
def test_new_symbols_are_declared():
    """fails on a tree without the feature: the public header, the binding and the record"""
    ext = open(os.path.join(ROOT, "include", "ppo_ext.h")).read()
    assert re.search(r"enum\s*\{\s*PPO_LR_CONSTANT = 0, PPO_LR_LINEAR = 1, PPO_LR_ADAPTIVE = 2\s*\}", ext)
    import exports
    import ppo_ffi
    declared = {n for _, n in exports.declared_functions()}
    names = ["ppo_set_lr_schedule", "ppo_get_lr_schedule", "ppo_lr_couple_value", "ppo_get_lr", "ppo_lr_history",
             "ppo_adam_update_lr_device"]
    for n in names:
        assert n in declared and n in ppo_ffi._SIGS, n
    hip = open(os.path.join(ROOT, "ppo.c_amd", "csrc", "ppo_hip.h")).read()
    rec = hip[hip.index("float hist[PHIP_KL_HIST]"):hip.index("} PhipKlRec;")]
    for field in ("float lr;", "float lr_v;", "lr_kl, lr_min, lr_max", "lr_raised, lr_lowered", "lr_hist[PHIP_KL_HIST]"):
        assert field in rec, field                                         # behind every field the record had


# ----------------------------------------------------------------------------- the checkpoint section
def pack_lr(kind=lr.ADAPTIVE, p=(0.01, 1e-5, 1e-2), couple=1, pad=0, u=2, rate=3e-4, rate_v=1e-3, raised=3, lowered=5):
    return struct.pack("<I3fIIQ2f2I", kind, *p, couple, pad, u, rate, rate_v, raised, lowered)


def with_lr(secs, payload):
    flags = (ck.F_BUFFER if ck.BUFFER in dict(secs) else 0) | (ck.F_ROLLOUT if ck.ROLLOUT in dict(secs) else 0)
    return ck.write_image(secs + [(LRSCHED, payload)], flags=flags | F_LRSCHED)


def test_checkpoint_section_validates(dump):  # noqa: F811
    rng = np.random.default_rng(11)
    secs = small_sections(rng)
    assert len(pack_lr()) == 48
    good = [with_lr(secs, pack_lr()),
            with_lr(secs, pack_lr(couple=0, rate=1e-5, rate_v=0.0)),
            with_lr(small_sections(rng, obs=False, rollout=False, buffer=False, masked=False),
                    pack_lr(kind=lr.LINEAR, p=(4.0, 0.1, 0.0), couple=0, u=7, rate=0.0, rate_v=0.0, raised=0, lowered=0))]
    for line in dump(good):
        assert line.startswith("OK 1 ") and " 7:48 " in line, line
    assert dump(good[:1])[0].split()[2] == str(ck.F_BUFFER | ck.F_ROLLOUT | F_LRSCHED)
    # an image without the section is what it was: same bytes in, same table out, no tag 7
    plain = ck.write_image(secs)
    assert " 7:" not in dump([plain])[0]


def test_checkpoint_section_damage_is_declined(dump):  # noqa: F811
    rng = np.random.default_rng(12)
    secs = small_sections(rng)
    good = with_lr(secs, pack_lr())
    at = len(good) - 48                                   # the section is the last one; 48 is a multiple of 8
    cases = {}
    for off in range(48):                                 # every byte of the payload: the checksum
        b = bytearray(good)
        b[at + off] ^= 0x10
        cases[f"payload byte {off} damaged"] = bytes(b)
    flags = ck.F_BUFFER | ck.F_ROLLOUT
    cases.update({
        "the section without its header flag": ck.write_image(secs + [(LRSCHED, pack_lr())], flags=flags),
        "the header flag without the section": ck.write_image(secs, flags=flags | F_LRSCHED),
        "the section twice": ck.write_image(secs + [(LRSCHED, pack_lr())] * 2, flags=flags | F_LRSCHED),
        "a short section": with_lr(secs, pack_lr()[:44]),
        "a long section": with_lr(secs, pack_lr() + b"\0" * 8),
        "the constant kind": with_lr(secs, pack_lr(kind=0)),
        "an unknown kind": with_lr(secs, pack_lr(kind=3)),
        "a coupling flag of 2": with_lr(secs, pack_lr(couple=2)),
        "a non-zero reserved word": with_lr(secs, pack_lr(pad=1)),
        "desired_kl = 0": with_lr(secs, pack_lr(p=(0.0, 1e-5, 1e-2))),
        "desired_kl = NaN": with_lr(secs, pack_lr(p=(float("nan"), 1e-5, 1e-2))),
        "lr_max < lr_min": with_lr(secs, pack_lr(p=(0.01, 1e-2, 1e-5))),
        "lr_max = inf": with_lr(secs, pack_lr(p=(0.01, 1e-5, float("inf")))),
        "a rate below lr_min": with_lr(secs, pack_lr(rate=1e-6)),
        "a rate above lr_max": with_lr(secs, pack_lr(rate=1.0)),
        "a NaN rate": with_lr(secs, pack_lr(rate=float("nan"))),
        "a NaN value rate": with_lr(secs, pack_lr(rate_v=float("nan"))),
        "linear with N = 0": with_lr(secs, pack_lr(kind=lr.LINEAR, p=(0.0, 0.1, 0.0), rate=0.0, rate_v=0.0, raised=0, lowered=0)),
        "linear with f = 1.5": with_lr(secs, pack_lr(kind=lr.LINEAR, p=(4.0, 1.5, 0.0), rate=0.0, rate_v=0.0, raised=0, lowered=0)),
        "linear with a rate word": with_lr(secs, pack_lr(kind=lr.LINEAR, p=(4.0, 0.1, 0.0), rate=3e-4, rate_v=0.0, raised=0, lowered=0)),
    })
    lines = dump(list(cases.values()) + [good])
    for what, line in zip(cases, lines):
        assert line.startswith("ERR ") and len(line) > 8, f"{what}: {line}"
    assert lines[-1].startswith("OK ")
    byte0 = lines[0]
    assert "section 7" in byte0 and "checksum" in byte0, byte0            # the message names the section and the cause
