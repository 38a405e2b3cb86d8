"""Per-minibatch advantage normalisation on the CPU (DESIGN.md §4 "Per-minibatch advantage normalisation"): the numpy
restatement of the definition (tests/advnorm_ref.py) against the textbook formula and at its edge cases, the
checkpoint container's new optional section (tag 8, header flag 8) through the HIP-free indexer compiled for the CPU,
and the five new symbols of the C ABI."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import advnorm_ref as an
import checkpoint_ref as ck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppo.c_amd", "host")
F32, F64 = np.float32, np.float64

SHAPES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 4099]

# measured here (numpy on the CPU), seeds 0 … 19, every B of SHAPES >= 63, standard normal float32 data: the largest
# |advnorm_ref − textbook float64| over all elements.  The difference is fp32 rounding: x − m (m = fl32(mean), the
# difference rounded to fp32: ≤ 2^-24 relative, plus |mean − m| ≤ 2^-25·|mean|) and the result's own rounding to fp32
# (≤ 2^-24 relative), on values of magnitude ≤ ~4.5 — about 4.5 · 2 · 6e-8 = 5.4e-7 by that estimate.
TEXTBOOK_MEASURED = 4.64e-7
TEXTBOOK_BOUND = 2 * TEXTBOOK_MEASURED          # the stated margin: twice the measured figure


def textbook(x):
    x = np.asarray(x, F64)
    return (x - x.mean()) / (x.std(ddof=1) + 1e-8)


def test_ref_matches_the_textbook_formula_on_well_conditioned_data():
    """Largest |ref − textbook| measured 4.64e-7 (20 seeds × B ∈ {63 … 4099}, standard normal); the bound is twice
    that.  (m, sd) against float64 mean and std: within one fp32 rounding of each."""
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(seed)
        for B in [b for b in SHAPES if b >= 63]:
            x = rng.standard_normal(B).astype(F32)
            y, m, sd = an.normalize_segment(x)
            assert y.dtype == F32 and y.shape == (B,)
            worst = max(worst, float(np.abs(y.astype(F64) - textbook(x)).max()))
            x64 = x.astype(F64)
            assert abs(float(m) - x64.mean()) <= 2.0 ** -24 * abs(x64.mean()) + 1e-12
            assert abs(float(sd) - x64.std(ddof=1)) <= 2.0 ** -23 * x64.std(ddof=1)
    print(f"advnorm_ref vs textbook float64: max |err| {worst:.3g} (bound {TEXTBOOK_BOUND:.3g})")
    assert worst <= TEXTBOOK_BOUND


def test_two_pass_statistics_survive_a_large_offset():
    """mean 1e4, std 1e-3: fp32 spacing at 1e4 is ≈ 1e-3, so the data are a few distinct floats — a one-pass
    Σx² − (Σx)²/B in any precision below double, or fp32 sums, would lose sd entirely.  (m, sd) must match the float64
    statistics of the same floats to fp32 rounding."""
    rng = np.random.default_rng(5)
    x = (1e4 + 1e-3 * rng.standard_normal(1000)).astype(F32)
    _, m, sd = an.normalize_segment(x)
    x64 = x.astype(F64)
    assert float(m) == float(F32(x64.mean()))
    assert abs(float(sd) - x64.std(ddof=1)) <= 2.0 ** -23 * x64.std(ddof=1)


def test_edge_cases():
    # B == 1: y = 0, sd = 0, m = x
    y, m, sd = an.normalize_segment(np.array([3.25], F32))
    assert y.tolist() == [0.0] and float(m) == 3.25 and float(sd) == 0.0
    # B == 2: ±1/√2 up to the 1e-8 and fp32 rounding (x = {1, 3}: mean 2, sd √2)
    y, m, sd = an.normalize_segment(np.array([1.0, 3.0], F32))
    assert float(m) == 2.0 and float(sd) == float(F32(np.sqrt(2.0)))
    ref = 1.0 / (float(F32(np.sqrt(2.0))) + 1e-8)
    assert y.tolist() == [float(F32(-ref)), float(F32(ref))]
    # a constant segment: y = 0 exactly, at every B (the lane sums of a constant are exact)
    for B in SHAPES:
        y, m, sd = an.normalize_segment(np.full(B, 0.1, F32))
        assert not y.any() and float(m) == float(F32(0.1)) and float(sd) == 0.0


def test_nan_stays_inside_its_segment():
    rng = np.random.default_rng(2)
    B = 65
    x = rng.standard_normal(3 * B).astype(F32)
    clean, clean_stats = an.normalize(x, B)
    x[B + 7] = np.nan
    y, stats = an.normalize(x, B)
    y, clean = y.reshape(3, B), clean.reshape(3, B)
    assert np.isnan(y[1]).all() and np.isnan(stats[1]).all()
    for s in (0, 2):
        assert y[s].tobytes() == clean[s].tobytes() and stats[s].tobytes() == clean_stats[s].tobytes()


# ------------------------------------------------------------------------------------- the checkpoint section
ADVNORM, F_ADVNORM = 8, 8

MAIN_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include "checkpoint.h"

/* one line per image: "OK flags count tag:bytes ..." or "ERR message" */
int main(int argc, char** argv) {
    for (int i = 1; i < argc; i++) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { printf("ERR cannot open\n"); continue; }
        fseek(f, 0, SEEK_END);
        long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        unsigned char* buf = (unsigned char*)malloc(n > 0 ? (size_t)n : 1);
        if (!buf || fread(buf, 1, (size_t)n, f) != (size_t)n) { printf("ERR cannot read\n"); fclose(f); free(buf); continue; }
        fclose(f);
        CkptIndex ix;
        if (ckpt_index(buf, (size_t)n, &ix) != 0) {
            printf("ERR %s\n", ix.err);
        } else {
            printf("OK %u %u", ix.flags, ix.count);
            for (int t = 1; t < CKPT_NTAG; t++)
                if (ix.sec[t].present) printf(" %d:%llu", t, (unsigned long long)ix.sec[t].len);
            printf("\n");
        }
        free(buf);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def index(tmp_path_factory):
    """checkpoint_index.c and a stand-alone main, built with the host C compiler; run(images) → a line per image"""
    d = tmp_path_factory.mktemp("advnorm_ckpt")
    (d / "main.c").write_text(MAIN_C)
    exe = str(d / "ckpt_dump")
    cc = os.environ.get("CC", "gcc")
    r = subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", HOST,
                        os.path.join(HOST, "checkpoint_index.c"), str(d / "main.c"), "-lm", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(images):
        paths = []
        for i, img in enumerate(images):
            p = d / f"img{i}.bin"
            p.write_bytes(img)
            paths.append(str(p))
        r = subprocess.run([exe] + paths, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, f"exit {r.returncode}: {r.stderr[-2000:]}"
        lines = r.stdout.splitlines()
        assert len(lines) == len(images)
        return lines

    return run


def base_sections():
    """the four required sections of a small image (S = 3, A = 2, capacity 8, Gaussian policy, nothing optional)"""
    legacy = struct.pack("<5f3i", 0.95, 0.2, 0.0, 3e-4, 1e-3, 3, 2, 8) + b"\x07" * 11
    settings = dict(max_grad_norm=0.0, target_kl=0.0, value_clip=0.0, obs_clip=0.0, obs_frozen=0, rew_clip=0.0,
                    rew_frozen=0, ep_gamma=0.99, action_dist=0, nvec=[], mask_on=0, dtype_V=0, dtype_mu=0)
    return [(ck.LEGACY, legacy), (ck.SETTINGS, ck.pack_settings(settings)),
            (ck.NORMALISERS, ck.pack_normalisers(None, [0.0, 0.0, 0.0])), (ck.SHUFFLE, ck.pack_shuffle(1, 2, 1))]


def adv_payload(mode=1, pad=0):
    return struct.pack("<II", mode, pad)


def test_section_8_with_flag_8_indexes(index):
    secs = base_sections()
    with_adv = ck.write_image(secs + [(ADVNORM, adv_payload())], flags=F_ADVNORM)
    plain = ck.write_image(secs, flags=0)
    got = index([with_adv, plain])
    known = " ".join(f"{t}:{len(p)}" for t, p in secs)
    assert got[0] == f"OK {F_ADVNORM} 5 {known} 8:8"
    # an image without the section and without the flag is what it was: the same verdict, the same sections
    assert got[1] == f"OK 0 4 {known}"


def test_malformed_variants_are_declined(index):
    secs = base_sections()
    bad = {
        "the flag without its section": ck.write_image(secs, flags=F_ADVNORM),
        "the section without its flag": ck.write_image(secs + [(ADVNORM, adv_payload())], flags=0),
        "a payload of 4 bytes": ck.write_image(secs + [(ADVNORM, struct.pack("<I", 1))], flags=F_ADVNORM),
        "a payload of 12 bytes": ck.write_image(secs + [(ADVNORM, adv_payload() + b"\0\0\0\0")], flags=F_ADVNORM),
        "an empty payload": ck.write_image(secs + [(ADVNORM, b"")], flags=F_ADVNORM),
        "a mode above 1": ck.write_image(secs + [(ADVNORM, adv_payload(mode=2))], flags=F_ADVNORM),
        "a huge mode": ck.write_image(secs + [(ADVNORM, adv_payload(mode=0xFFFFFFFF))], flags=F_ADVNORM),
        "a non-zero reserved word": ck.write_image(secs + [(ADVNORM, adv_payload(pad=1))], flags=F_ADVNORM),
        "the section twice": ck.write_image(secs + [(ADVNORM, adv_payload())] * 2, flags=F_ADVNORM),
    }
    for what, line in zip(bad, index(list(bad.values()))):
        assert line.startswith("ERR "), f"{what}: {line}"
        assert len(line) > 8, f"{what}: no message"


# ------------------------------------------------------------------------------------- the ABI
NEW_SYMBOLS = ["ppo_set_adv_norm", "ppo_get_adv_norm", "ppo_adv_normalize_device", "ppo_adv_norm_history",
               "ppo_adv_norm_read"]


def test_new_symbols_are_declared_and_exported(lib_built):
    import ppo_ffi
    from exports import declared_functions

    declared = {n for h, n in declared_functions() if h == "ppo_ext.h"}
    out = subprocess.run(["nm", "-D", "--defined-only", ppo_ffi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/ppo_ext.h"
        assert name in exported, f"{name} is not exported from libppo.so"
        assert getattr(lib_built, name).argtypes is not None, f"{name} has no ctypes signature"
    header = open(os.path.join(ROOT, "include", "ppo_ext.h"), encoding="utf-8").read()
    assert re.search(r"PPO_ADV_NORM_GLOBAL\s*=\s*0\s*,\s*PPO_ADV_NORM_MINIBATCH\s*=\s*1", header)
    # NULL handling that needs no device: the getter's 0 and the setter's −1
    assert lib_built.ppo_get_adv_norm(None) == 0
    assert lib_built.ppo_set_adv_norm(None, 1) == -1
    assert lib_built.ppo_adv_normalize_device(None, None, 1, 1, None) == -1
