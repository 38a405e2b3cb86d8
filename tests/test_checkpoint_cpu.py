"""The training-state checkpoint container on the CPU (DESIGN.md §4 "Training-state checkpoints").

The HIP-free half of the checkpoint code (ppo.c_amd/host/checkpoint_index.c: ckpt_index over (buf, len), libc alone;
the library has one build, so the split is by file, not by preprocessor) is compiled together with a small
stand-alone program — its own main, nothing loaded into python — with the host C compiler and
-fsanitize=address,undefined where that links (plain otherwise; the test prints which).  The program reads
image files and prints each one's section table or the validator's error; it must exit 0 on every bad image: no crash,
no sanitizer report.  The images come from checkpoint_ref's writer, and checkpoint_ref's own reader must reach the
same verdict on each.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import checkpoint_ref as ck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppo.c_amd", "host")

MAIN_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include "checkpoint.h"

/* one line per image: "OK version flags count tag:bytes ..." or "ERR message" */
int main(int argc, char** argv) {
    for (int i = 1; i < argc; i++) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { printf("ERR cannot open\n"); continue; }
        fseek(f, 0, SEEK_END);
        long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        unsigned char* buf = (unsigned char*)malloc(n > 0 ? (size_t)n : 1);   /* exactly n: a read past it is caught */
        if (!buf || fread(buf, 1, (size_t)n, f) != (size_t)n) { printf("ERR cannot read\n"); fclose(f); free(buf); continue; }
        fclose(f);
        CkptIndex ix;
        if (ckpt_index(buf, (size_t)n, &ix) != 0) {
            printf("ERR %s\n", ix.err);
        } else {
            printf("OK %u %u %u", ix.version, ix.flags, ix.count);
            for (int t = 1; t < CKPT_NTAG; t++)
                if (ix.sec[t].present) printf(" %d:%llu", t, (unsigned long long)ix.sec[t].len);
            printf(" S=%d A=%d cap=%d\n", ix.S, ix.A, ix.cap);
        }
        free(buf);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """the stand-alone program; returns run(list of image bytes) → one output line per image"""
    d = tmp_path_factory.mktemp("ckpt")
    (d / "main.c").write_text(MAIN_C)
    exe = str(d / "ckpt_dump")
    cc = os.environ.get("CC", "gcc")
    base = [cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", HOST,
            os.path.join(HOST, "checkpoint_index.c"), str(d / "main.c"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    # the sanitizer runtime linked statically first: the program then starts whatever else the loader brings along
    modes = [("address,undefined sanitizers (static runtime)", san + ["-static-libasan", "-static-libubsan"]),
             ("address,undefined sanitizers", san), ("plain (no sanitizer build links and starts here)", [])]
    for mode, extra in modes:
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0:
            break
    else:
        raise AssertionError(r.stderr)
    print(f"checkpoint validator built with: {mode}")

    def run(images):
        paths = []
        for i, img in enumerate(images):
            p = d / f"img{i}.bin"
            p.write_bytes(img)
            paths.append(str(p))
        lines = []
        for at in range(0, len(paths), 256):
            r = subprocess.run([exe] + paths[at:at + 256], capture_output=True, text=True)
            assert r.returncode == 0 and not r.stderr, f"exit {r.returncode}: {r.stderr[-2000:]}"
            lines += r.stdout.splitlines()
        assert len(lines) == len(images)
        return lines

    return run


S, A, CAP, E, T = 3, 5, 8, 2, 3


def small_sections(rng, obs=True, rollout=True, buffer=True, masked=True):
    """every section of a small image: S = 3, A = 5 (nvec {3, 2}), capacity 8, a 2 × 3 Pendulum-shaped rollout"""
    legacy = struct.pack("<5f3i", 0.95, 0.2, 0.01, 3e-4, 1e-3, S, A, CAP) + rng.bytes(13)
    settings = dict(max_grad_norm=0.5, target_kl=float("inf"), value_clip=0.2, obs_clip=10.0, obs_frozen=0, rew_clip=10.0,
                    rew_frozen=1, ep_gamma=0.99, action_dist=2 if masked else 0, nvec=[3, 2] if masked else [],
                    mask_on=int(masked), dtype_V=0, dtype_mu=0)
    secs = [(ck.LEGACY, legacy), (ck.SETTINGS, ck.pack_settings(settings)),
            (ck.NORMALISERS, ck.pack_normalisers(rng.uniform(0, 2, 1 + 2 * S) if obs else None, [7.0, 0.5, 3.0])),
            (ck.SHUFFLE, ck.pack_shuffle(0x0123456789ABCDEF, 7, 1))]
    if rollout:
        secs.append((ck.ROLLOUT, ck.pack_rollout(dict(
            E=E, T=T, kind=1, S=S, step=6, laid=int(buffer), rew_scanned=1, env_state=rng.uniform(-1, 1, (E, 5)),
            cont=[1, 0], carry_in=rng.uniform(-1, 1, E), carry_out=rng.uniform(-1, 1, E), ep_fresh=0, ext_done=0,
            ep_state=rng.uniform(0, 1, (E, 4)), ep_agg=rng.uniform(0, 1, 16), ext_key=0))))
    if buffer:
        n = E * T
        secs.append((ck.BUFFER, ck.pack_buffer(dict(
            idx=n, full=0, limit=n, W=int(masked), state=rng.uniform(-1, 1, (n, S)), action=rng.uniform(-1, 1, (n, A)),
            logprob=rng.uniform(-3, 0, n), reward=rng.uniform(-1, 1, n), next_state=rng.uniform(-1, 1, (n, S)),
            terminated=rng.integers(0, 2, n), truncated=rng.integers(0, 2, n), mask=rng.integers(1, 32, (n, 1))))))
    return secs


def verdict(img):
    """checkpoint_ref's own: None when it parses, else the message"""
    try:
        ck.parse(img)
        return None
    except ck.CheckpointError as e:
        return str(e)


def section_header_offsets(img):
    pos, out = ck.HEADER, []
    for _, payload in ck.read_image(img)[2]:
        out.append(pos)
        pos += ck.SECTION + ck.pad8(len(payload))
    return out


def test_valid_images_list_exactly_their_sections(dump):
    rng = np.random.default_rng(1)
    cases = [small_sections(rng), small_sections(rng, obs=False, rollout=False, buffer=False, masked=False),
             small_sections(rng, buffer=False), small_sections(rng, rollout=False, masked=False)]
    # a later version's section is skipped, wherever it stands
    cases.append(cases[0][:2] + [(99, b"from the future")] + cases[0][2:])
    imgs = [ck.write_image(c) for c in cases]
    for line, secs, img in zip(dump(imgs), cases, imgs):
        assert verdict(img) is None
        known = sorted((t, len(p)) for t, p in secs if t in ck.NAMES)
        flags = (ck.F_BUFFER if ck.BUFFER in dict(secs) else 0) | (ck.F_ROLLOUT if ck.ROLLOUT in dict(secs) else 0)
        want = f"OK 1 {flags} {len(secs)} " + " ".join(f"{t}:{n}" for t, n in known) + f" S={S} A={A} cap={CAP}"
        assert line == want


def test_every_truncation_is_declined(dump):
    img = ck.write_image(small_sections(np.random.default_rng(2)))
    assert 900 < len(img) < 2000
    lines = dump([img[:n] for n in range(len(img))] + [img])
    for n, line in enumerate(lines[:-1]):
        assert line.startswith("ERR "), f"truncated to {n} bytes: {line}"
        assert verdict(img[:n]) is not None
    assert lines[-1].startswith("OK ")


def test_single_byte_corruptions_are_declined(dump):
    """64 seeded positions: 8 in the header, 24 in the section headers, 32 anywhere; each byte XOR a non-zero value"""
    rng = np.random.default_rng(3)
    img = ck.write_image(small_sections(rng))
    heads = np.concatenate([np.arange(o, o + ck.SECTION) for o in section_header_offsets(img)])
    pos = np.concatenate([rng.choice(ck.HEADER, 8, replace=False), rng.choice(heads, 24, replace=False),
                          rng.choice(len(img), 32, replace=False)])
    assert len(pos) == 64
    bad = []
    for p in pos:
        b = bytearray(img)
        b[p] ^= int(rng.integers(1, 256))
        bad.append(bytes(b))
    for p, b, line in zip(pos, bad, dump(bad)):
        assert line.startswith("ERR "), f"byte {p}: {line}"
        assert verdict(b) is not None, f"byte {p}"


def test_hostile_lengths_and_counts_are_declined(dump):
    rng = np.random.default_rng(4)
    secs = small_sections(rng)
    good = ck.write_image(secs)
    head = good[:ck.HEADER]
    body = lambda i, **kw: b"".join(ck.section_bytes(t, p, **(kw if j == i else {})) for j, (t, p) in enumerate(secs))  # noqa: E731
    cases = {
        "a section length of 2^63": head + body(1, length=1 << 63),
        "a section length of 2^64 - 1": head + body(2, length=(1 << 64) - 1),
        "a section length that pads past the end": head + body(len(secs) - 1, length=len(secs[-1][1]) + 1),
        "a count the file could not hold": ck.write_image(secs, count=0xFFFFFFFF),
        "one section too many": ck.write_image(secs, count=len(secs) + 1),
        "one section too few": ck.write_image(secs, count=len(secs) - 1),
        "a wrong magic": ck.write_image(secs, magic=b"PPOSTATS"),
        "version 2": ck.write_image(secs, version=2),
        "version 0": ck.write_image(secs, version=0),
        "an unknown header flag": ck.write_image(secs, flags=7),
        "the buffer flag without the section": ck.write_image(secs[:-1], flags=ck.F_BUFFER | ck.F_ROLLOUT),
        "a non-zero reserved word": head + body(0, reserved=1),
        "a required section missing": ck.write_image(secs[:2] + secs[3:]),
        "a section twice": ck.write_image(secs + [secs[3]]),
        "an observation triple of the wrong length":
            ck.write_image(secs[:2] + [(ck.NORMALISERS, ck.pack_normalisers(np.ones(2 * S), [1.0, 0.0, 0.0]))] + secs[3:]),
        "a settings section shorter than its nvec": ck.write_image(secs[:1] + [(ck.SETTINGS, secs[1][1][:-4])] + secs[2:]),
        "a rollout larger than the capacity":
            ck.write_image(secs[:4] + [(ck.ROLLOUT, struct.pack("<I", 1 << 30) + secs[4][1][4:])] + secs[5:]),
        "a buffer limit that contradicts idx":
            ck.write_image(secs[:5] + [(ck.BUFFER, secs[5][1][:8] + struct.pack("<I", 5) + secs[5][1][12:])]),
        "an empty file": b"",
        "the header alone with a count": good[:ck.HEADER],
    }
    for (what, img), line in zip(cases.items(), dump(list(cases.values()))):
        assert line.startswith("ERR "), f"{what}: {line}"
        assert verdict(img) is not None, what
    assert dump([good])[0].startswith("OK ")


def test_reader_and_writer_round_trip():
    rng = np.random.default_rng(5)
    secs = small_sections(rng) + [(77, b"x" * 9)]
    img = ck.write_image(secs)
    version, flags, got = ck.read_image(img)
    assert (version, flags) == (1, ck.F_BUFFER | ck.F_ROLLOUT) and got == [(t, bytes(p)) for t, p in secs]
    assert ck.write_image(got) == img
    p = ck.parse(img)
    assert p["unknown"] == [(77, b"x" * 9)] and p["header"]["S"] == S and p["header"]["cap"] == CAP
    # every section's packer inverts its parser, byte for byte
    d = dict(secs)
    assert ck.pack_settings(p["settings"]) == d[ck.SETTINGS]
    assert ck.pack_normalisers(*p["normalisers"]) == d[ck.NORMALISERS]
    assert ck.pack_shuffle(**p["shuffle"]) == d[ck.SHUFFLE]
    assert ck.pack_rollout(p["rollout"]) == d[ck.ROLLOUT]
    assert ck.pack_buffer(p["buffer"]) == d[ck.BUFFER]
    assert p["settings"]["nvec"] == [3, 2] and p["settings"]["target_kl"] == float("inf")
    assert ck.fnv1a64(b"") == 0xcbf29ce484222325 and ck.fnv1a64(b"a") == 0xaf63dc4c8601ec8c
