"""tests/kl_exact_ref.py — the float64 model of the closed-form KL(old ‖ new) the KL monitor can decide from
(ppo_ext.h ppo_set_kl_estimator) — pinned against torch.distributions.kl_divergence on float64 inputs, plus its
properties: non-negative, exactly 0 for identical inputs, blind to masked columns.  And the ABI of the feature.
"""
import ctypes as C

import numpy as np
import pytest

import kl_exact_ref as kx

F32, F64 = np.float32, np.float64


def gaussian_case(rng, m, A):
    return (rng.standard_normal((m, A)).astype(F32), rng.uniform(-1, 0.5, A).astype(F32),
            rng.standard_normal((m, A)).astype(F32), rng.uniform(-1, 0.5, A).astype(F32))


@pytest.mark.parametrize("A", [1, 3, 17, 33])
def test_gaussian_matches_torch(A):
    import torch
    rng = np.random.default_rng(A)
    mo, lo, mn, ln = gaussian_case(rng, 40, A)
    kl, mag = kx.gaussian(mo, lo, mn, ln)
    t = lambda x: torch.tensor(np.asarray(x, F64))  # noqa: E731
    ref = torch.distributions.kl_divergence(torch.distributions.Normal(t(mo), t(lo).exp()),
                                            torch.distributions.Normal(t(mn), t(ln).exp())).sum(1).numpy()
    # torch forms log(σn/σo) + (σo² + Δμ²)/(2σn²) − ½: a few ulp of each term's magnitude (≤ 1 + that term)
    assert np.all(np.abs(kl - ref) <= 1e-13 * (A + mag))
    assert np.all(kl >= 0) and np.all(mag >= kl)


NVECS = [[2], [3, 2, 4], [33], [70, 2]]


def discrete_case(rng, m, nvec, masked):
    A = sum(nvec)
    zo = (2 * rng.standard_normal((m, A))).astype(F32)
    zn = (zo + rng.standard_normal((m, A))).astype(F32)
    action = np.zeros((m, A), F32)
    for d, n in enumerate(nvec):
        action[:, d] = rng.integers(0, n, m)
    mask = None
    if masked:
        mask = rng.random((m, A)) < 0.6
        mask[0, :nvec[0]] = False                       # a component with no bit set: all allowed
        mask[1, int(action[1, 0])] = False              # a chosen action outside its mask: allowed anyway
    return zo, zn, action, mask


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nvec", NVECS, ids=str)
def test_discrete_matches_torch(nvec, masked):
    import torch
    rng = np.random.default_rng(sum(nvec) + masked)
    m = 12
    zo, zn, action, mask = discrete_case(rng, m, nvec, masked)
    kl, mag = kx.discrete(zo, zn, nvec, mask, action)
    for i in range(m):
        want, o = 0.0, 0
        for d, n in enumerate(nvec):
            eff = kx.effective_mask(None if mask is None else mask[i, o:o + n], n, action[i, d] if masked else None)
            idx = np.flatnonzero(eff) + o
            p = torch.distributions.Categorical(logits=torch.tensor(zo[i, idx].astype(F64)))
            q = torch.distributions.Categorical(logits=torch.tensor(zn[i, idx].astype(F64)))
            want += float(torch.distributions.kl_divergence(p, q))
            o += n
        assert abs(kl[i] - want) <= 1e-13 * (1 + mag[i]), (i, kl[i], want)
    assert np.all(kl >= 0)


def test_mask_rules():
    bits = np.array([0, 1, 0, 1], bool)
    assert kx.effective_mask(None, 4, 2).all()
    assert kx.effective_mask(bits, 4, None).tolist() == [False, True, False, True]
    assert kx.effective_mask(bits, 4, 2).tolist() == [False, True, True, True]
    assert kx.effective_mask(np.zeros(4, bool), 4, None).all()
    assert kx.effective_mask(bits, 4, 9).tolist() == [False, True, False, True]        # clamped to column 3
    words = kx.pack_mask(np.arange(70)[None, :] % 3 == 0)
    assert words.shape == (1, 3) and np.array_equal(kx.unpack_mask(words, 70)[0], np.arange(70) % 3 == 0)


def test_identical_inputs_give_exactly_zero():
    rng = np.random.default_rng(5)
    mo, lo, _, _ = gaussian_case(rng, 50, 7)
    kl, mag = kx.gaussian(mo, lo, mo, lo)
    assert not kl.any() and not mag.any()
    for nvec in NVECS:
        zo, _, action, mask = discrete_case(rng, 9, nvec, True)
        for mk in (None, mask):
            kl, mag = kx.discrete(zo, zo, nvec, mk, action)
            assert not kl.any() and not mag.any()


def test_masked_columns_are_never_read():
    rng = np.random.default_rng(6)
    for nvec in NVECS:
        zo, zn, action, mask = discrete_case(rng, 9, nvec, True)
        clean = kx.discrete(zo, zn, nvec, mask, action)
        eff = np.zeros_like(mask)
        for i in range(mask.shape[0]):
            o = 0
            for d, n in enumerate(nvec):
                eff[i, o:o + n] = kx.effective_mask(mask[i, o:o + n], n, action[i, d])
                o += n
        po, pn = zo.copy(), zn.copy()
        po[~eff], pn[~eff] = np.nan, F32(1e30)
        got = kx.discrete(po, pn, nvec, mask, action)
        assert got[0].tobytes() == clean[0].tobytes() and got[1].tobytes() == clean[1].tobytes()
        assert np.isfinite(clean[0]).all()


def test_nan_stays_nan_and_negative_sum_clamps():
    kl, _ = kx.component(np.array([0.0, np.nan], F32), np.array([0.0, 1.0], F32), np.ones(2, bool))
    assert np.isnan(kl)
    # a sum that rounding could push below 0 is reported as 0, never as a negative KL
    z = np.array([1.0, 2.0, 3.0], F32)
    kl, _ = kx.component(z, z + F32(1e-7), np.ones(3, bool))
    assert kl >= 0


# ------------------------------------------------------------------------------------------------- the ABI
NEW_SYMBOLS = ["ppo_set_kl_estimator", "ppo_get_kl_estimator", "ppo_kl_history_est", "ppo_kl_old_dist",
               "ppo_policy_kl_exact_device"]


def test_new_symbols_are_declared_and_exported(lib_built):
    import ppo_ffi
    from exports import declared_functions

    declared = {n for _, n in declared_functions()}
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/*.h"
        assert name in ppo_ffi._SIGS, f"{name} has no ctypes signature"
        assert hasattr(lib_built, name), f"{name} is not exported"
    # the getter and the setter decline a NULL PPO without touching the device
    assert lib_built.ppo_get_kl_estimator(None) == 0
    assert lib_built.ppo_set_kl_estimator(None, 1) == -1
    assert lib_built.ppo_kl_old_dist(None, None) is None
    out = C.c_double(-1.0)
    assert lib_built.ppo_policy_kl_exact_device(3, None, None, None, None, None, None, None, 4, 2, None, 0, None,
                                                C.byref(out)) == -1 and out.value == -1.0


# ------------------------------------------------------------------------------------- the checkpoint section
import os  # noqa: E402
import struct  # noqa: E402
import subprocess  # noqa: E402

import checkpoint_ref as ck  # noqa: E402

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ppo.c_amd", "host")
KLEST, F_KLEST = 9, 16

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


def test_checkpoint_section_9_with_flag_16(tmp_path):
    """checkpoint_index.c, built stand-alone with the host C compiler: the KL-estimator section indexes with its flag,
    an image without either is what it was, and every malformed variant is declined with a message"""
    (tmp_path / "main.c").write_text(MAIN_C)
    exe = str(tmp_path / "ckpt_dump")
    r = subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", HOST,
                        os.path.join(HOST, "checkpoint_index.c"), str(tmp_path / "main.c"), "-lm", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def index(images):
        paths = []
        for i, img in enumerate(images):
            (tmp_path / f"img{i}.bin").write_bytes(img)
            paths.append(str(tmp_path / f"img{i}.bin"))
        out = subprocess.run([exe] + paths, capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
        return out.stdout.splitlines()

    legacy = struct.pack("<5f3i", 0.95, 0.2, 0.0, 3e-4, 1e-3, 3, 2, 8) + b"\x07" * 11
    settings = dict(max_grad_norm=0.0, target_kl=0.0, value_clip=0.0, obs_clip=0.0, obs_frozen=0, rew_clip=0.0,
                    rew_frozen=0, ep_gamma=0.99, action_dist=0, nvec=[], mask_on=0, dtype_V=0, dtype_mu=0)
    secs = [(ck.LEGACY, legacy), (ck.SETTINGS, ck.pack_settings(settings)),
            (ck.NORMALISERS, ck.pack_normalisers(None, [0.0, 0.0, 0.0])), (ck.SHUFFLE, ck.pack_shuffle(1, 2, 1))]
    pay = lambda est=1, pad=0: struct.pack("<II", est, pad)  # noqa: E731
    known = " ".join(f"{t}:{len(p)}" for t, p in secs)
    got = index([ck.write_image(secs + [(KLEST, pay())], flags=F_KLEST), ck.write_image(secs, flags=0)])
    assert got == [f"OK {F_KLEST} 5 {known} 9:8", f"OK 0 4 {known}"]
    bad = {
        "the flag without its section": ck.write_image(secs, flags=F_KLEST),
        "the section without its flag": ck.write_image(secs + [(KLEST, pay())], flags=0),
        "a payload of 4 bytes": ck.write_image(secs + [(KLEST, struct.pack("<I", 1))], flags=F_KLEST),
        "a payload of 12 bytes": ck.write_image(secs + [(KLEST, pay() + b"\0\0\0\0")], flags=F_KLEST),
        "an estimator above 1": ck.write_image(secs + [(KLEST, pay(est=2))], flags=F_KLEST),
        "a non-zero reserved word": ck.write_image(secs + [(KLEST, pay(pad=1))], flags=F_KLEST),
        "the section twice": ck.write_image(secs + [(KLEST, pay())] * 2, flags=F_KLEST),
        "a flag this version does not know": ck.write_image(secs, flags=32),
    }
    for what, line in zip(bad, index(list(bad.values()))):
        assert line.startswith("ERR ") and len(line) > 8, f"{what}: {line}"
