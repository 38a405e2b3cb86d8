"""The state-dependent-σ Gaussian policy on the CPU: tests/gauss_sd_ref.py pinned against torch.distributions.Normal
in float64, its fp32 mirror inside its own bounds, the inputs' class condition, the checkpoint section's layout
through the stand-alone validator, and the single definition of the sd_* atoms."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import checkpoint_ref as ck
import gauss_sd_ref as sd
from gauss_sd_ref import ENT, EPS, F32, F64, LS_MAX, LS_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppo.c_amd", "csrc")
HOST = os.path.join(ROOT, "ppo.c_amd", "host")


def torch_head(i, ent):
    z = torch.tensor(np.asarray(i["z"], F64), requires_grad=True)
    a, adv, old = (torch.tensor(np.asarray(i[k], F64)) for k in ("act", "adv", "old"))
    m, A = z.shape
    Aa = A // 2
    dist = torch.distributions.Normal(z[:, :Aa], torch.exp(torch.clamp(z[:, Aa:], LS_MIN, LS_MAX)))
    lp = dist.log_prob(a[:, :Aa]).sum(-1)
    H = dist.entropy().sum(-1)
    ratio = torch.exp(lp - old)
    sur = torch.minimum(ratio * adv, torch.clamp(ratio, 1 - EPS, 1 + EPS) * adv)
    loss = -sur.mean() - ent * H.mean()
    loss.backward()
    return lp.detach().numpy(), H.detach().numpy(), loss.item(), z.grad.numpy()


@pytest.mark.parametrize("Aa", sd.HEAD_AA)
def test_model_is_torch_normal(Aa):
    """lp, H, the loss and both gradient halves (torch.clamp's zero included) within 1e-12 of torch in float64."""
    i = sd.smallest_covering(Aa, 300)
    ref = sd.head_f64(i["z"], i["act"], i["adv"], i["old"], EPS, ENT, LS_MIN, LS_MAX)
    lp, H, loss, grad = torch_head(i, ENT)
    np.testing.assert_allclose(ref["lp"], lp, rtol=0, atol=1e-12 * max(1.0, np.abs(lp).max()))
    np.testing.assert_allclose(ref["H"], H, rtol=0, atol=1e-12 * max(1.0, np.abs(H).max()))
    assert abs(ref["loss"] - loss) <= 1e-12
    np.testing.assert_allclose(ref["grad"], grad, rtol=0, atol=1e-12)
    assert (ref["grad"][:, Aa:][~ref["inside"]] == 0).all() and (grad[:, Aa:][~ref["inside"]] == 0).all()


def test_row_kl_is_torch_kl_divergence():
    rng = np.random.default_rng(3)
    for Aa in sd.HEAD_AA:
        zo = sd.head_inputs(Aa)["z"]
        zn = (zo + rng.normal(scale=0.3, size=zo.shape)).astype(F32)
        mk = lambda z: torch.distributions.Normal(                                  # noqa: E731
            torch.tensor(np.asarray(z[:, :Aa], F64)),
            torch.exp(torch.clamp(torch.tensor(np.asarray(z[:, Aa:], F64)), LS_MIN, LS_MAX)))
        want = torch.distributions.kl_divergence(mk(zo), mk(zn)).sum(-1).numpy()
        got = sd.kl_rows_f64(zo, zn, LS_MIN, LS_MAX)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * max(1.0, want.max()))
        assert (sd.kl_rows_f64(zo, zo, LS_MIN, LS_MAX) == 0).all()


@pytest.mark.parametrize("Aa", sd.HEAD_AA)
@pytest.mark.parametrize("m", sd.HEAD_M)
def test_inputs_and_mirror(Aa, m):
    """every head case of the GPU tests meets the class condition on the model (m = 1 holds one row: it is the one
    case the condition cannot describe), and the fp32 mirror lies inside the bounds the GPU tests use."""
    i = sd.smallest_covering(Aa, m)
    if m > 1:
        ref = sd.check_input_condition(i, f"Aa {Aa} m {m}")
    else:
        ref = sd.head_f64(i["z"], i["act"], i["adv"], i["old"], EPS, ENT, LS_MIN, LS_MAX)
    args = (i["z"], i["act"], i["adv"], i["old"], EPS, ENT, LS_MIN, LS_MAX)
    b, f = sd.head_bounds(*args), sd.head_f32(*args)
    for name in ("lp", "H", "grad"):
        err = np.abs(f[name].astype(F64) - ref[name])
        assert (err <= b[name]).all(), f"{name}: {float((err / np.maximum(b[name], 1e-300)).max()):.3g} of the bound"
    cl = ~ref["inside"]
    assert (f["grad"][:, Aa:][cl].view(np.uint32) == 0).all()                   # +0, bit for bit
    # the bounds are tight enough to tell a wrong head: dropping the clamp moves lp far outside
    if m > 1:
        wrong = sd.head_f64(i["z"], i["act"], i["adv"], i["old"], EPS, ENT, -1e9, 1e9)
        assert (np.abs(wrong["lp"] - ref["lp"]) > b["lp"]).mean() > 0.3


def test_constant_sigma_rows_are_the_gaussian_head():
    """a row whose raw log σ is an in-range vector L gets policy_head_f32's bits at width Aa under log_std = L"""
    import policy_head_ref as ph
    rng = np.random.default_rng(11)
    Aa, m = 3, 65
    i = sd.head_inputs(Aa, m)
    L = rng.uniform(LS_MIN + 0.1, LS_MAX - 0.1, Aa).astype(F32)
    z = np.array(i["z"])
    z[:, Aa:] = L
    f = sd.head_f32(z, i["act"], i["adv"], i["old"], EPS, 0.0, LS_MIN, LS_MAX)
    g = ph.policy_head_f32(z[:, :Aa], L, i["act"][:, :Aa], i["adv"], i["old"], EPS)
    assert f["lp"].tobytes() == g["lp"].tobytes()
    assert f["grad"][:, :Aa].tobytes() == g["grad_mu"].tobytes()


# ------------------------------------------------------------------------------------------ checkpoint section
MAIN_C = r"""
#include <stdio.h>
#include <stdlib.h>
#include "checkpoint.h"
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
        if (ckpt_index(buf, (size_t)n, &ix) != 0) printf("ERR %s\n", ix.err);
        else printf("OK dist=%d sd=%d lo=%g hi=%g\n", ix.action_dist, ix.sec[CKPT_TAG_GAUSS_SD].present,
                    (double)ix.sd_ls[0], (double)ix.sd_ls[1]);
        free(buf);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("ckpt_sd")
    (d / "main.c").write_text(MAIN_C)
    exe = str(d / "ckpt_dump")
    cc = os.environ.get("CC", "gcc")
    r = subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", HOST,
                        os.path.join(HOST, "checkpoint_index.c"), str(d / "main.c"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(images):
        paths = []
        for k, img in enumerate(images):
            p = d / f"img{k}.bin"
            p.write_bytes(img)
            paths.append(str(p))
        r = subprocess.run([exe] + paths, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return r.stdout.splitlines()

    return run


def sections(A=4, dist=3):
    S, CAP = 3, 8
    legacy = struct.pack("<5f3i", 0.95, 0.2, 0.01, 3e-4, 1e-3, S, A, CAP) + b"\0" * 13
    settings = dict(max_grad_norm=0.0, target_kl=0.0, value_clip=0.0, obs_clip=0.0, obs_frozen=0, rew_clip=0.0,
                    rew_frozen=0, ep_gamma=0.99, action_dist=dist, nvec=[], mask_on=0, dtype_V=0, dtype_mu=0)
    return [(ck.LEGACY, legacy), (ck.SETTINGS, ck.pack_settings(settings)),
            (ck.NORMALISERS, ck.pack_normalisers(None, [0.0, 0.0, 0.0])), (ck.SHUFFLE, ck.pack_shuffle(1, 2, 1))]


def test_checkpoint_section_layout(dump):
    """tag 10, header flag 32, 16 bytes {1, 0, ls_min, ls_max}; present exactly while the distribution is 3"""
    sec = (sd.TAG_GAUSS_SD, sd.pack_section(-20.0, 2.0))
    assert len(sec[1]) == sd.GAUSS_SD_BYTES
    good = ck.write_image(sections() + [sec], flags=sd.F_GAUSS_SD)
    cases = {
        "good": (good, "OK dist=3 sd=1 lo=-20 hi=2"),
        "a Gaussian image as ever": (ck.write_image(sections(dist=0), flags=0), "OK dist=0 sd=0 lo=0 hi=0"),
        "the flag without the section": (ck.write_image(sections(), flags=sd.F_GAUSS_SD), "ERR"),
        "the section without the flag": (ck.write_image(sections() + [sec], flags=0), "ERR"),
        "distribution 3 without the section": (ck.write_image(sections(), flags=0), "ERR"),
        "the section under distribution 0": (ck.write_image(sections(dist=0) + [sec], flags=sd.F_GAUSS_SD), "ERR"),
        "an odd action size": (ck.write_image(sections(A=5) + [sec], flags=sd.F_GAUSS_SD), "ERR"),
        "Aa = 33": (ck.write_image(sections(A=66) + [sec], flags=sd.F_GAUSS_SD), "ERR"),
        "ls_min >= ls_max": (ck.write_image(sections() + [(10, sd.pack_section(1.0, 1.0))], flags=32), "ERR"),
        "a bound outside [-20, 20]": (ck.write_image(sections() + [(10, sd.pack_section(-21.0, 1.0))], flags=32), "ERR"),
        "a NaN bound": (ck.write_image(sections() + [(10, sd.pack_section(float("nan"), 1.0))], flags=32), "ERR"),
        "a short section": (ck.write_image(sections() + [(10, sec[1][:12])], flags=32), "ERR"),
        "a non-zero reserved word": (ck.write_image(sections() + [(10, struct.pack("<IIff", 1, 1, -1.0, 1.0))], flags=32),
                                     "ERR"),
    }
    for (what, (img, want)), line in zip(cases.items(), dump([c[0] for c in cases.values()])):
        assert line.startswith(want), f"{what}: {line}"


# ------------------------------------------------------------------------------------------ one definition
def test_sd_atoms_have_one_definition():
    """the sd_* atoms are defined in ppo_math.h alone; the head, both forms of the sampler (one kernel, one device
    function) and the KL launch call them and restate none of the arithmetic"""
    src = {fn: open(os.path.join(CSRC, fn)).read() for fn in sorted(os.listdir(CSRC)) if fn.endswith((".hip", ".h"))}
    defs = re.compile(r"__device__\s+__forceinline__\s+[\w:]+\s+(sd_\w+)\s*\(")
    atoms = set(defs.findall(src["ppo_math.h"]))
    assert atoms == {"sd_clamp", "sd_inside", "sd_lp_step", "sd_row", "sd_grad_mu", "sd_grad_ls", "sd_kl_row"}
    for fn, text in src.items():
        if fn != "ppo_math.h":
            assert not [n for n in defs.findall(text) if n in atoms], fn
    head = src["gauss_sd.hip"]
    for name in ("sd_row", "sd_grad_mu", "sd_grad_ls", "sd_clamp", "sd_lp_step"):
        assert f"ppo::{name}(" in head, name
    assert "ppo::sd_row(" in src["kl.hip"] and "ppo::sd_kl_row(" in src["kl.hip"]
    # one sampler: both launch forms reach sd_sample_row through sd_sample_kernel
    assert head.count("sd_sample_row<DET>(") == 1 and "phip_sd_sample(z, rows, action, logprob, E" in head
    # no clamp written out anywhere else
    for fn in ("gauss_sd.hip", "kl.hip"):
        assert "< lo ?" not in src[fn] and "expf(-2" not in src[fn], fn
    # no floating-point atomic in the head's file: the two atomics are the integer counters
    assert re.findall(r"atomicAdd\(&rec->counts\[\d\]", head) and len(re.findall(r"atomicAdd\(", head)) == 2
