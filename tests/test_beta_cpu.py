"""tests/beta_ref.py against torch in float64; numpy's Beta sampler; the checkpoint section's layout."""
import struct

import numpy as np
import pytest
import torch

import beta_ref as br
import checkpoint_ref as ck
from beta_ref import ENT, EPS, F64, Z_MAX
from test_gauss_sd_cpu import dump, sections  # noqa: F401  (dump: the stand-alone validator over checkpoint_index.c)

SAMPLER_PAIRS = [(1.0, 1.0), (2.0, 5.0), (8.5, 3.0)]    # (α, β) of the sampler's moment test, here and on the GPU


def torch_dist(z, Aa):
    s = 1 + torch.nn.functional.softplus(torch.clamp(z, -Z_MAX, Z_MAX), threshold=1e9)
    return torch.distributions.Beta(s[:, :Aa], s[:, Aa:])


@pytest.mark.parametrize("Aa", [1, 3, 17, 32])
def test_model_is_torch_beta(Aa):
    """within 1e−12·(1 + |want|) of torch, all finite with z = −z_max and x on both storage clamps among the inputs"""
    i = br.head_inputs(Aa, 300)
    ref = br.head_f64(i["z"], i["act"], i["adv"], i["old"], EPS, ENT, Z_MAX)
    assert (i["z"] == -Z_MAX).any() and (i["act"][:, :Aa] == br.X_LO).any() and (i["act"][:, :Aa] == br.X_HI).any()
    z = torch.tensor(np.asarray(i["z"], F64), requires_grad=True)
    d = torch_dist(z, Aa)
    lp, H = d.log_prob(torch.tensor(np.asarray(i["act"][:, :Aa], F64))).sum(-1), d.entropy().sum(-1)
    (torch.tensor(ref["g"]) * lp - ENT / 300 * H).sum().backward()      # the model's g is the fp32 surrogate's
    zn = (i["z"] + np.random.default_rng(Aa).normal(scale=0.5, size=i["z"].shape)).astype(np.float32)
    kl = torch.distributions.kl_divergence(d, torch_dist(torch.tensor(np.asarray(zn, F64)), Aa)).sum(-1)
    for got, want in ((ref["lp"], lp), (ref["H"], H), (ref["grad"], z.grad), (br.kl_rows_f64(i["z"], zn, Z_MAX)[0], kl)):
        want = want.detach().numpy()
        assert np.isfinite(got).all() and (np.abs(got - want) <= 1e-12 * (1 + np.abs(want))).all()
    assert (ref["grad"][~ref["inside"]] == 0).all() and ref["clamped"] > 0


def test_numpy_sampler_within_6_standard_errors_at_65536():
    for k, (a, b) in enumerate(SAMPLER_PAIRS):
        x = np.random.default_rng(100 + k).beta(a, b, 65536)
        for p in (1, 2):
            se = np.sqrt((br.moments(a, b, 2 * p) - br.moments(a, b, p) ** 2) / 65536)
            assert abs((x ** p).mean() - br.moments(a, b, p)) <= 6 * se, (a, b, p)


def test_checkpoint_section_layout(dump):  # noqa: F811
    """tag 11, header flag 64, {u32 1, u32 0, f32 z_max, u32 0}, present exactly while the distribution is 4"""
    pack = lambda z_max: struct.pack("<IIfI", 1, 0, z_max, 0)                                   # noqa: E731
    img = lambda dist, payload, flags: ck.write_image(sections(dist=dist) + ([(11, payload)] if payload else []), flags=flags)  # noqa: E731
    cases = [(img(4, pack(15.0), 64), "OK dist=4"), (img(0, None, 0), "OK dist=0"), (img(4, None, 0), "ERR"),
             (img(4, pack(15.0), 0), "ERR"), (img(0, pack(15.0), 64), "ERR"), (img(4, pack(0.0), 64), "ERR"),
             (img(4, pack(float("nan")), 64), "ERR"), (img(4, pack(15.0)[:12], 64), "ERR")]
    for (_, want), line in zip(cases, dump([c[0] for c in cases])):
        assert line.startswith(want), line
