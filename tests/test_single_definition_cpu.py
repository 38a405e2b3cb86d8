"""The per-row PPO arithmetic and the Feistel order are written once in ppo.c_amd ("One definition
per arithmetic"): csrc/ppo_math.h, csrc/feistel.h and csrc/ppo_hip.h hold them, and no kernel restates them.  So are
the fixed-order reductions of the statistics kernels, in csrc/reduce.h.

Each token below marks one of those definitions — a constant or an expression that a pasted copy would carry
with it — and has to occur on exactly one line of exactly one file under ppo.c_amd/csrc and ppo.c_amd/host.
The oracle and tests/*_ref.py are the other side of every comparison and stay independent restatements.
"""
import pathlib

import pytest

PKG = pathlib.Path(__file__).resolve().parent.parent / "ppo.c_amd"

TOKENS = [
    "0x7feb352dU",                  # mix32 (the Feistel round function)
    "logf((float)(2 * M_PI))",      # log_prob_start
    "sqrtf(v / bc2)",               # adam_elem
    "ratio_pos = ",                 # surrogate
    "(1 + log(2 * M_PI))",          # entropy_start
    "while ((1ULL << bits)",        # feistel_domain
    "0x9E3779B97F4A7C15",           # splitmix64
    "delta * delta * (na * (nb / n))",                  # reduce.h chan
    "d * d * n * nb / nn",                              # reduce.h chan_ref_order (gae.hip's other order)
    "min(count, (t + 1) * per)",                        # reduce.h fold_runs_tree: the runs
    "(t & (2 * stride - 1)) == 0",                      # reduce.h tree_fold: the pairwise tree
    "bs / (double)bn",                                  # reduce.h block_two_pass_triple
    "a.d + a.c * b.d",                                  # reduce.h compose of two affine maps
    "w > 0; w >>= 1",                                   # reduce.h block_sum_halving
    '__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")',  # reduce.h ticket_publish
]


@pytest.fixture(scope="module")
def lines():
    files = sorted(p for d in ("csrc", "host") for p in (PKG / d).iterdir() if p.is_file())
    assert len(files) > 20, files
    return [(p.relative_to(PKG).as_posix(), n, text) for p in files
            for n, text in enumerate(p.read_text(encoding="utf-8").splitlines(), 1)]


@pytest.mark.parametrize("token", TOKENS)
def test_defined_once(lines, token):
    hits = [f"{path}:{n}" for path, n, text in lines if token in text]
    assert len(hits) == 1, f"{token!r} occurs on {len(hits)} lines: {hits}"
