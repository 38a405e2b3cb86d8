"""bench.py's command line on the GPU (config C2, a few ms per update): the plain run's result line,
`--dump-outputs` (files, dtype, run-to-run equality, the state restore before the last timed step)
and what `--full` adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ["adv_target", "advantage"]


def bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_line_and_repeatable_dump(lib, tmp_path):
    """Two plain runs with --dump-outputs: the result line holds the headline fields and none of the
    --full legs; both runs write the same float32 files, equal bit for bit."""
    out = []
    for d in ("a", "b"):
        res = bench("--config", "c2", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / d))
        assert res["steps"] == 2 and res["warmup"] == 1 and res["full"] is False
        assert res["unit"] == "env-steps/s" and res["higher_is_better"] is True and res["dtype"] == "fp32"
        assert res["ms_per_step"] > 0
        assert res["value"] == pytest.approx(4096 / (res["ms_per_step"] * 1e-3), rel=1e-9)
        assert "roofline" not in res and "cpu_baseline" not in res and res["rollout_env_steps_per_sec"] is None
        assert sorted(os.listdir(tmp_path / d)) == [n + ".npy" for n in DUMPED]
        out.append({n: np.load(tmp_path / d / (n + ".npy")) for n in DUMPED})
    for n in DUMPED:
        a, b = out[0][n], out[1][n]
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n
    assert out[0]["advantage"].shape == out[0]["adv_target"].shape == (4096,)


def test_dump_does_not_depend_on_step_count(lib, tmp_path):
    """The last timed step starts from the seeded initial learner state, so the dumped arrays are the
    same after one timed step without warm-up and after three with one."""
    bench("--config", "c2", "--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "one"))
    bench("--config", "c2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "three"))
    for n in DUMPED:
        assert np.array_equal(np.load(tmp_path / "one" / (n + ".npy")), np.load(tmp_path / "three" / (n + ".npy"))), n


def test_full_adds_its_legs(lib):
    res = bench("--config", "c2", "--steps", "1", "--warmup", "1", "--full")
    assert res["full"] is True and res["ms_per_step"] > 0
    assert res["rollout_env_steps_per_sec"] > 0
    assert res["cpu_baseline"]["value"] > 0 and res["cpu_baseline"]["gpu_over_cpu"] > 0
