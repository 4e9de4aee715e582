"""bench.py as a plain run: ONE timed region of exactly --steps steps, the headline keys of the result line, and --dump-outputs
(what the last timed call returned, float64, identical across two runs with the same arguments)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(dump_dir):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "cfg1", "--steps", "31", "--warmup", "3",
                          "--dump-outputs", str(dump_dir)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    d = _run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 31 and d["warmup"] == 3 and d["repeats"]["n"] == 1
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-9 * 1e3          # one region of exactly --steps steps
    assert "roofline" not in d and "cpu_baseline" not in d and "li_ba" not in d  # --full only
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("poses", "residuals", "lm_steps")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["poses"].shape == (5, 12) and np.isfinite(got["poses"]).all()
    assert got["residuals"][1] == d["config"]["final_residual"]
    assert (got["lm_steps"][1], got["lm_steps"][2]) == (d["config"]["lm_steps_accepted"], d["config"]["lm_steps_rejected"])
    # same arguments, same inputs: a second run returns the same poses
    _run(tmp_path / "b")
    again = np.load(tmp_path / "b" / "poses.npy")
    assert np.allclose(again, got["poses"], rtol=0, atol=1e-12)
