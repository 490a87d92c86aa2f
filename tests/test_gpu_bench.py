"""-m gpu: bench.py as the driver runs it.  A plain run prints the headline line only and, with --dump-outputs, the final latent of
its timed trajectory; --full adds the measurements beside the headline (roofline, power, repeats, kernel breakdown, box probe)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("ms_per_step_repeats", "roofline", "roofline_attention", "kernel_time_ms_per_step", "power", "box", "cpu_baseline")


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", *args], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    rec = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert rec["steps"] == 3 and rec["config"]["nfe_timed"] == 3 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["unit"] == "latent-tokens/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert not [k for k in FULL_ONLY if k in rec], rec.keys()
    lat = np.load(tmp_path / "final_latent.npy")
    assert lat.dtype == np.float32 and lat.shape == (1, 2, 4, 128, 128) and np.isfinite(lat).all() and lat.std() > 0


def test_full_bench_keeps_the_measurements_beside_the_headline():
    rec = _bench("--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--repeats", "2")
    assert rec["steps"] == 2 and len(rec["ms_per_step_repeats"]) == 2 and rec["ms_per_step_repeats"][0] == rec["ms_per_step"]
    assert rec["roofline"]["launches"] > 0 and rec["roofline"]["achieved"] > 0
    assert rec["roofline_attention"]["launches"] > 0 and set(rec["kernel_time_ms_per_step"]) >= {"gemm", "attention", "other"}
    assert "power" in rec and rec["box"]["probe_tflops"] is not None
