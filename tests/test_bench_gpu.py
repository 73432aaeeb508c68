"""bench.py's two kinds of run on a device.  A plain run (`--gpus 1 --steps K --warmup W`) sets up, warms up, times the K steps,
writes --dump-outputs and prints the line; it measures nothing besides the headline.  --full adds the per-kernel roofline of the
headline step (and the CPU baseline, the parity check and the secondary workloads, skipped here for time)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_line(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--n", str(1 << 22),
           "--pre-warm-s", "0.05"] + list(extra)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_measures_the_headline_alone(tmp_path):
    line = bench_line("--dump-outputs", str(tmp_path))
    assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "Gelem/s" and line["higher_is_better"] is True
    assert line["config"]["elements_total"] == 1 << 22
    for key in ("roofline", "cpu_baseline", "parity", "also", "weak"):
        assert line[key] is None, key
    assert line["parity_checked"] is False
    assert sorted(os.listdir(tmp_path)) == ["gA.npy", "gB.npy", "y.npy"]
    # the loss in the line is the one the last timed step returned (no further step runs after the timed ones)
    assert float(np.load(tmp_path / "y.npy")[0]) == line["result_y"]


def test_full_run_adds_the_roofline_of_the_headline_step():
    line = bench_line("--full", "--no-also", "--no-cpu-baseline", "--profile-steps", "1")
    assert line["full"] is True and line["value"] > 0
    roof = line["roofline"]
    assert roof["kernels"] and roof["kernel"] == roof["kernels"][0]["kernel"] and roof["whole_step"]["algorithmic_bytes"] > 0
    assert roof["trace_check"]["sum_live_kernel_ms"] > 0 and "measured_stream_ceiling" in roof
    assert line["cpu_baseline"] is None and line["also"] is None
