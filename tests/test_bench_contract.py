"""bench.py driver-contract checks (CPU: gloo backend, world_size 2).

The round-end driver runs `python bench.py --gpus N ...` (N>1 under
torch.distributed.run); this guards that exact launch path so a scaling
run on an 8-GPU node cannot fail on plumbing.
"""

from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_result(line: str, n_gpus: int) -> None:
    result = json.loads(line)
    assert result["metric"] == "map_items_per_sec"
    assert result["n_gpus"] == n_gpus
    assert result["value"] > 0
    assert result["scaling"] == "weak"
    assert result["data"] == "synthetic"
    assert result["config"]["global_batch"] > 0
    assert result["steps"] >= 1 and result["ms_per_step"] > 0
    # ms_per_step is the time of ONE timed step, consistent with the headline
    items = result["steps"] * result["config"]["global_batch"]
    assert result["value"] == pytest.approx(
        items / (result["steps"] * result["ms_per_step"] / 1000.0), rel=1e-6
    )


def test_bench_single_process(tmp_path):
    proc = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "1",
         "--warmup", "0", "--items-per-gpu", "64",
         "--dump-outputs", str(tmp_path / "out")],
        cwd=REPO, capture_output=True, text=True, timeout=180,
        env={**os.environ, "MASTER_PORT": "0"},
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    line = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1]
    _check_result(line, 1)
    # a plain run skips the secondary p50 probe (it lives behind --full)
    assert json.loads(line)["config"]["p50_remote_ms"] is None
    # --dump-outputs: the last timed step's results, sorted (the CPU payload
    # is the identity, so exactly 0..63)
    import numpy as np

    out = np.load(tmp_path / "out" / "map_outputs_sorted.npy")
    assert out.dtype == np.float64
    assert out.tolist() == [float(x) for x in range(64)]


@pytest.mark.timeout(240)
def test_bench_torchrun_world2(tmp_path):
    """The N>1 launch the driver uses, on CPU (gloo, 127.0.0.1)."""
    proc = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29531", "bench.py", "--gpus", "2",
         "--steps", "1", "--warmup", "0", "--items-per-gpu", "64"],
        cwd=REPO, capture_output=True, text=True, timeout=220,
    )
    assert proc.returncode == 0, (proc.stdout[-1000:], proc.stderr[-2000:])
    line = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1]
    _check_result(line, 2)
