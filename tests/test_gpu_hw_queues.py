"""GPU: the hardware queues the library asks for at load change scheduling only, never results.  A smoke check, not a timing test:
`bench.py --dump-outputs` in a child process that starts with GPU_MAX_HW_QUEUES=4 exported (the library raises it to 16 before the
runtime initialises) returns the same arrays as a child that starts with 16 exported (the library keeps it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, hwq):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SLAM_BENCH_TEST_STUB", "SLAM_BENCH_FORCE_LAUNCH", "SLAM_HW_QUEUES")}
    env["GPU_MAX_HW_QUEUES"] = hwq
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg2", "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    assert json.loads(lines[0])["ms_per_step"] > 0
    return {k: np.load(out_dir / f"{k}.npy") for k in ("best_loss", "best_x", "best_cycles")}


def test_results_do_not_depend_on_the_exported_queue_count(tmp_path):
    (tmp_path / "q4").mkdir()
    (tmp_path / "q16").mkdir()
    a, b = _bench(tmp_path / "q4", "4"), _bench(tmp_path / "q16", "16")
    for k in a:
        assert a[k].shape == b[k].shape and a[k].size > 0, k
        assert np.array_equal(a[k], b[k]), k
    assert float(np.mean(a["best_loss"] < 1e-8)) > 0.99
