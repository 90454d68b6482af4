"""GPU: `bench.py --dump-outputs` writes what the timed path returned for its last step -- the same best_loss / best_x /
best_cycles a caller gets from the library for that window of the resident targets on its own (ordered early exit: a window's
results do not depend on what else is in the call)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dumped_outputs_are_the_last_steps_results(tmp_path):
    from benchlib.workloads import OPT_SEED, TARGET_SEED0, WORKLOADS, gate_table
    from slam_decomposition_amd import _ffi

    steps, warmup = 4, 2
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SLAM_BENCH_TEST_STUB", "SLAM_BENCH_FORCE_LAUNCH")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg2", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["repetitions"] == 1 and out["ms_per_step"] > 0
    got = {k: np.load(tmp_path / f"{k}.npy") for k in ("best_loss", "best_x", "best_cycles")}
    assert all(a.dtype == np.float64 for a in got.values())

    gname, n, restarts, _ = WORKLOADS["cfg2"]
    table = gate_table(gname)
    ctx = _ffi.Context(0)
    ctx.set_gates(table)
    ctx.sample_haar(TARGET_SEED0, (steps + warmup) * n)
    prm = _ffi.OptParams(restarts=restarts, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=OPT_SEED, flags=_ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED)
    seqs = [[i % len(table) for i in range(k)] for k in (1, 2, 3)]
    loss, x, cyc = ctx.decompose_range((steps + warmup - 1) * n, n, 1, 3, seqs, prm, 1e-10)
    ctx.close()
    assert got["best_loss"].shape == (n,) and got["best_x"].shape == x.shape
    assert np.array_equal(got["best_cycles"], cyc.astype(np.float64))
    assert np.array_equal(got["best_loss"], loss) and np.array_equal(got["best_x"], x)
    assert float(np.mean(loss < 1e-8)) > 0.99
