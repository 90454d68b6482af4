"""Dev tool (GPU): the outputs that tests/test_gpu_span1_roomy.py pins, and -- run as a script at the PARENT commit -- the fixture
tests/golden/span1_parent_outputs.npz they are compared with.  The span-1 optimizer kernel's register-budget hoists change no
floating-point operation, so every array here has to come out byte-equal.

    python tools/make_span1_parent_fixture.py [out.npz]     (SLAM_HIP_LIB honoured)

Cases (64 Haar targets x 4 restarts each, per-span launches -- SLAM_FLAG_STAGED: at this size the span loop would otherwise run in the
one-wavefront-per-target kernel and never enter minimize_kernel<1, *>):
  loop_<gate>   spans 1..3, ordered early exit, sqrt(iSWAP) / CNOT / B (dense class): best_loss, best_x, best_cycles
  stage_<gate>  the span-1 stage of the same batch alone, ordered early exit: winner and per-item records
  stage_x0      span 1, explicit start points (the refill path without the seed ring), no early exit
  stage_noext   span 1, SLAM_FLAG_NO_EXTERIOR, no early exit
  stage_square  span 1, SquareCost, ordered early exit
Per-item records are loss, iterations, status and evaluations; the accepted evaluations are not kept per item by the C ABI, so
the stage's total (Stats.evals_accepted[1]) stands for them where it is reproducible (no early exit).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_TARGETS, RESTARTS, EXIT_LOSS = 64, 4, 1e-10
STAGE_EXIT_LOSS = 1e-13  # a single stage's ordered early exit is at OptParams.stop_loss (its default)
SEQS = [[0], [0, 0], [0, 0, 0]]
ITEM_KEYS = ("item_loss", "item_iters", "item_status", "item_evals")


def _gates():
    from oracle import slam_oracle as o

    return {"sqiswap": o.riswap_matrix(0.5), "cx": o.cx_matrix(), "b": o.berkeley_matrix()}


def run_cases(ctx) -> dict:
    """Every pinned array, keyed '<case>.<name>'."""
    from oracle import slam_oracle as o
    from slam_decomposition_amd import _ffi

    ordered = _ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED | _ffi.FLAG_STAGED
    out = {}

    def stage(case, prm, **kw):
        ctx.reset_stats()
        r = ctx.minimize_stage([0], prm, **kw)
        for key in ("best_loss", "best_x", "best_restart") + ITEM_KEYS:
            out[f"{case}.{key}"] = r[key]
        st = ctx.stats()
        out[f"{case}.evals"] = np.array([st["evals"][1], st["evals_accepted"][1]], dtype=np.int64)

    ctx.set_cost(_ffi.COST_BASIC)
    for i, (name, gate) in enumerate(_gates().items()):
        ctx.set_targets(o.haar_batch(N_TARGETS, seed0=5100 + 100 * i))
        ctx.set_gates(gate[None])
        prm = _ffi.OptParams(restarts=RESTARTS, seed=11 + i, flags=ordered)
        best_loss, best_x, best_cycles = ctx.decompose(1, 3, SEQS, prm, EXIT_LOSS)
        out[f"loop_{name}.best_loss"], out[f"loop_{name}.best_x"], out[f"loop_{name}.best_cycles"] = best_loss, best_x, best_cycles
        stage(f"stage_{name}", prm)

    ctx.set_targets(o.haar_batch(N_TARGETS, seed0=5500))
    ctx.set_gates(_gates()["sqiswap"][None])
    x0 = np.random.default_rng(77).uniform(0.0, 2.0 * np.pi, size=(N_TARGETS, RESTARTS, 12))
    stage("stage_x0", _ffi.OptParams(restarts=RESTARTS, seed=3, flags=0), x0=x0)
    stage("stage_noext", _ffi.OptParams(restarts=RESTARTS, seed=4, flags=_ffi.FLAG_NO_EXTERIOR))
    ctx.set_cost(_ffi.COST_SQUARE)
    try:
        stage("stage_square", _ffi.OptParams(restarts=RESTARTS, seed=5, flags=ordered))
    finally:
        ctx.set_cost(_ffi.COST_BASIC)
    return out


if __name__ == "__main__":
    from slam_decomposition_amd import _ffi

    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "span1_parent_outputs.npz")
    with _ffi.Context(0) as ctx:
        arrays = run_cases(ctx)
        again = run_cases(ctx)
    # what the scheduling can change (records of restarts behind a winner) must not be pinned: list what differs between two runs
    for key in arrays:
        if not np.array_equal(arrays[key], again[key]):
            print("differs between two runs of one build:", key)
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
