"""Dev tool (GPU): the outputs that tests/test_gpu_round_order.py pins, and -- run as a script at the PARENT commit -- the fixture
tests/golden/round_order_parent.npz they are compared with.  Reordering independent instructions of the optimizer round
(minimize_body, eval_quad) changes no floating-point operation, so every array here has to come out byte-equal.

    python tools/make_round_order_parent_fixture.py [out.npz]     (SLAM_HIP_LIB honoured)

What tests/golden/span1_parent_outputs.npz and host_paths_parent.npz do not reach in that code.  64 Haar targets x 4 restarts each,
per-span launches (SLAM_FLAG_STAGED); the basis is sqrt(iSWAP) unless the case names another:
  k2_ordered_<gate>  the span-2 stage alone, ordered early exit, sqrt(iSWAP) / B: winner and per-item records
  k2_plain_<gate>    the same stage without early exit: whole records and the stage's evaluation totals
  multi_k<k>         spans 1 and 2 through the multi-queue instantiation: slam_decompose_multi over two contexts (sqrt(iSWAP) and
                     the quarter iSWAP, one structure class, hence one launch with two queues), one span per call: the resident
                     results of both contexts
  bigx0              span 1, explicit start points, no early exit; every eighth start point has one entry of 1e8 - 1 (the largest
                     magnitude the host lets through): the finite / Armijo decisions at an argument where the trial point x + alpha p
                     loses all of alpha p but its leading bits
  maxiter1           the same start points with maxiter = 1: every item ends on its first accepted step or in the line search
  trace              span 1 in trace mode (use_callback), trace_cap = 8, ordered early exit: the records and, per item, the
                     recorded losses and points (the trace reads x after the accepted step was added to it)
Per-item records are loss, iterations, status and evaluations (no evaluations in trace mode: the C ABI has none there).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_TARGETS, RESTARTS, EXIT_LOSS = 64, 4, 1e-10
STAGE_EXIT_LOSS = 1e-13  # a single stage's ordered early exit is at OptParams.stop_loss (its default)
TRACE_CAP = 8
BIG_X = 1e8 - 1.0
ITEM_KEYS = ("item_loss", "item_iters", "item_status", "item_evals")
TRACE_ITEM_KEYS = ("item_loss", "item_iters", "item_status")
GATES_K2 = ("sqiswap", "b")


def _gates():
    from oracle import slam_oracle as o

    return {"sqiswap": o.riswap_matrix(0.5), "b": o.berkeley_matrix(), "qiswap": o.riswap_matrix(0.25)}


def big_x0():
    x0 = np.random.default_rng(91).uniform(0.0, 2.0 * np.pi, size=(N_TARGETS, RESTARTS, 12))
    flat = x0.reshape(-1, 12)
    for n, i in enumerate(range(0, flat.shape[0], 8)):
        flat[i, n % 12] = BIG_X if n % 2 == 0 else -BIG_X
    return x0


def run_cases(ctx) -> dict:
    """Every pinned array, keyed '<case>.<name>'."""
    from oracle import slam_oracle as o
    from slam_decomposition_amd import _ffi

    ordered = _ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED | _ffi.FLAG_STAGED
    gates = _gates()
    out = {}

    def keep(case, r, keys, k):
        for key in ("best_loss", "best_x", "best_restart") + keys:
            out[f"{case}.{key}"] = r[key]
        st = ctx.stats()
        out[f"{case}.evals"] = np.array([st["evals"][k], st["evals_accepted"][k]], dtype=np.int64)

    ctx.set_cost(_ffi.COST_BASIC)
    for i, name in enumerate(GATES_K2):
        ctx.set_targets(o.haar_batch(N_TARGETS, seed0=6100 + 100 * i))
        ctx.set_gates(gates[name][None])
        for case, flags in (("k2_ordered", ordered), ("k2_plain", 0)):
            ctx.reset_stats()
            keep(f"{case}_{name}", ctx.minimize_stage([0, 0], _ffi.OptParams(restarts=RESTARTS, seed=21 + i, flags=flags)), ITEM_KEYS, 2)

    targets = o.haar_batch(N_TARGETS, seed0=6500)
    others = [_ffi.Context(0), _ffi.Context(0)]
    try:
        for c, name in zip(others, ("sqiswap", "qiswap")):
            c.set_targets(targets)
            c.set_gates(gates[name][None])
        prm = _ffi.OptParams(restarts=RESTARTS, seed=23, flags=ordered)
        for k in (1, 2):
            _ffi.decompose_multi(others, 0, N_TARGETS, k, k, [[0] * k], prm, EXIT_LOSS)
            for c, name in zip(others, ("sqiswap", "qiswap")):
                best_loss, best_x, best_cycles = c.fetch_results_range(k, 0, N_TARGETS)
                out[f"multi_k{k}.{name}.best_loss"], out[f"multi_k{k}.{name}.best_x"] = best_loss, best_x
                out[f"multi_k{k}.{name}.best_cycles"] = best_cycles
    finally:
        for c in others:
            c.close()

    ctx.set_targets(targets)
    ctx.set_gates(gates["sqiswap"][None])
    x0 = big_x0()
    ctx.reset_stats()
    keep("bigx0", ctx.minimize_stage([0], _ffi.OptParams(restarts=RESTARTS, seed=24, flags=0), x0=x0), ITEM_KEYS, 1)
    ctx.reset_stats()
    keep("maxiter1", ctx.minimize_stage([0], _ffi.OptParams(restarts=RESTARTS, maxiter=1, seed=25, flags=0), x0=x0), ITEM_KEYS, 1)
    ctx.reset_stats()
    r = ctx.minimize_stage_trace([0], _ffi.OptParams(restarts=RESTARTS, seed=26, flags=ordered), STAGE_EXIT_LOSS, TRACE_CAP)
    keep("trace", r, TRACE_ITEM_KEYS + ("trace_loss", "trace_x"), 1)
    return out


if __name__ == "__main__":
    from slam_decomposition_amd import _ffi

    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "round_order_parent.npz")
    with _ffi.Context(0) as ctx:
        arrays = run_cases(ctx)
        again = run_cases(ctx)
    # what the scheduling can change (records of restarts behind a winner, evaluation totals under early exit) is not pinned by the
    # test: list what differs between two runs of one build
    for key in arrays:
        if not np.array_equal(arrays[key], again[key], equal_nan=arrays[key].dtype.kind == "f"):
            print("differs between two runs of one build:", key)
    for case in ("bigx0", "maxiter1"):
        print(case, "statuses", np.unique(arrays[f"{case}.item_status"], return_counts=True), "non-finite losses",
              int(np.sum(~np.isfinite(arrays[f"{case}.item_loss"]))))
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
