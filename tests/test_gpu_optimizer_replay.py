"""GPU: the quasi-Newton iteration of ``minimize_body`` (csrc/slam_kernels.hpp) and of its twin for 6..16 gates
(csrc/slam_long_minimize.inc), step by step against oracle/bfgs_port.py.

``slam_minimize_stage_trace`` returns the point after every accepted step.  tests/bfgs_replay.py replays the port along that trajectory
(teacher forcing): at step j it starts from the device's x_j, predicts x_{j+1} with the port's line search on oracle evaluations, and
updates its metric from the pair (s, y) the device took -- so a difference in float32 rounding does not compound into another path, and
a wrong growth factor, back-track clamp, first-update scaling, update rule or restart period shows as a step deviation of tenths.

Per group of tests/golden/optimizer_replay_cases.json (tools/make_replay_cases.py; everything in it comes from the reference alone):

  * tolerance min(8 e_ref, 1e-2) on |s_obs - s_pred| / |s_pred| of every step, e_ref = the worst deviation of the float64-metric replay
    along the float32 port's own trajectory; 8 = two for each of the mat-vec's summation order through the quad exchange, the rank-2
    update's accumulate order on the matrix pipe, and refined-seed reciprocals / 1e-13-level differences of loss and gradient in y;
  * every item without an unclear decision has the replay's iters, evals and status;
  * from the first noise-floor step on an item is checked for a non-increasing trace, its recorded losses, a final status of
    converged or stalled, and a final loss not above the last clear one.

One ``REPLAY`` line per group (pytest -s; DESIGN.md has the table).

Outside the trace facility: the wave-local, speculative and multi-queue forms of the loop are not traced.  test_gpu_refill_paths.py,
test_gpu_span_bookkeeping.py and test_gpu_round4.py / test_gpu_round5.py tie them bit for bit to the per-span launches, which are
what this module pins.  The three-qubit kernels (csrc/slam_q3.hpp, a re-laid copy of the long kernels' body) have no trace export;
tests/test_gpu_q3_replay.py replays them along trajectories it collects from one launch per ``maxiter``.  The V2 and parallel-drive
optimizers have their own port (oracle/pqn_port.py) and no replay yet.
"""
import numpy as np
import pytest

import bfgs_replay as br
import hp_ref as hp
from slam_decomposition_amd import _ffi

pytestmark = pytest.mark.gpu

FIX = br.load_fixture()["groups"]
COST_KIND = {"basic": _ffi.COST_BASIC, "square": _ffi.COST_SQUARE, "makhlin": _ffi.COST_MAKHLIN}


def _run_case(ctx, case):
    """One restart per slot with explicit x0 (best_x is the item's final point): the traced and the plain launch."""
    k, items = int(case["k"]), case["items"]
    ctx.set_targets(np.stack([br.target_matrix(case, t) for t, _ in items]))
    ctx.set_gates(br.gate_matrix(case["gate"])[None])
    ctx.set_cost(COST_KIND[case["cost"]])
    x0 = np.stack([br.start_point(case, t, r) for t, r in items])[:, None, :]
    prm = _ffi.OptParams(restarts=1, maxiter=int(case["maxiter"]), seed=1, flags=int(case["flags"]))
    try:
        tr = ctx.minimize_stage_trace([0] * k, prm, 1e-10, int(case["trace_cap"]), x0=x0)
        pl = ctx.minimize_stage([0] * k, prm, x0=x0)
    finally:
        ctx.set_cost(_ffi.COST_BASIC)
    return x0[:, 0, :], tr, pl


def _check_group(ctx, group):
    grp = FIX[group]
    tol = br.tolerance(grp["e_ref"])
    failures, results = [], []
    for case in grp["cases"]:
        x0, tr, pl = _run_case(ctx, case)
        lg = br.objective(case)
        gates = [br.gate_matrix(case["gate"])] * int(case["k"])
        cap = int(case["trace_cap"])
        for key in ("item_loss", "item_iters", "item_status", "best_x", "best_loss"):
            if not np.array_equal(tr[key], pl[key], equal_nan=True):
                failures.append(f"{case['name']}: {key} of the traced and the plain launch differ")
        for i, (t, r) in enumerate(case["items"]):
            tag = f"{case['name']} ({t}, {r})"
            it, st, nev = int(tr["item_iters"][i, 0]), int(tr["item_status"][i, 0]), int(pl["item_evals"][i, 0])
            T = br.target_matrix(case, t)
            if case.get("nan_target"):
                # a loss that is not finite at the start point: ST_NONFINITE at the first evaluation
                if (it, nev, st) != (0, 1, br.ST_NONFINITE):
                    failures.append(f"{tag}: iters, evals, status {(it, nev, st)} for a non-finite first evaluation")
                if not np.all(np.isnan(tr["trace_loss"][i, 0])):
                    failures.append(f"{tag}: trace entries beyond item_iters are not NaN")
                continue
            if not 1 <= it <= cap:
                failures.append(f"{tag}: {it} iterations, trace capacity {cap}")
                continue
            xs, fl = tr["trace_x"][i, 0, :it], tr["trace_loss"][i, 0, :it]
            if not (np.all(np.isnan(tr["trace_loss"][i, 0, it:])) and np.all(np.isnan(tr["trace_x"][i, 0, it:]))):
                failures.append(f"{tag}: trace entries beyond item_iters are not NaN")
            if not (np.array_equal(xs[-1], tr["best_x"][i]) and fl[-1] == tr["item_loss"][i, 0]):
                failures.append(f"{tag}: the last recorded point is not best_x / item_loss")
            rp = br.replay_item(case, t, r, xs)
            results.append(rp)
            n_chk = len(rp["f"]) - 1  # the points the replay evaluated: all of them, or up to the first noise-floor step
            f_or = np.array(rp["f"][1:] + [lg(x, gates, T)[0] for x in xs[n_chk:]])
            err = np.abs(fl - f_or).max()
            if not err <= hp.TOL_CAP:
                failures.append(f"{tag}: recorded losses off the oracle's by {err:.2e}")
            worst = max(rp["dev"], default=0.0)
            if worst > tol:
                j = int(np.argmax(rp["dev"]))
                failures.append(f"{tag}: step {j} deviates by {worst:.2e} (tolerance {tol:.2e}, unclear {rp['unclear'][j]})")
            port = case["port"][case["items"].index([t, r])]
            if rp["noise_from"] is not None:
                j0 = rp["noise_from"]
                tail = np.concatenate([[rp["f"][j0]], fl[j0:]])  # the last clear loss, then the recorded ones
                if np.any(np.diff(fl[j0:]) > 0) or fl[j0] > rp["f"][j0] + br.bands(case)[0]:
                    failures.append(f"{tag}: the trace increases after the noise floor is reached (step {j0})")
                if st not in (br.ST_CONVERGED, br.ST_STALLED):
                    failures.append(f"{tag}: status {st} at the noise floor")
                if not tail[-1] <= tail[0] + br.bands(case)[0]:
                    failures.append(f"{tag}: final loss {tail[-1]:.3e} above the last clear loss {tail[0]:.3e}")
            elif not rp["item_unclear"]:
                if (it, nev, st) != (rp["iters"], rp["evals"], rp["status"]):
                    failures.append(f"{tag}: iters, evals, status {(it, nev, st)}, the replay predicts {(rp['iters'], rp['evals'], rp['status'])}"
                                    f" (free-running port: {port[:3]})")
        n_new = len(case["items"]) - int(bool(case.get("nan_target")))
        mine = results[len(results) - n_new:] if n_new else []
        print(f"REPLAY   {case['name']:24s} steps {sum(len(r['dev']) for r in mine):5d} worst {max([d for r in mine for d in r['dev']], default=0.0):9.2e}")
    cen = br.census(results)
    worst = max([d for r in results for d in r["dev"]], default=0.0)
    print(f"REPLAY {group:12s} items {len(results):2d} steps {cen['steps']:5d} unclear {cen['unclear']:3d} (items {cen['items_unclear']})"
          f" worst {worst:9.2e} tol {tol:9.2e}  back-tracks {cen['backtracks']} short {cen['short']} skipped {cen['skipped']}"
          f" first-scaling {cen['first_scaling']} non-descent {cen['nondescent']} restarts {cen['periodic']} max-grow {cen['max_grow']:g}"
          f" max-iters {cen['max_iters']}" + ("  FAIL" if failures else ""))
    # the caps of the reference hold for the device's trajectories too
    if cen["unclear"] > 0.02 * max(cen["steps"], 1):
        failures.append(f"{group}: {cen['unclear']} of {cen['steps']} steps unclear")
    if group == "noise_floor":
        print(f"REPLAY {group:12s} clear prefixes {sorted(len(r['dev']) for r in results)} (the reference's shortest: {grp['min_clear_prefix']})")
        short = [len(r["dev"]) for r in results if len(r["dev"]) < grp["min_clear_prefix"] // 2]
        if short:
            failures.append(f"{group}: clear prefixes {short}, the reference's shortest is {grp['min_clear_prefix']}")
    elif cen["items_unclear"] > 0.1 * len(results):
        failures.append(f"{group}: {cen['items_unclear']} of {len(results)} items have an unclear decision")
    assert not failures, "\n" + "\n".join(failures)
    return cen


def test_ordinary_runs_follow_the_port_step_by_step(hip_ctx):
    """CX, sqrt(iSWAP), a dense and a phased conversion-gain gate at spans 1..5: back-tracks, too-short steps, skipped updates, growth
    (to 512 at sqrt(iSWAP) k = 1), first-update scaling, convergence by stop_loss and by the far criterion."""
    cen = _check_group(hip_ctx, "ordinary")
    assert cen["backtracks"] > 0 and cen["short"] > 0 and cen["skipped"] > 0 and cen["first_scaling"] >= 12 and cen["max_grow"] >= 64.0


def test_restarted_runs_follow_the_port_step_by_step(hip_ctx):
    """riswap(1/8) at spans 3 and 5, 173..333 iterations: the periodic restart of the metric (every item once, one item twice)."""
    cen = _check_group(hip_ctx, "restarted")
    assert cen["periodic"] >= 8


def test_noise_floor_runs_follow_the_port_up_to_the_noise_floor(hip_ctx):
    """sqrt(iSWAP) k = 3 on SWAP (a degenerate minimum: half the items stall) and a target two CX just miss (|g| < gtol fires)."""
    _check_group(hip_ctx, "noise_floor")


def test_long_kernels_follow_the_port_step_by_step(hip_ctx):
    """slam_long_minimize.inc: riswap(1/4) at 6 gates, riswap(1/8) at 7 gates (one item through a periodic restart)."""
    cen = _check_group(hip_ctx, "long")
    assert cen["periodic"] >= 1


def test_other_instantiations_follow_the_port_step_by_step(hip_ctx):
    """SLAM_FLAG_NO_EXTERIOR, SquareCost, MakhlinFunctionalCost, maxiter = 5 (ST_MAXITER) and a first evaluation that is not finite
    (ST_NONFINITE; from a NaN in the target -- a NaN in an explicit start point never reaches the kernel: the call refuses it)."""
    _check_group(hip_ctx, "other")
    case = next(c for c in FIX["other"]["cases"] if c["name"] == "sqiswap-k2-maxiter5")
    hip_ctx.set_targets(np.stack([br.target_matrix(case, 0)]))
    hip_ctx.set_gates(br.gate_matrix(case["gate"])[None])
    x0 = br.start_point(case, 0, 0)[None, None, :].copy()
    x0[0, 0, 0] = np.nan
    with pytest.raises(_ffi.SlamHipError, match="explicit seeds must be finite"):
        hip_ctx.minimize_stage([0, 0], _ffi.OptParams(restarts=1, seed=1), x0=x0)
