"""GPU: the quasi-Newton iteration of ``minimize_q3_kernel<false>`` and ``<true>`` (csrc/slam_q3.hpp), step by step against
oracle/bfgs_port.py, and the paths of the two three-qubit kernels no other test takes.

The trajectory without a trace facility.  With ``restarts = 1``, ``flags = 0`` and an explicit ``x0`` an item's run is a
deterministic function of its inputs, and ``maxiter`` enters only through ``iters >= maxiter``: the launch with ``maxiter = j``
returns, as ``item_x`` / ``item_loss`` / ``item_evals``, the state after accepted step j of the full run.  ``_trajectories`` makes one
launch per j over all items of a case and asserts what makes that argument sound (iters = min(j, full), ST_MAXITER exactly below the
full count, bit-equal results from it on, non-increasing losses, strictly increasing evaluation counts).  Its by-product
``item_evals[j] - item_evals[j - 1] - 1`` is the observed number of back-tracks of step j and is compared exactly with the replay's at
every clear step -- the two-qubit replay (test_gpu_optimizer_replay.py) sees only the final count.

Per group of tests/golden/q3_replay_cases.json (tools/make_q3_replay_cases.py; everything in it comes from the models alone):

  * tolerance min(8 e_ref, 1e-2) on |s_obs - s_pred| / |s_pred| of every step (tests/bfgs_replay.py); here the factor's three
    effects are the mat-vec's even / odd row accumulators, the rank-2 update deferred to the next step's pass, and refined-seed
    reciprocals / 1e-15-level differences of loss and gradient in y;
  * the bands of an unclear decision are twice the parity bounds of test_gpu_q3.py / test_gpu_q3m.py, and every recorded loss is
    held to those bounds themselves (3.4e-15, mixed 6.8e-15) against the model at the recorded point -- the optimizer evaluates with
    ``eval_q3<HUGE_ARGS = false>`` (the sincos table), which the parity tests never run;
  * every item without an unclear decision has the replay's iters, evals and status; at most 2 % of the steps and 10 % of the items
    of a group may be unclear; from a noise-floor step on an item is held to the tail rules of the two-qubit module.

One ``REPLAY`` line per group (pytest -s; DESIGN.md has the table).

Further: a wavefront's second and later items against the same items as first items, the evaluation kernel's grid stride and its
``target_of`` map, and explicit start points far from the origin (refused beyond 1e8, followed inside).
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import bfgs_replay as br
import q3_cases
import q3_ref
import q3_replay_cases as qc
import q3m_cases
import q3m_ref
from slam_decomposition_amd import _ffi

pytestmark = pytest.mark.gpu

FIX = qc.load_fixture()["groups"]
KEYS = ("item_x", "item_loss", "item_status", "item_evals", "item_iters")


def _launch(ctx, case, targets, x0, maxiter):
    prm = _ffi.OptParams(restarts=1, maxiter=int(maxiter), seed=1, flags=0, **qc.DEFAULTS)
    return qc.template(case).minimize(ctx, targets, prm, x0, int(case["cost"] == "square"))


def _trajectories(ctx, case):
    """Per item of the case (xs [iters, n], losses [iters], evals [iters + 1], iters, evals, status) of the full run, from one launch
    per j = 1 .. the largest iteration count."""
    items = case["items"]
    targets = np.stack([qc.target_matrix(case, it) for it in items])
    x0 = np.stack([qc.start_point(case, it) for it in items])[:, None, :]
    full = _launch(ctx, case, targets, x0, case["maxiter"])
    it_full = full["item_iters"][:, 0]
    assert np.all(full["item_status"] != 5) and np.all(it_full <= int(case["maxiter"]))
    J = int(it_full.max())
    xs = [np.empty((int(n), x0.shape[2])) for n in it_full]
    fl = [np.empty(int(n)) for n in it_full]
    ev = [np.ones(int(n) + 1, dtype=np.int64) for n in it_full]  # (before step 1: the evaluation of the start point)
    for j in range(1, J + 1):
        out = _launch(ctx, case, targets, x0, j)
        assert np.array_equal(out["item_iters"][:, 0], np.minimum(j, it_full)), j
        for i in range(len(items)):
            if j < it_full[i]:
                assert out["item_status"][i, 0] == br.ST_MAXITER, (i, j)
            else:
                # (the full run's own status is ST_MAXITER only where it used up the case's maxiter)
                assert (full["item_status"][i, 0] == br.ST_MAXITER) == (it_full[i] == int(case["maxiter"])), i
                for key in KEYS:  # from the full count on: the full run, bit for bit
                    assert np.array_equal(out[key][i], full[key][i], equal_nan=True), (key, i, j)
            if j <= it_full[i]:
                xs[i][j - 1], fl[i][j - 1], ev[i][j] = out["item_x"][i, 0], out["item_loss"][i, 0], out["item_evals"][i, 0]
    for i in range(len(items)):
        assert np.all(np.diff(fl[i]) <= 0), i           # accepted steps only lower the loss
        assert np.all(np.diff(ev[i]) >= 1), i           # every step costs an evaluation
        if it_full[i]:
            assert np.array_equal(xs[i][-1], full["item_x"][i, 0]) and fl[i][-1] == full["item_loss"][i, 0]
    return [(xs[i], fl[i], ev[i], int(it_full[i]), int(full["item_evals"][i, 0]), int(full["item_status"][i, 0]), full["item_loss"][i, 0])
            for i in range(len(items))]


def _check_group(ctx, group):
    grp = FIX[group]
    tol = br.tolerance(grp["e_ref"])
    failures, results = [], []
    worst_loss, loss_bound = 0.0, 0.0
    for case in grp["cases"]:
        lg = qc.objective(case)
        gates = qc.template(case).model_gates
        band_f = qc.bands(case)[0]
        mine = []
        for item, port, (xs, fl, ev, it, nev, st, f_end) in zip(case["items"], case["port"], _trajectories(ctx, case)):
            tag = f"{case['name']} {item}"
            if case.get("nan_target"):
                # a loss that is not finite at the start point: ST_NONFINITE at the first evaluation
                if (it, nev, st) != (0, 1, br.ST_NONFINITE) or np.isfinite(f_end):
                    failures.append(f"{tag}: iters, evals, status {(it, nev, st)}, loss {f_end} for a non-finite first evaluation")
                continue
            T = qc.target_matrix(case, item)
            rp = qc.replay_item(case, item, xs)
            results.append(rp)
            mine.append(rp)
            n_chk = len(rp["f"]) - 1  # the points the replay evaluated: all of them, or up to the first noise-floor step
            f_or = np.array(rp["f"][1:] + [lg(x, gates, T)[0] for x in xs[n_chk:]])
            err = np.abs(fl - f_or).max() if it else abs(f_end - rp["f"][0])
            worst_loss, loss_bound = max(worst_loss, err), max(loss_bound, qc.loss_bound(case))
            if not err <= qc.loss_bound(case):
                failures.append(f"{tag}: recorded losses off the model's by {err:.2e} (bound {qc.loss_bound(case):.1e})")
            worst = max(rp["dev"], default=0.0)
            if worst > tol:
                j = int(np.argmax(rp["dev"]))
                failures.append(f"{tag}: step {j} deviates by {worst:.2e} (tolerance {tol:.2e}, unclear {rp['unclear'][j]})")
            # back-tracks of every clear step, exactly (the last step's count includes the trailing failed trials of a run that
            # ended in the line search: not compared)
            n_cmp = len(rp["dev"]) - int(len(rp["dev"]) == it and st in (br.ST_LINESEARCH, br.ST_STALLED))
            for j in range(n_cmp):
                n_back = int(ev[j + 1] - ev[j] - 1)
                if not rp["unclear"][j] and n_back != rp["steps"][j]["n_back"]:
                    failures.append(f"{tag}: step {j} took {n_back} back-tracks, the replay predicts {rp['steps'][j]['n_back']}")
            if rp["noise_from"] is not None:
                j0 = rp["noise_from"]
                tail = np.concatenate([[rp["f"][j0]], fl[j0:]])  # the last clear loss, then the recorded ones
                if np.any(np.diff(fl[j0:]) > 0) or fl[j0] > rp["f"][j0] + band_f:
                    failures.append(f"{tag}: the losses increase after the noise floor is reached (step {j0})")
                if st not in (br.ST_CONVERGED, br.ST_STALLED):
                    failures.append(f"{tag}: status {st} at the noise floor")
                if not tail[-1] <= tail[0] + band_f:
                    failures.append(f"{tag}: final loss {tail[-1]:.3e} above the last clear loss {tail[0]:.3e}")
            elif not rp["item_unclear"]:
                if (it, nev, st) != (rp["iters"], rp["evals"], rp["status"]):
                    failures.append(f"{tag}: iters, evals, status {(it, nev, st)}, the replay predicts {(rp['iters'], rp['evals'], rp['status'])}"
                                    f" (free-running port: {port[:3]})")
        print(f"REPLAY   {case['name']:20s} steps {sum(len(r['dev']) for r in mine):5d} worst {max([d for r in mine for d in r['dev']], default=0.0):9.2e}")
    cen = br.census(results)
    worst = max([d for r in results for d in r["dev"]], default=0.0)
    print(f"REPLAY {group:8s} items {len(results):2d} steps {cen['steps']:5d} unclear {cen['unclear']:3d} (items {cen['items_unclear']})"
          f" worst {worst:9.2e} tol {tol:9.2e}  loss error {worst_loss:8.2e} bound {loss_bound:7.1e}  back-tracks {cen['backtracks']}"
          f" short {cen['short']} skipped {cen['skipped']} first-scaling {cen['first_scaling']} non-descent {cen['nondescent']}"
          f" restarts {cen['periodic']} max-grow {cen['max_grow']:g} max-iters {cen['max_iters']}" + ("  FAIL" if failures else ""))
    # the caps of the reference hold for the device's trajectories too
    if cen["unclear"] > 0.02 * max(cen["steps"], 1):
        failures.append(f"{group}: {cen['unclear']} of {cen['steps']} steps unclear")
    if cen["items_unclear"] > 0.1 * len(results):
        failures.append(f"{group}: {cen['items_unclear']} of {len(results)} items have an unclear decision")
    assert not failures, "\n" + "\n".join(failures)
    return cen


def test_small_templates_follow_the_port_step_by_step(hip_ctx):
    """k = 1 (n = 15: the rows of one partial batch only) and the sqrt(iSWAP) line at k = 3 (n = 27): back-tracks, short steps,
    skipped updates, growth to 64, first-update scaling, ends by stop_loss and by the far criterion."""
    cen = _check_group(hip_ctx, "small")
    assert cen["backtracks"] > 0 and cen["short"] > 0 and cen["skipped"] > 0 and cen["first_scaling"] >= 6 and cen["max_grow"] >= 64.0


def test_toffoli_runs_follow_the_port_step_by_step(hip_ctx):
    """Six CX on TOFFOLI_EDGES to CCX (n = 45) under BasicCost and SquareCost: the second cost kind, many back-tracks."""
    cen = _check_group(hip_ctx, "toffoli")
    assert cen["backtracks"] >= 20 and cen["first_scaling"] >= 6


def test_runs_at_the_parameter_cap_follow_the_port_step_by_step(hip_ctx):
    """n = 99: six row batches of 16 and one of three rows; 183 and 256 iterations, each through a periodic restart."""
    cen = _check_group(hip_ctx, "cap")
    assert cen["periodic"] >= 2


def test_mixed_templates_follow_the_port_step_by_step(hip_ctx):
    """MIXED = true: [VSwap, sqrt(iSWAP), VSwap] from far starts (n = 33), [CCZ, CX] under SquareCost (n = 24, growth to 512) and ten
    three-qubit positions (n = 99)."""
    cen = _check_group(hip_ctx, "mixed")
    assert cen["backtracks"] > 0 and cen["short"] > 0 and cen["max_grow"] >= 64.0


def test_other_endings_follow_the_port_step_by_step(hip_ctx):
    """maxiter = 5 (ST_MAXITER), a first evaluation that is not finite (ST_NONFINITE, from a NaN in the target), a start point that is
    the solution (converged at iters 0) and runs to stop_loss from 0.05 N(0, 1) beside a solution, in both instantiations."""
    _check_group(hip_ctx, "other")


# ---- a wavefront's later items ---------------------------------------------------------------------------------------------------
def _cus(ctx):
    """The device's CU count as the library's own context reports it -- the number its launches cap their grids with.  (PyTorch reports
    the same count, but a second HIP runtime initialised in a process where the library already holds the device finds no GPU.)"""
    cus = int(ctx.device_info()[1])
    assert cus >= 1
    return cus


@pytest.mark.parametrize("name", ["table-k1", "ccz-cx"])
def test_a_wavefront_s_later_items_equal_its_first(hip_ctx, name):
    """N = 8 targets x R = 4 CUs + 1 restarts of ``maxiter = 6`` from explicit start points: M > 2 * 16 CUs items on a grid of at most
    16 CUs persistent wavefronts (LDS lets 16 wavefronts onto a CU, 12 of the mixed kernel), so every item at queue position
    >= 16 CUs -- restart-major: restart index >= 2 CUs -- is some wavefront's second or later item: it meets ``ident`` / ``pend`` /
    ``hs1`` reset, a used ``hmem`` slab and used ``f32b`` / ``f32c`` vectors.  256 of those items (32 restart indices >= 2 CUs, the last
    one, 4 CUs, among them, for all 8 targets) run again in a launch of their own, where with M = 256 every item is a first item: the
    same loss, x, iters, status and evals, bit for bit."""
    cus = _cus(hip_ctx)
    if name == "table-k1":
        case = {"template": ["parity", 1], "cost": "basic"}
        targets = q3_cases.parity_case(1)[3][:8]
    else:
        case = {"template": ["ccz_cx"], "cost": "basic"}
        targets = q3m_cases.ccz_cx_targets()
    tp = qc.template(case)
    R = 4 * cus + 1
    rng = np.random.default_rng(4600 + tp.n)
    x0 = rng.uniform(0.0, 2.0 * math.pi, (8, R, tp.n))
    prm = _ffi.OptParams(restarts=R, maxiter=6, seed=1, flags=0, **qc.DEFAULTS)
    big = tp.minimize(hip_ctx, targets, prm, x0, 0)
    assert 8 * R > 2 * 16 * cus and not np.any(big["item_status"] == 5)
    later = np.sort(np.concatenate([rng.choice(np.arange(2 * cus, 4 * cus), 31, replace=False), [4 * cus]]))
    assert len(later) == 32 and later.min() * 8 >= 16 * cus
    small = tp.minimize(hip_ctx, targets, prm.replace(restarts=32), np.ascontiguousarray(x0[:, later]), 0)
    assert not np.any(small["item_status"] == 5)
    for key in KEYS:
        assert np.array_equal(big[key][:, later], small[key]), key
    # (the items did run: six accepted steps each, or an earlier regular end)
    assert np.all(small["item_iters"] >= 1) and np.mean(small["item_iters"] == 6) > 0.9 and np.all(small["item_evals"] > small["item_iters"])


# ---- the evaluation kernel's stride and target map ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["table-k1", "one-3"])
def test_evaluation_strides_and_follows_target_of(hip_ctx, name):
    """M = 2 * 16 CUs + 37 rows on a grid capped at 16 CUs blocks: every block strides, twice or three times.  ``target_of`` is a
    seeded map onto 5 targets, non-monotone and with repeats.  A seeded sample of 64 rows -- the first, the last and the rows on
    either side of index 16 CUs among them -- is held to the parity bounds against the model (rows under the 0.05 overlap floor
    dropped from this comparison only), and every row equals, bit for bit, the same row evaluated in a launch of 64."""
    cus = _cus(hip_ctx)
    M = 2 * 16 * cus + 37
    rng = np.random.default_rng(4700 + len(name))
    targets = np.stack([q3_cases.haar(rng, 8) for _ in range(5)])
    tof = rng.integers(0, 5, M).astype(np.int32)
    assert np.any(np.diff(tof) < 0) and len(set(tof.tolist())) == 5
    if name == "table-k1":
        gates, gate_index, edges, _, _ = q3_cases.parity_case(1)
        n, mixed, ref, model_gates = 15, False, q3_ref, [gates[i] for i in gate_index]
        ev = lambda xx, tt: hip_ctx.q3_eval(gates, gate_index, edges, targets, xx, tt)  # noqa: E731
    else:
        case = q3m_cases.parity_template(name)
        n, mixed, ref, model_gates, edges = case.n, True, q3m_ref, case.model_gates, case.edges
        ev = lambda xx, tt: hip_ctx.q3m_eval(*case.description(), targets, xx, tt)  # noqa: E731
    x = rng.uniform(-math.pi, 3.0 * math.pi, (M, n))
    loss, grad, _ = ev(x, tof)
    fixed = np.array([0, 16 * cus - 1, 16 * cus, M - 1])
    rows = np.sort(np.concatenate([fixed, rng.choice(np.setdiff1d(np.arange(M), fixed), 60, replace=False)]))
    assert len(set(rows.tolist())) == 64
    kept, e_loss, e_grad = 0, 0.0, 0.0
    for m in rows:
        f, g, w = ref.loss_grad(x[m], model_gates, edges, targets[tof[m]])
        if q3_ref.overlap(w, targets[tof[m]]) >= qc.OVERLAP_FLOOR:
            kept += 1
            e_loss, e_grad = max(e_loss, abs(loss[m] - f)), max(e_grad, np.abs(grad[m] - g).max())
    print(f"q3 stride {name}: M {M}, kept {kept}/64, max errors loss {e_loss:.3e} grad {e_grad:.3e}")
    assert kept >= 48
    assert e_loss < qc.LOSS_BOUND[mixed] and e_grad < qc.GRAD_BOUND[mixed]
    for lo in range(0, M, 64):
        l64, g64, _ = ev(x[lo:lo + 64], tof[lo:lo + 64])
        assert np.array_equal(l64, loss[lo:lo + 64]) and np.array_equal(g64, grad[lo:lo + 64]), lo


# ---- explicit start points far from the origin -------------------------------------------------------------------------------------
_TWO_PI = 2 * Fraction("3.14159265358979323846264338327950288419716939937510582097494")


def _reduced(x):
    """Every component minus its whole number of turns, in exact rational arithmetic on the double itself (2 pi to 60 digits), rounded
    once: the same angles to 1e-16, at a size where the model's own sums are harmless."""
    return np.array([float(Fraction(float(v)) - round(Fraction(float(v)) / _TWO_PI) * _TWO_PI) for v in x])


def test_start_points_far_from_the_origin_are_followed_or_refused(hip_ctx):
    """x0 shifted by 2 pi 10^6 per component (inside the sincos table's range): after ``maxiter = 3`` the recorded loss is the
    model's at the recorded point, to the recorded-loss bound.  The model takes the recorded point reduced exactly (``_reduced``):
    its u3 forms exp(i (phi + lam)) from a double sum, which at 6e6 rounds the angle by up to 9e-10, where the kernel multiplies
    exp(i phi) and exp(i lam) -- fed the unreduced point the model differed from the device by 9.5e-11, and the error was the model's.
    Beyond 1e8, or not finite: refused, as the two-qubit stage does."""
    case = next(c for c in FIX["small"]["cases"] if c["name"] == "table-k1")
    item = case["items"][1]
    target = qc.target_matrix(case, item)[None]
    x0 = (qc.start_point(case, item) + 2.0 * math.pi * 1e6)[None, None, :]
    out = _launch(hip_ctx, case, target, x0, 3)
    assert (out["item_iters"][0, 0], out["item_status"][0, 0]) == (3, br.ST_MAXITER)
    lg = qc.objective(case)
    f_end = lg(_reduced(out["item_x"][0, 0]), qc.template(case).model_gates, target[0])[0]
    f_start = lg(_reduced(x0[0, 0]), qc.template(case).model_gates, target[0])[0]
    print(f"q3 far start: loss {f_start:.6f} -> {out['item_loss'][0, 0]:.6f}, error {abs(out['item_loss'][0, 0] - f_end):.3e}")
    assert abs(out["item_loss"][0, 0] - f_end) <= qc.loss_bound(case) and out["item_loss"][0, 0] < f_start
    assert np.all(np.abs(out["item_x"][0, 0] - x0[0, 0]) < 3 * 2.0 + 1e-9)  # three steps of at most STEP_MAX each
    for bad in (np.nan, np.inf, 1e12):
        xb = x0.copy()
        xb[0, 0, -1] = bad
        with pytest.raises(_ffi.SlamHipError, match="explicit seeds must be finite"):
            _launch(hip_ctx, case, target, xb, 3)
    mcase = next(c for c in FIX["other"]["cases"] if c["name"] == "ccz-cx-own")
    mitem = mcase["items"][0]
    xb = qc.start_point(mcase, mitem)[None, None, :].copy()
    xb[0, 0, 0] = -1e12
    with pytest.raises(_ffi.SlamHipError, match="explicit seeds must be finite"):
        _launch(hip_ctx, mcase, qc.target_matrix(mcase, mitem)[None], xb, 3)
