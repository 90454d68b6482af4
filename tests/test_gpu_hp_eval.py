"""GPU: the four families of fused "loss + analytic gradient" kernels against a 40-digit reference at general-position AND hard inputs.

The expected values come from tests/golden/hp_eval_reference.npz alone (tools/make_hp_reference.py, tests/hp_ref.py: mpmath at 40 digits,
gradients by central differences of the 40-digit loss); nothing here imports mpmath or the fp64 oracles' evaluation code.

Tolerance per (group, cost, input kind): 8 * max(e_ref), e_ref = the fp64 oracle's own error against the 40-digit value at the same inputs,
never above 1e-13 (ten times below the 1e-12 of the oracle parity tests) and never derived from what a kernel returns (hp_ref.tolerances).
The factor: the kernels' sincos is within 2 ulp where libm is within 1, their products are contracted and summed in another order, and
1 / |t| comes from a refined hardware seed -- each worth a factor of two over the oracle's own error.

Large angles: the fp64 oracle forms phi + lam in fp64 before it exponentiates and is off by 3e-11 at |x| = 3e7, 1e-8 at 1.9e9 (pinned in
tests/test_hp_ref_host.py), which is why test_gpu_eval_parity.py::test_eval_large_angles_and_empty sits at 1e-10 and cannot be tightened
with the oracle.  The kernels take sincos per parameter; here they meet the tolerance of the general-position inputs of the same group at
|x| = 3e7 .. 1.9e9, on both sides of the table path's limit 2e8.

Every test prints one line per (group, cost, kind): worst observed error and tolerance (pytest -s shows them; DESIGN.md has the table).
"""
import numpy as np
import pytest

import hp_ref as hp
from slam_decomposition_amd import _ffi

pytestmark = pytest.mark.gpu

GROUPS = hp.load_fixture()
TOL = hp.tolerances(GROUPS)
COST_KIND = {"basic": _ffi.COST_BASIC, "square": _ffi.COST_SQUARE, "makhlin": _ffi.COST_MAKHLIN}
FIXED = [gi for gi, g in enumerate(GROUPS) if g["meta"]["family"] in ("short", "long")]
V2 = [gi for gi, g in enumerate(GROUPS) if g["meta"]["family"] == "v2"]
SMUSH = [gi for gi, g in enumerate(GROUPS) if g["meta"]["family"] == "smush"]
STEP_BOUND = 2.0**-22


def _label(gi):
    m = GROUPS[gi]["meta"]
    cls = hp.GC_NAMES[m["gclass"]] if m["family"] == "short" else m.get("mode", "")
    return f"{m['family']}-{m['gate']}-k{m['k']}" + (f"-{cls}" if cls else "")


def _ids(gis):
    return [_label(gi) for gi in gis]


def _check(gi, ci, what, err_per_case, failures, tol_of=None):
    """One printed line per input kind; a failure entry where the worst error of the kind is above its tolerance."""
    g = GROUPS[gi]
    kinds = g["meta"]["kinds"]
    for kind in sorted(set(kinds)):
        sel = [m for m, kd in enumerate(kinds) if kd == kind and np.isfinite(err_per_case[m])]
        nan = [m for m, kd in enumerate(kinds) if kd == kind and np.isnan(err_per_case[m])]
        if not sel and not nan:
            continue
        worst = max([float(err_per_case[m]) for m in sel], default=0.0)
        tol = TOL[(gi, ci, kind)] if tol_of is None else tol_of(kind)
        line = f"HP {_label(gi):34s} {g['meta']['costs'][ci]:8s} {kind:14s} {what:10s} worst {worst:9.2e}  tol {tol:9.2e}"
        bad = worst > tol or bool(nan)
        print(line + ("  FAIL" if bad else ""))
        if bad:
            failures.append(line + (f" (not finite: cases {nan})" if nan else ""))


def _err(a, b):
    """max |a - b| per case; NaN where the kernel's value is not finite."""
    d = np.abs(np.asarray(a) - np.asarray(b)).reshape(len(a), -1).max(axis=1)
    return np.where(np.isfinite(d), d, np.nan)


def test_the_fixture_reaches_all_five_gate_classes_and_no_tolerance_is_above_the_cap():
    seen = set()
    for gi in FIXED:
        g = GROUPS[gi]
        if g["meta"]["family"] == "short":
            cls = hp.classify_gates_host(hp.gate_list(g))  # the rule of classify_gates on the fp64 matrices the context receives
            assert cls == g["meta"]["gclass"]
            seen.add(cls)
    assert seen == {hp.GC_DENSE, hp.GC_XGEN, hp.GC_XRI, hp.GC_CX, hp.GC_XRI1}
    assert {GROUPS[gi]["meta"]["k"] for gi in FIXED} == {1, 2, 3, 4, 5, 6, 7, 8, 12, 16}
    assert max(TOL.values()) <= 1e-13 and min(TOL.values()) > 0.0


@pytest.mark.parametrize("gi", FIXED, ids=_ids(FIXED))
def test_fixed_gate_evaluation_matches_40_digits(hip_ctx, gi):
    """slam_eval_loss_grad (eval_quad<K, HUGE_ARGS = true, GC> for spans 1..5, the wavefront-per-item kernel for 6..16)."""
    g = GROUPS[gi]
    hip_ctx.set_targets(g["targets"])
    hip_ctx.set_gates(g["gates"])
    failures = []
    try:
        for ci, cost in enumerate(g["meta"]["costs"]):
            hip_ctx.set_cost(COST_KIND[cost])
            loss, grad = hip_ctx.eval_loss_grad(list(g["seq"]), g["x"], g["tof"])
            _check(gi, ci, "loss", _err(loss, g["loss"][ci]), failures)
            _check(gi, ci, "gradient", _err(grad, g["grad"][ci]), failures)
    finally:
        hip_ctx.set_cost(_ffi.COST_BASIC)
    assert not failures, "\n" + "\n".join(failures)


def _w_tol(g):
    kinds = g["meta"]["kinds"]
    return lambda kind: min(hp.TOL_FACTOR * max(g["e_ref_w"][m] for m, kd in enumerate(kinds) if kd == ("general" if kind in hp.LARGE_KINDS else kind)), hp.TOL_CAP)


@pytest.mark.parametrize("gi", V2, ids=_ids(V2))
def test_v2_evaluation_matches_40_digits(hip_ctx, gi):
    """slam_v2_eval_loss_grad in device order: loss, the gradient with respect to the U-gate AND the gate parameters, W(x).  vz_only and
    no_exterior_1q templates are the device vectors whose pinned slots are zero."""
    g = GROUPS[gi]
    qn = int(g["meta"]["qn"])
    hip_ctx.set_targets(g["targets"])
    hip_ctx.v2_set_gates([_ffi.V2Gate(qn, g["sel"][i], g["scale"][i], g["offset"][i]) for i in range(len(g["sel"]))])
    failures = []
    try:
        for ci, cost in enumerate(g["meta"]["costs"]):
            hip_ctx.set_cost(COST_KIND[cost])
            loss, grad, W = hip_ctx.v2_eval(list(g["seq"]), g["x"], g["tof"], want_unitary=True)
            _check(gi, ci, "loss", _err(loss, g["loss"][ci]), failures)
            _check(gi, ci, "gradient", _err(grad, g["grad"][ci]), failures)
            _check(gi, ci, "unitary", _err(W, g["W"]), failures, _w_tol(g))
    finally:
        hip_ctx.set_cost(_ffi.COST_BASIC)
    assert not failures, "\n" + "\n".join(failures)


@pytest.mark.parametrize("gi", SMUSH, ids=_ids(SMUSH))
def test_smush_evaluation_matches_40_digits(hip_ctx, gi):
    """slam_smush_eval_loss_grad with u = (tau w)^2 of both 2x2 blocks of every slice at 0, ~1e-18, inside the series range, and on both
    sides of the hand-over u = 0.04 between the series and the closed form of ``sm_slice``."""
    g = GROUPS[gi]
    qn, N = int(g["meta"]["qn"]), int(g["meta"]["n_slices"])
    hip_ctx.set_targets(g["targets"])
    hip_ctx.smush_set_gates([_ffi.SmushGate(qn, N, g["t"][i], list(g["sel"][i]), list(g["scale"][i]), list(g["offset"][i])) for i in range(len(g["sel"]))])
    failures = []
    try:
        for ci, cost in enumerate(g["meta"]["costs"]):
            hip_ctx.set_cost(COST_KIND[cost])
            loss, grad, W = hip_ctx.smush_eval(list(g["seq"]), g["x"], g["tof"], want_unitary=True)
            _check(gi, ci, "loss", _err(loss, g["loss"][ci]), failures)
            _check(gi, ci, "gradient", _err(grad, g["grad"][ci]), failures)
            _check(gi, ci, "unitary", _err(W, g["W"]), failures, _w_tol(g))
    finally:
        hip_ctx.set_cost(_ffi.COST_BASIC)
    assert not failures, "\n" + "\n".join(failures)


@pytest.mark.parametrize("gi", FIXED, ids=_ids(FIXED))
def test_the_optimizers_instantiation_matches_40_digits(hip_ctx, gi):
    """``minimize_body`` runs eval_quad<K, HUGE_ARGS = false, GC> (another sincos entry, the ldexp half angle), not the instantiation
    slam_eval_loss_grad launches.  From every input with |x| < 2e8 as its own start point, one restart:

      * maxiter = 0 returns the loss at x0: within the tolerance of the stand-alone loss (BasicCost and SquareCost);
      * maxiter = 1 (BasicCost) returns x0 + s with s parallel to minus the 40-digit gradient: max_i |d_i / |d| + g_i / |g|| <= 2^-22.
        Derived, not measured: the first direction is -H g with H = 1 applied in float32 (oracle/bfgs_port.py), a relative rounding of at
        most 2^-24 per component, doubled once for the normalisation and once for the fp64 rounding of x0 + s.  The generator kept only
        inputs from which oracle.bfgs_port.minimize_port(maxiter = 1) accepts a step (``step`` = 1); near-solution inputs with
        eps = 0 / 1e-8 converge at x0 (``step`` = 0) and are in the maxiter = 0 check only.  An item with item_iters == 0 among the
        ``step`` = 1 inputs is a failure, not an exclusion.
    """
    g = GROUPS[gi]
    step = np.array(g["meta"]["step"])
    use = np.nonzero(step >= 0)[0]
    x0 = g["x"][use]
    hip_ctx.set_targets(g["targets"][g["tof"][use]])  # one target per item
    hip_ctx.set_gates(g["gates"])
    seq = list(g["seq"])
    failures = []
    try:
        for ci, cost in enumerate(g["meta"]["costs"]):
            if cost == "makhlin":
                continue
            hip_ctx.set_cost(COST_KIND[cost])
            out = hip_ctx.minimize_stage(seq, _ffi.OptParams(restarts=1, maxiter=0, seed=1), x0=x0[:, None, :])
            err = np.full(len(step), -np.inf)
            err[use] = _err(out["item_loss"][:, 0], g["loss"][ci][use])
            _check(gi, ci, "x0 loss", err, failures)
            assert np.array_equal(out["best_x"], x0)
        hip_ctx.set_cost(_ffi.COST_BASIC)
        ci = g["meta"]["costs"].index("basic")
        out = hip_ctx.minimize_stage(seq, _ffi.OptParams(restarts=1, maxiter=1, seed=1), x0=x0[:, None, :])
        stepped = step[use] == 1
        iters = out["item_iters"][:, 0]
        no_step = [int(use[i]) for i in np.nonzero(stepped & (iters == 0))[0]]
        if no_step:
            failures.append(f"HP {_label(gi)}: no first step from cases {no_step} (item_status {out['item_status'][:, 0][stepped & (iters == 0)]})")
        dev = np.full(len(step), -np.inf)
        for i in np.nonzero(stepped & (iters >= 1))[0]:
            d = out["best_x"][i] - x0[i]
            gr = g["grad"][ci][use[i]]
            dev[use[i]] = np.max(np.abs(d / np.linalg.norm(d) + gr / np.linalg.norm(gr)))
        _check(gi, ci, "first step", dev, failures, lambda kind: STEP_BOUND)
    finally:
        hip_ctx.set_cost(_ffi.COST_BASIC)
    assert not failures, "\n" + "\n".join(failures)


def test_non_finite_parameters_give_a_non_finite_loss(hip_ctx):
    """NaN or +-inf in x through slam_eval_loss_grad (no argument check on the values of x): the call returns and the loss of exactly the
    affected items is NaN -- never a finite number; the other items of the batch keep their values."""
    g = GROUPS[FIXED[1]]
    hip_ctx.set_targets(g["targets"])
    hip_ctx.set_gates(g["gates"])
    hip_ctx.set_cost(_ffi.COST_BASIC)
    seq, n = list(g["seq"]), g["x"].shape[1]
    x = np.repeat(g["x"][:1], 5, axis=0)
    x[1, 0] = np.nan       # a half angle
    x[2, n - 1] = np.inf   # a phase of the last layer
    x[3, 4] = -np.inf
    tof = np.zeros(5, np.int32)
    loss, grad = hip_ctx.eval_loss_grad(seq, x, tof)
    print("HP non-finite x: loss", loss)
    assert np.all(np.isnan(loss[1:4])), loss
    assert loss[0] == loss[4] and np.isfinite(loss[0]) and np.array_equal(grad[0], grad[4]) and np.all(np.isfinite(grad[0]))
    assert not np.any(np.isfinite(grad[1:4]).all(axis=1)), grad[1:4]


def test_smush_arguments_from_2e8_on_are_nan_by_design(hip_ctx):
    """``sm_sincos`` (csrc/slam_smush.hpp) has the table path only and returns NaN from |argument| = 2e8 on -- far outside any pulse or
    angle an optimizer reaches -- where the fixed-gate and V2 evaluations switch to the out-of-line path.  That is why the fixture has
    no large-angle kind for this family; the behaviour is pinned here: NaN, never a finite number, and finite just below the limit."""
    gi = next(i for i in SMUSH if GROUPS[i]["meta"]["gate"] == "N4_off0")
    g = GROUPS[gi]
    qn, N = int(g["meta"]["qn"]), int(g["meta"]["n_slices"])
    hip_ctx.set_targets(g["targets"])
    hip_ctx.smush_set_gates([_ffi.SmushGate(qn, N, g["t"][i], list(g["sel"][i]), list(g["scale"][i]), list(g["offset"][i])) for i in range(len(g["sel"]))])
    hip_ctx.set_cost(_ffi.COST_BASIC)
    x = np.repeat(g["x"][:1], 4, axis=0)
    x[1, 1] = 2.1e8    # a phase of layer 0
    x[2, 0] = -4.2e8   # a theta: the half angle is at -2.1e8
    x[3, 1] = 1.9e8    # still the table path
    loss, grad, _ = hip_ctx.smush_eval(list(g["seq"]), x, np.zeros(4, np.int32))
    print("HP smush large angles: loss", loss)
    assert np.isfinite(loss[0]) and np.isfinite(loss[3]) and np.all(np.isfinite(grad[[0, 3]]))
    assert np.all(np.isnan(loss[1:3])), loss
