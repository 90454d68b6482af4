"""GPU: the state objectives of the three-qubit templates (csrc/slam_q3.hpp STATE = true, slam_q3s_eval / slam_q3s_minimize,
cost_function.MutualInformation / MutualInformationSquare through TemplateOptimizer) against the NumPy model tests/ent_ref.py, which
takes the literal definition (4x4 partial traces, eigvalsh) where the kernel takes determinants of the 2x2 reduced states.
tests/test_ent_host.py holds the CPU side."""
import functools
import math

import numpy as np
import pytest

import bfgs_replay as br
import ent_ref
import q3_cases
from oracle import bfgs_port as bp
from slam_decomposition_amd import _ffi
from slam_decomposition_amd.basis3q import ThreeQubitCircuitTemplate
from slam_decomposition_amd.cost_function import MutualInformation, MutualInformationSquare
from slam_decomposition_amd.gates import CCZGate, CXGate
from slam_decomposition_amd.optimizer import TemplateOptimizer

pytestmark = pytest.mark.gpu

CX = q3_cases.CX
CCZ = CCZGate().to_matrix()
NO3 = np.zeros((0, 8, 8), dtype=np.complex128)
# name -> (device description (gates2, gates3, arity, gate_index, qubits), model gates, model edges)
TEMPLATES = {
    "cx-k1": ((CX[None], NO3, [2], [0], [(0, 1, 0)]), [CX], [(0, 1)]),
    "cx-k3": ((CX[None], NO3, [2, 2, 2], [0, 0, 0], [(0, 1, 0), (1, 2, 0), (0, 1, 0)]), [CX] * 3, [(0, 1), (1, 2), (0, 1)]),
    "cx-ccz-cx": ((CX[None], CCZ[None], [2, 3, 2], [0, 0, 0], [(0, 1, 0), (0, 1, 2), (1, 2, 0)]), [CX, CCZ, CX], [(0, 1), (0, 1, 2), (1, 2)]),
}
KIND = {False: _ffi.COST_MUTUAL_INFO, True: _ffi.COST_MUTUAL_INFO_SQUARE}
# Parity bounds, keyed by ``square``: ten times the largest deviation measured on the MI355X over the three templates of
# test_evaluation_parity -- loss 2.04e-14 (squared 3.51e-14), gradient 1.53e-14 (squared 3.69e-14), final state 9.03e-16
LOSS_BOUND, GRAD_BOUND, STATE_BOUND = {False: 2.1e-13, True: 3.6e-13}, {False: 1.6e-13, True: 3.7e-13}, 9.1e-15


@functools.lru_cache(maxsize=None)
def _parity_items(name):
    """Per template: the states W, GHZ and two random ones, four random points each -- 16 items (states [4, 8], state_of, x)."""
    n = 9 + 3 * sum(len(e) for e in TEMPLATES[name][2])
    rng = np.random.default_rng(5300 + n)
    states = np.stack([ent_ref.w_state(), ent_ref.ghz_state(), ent_ref.random_state(rng), ent_ref.random_state(rng)])
    return states, np.repeat(np.arange(4), 4).astype(np.int32), rng.uniform(0.0, 2.0 * math.pi, (16, n))


@functools.lru_cache(maxsize=None)
def _parity_reference(name, square):
    _, gates, edges = TEMPLATES[name]
    states, sof, x = _parity_items(name)
    out = [ent_ref.loss_grad(x[m], gates, edges, states[sof[m]], square) for m in range(len(x))]
    return np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


@pytest.mark.parametrize("square", [False, True], ids=["mi", "mi-square"])
@pytest.mark.parametrize("name", sorted(TEMPLATES))
def test_evaluation_parity(hip_ctx, name, square):
    """Loss, gradient and final state of 16 items per template -- one CX (n = 15), three CX on the line (n = 27), CX / CCZ / CX
    (n = 30, the MIXED instantiation) -- against the model.  Measured on the MI355X (loss / gradient / state):
        MutualInformation        cx-k1 1.64e-14 / 1.34e-14 / 7.0e-16   cx-k3 2.04e-14 / 1.53e-14 / 6.7e-16   cx-ccz-cx 1.78e-14 / 1.24e-14 / 9.0e-16
        MutualInformationSquare  cx-k1 3.46e-14 / 3.69e-14             cx-k3 3.35e-14 / 2.71e-14             cx-ccz-cx 3.51e-14 / 2.82e-14
    against gradient components up to 2.6; the bounds (LOSS_BOUND, GRAD_BOUND, STATE_BOUND) are ten times the largest of each row.
    The model's own two formulations of the loss differ by up to 2.7e-14 on the CPU (tests/test_ent_host.py), so most of the loss
    figure is the model's eigvalsh."""
    desc = TEMPLATES[name][0]
    states, sof, x = _parity_items(name)
    loss_ref, grad_ref, v_ref = _parity_reference(name, square)
    loss, grad, v = hip_ctx.q3s_eval(*desc, states, x, sof, cost_kind=KIND[square], want_state=True)
    e_loss, e_grad, e_v = np.max(np.abs(loss - loss_ref)), np.max(np.abs(grad - grad_ref)), np.max(np.abs(v - v_ref))
    print(f"ent parity {name} square={square}: max errors loss {e_loss:.3e} grad {e_grad:.3e} state {e_v:.3e}"
          f" (max |grad| {np.max(np.abs(grad_ref)):.2f})")
    assert np.all(np.isfinite(loss)) and np.all(np.isfinite(grad))
    assert e_loss < LOSS_BOUND[square] and e_v < STATE_BOUND
    assert e_grad < GRAD_BOUND[square]
    # the gradient is optional, and the loss does not depend on asking for it
    l2, g2, v2 = hip_ctx.q3s_eval(*desc, states, x, sof, cost_kind=KIND[square], want_grad=False)
    assert g2 is None and v2 is None and np.array_equal(l2, loss)


@pytest.mark.parametrize("square", [False, True], ids=["mi", "mi-square"])
def test_singular_inputs(hip_ctx, square):
    """One CX on (0, 1) at x = 0, where both singular points of dS/dD are met exactly.
      * GHZ: the CX (control q0, target q1) takes |111> to |101>, so q1 leaves the state: rho_0 = rho_2 = I / 2 (D = 1/4, the 0/0
        of dS/dD) and rho_1 is pure (D = 0, the divergence) in ONE item -- loss 2 (4 squared), not the 3 of GHZ itself;
      * (|000> + |101>) / sqrt 2, which the CX maps onto GHZ: every rho_q = I / 2, loss 3;
      * |000>: a product state; loss and every gradient component at most 1e-12 in magnitude (eigenvalues at rounding level give at
        most about 1e-14).
    The first two against the model within the parity bounds; nothing non-finite anywhere."""
    desc, gates, edges = TEMPLATES["cx-k1"]
    states = np.stack([ent_ref.ghz_state(), ent_ref.pre_ghz_state(), np.eye(8, dtype=np.complex128)[0]])
    x = np.zeros((3, 15))
    loss, grad, v = hip_ctx.q3s_eval(*desc, states, x, np.arange(3), cost_kind=KIND[square], want_state=True)
    print(f"ent singular square={square}: loss {loss.tolist()} max |grad| {np.abs(grad).max(axis=1).tolist()}")
    assert np.all(np.isfinite(loss)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(v.view(np.float64)))
    for m, want in ((0, 4.0 if square else 2.0), (1, 3.0)):
        f, g, vv = ent_ref.loss_grad(x[m], gates, edges, states[m], square)
        assert f == pytest.approx(want, abs=1e-14)
        assert abs(loss[m] - f) < LOSS_BOUND[square] and np.max(np.abs(grad[m] - g)) < GRAD_BOUND[square], m
        assert np.max(np.abs(v[m] - vv)) < STATE_BOUND
    assert np.max(np.abs(v[1] - ent_ref.ghz_state())) < STATE_BOUND
    assert abs(loss[2]) <= 1e-12 and np.max(np.abs(grad[2])) <= 1e-12


# ---- the optimizer ---------------------------------------------------------------------------------------------------------------
def _purities_after(opt, entry):
    v = opt.basis.eval(entry.Xk) @ opt.objective.state_vector
    return ent_ref.purities(v)


def test_ghz_is_disentangled_by_two_cx():
    """GHZ, CX on (0, 2) then (0, 1), spans 1..2, eight restarts, the default threshold 1e-10: one CX leaves two bits of mutual
    information (the floor found with SciPy BFGS on the model), two remove all of it."""
    basis = ThreeQubitCircuitTemplate([CXGate()], [[(0, 2)], [(0, 1)]], maximum_span_guess=2)
    opt = TemplateOptimizer(basis, MutualInformation("ghz"), training_restarts=8, seed=11)
    entry = opt.approximate_target_U(None)
    stage1 = opt.span_best_losses[1][0]
    print(f"ent ghz: cycles {entry.cycles} loss {entry.loss_result:.3e} stage k=1 {stage1!r} k=2 {opt.span_best_losses[2][0]:.3e}")
    assert entry.cycles == 2 and entry.success_label == 1 and entry.loss_result < 1e-10
    assert 2.0 - 1e-9 <= stage1 <= 2.0 + 1e-6
    assert max(abs(p - 1.0) for p in _purities_after(opt, entry)) < 1e-6


def test_w_is_disentangled_by_three_cx():
    """W, CX on (0, 1), (1, 2), (0, 1), spans 1..3: the stage floors 2.2183406773 and 1.1000955192 at k = 1, 2 (SciPy BFGS on the model:
    the best three of six starts agree on each to 1e-11), zero at k = 3."""
    basis = ThreeQubitCircuitTemplate([CXGate()], [[(0, 1)], [(1, 2)], [(0, 1)]], maximum_span_guess=3)
    opt = TemplateOptimizer(basis, MutualInformation("w"), training_restarts=8, seed=12)
    entry = opt.approximate_target_U(None)
    s1, s2 = opt.span_best_losses[1][0], opt.span_best_losses[2][0]
    print(f"ent w: cycles {entry.cycles} loss {entry.loss_result:.3e} stage k=1 {s1!r} k=2 {s2!r}")
    assert entry.cycles == 3 and entry.success_label == 1 and entry.loss_result < 1e-10
    assert 2.2183406773 - 1e-9 <= s1 <= 2.2183406773 + 1e-6
    assert 1.1000955192 - 1e-9 <= s2 <= 1.1000955192 + 1e-6
    assert max(abs(p - 1.0) for p in _purities_after(opt, entry)) < 1e-6


def test_mutual_information_square_on_ghz():
    """MutualInformationSquare, GHZ, two CX.  The success threshold is taken from the model, not from the device: SciPy BFGS (analytic
    gradient of ent_ref, gtol 1e-9, 16 uniform starts, CPU) ends with a median loss of 3.19e-14 (range 1.9e-14 .. 6.9e-14); times
    100: 3.19e-12.  Measured on the MI355X: 6.9e-14 at k = 2, 2.39 at k = 1."""
    threshold = 100 * 3.19e-14
    basis = ThreeQubitCircuitTemplate([CXGate()], [[(0, 2)], [(0, 1)]], maximum_span_guess=2)
    opt = TemplateOptimizer(basis, MutualInformationSquare("ghz"), training_restarts=8, seed=13, success_threshold=threshold)
    entry = opt.approximate_target_U(None)
    print(f"ent ghz square: cycles {entry.cycles} loss {entry.loss_result:.3e} stage k=1 {opt.span_best_losses[1][0]!r}")
    assert entry.cycles == 2 and entry.success_label == 1 and entry.loss_result < threshold
    assert opt.span_best_losses[1][0] > 1.0  # one CX leaves two bits between q0 and the rest: 4 in squares, far from the threshold
    assert max(abs(p - 1.0) for p in _purities_after(opt, entry)) < 1e-6


def test_determinism(hip_ctx):
    desc = (CX[None], NO3, [2, 2], [0, 0], [(0, 2, 0), (0, 1, 0)])
    prm = _ffi.OptParams(restarts=8, maxiter=2500, seed=21, flags=_ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED)
    a = hip_ctx.q3s_minimize(*desc, ent_ref.ghz_state()[None], prm, 1e-10)
    b = hip_ctx.q3s_minimize(*desc, ent_ref.ghz_state()[None], prm, 1e-10)
    assert a["best_loss"][0] < 1e-10
    for key in ("best_loss", "best_x", "best_restart"):
        assert np.array_equal(a[key], b[key]), key
    other = hip_ctx.q3s_minimize(*desc, ent_ref.ghz_state()[None], prm.replace(seed=22), 1e-10)
    assert not np.array_equal(other["best_x"], a["best_x"])  # (the seed does enter)


# ---- the iteration, step by step -------------------------------------------------------------------------------------------------
REPLAY_STARTS = (5401, 5402, 5403, 5404)
# Where the replay is sound.  Model and kernel take log2 of the small eigenvalue lam of a reduced state, and lam is known to a few eps
# ABSOLUTE only (a 2x2 determinant, or eigvalsh): the gradient's error is about eps / (ln 2 sqrt(lam)) and grows towards the minimum,
# where lam -> 0.  Measured on the CPU between ent_ref and a determinant-based NumPy evaluation along the port's trajectory from
# start 5402: at most 15 times that estimate, 7e-15 at lam = 6e-2, 1.5e-11 at 4e-9, 7e-8 at 4e-15 (against gradient components of 4e-6
# there).  bfgs_replay.py presumes a reference whose gradient is good to its band and float32 rounding of the metric as the leading
# difference; the reference's RELATIVE gradient error, 15 eps / (ln 2 lam log2(1 / lam)), reaches float32's 6e-8 at lam = 4e-9.  So
# the steps are replayed while every point has lam >= 1e-8 under the model, with the gradient band at the reference's error there;
# the rest of a run is held to the tail rules of tests/test_gpu_q3_replay.py.
LAM_CUT = 1e-8
GRAD_ERR_AT_CUT = 15.0 * 2.220446049250313e-16 / (math.log(2.0) * math.sqrt(LAM_CUT))  # 4.8e-11


def _smallest_eigenvalue(x, gates, edges, psi):
    v = ent_ref.final_state(x, gates, edges, psi)
    rho8 = np.outer(v, v.conj())
    return min(float(np.linalg.eigvalsh(ent_ref.partial_trace(rho8, (q,)))[0]) for q in range(3))


def _sound_prefix(xs, gates, edges, psi):
    """The number of leading points of xs with lam >= LAM_CUT."""
    for j, x in enumerate(xs):
        if _smallest_eigenvalue(x, gates, edges, psi) < LAM_CUT:
            return j
    return len(xs)


def test_w_runs_follow_the_port_step_by_step(hip_ctx):
    """The machinery of tests/bfgs_replay.py (as tests/test_gpu_q3_replay.py drives it) with ent_ref as the objective: W, three CX on
    the line, from four uniform start points.  ``restarts = 1``, ``flags = 0``, explicit ``x0``: the launch with ``maxiter = j``
    returns the state after accepted step j, j = 1 .. J.  Every replayed step (see LAM_CUT) is held to min(8 e_ref, 1e-2), e_ref = the
    worst clear-step deviation of the float64-metric replay along the float32 port's own trajectories over the same domain (from the
    model alone); the bands are twice the parity bound on the loss and twice the larger of the parity bound and the reference's own
    error at the cut on the gradient; every recorded loss of the whole run is held to the parity bound against the model, and the
    run ends converged or stalled with non-increasing losses.  Measured on the MI355X: 79 steps replayed over the four items, none
    unclear, worst deviation 1.2e-5 against a tolerance of 5.2e-5 (e_ref 6.5e-6), recorded losses within 5.4e-14 of the model.  (With
    every step replayed, the last step of start 5402 -- at lam = 2e-15 -- deviated by 1.6e-2.)"""
    desc, gates, edges = TEMPLATES["cx-k3"]
    psi = ent_ref.w_state()
    defaults = dict(gtol=1e-9, stop_loss=1e-13, gtol_far=1e-5, far_loss=1e-6)
    N = len(REPLAY_STARTS)

    def lg(x, gate_seq, target):
        f, g, _ = ent_ref.loss_grad(x, gate_seq, edges, target)
        return f, g

    band = (2.0 * LOSS_BOUND[False], 2.0 * max(GRAD_BOUND[False], GRAD_ERR_AT_CUT))
    x0 = np.stack([np.random.default_rng(s).uniform(0.0, 2.0 * math.pi, 27) for s in REPLAY_STARTS])
    refs = []  # e_ref from the model alone
    for xs0 in x0:
        xs = []
        bp.minimize_port(xs0, gates, psi, h_dtype=np.float32, loss_and_grad=lg, xs=xs, record=[], maxiter=2500, **defaults)
        refs.append(br.replay(lg, gates, psi, xs0, xs[:_sound_prefix(xs, gates, edges, psi)], band, h_dtype=np.float64, maxiter=2500, **defaults))
    tol = br.tolerance(br.worst_clear(refs))

    def launch(maxiter):
        prm = _ffi.OptParams(restarts=1, maxiter=int(maxiter), seed=1, flags=0, **defaults)
        return hip_ctx.q3s_minimize(*desc, np.tile(psi, (N, 1)), prm, 1e-10, x0=x0[:, None, :])

    full = launch(2500)
    it_full = full["item_iters"][:, 0]
    assert np.all(full["item_status"] != 5) and np.all(it_full >= 1)
    J = int(it_full.max())
    xs = [np.empty((int(n), 27)) for n in it_full]
    fl = [np.empty(int(n)) for n in it_full]
    for j in range(1, J + 1):
        out = launch(j)
        assert np.array_equal(out["item_iters"][:, 0], np.minimum(j, it_full)), j
        for i in range(N):
            if j <= it_full[i]:
                xs[i][j - 1], fl[i][j - 1] = out["item_x"][i, 0], out["item_loss"][i, 0]
    failures, results = [], []
    for i in range(N):
        assert np.array_equal(xs[i][-1], full["item_x"][i, 0]) and fl[i][-1] == full["item_loss"][i, 0]
        m = _sound_prefix(xs[i], gates, edges, psi)
        rp = br.replay(lg, gates, psi, x0[i], xs[i][:m], band, **dict(defaults, maxiter=2500))
        results.append(rp)
        f_model = np.array([lg(x, gates, psi)[0] for x in xs[i]])
        err = np.abs(fl[i] - f_model).max()
        worst = max(rp["dev"], default=0.0)
        status = int(full["item_status"][i, 0])
        print(f"ent replay start {REPLAY_STARTS[i]}: iters {it_full[i]} replayed {len(rp['dev'])} of {m} sound steps, unclear {sum(rp['unclear'])},"
              f" worst {worst:.2e} tol {tol:.2e} loss error {err:.2e} status {status} end loss {fl[i][-1]:.3e}")
        if not err <= LOSS_BOUND[False]:
            failures.append(f"start {i}: recorded losses off the model's by {err:.2e}")
        if worst > tol:
            failures.append(f"start {i}: step {int(np.argmax(rp['dev']))} deviates by {worst:.2e} (tolerance {tol:.2e})")
        if len(rp["dev"]) < min(m, 10):
            failures.append(f"start {i}: only {len(rp['dev'])} of {m} steps replayed")
        if np.any(np.diff(fl[i]) > 0):
            failures.append(f"start {i}: the recorded losses increase")
        if status not in (br.ST_CONVERGED, br.ST_STALLED):
            failures.append(f"start {i}: status {status}")
        if m == it_full[i] and rp["noise_from"] is None and not rp["item_unclear"]:  # replayed to the end: the port's counts
            got = (int(it_full[i]), int(full["item_evals"][i, 0]), status)
            if got != (rp["iters"], rp["evals"], rp["status"]):
                failures.append(f"start {i}: iters, evals, status {got}, the replay predicts {(rp['iters'], rp['evals'], rp['status'])}")
    cen = br.census(results)
    print(f"ENT REPLAY items {N} steps {cen['steps']} unclear {cen['unclear']} (items {cen['items_unclear']}) back-tracks {cen['backtracks']}"
          f" short {cen['short']} first-scaling {cen['first_scaling']} e_ref {br.worst_clear(refs):.2e} tol {tol:.2e}")
    if cen["steps"] < 40:
        failures.append(f"only {cen['steps']} steps replayed over the four items")
    if cen["unclear"] > 0.02 * max(cen["steps"], 1):  # (the step cap of the q3 module; its item cap, 10 %, is below one of four items)
        failures.append(f"{cen['unclear']} of {cen['steps']} steps unclear")
    assert not failures, "\n" + "\n".join(failures)
