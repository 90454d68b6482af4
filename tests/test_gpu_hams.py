"""GPU: time-sliced Hamiltonian templates (csrc/slam_hams.hpp, slam_hams_eval / slam_hams_minimize, hamiltonian.TimeSliced and the
n_slices constructors through basis.HamiltonianTemplate) against the NumPy model tests/hams_ref.py.  The fixed cases come from
tests/hams_cases.py; tests/test_hams_host.py holds the CPU side (the model against mpmath, SciPy BFGS on the model from the start points
used here)."""
import numpy as np
import pytest

import ham_cases
import hams_cases
import hams_ref
from slam_decomposition_amd import _ffi
from slam_decomposition_amd import hamiltonian as hm
from slam_decomposition_amd.basis import HamiltonianTemplate
from slam_decomposition_amd.cost_function import BasicCost
from slam_decomposition_amd.optimizer import TemplateOptimizer

pytestmark = pytest.mark.gpu

# Evaluation parity, per number of slices S: 10 x the largest difference measured on an MI355X against tests/hams_ref.py over all cases
# of test_evaluation_parity (and, at S = 3, test_evaluation_parity_many_items) -- the project's convention; DESIGN.md has the table.
# Measured (loss, gradient, unitary, U U^+ - 1):
#   S = 1: 3.7e-15 (smush, SquareCost), 1.8e-13 (smush, BasicCost), 6.0e-15 (circulator), 2.0e-15 (smush1q)
#   S = 2: 2.3e-15 (smush, BasicCost), 7.7e-14 (smush, BasicCost), 7.3e-15 (smush), 3.6e-15 (smush)
#   S = 3: 3.3e-15 (the 4096 rows, SquareCost), 1.3e-13 (smush, BasicCost), 5.4e-15 (smush1q), 5.3e-15 (the 4096 rows)
#   S = 8: 5.4e-15 (smush, SquareCost), 3.6e-14 (circulator, BasicCost), 1.1e-14 (smush1q), 1.1e-14 (smush1q)
# The model itself is within 7.0e-15 / 7.1e-15 / 6.6e-15 / 7.6e-15 (U) and 1.6e-15 / 1.6e-15 / 1.7e-15 / 1.8e-15 (loss) of a 40-digit
# reference on these rows at S = 1 / 2 / 3 / 8 (tests/test_hams_host.py).
BOUNDS = {  # S: (loss, gradient, unitary, U U^+ - 1)
    1: (3.7e-14, 1.8e-12, 6.0e-14, 2.0e-14),
    2: (2.3e-14, 7.7e-13, 7.3e-14, 3.6e-14),
    3: (3.3e-14, 1.3e-12, 5.4e-14, 5.3e-14),
    8: (5.4e-14, 3.6e-13, 1.1e-13, 1.1e-13),
}
# slam_ham_eval against its own model (tests/test_gpu_ham.py: LOSS_BOUND, GRAD_BOUND), for the comparisons of the two device paths
HAM_LOSS_BOUND, HAM_GRAD_BOUND = 8.3e-14, 1.8e-13


def _compare(tag, n_slices, got, ref, keep=None):
    loss, grad, u = got
    loss_ref, grad_ref, u_ref = ref
    keep = slice(None) if keep is None else keep
    e_loss = np.max(np.abs(loss - loss_ref)[keep])
    e_grad = np.max(np.abs(grad - grad_ref)[keep])
    e_u = np.max(np.abs(u - u_ref))
    e_unit = np.max(np.abs(u @ u.conj().transpose(0, 2, 1) - np.eye(u.shape[1])))
    print(f"hams parity {tag}: max errors loss {e_loss:.3e} grad {e_grad:.3e} unitary {e_u:.3e} U U^+ - 1 {e_unit:.3e}")
    b = BOUNDS[n_slices]
    assert e_loss < b[0] and e_grad < b[1]
    assert e_u < b[2] and e_unit < b[3]


@pytest.mark.parametrize("square", [False, True], ids=["basic", "square"])
@pytest.mark.parametrize("n_slices", hams_cases.SLICES)
@pytest.mark.parametrize("name", hams_cases.NAMES)
def test_evaluation_parity(hip_ctx, name, n_slices, square):
    """ConversionGainSmush (4x4), ConversionGainSmush1QPhase (4x4: z terms, phases, free t) and the sliced circulator (8x8, free t) at
    S = 1, 2, 3, 8: 2 targets, per target the fixed rows of hams_cases.special_rows (x = 0, one slice with H = 0, all slices equal, a
    parameter read by one slice only, strengths of 2 pi, a negative time, a slice with degenerate eigenvalues) and 8 random rows in
    [-pi, pi), target_of out of order; every row has |z| >= 0.05 and every fixed row is among them."""
    terms, targets, x, tof, kept = hams_cases.parity_items(name, n_slices)
    assert np.any(np.diff(tof) < 0) and np.all(kept >= 1)
    ref = hams_cases.parity_reference(name, n_slices, square)
    assert np.all(1.0 - hams_cases.parity_reference(name, n_slices, False)[0] >= ham_cases.Z_FLOOR)
    _compare(f"{name} S={n_slices} square={square}", n_slices, hip_ctx.hams_eval(terms, targets, x, tof, cost_kind=int(square), want_unitary=True), ref)


@pytest.mark.parametrize("square", [False, True], ids=["basic", "square"])
def test_evaluation_parity_many_items(hip_ctx, square):
    """4096 rows at S = 3 in one call: every wavefront takes several items and uses its workspace again.  Loss and gradient are
    compared on the rows with |z| >= 0.05."""
    terms, targets, x, tof = hams_cases.big_items()
    keep = (1.0 - hams_cases.big_reference(False)[0]) >= ham_cases.Z_FLOOR
    assert keep.sum() > 3500
    _compare(f"4096 rows S=3 square={square}", 3, hip_ctx.hams_eval(terms, targets, x, tof, cost_kind=int(square), want_unitary=True),
             hams_cases.big_reference(square), keep)


@pytest.mark.parametrize("name", ["smush", "circulator"])
def test_one_slice_is_slam_ham_eval(hip_ctx, name):
    """S = 1 against slam_ham_eval on the same description (ConversionGainSmush1QPhase is left out: its z terms put four contributions on
    one entry, which slam_ham_eval refuses).  Both are within their bounds of one model, so within the sum of each other."""
    terms, targets, x, tof, _ = hams_cases.parity_items(name, 1)
    loss, grad, u = hip_ctx.hams_eval(terms, targets, x, tof, want_unitary=True)
    loss1, grad1, u1 = hip_ctx.ham_eval(hm.slice_terms(terms, 0), targets, x, tof, want_unitary=True)
    print(f"hams S=1 vs ham {name}: loss {np.max(np.abs(loss - loss1)):.3e} grad {np.max(np.abs(grad - grad1)):.3e} U {np.max(np.abs(u - u1)):.3e}")
    assert np.max(np.abs(loss - loss1)) < BOUNDS[1][0] + HAM_LOSS_BOUND and np.max(np.abs(grad - grad1)) < BOUNDS[1][1] + HAM_GRAD_BOUND


@pytest.mark.parametrize("n_slices", [2, 3, 8])
def test_equal_slices_are_the_unsliced_circulator(hip_ctx, n_slices):
    """All slices equal: the loss is the unsliced circulator's (slam_ham_eval), the gradients of the shared parameters (phases, time)
    are equal, and the per-slice gradients of a strength sum to the unsliced one."""
    S = n_slices
    terms, targets, _, _, _ = hams_cases.parity_items("circulator", S)
    base = hm.CirculatorHamiltonian().device_terms()
    rng = np.random.default_rng(80 + S)
    xb = rng.uniform(-1.5, 1.5, (16, 7))
    keep = np.array([1.0 - abs(np.trace(targets[0].conj().T @ hm.CirculatorHamiltonian.construct_U(*row))) / 8 for row in xb]) <= 1.0 - ham_cases.Z_FLOOR
    assert keep.sum() >= 8
    x = np.concatenate([xb[:, :3], np.repeat(xb[:, 3:6], S, axis=1), xb[:, 6:]], axis=1)
    loss, grad, _ = hip_ctx.hams_eval(terms, targets, x, np.zeros(16, np.int32))
    loss1, grad1, _ = hip_ctx.ham_eval(base, targets, xb, np.zeros(16, np.int32))
    folded = np.concatenate([grad[:, :3], grad[:, 3:3 + 3 * S].reshape(16, 3, S).sum(axis=2), grad[:, -1:]], axis=1)
    print(f"hams equal slices S={S}: loss {np.max(np.abs(loss - loss1)[keep]):.3e} folded grad {np.max(np.abs(folded - grad1)[keep]):.3e}")
    assert np.max(np.abs(loss - loss1)[keep]) < BOUNDS[S][0] + HAM_LOSS_BOUND
    assert np.max(np.abs(folded - grad1)[keep]) < S * BOUNDS[S][1] + HAM_GRAD_BOUND  # (a sum of S gradient entries)


@pytest.mark.parametrize("n_slices", hams_cases.SLICES)
@pytest.mark.parametrize("name", hams_cases.NAMES)
def test_zero_hamiltonian_is_exact(hip_ctx, name, n_slices):
    """x = 0: every H_s = 0, no rotation is made, every U_s and their product is the identity exactly."""
    terms, targets, _, _, _ = hams_cases.parity_items(name, n_slices)
    d = terms["dim"]
    loss, grad, u = hip_ctx.hams_eval(terms, targets, np.zeros((1, terms["n_params"])), [0], want_unitary=True)
    assert np.array_equal(u[0], np.eye(d)) and np.all(np.isfinite(grad))
    assert abs(loss[0] - (1.0 - abs(np.trace(targets[0])) / d)) < 4 * np.finfo(float).eps


def test_local_convergence(hip_ctx):
    """ConversionGainSmush1QPhase at S = 4 under SquareCost, the target construct_U_flat(p*) with p* uniform in [0.5, 1.5)^17 (see
    hams_cases.local_case for the range), 8 starts within +-0.05 of p*: every restart ends below 1e-10 (SciPy on the model: 8 of 8,
    tests/test_hams_host.py), and the model reproduces the returned losses."""
    terms, target, p, x0 = hams_cases.local_case()
    prm = _ffi.OptParams(restarts=8, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=1, flags=0)
    out = hip_ctx.hams_minimize(terms, target, prm, 1e-10, x0, cost_kind=_ffi.COST_SQUARE)
    print("hams local convergence: losses", out["item_loss"][0], "iterations", out["item_iters"].min(), "..", out["item_iters"].max(), "status",
          out["item_status"][0])
    assert np.all(out["item_loss"] < 1e-10)
    for r in range(8):
        assert abs(hams_ref.loss_grad(terms, out["item_x"][0, r], target[0], True)[0] - out["item_loss"][0, r]) < BOUNDS[8][0]  # (S = 4: the bound of the cap)


def _search(seed=hams_cases.SEARCH_SEED):
    low, high = hams_cases.search_range()
    basis = HamiltonianTemplate(hams_cases.search_hamiltonian(), low, high)
    return TemplateOptimizer(basis, BasicCost(), seed=seed, training_restarts=hams_cases.SEARCH_RESTARTS, override_fail=True)


def test_search_through_the_api(hip_ctx):
    """Which piecewise-constant pulse makes my gate: HamiltonianTemplate(ConversionGainSmush1QPhase(n_slices=4)) on two planted targets,
    16 restarts.  The best loss is below 1e-10, eval(Xk) is the target up to a phase, Xk has all 17 parameters; ordered early exit
    returns the lowest-index successful restart of a run without early exit (where at least one restart succeeds: SciPy on the model
    solves 16 of 16 from these start points, tests/test_hams_host.py; the device 14 and 15); two calls with one seed are bit-equal."""
    targets = hams_cases.search_targets()
    a, b = _search(), _search()
    da, db = a.approximate_target_U(targets), b.approximate_target_U(targets)
    n = a.basis.n_params
    for ea, eb, target in zip(da, db, targets):
        print(f"hams search: loss {ea.loss_result:.3e} Xk {np.round(ea.Xk, 4)}")
        assert ea.success_label == 1 and ea.loss_result < 1e-10 and ea.cycles == 1 and len(ea.Xk) == n == 17
        assert ham_cases.equal_up_to_phase(a.basis.eval(ea.Xk), target) < 1e-4  # (1 - |z| < 1e-10: entries within sqrt(2 d 1e-10))
        assert ea.loss_result == eb.loss_result and np.array_equal(ea.Xk, eb.Xk)
    out = a.last_ham_stage
    x0 = a.basis.start_points(hams_cases.SEARCH_SEED, len(targets), hams_cases.SEARCH_RESTARTS)
    full = hip_ctx.hams_minimize(a.basis.device_terms, targets, a._opt_params().replace(flags=0), 1e-10, x0)
    solved = (full["item_loss"] < 1e-10).sum(axis=1)
    print("hams search: restarts below 1e-10 per target", solved.tolist())
    assert np.all(solved >= 1) and not np.any(full["item_status"] == 5)  # nothing pre-empted without early exit
    for t in range(len(targets)):
        want = int(np.nonzero(full["item_loss"][t] < 1e-10)[0][0])
        assert out["best_restart"][t] == want and out["best_loss"][t] == full["item_loss"][t, want]
        assert np.array_equal(out["best_x"][t], full["item_x"][t, want]) and np.array_equal(da[t].Xk, full["item_x"][t, want])
        st = out["item_status"][t]
        assert np.all((st == 5) | (out["item_loss"][t] == full["item_loss"][t])) and np.all(st[: want + 1] != 5)
