"""GPU: three-qubit basis gates in three-qubit templates (csrc/slam_q3.hpp MIXED = true, slam_q3m_eval / slam_q3m_minimize,
basis3q.ThreeQubitCircuitTemplate with gates.Gate3Q) against the NumPy model tests/q3m_ref.py.  The fixed cases come from
tests/q3m_cases.py; tests/test_q3m_host.py holds the CPU side (SciPy BFGS on the model solves the targets chosen here)."""
import functools

import numpy as np
import pytest

import q3_cases
import q3_ref
import q3m_cases
import q3m_ref
from slam_decomposition_amd import _ffi
from slam_decomposition_amd.basis3q import ThreeQubitCircuitTemplate
from slam_decomposition_amd.cost_function import BasicCost
from slam_decomposition_amd.gates import CCXGate, CCZGate, CXGate
from slam_decomposition_amd.optimizer import TemplateOptimizer

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _parity_reference(name, square):
    case = q3m_cases.parity_template(name)
    targets, x = q3m_cases.parity_items(name)
    out = [q3m_ref.loss_grad(x[m], case.model_gates, case.edges, targets[m], square) for m in range(len(x))]
    return np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


@pytest.mark.parametrize("square", [False, True], ids=["basic", "square"])
@pytest.mark.parametrize("name", q3m_cases.PARITY_NAMES)
def test_evaluation_parity(hip_ctx, name, square):
    """Loss, gradient and unitary of 8 items per template of q3m_cases.parity_template against the model (all 8 have
    |Tr(T^+ W)| / 8 >= 0.05 by construction, the floor tests/test_gpu_q3.py applies).  Bounds:
    test_gpu_q3.py holds two-qubit templates to 3.4e-15 (loss), 4.8e-15 (gradient), 2.0e-14 (unitary); a three-qubit position is an
    8-term complex dot product where a two-qubit one has 4, so its rounding contribution is at most twice as large: twice those."""
    case = q3m_cases.parity_template(name)
    targets, x = q3m_cases.parity_items(name)
    loss_ref, grad_ref, w_ref = _parity_reference(name, square)
    loss, grad, w = hip_ctx.q3m_eval(*case.description(), targets, x, np.arange(8), cost_kind=int(square), want_unitary=True)
    e_loss = np.max(np.abs(loss - loss_ref))
    e_grad = np.max(np.abs(grad - grad_ref))
    e_w = np.max(np.abs(w - w_ref))
    print(f"q3m parity {name} square={square}: max errors loss {e_loss:.3e} grad {e_grad:.3e} unitary {e_w:.3e}")
    assert e_loss < 6.8e-15 and e_w < 4.0e-14
    assert e_grad < 9.6e-15


def test_two_qubit_only_templates_are_bit_equal(hip_ctx):
    """With no three-qubit position the new pair returns what slam_q3_eval / slam_q3_minimize return, bit for bit."""
    gates, gate_index, edges, targets, x = q3_cases.parity_case(5)
    qubits = [e + (0,) for e in edges]
    for square in (0, 1):
        a = hip_ctx.q3_eval(gates, gate_index, edges, targets, x, np.arange(64), cost_kind=square, want_unitary=True)
        b = hip_ctx.q3m_eval(gates, np.zeros((0, 8, 8)), [2] * 5, gate_index, qubits, targets, x, np.arange(64), cost_kind=square,
                             want_unitary=True)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    t4 = q3_cases.reachable_targets()[:4]
    prm = _ffi.OptParams(restarts=4, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=7, flags=_ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED)
    # with early exit the result of a target is fixed, when a later restart is pre-empted is not: every item is compared without it
    for p, keys in ((prm, ("best_loss", "best_x", "best_restart")),
                    (prm.replace(flags=0), ("best_loss", "best_x", "best_restart", "item_loss", "item_iters", "item_status", "item_evals", "item_x"))):
        a = hip_ctx.q3_minimize(q3_cases.SQISWAP[None], [0] * 3, q3_cases.LINE_EDGES, t4, p, 1e-10)
        # (an unused three-qubit table changes nothing)
        b = hip_ctx.q3m_minimize(q3_cases.SQISWAP[None], CCZGate().to_matrix()[None], [2] * 3, [0] * 3,
                                 [e + (0,) for e in q3_cases.LINE_EDGES], t4, p, 1e-10)
        for key in keys:
            assert np.array_equal(a[key], b[key]), key


def test_local_convergence(hip_ctx):
    """8 targets of [VSwap, sqrt(iSWAP), VSwap] on (0, 1, 2), (0, 1), (2, 1, 0), start points 0.05 N(0, 1) from their angles: every item
    ends below 1e-10 and the model reproduces the returned loss."""
    case = q3m_cases.vswap_case()
    targets, x0 = q3m_cases.local_cases()
    prm = _ffi.OptParams(restarts=1, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=1, flags=0)
    out = hip_ctx.q3m_minimize(*case.description(), targets, prm, 1e-10, x0=x0[:, None, :])
    print("q3m local convergence: max loss", out["item_loss"].max(), "iterations", out["item_iters"].min(), "..", out["item_iters"].max())
    assert np.all(out["item_loss"] < 1e-10)
    for i in range(8):
        assert abs(q3m_ref.loss(out["best_x"][i], case.model_gates, case.edges, targets[i]) - out["best_loss"][i]) < 1e-12


def test_ccx_from_one_ccz():
    """CCX = (H on q2) CCZ (H on q2): one CCZ on (0, 1, 2) reaches the Toffoli that takes six CX (tests/test_gpu_q3.py)."""
    basis = ThreeQubitCircuitTemplate([CCZGate()], [[(0, 1, 2)]], maximum_span_guess=1)
    opt = TemplateOptimizer(basis, BasicCost(), training_restarts=16, seed=1, override_fail=True)
    ccx = CCXGate().to_matrix()
    d = opt.approximate_target_U(ccx)
    print("q3m ccx from ccz: loss", d.loss_result, "cycles", d.cycles, "evals", opt.last_stats["evals"])
    assert d.cycles == 1 and d.loss_result < 1e-8
    assert len(d.Xk) == 18
    basis.build(d.cycles)
    w = basis.eval(d.Xk)
    assert abs(q3_ref.basic_cost(w, ccx) - d.loss_result) < 1e-12
    assert q3_ref.equal_up_to_phase(w, ccx) < 1e-3  # (loss < 1e-8 bounds the entries by about sqrt(16 loss))


def test_mixed_arity_through_the_api():
    """8 reachable targets of [CCZ on (0, 1, 2), CX on (0, 1)], 32 restarts: the model reproduces every returned loss, and at least 7
    are solved below 1e-8 at cycles <= 2 (SciPy BFGS on the model solves all 8 within 32 starts: tests/test_q3m_host.py)."""
    case = q3m_cases.ccz_cx_case()
    targets = q3m_cases.ccz_cx_targets()
    basis = ThreeQubitCircuitTemplate([CCZGate(), CXGate()], [[(0, 1, 2)], [(0, 1)]], maximum_span_guess=2)
    assert basis.edge_sequence(2) == case.edges
    opt = TemplateOptimizer(basis, BasicCost(), training_restarts=32, seed=5, override_fail=True)
    losses, _, data = opt.approximate_from_distribution(list(targets))
    print("q3m mixed arity: losses", [float(f"{d.loss_result:.2e}") for d in data], "cycles", [d.cycles for d in data])
    assert len(data) == 8 and len(losses) == 8
    for i, d in enumerate(data):
        k = d.cycles
        assert k in (1, 2)
        assert abs(q3m_ref.loss(np.asarray(d.Xk), case.model_gates[:k], case.edges[:k], targets[i]) - d.loss_result) < 1e-12
    assert sum(d.loss_result < 1e-8 and d.cycles <= 2 for d in data) >= 7


def test_determinism(hip_ctx):
    """The same seed twice, ordered restarts with early exit: bit-equal results."""
    case = q3m_cases.ccz_cx_case()
    targets = q3m_cases.ccz_cx_targets()
    prm = _ffi.OptParams(restarts=8, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=9, flags=_ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED)
    a = hip_ctx.q3m_minimize(*case.description(), targets, prm, 1e-10)
    b = hip_ctx.q3m_minimize(*case.description(), targets, prm, 1e-10)
    for key in ("best_loss", "best_x", "best_restart"):
        assert np.array_equal(a[key], b[key]), key
    assert np.all(np.isfinite(a["best_loss"]))
