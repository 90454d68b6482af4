"""CPU: three-qubit templates (slam_decomposition_amd/basis3q.py) -- structure of the template, the NumPy model the GPU tests compare
against (tests/q3_ref.py), the optimizer's refusals, and the C ABI's argument checks that need no GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import q3_cases
import q3_ref
from slam_decomposition_amd import _ffi
from slam_decomposition_amd.basis import CircuitTemplate
from slam_decomposition_amd.basis3q import MAX_SPAN, ThreeQubitCircuitTemplate
from slam_decomposition_amd.cost_function import BasicCost, MakhlinFunctionalCost, SquareCost
from slam_decomposition_amd.gates import CXGate, RiSwapGate
from slam_decomposition_amd.optimizer import TemplateOptimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- structure ---------------------------------------------------------------------------------------------------------------
def test_structure_parameters_and_sequences():
    b = ThreeQubitCircuitTemplate([CXGate(), RiSwapGate(1 / 2)], [[(0, 1), (1, 2), (2, 0)], [(0, 2)]], maximum_span_guess=7)
    assert b.n_qubits == 3 and b.spanning_range == range(1, 8)
    assert b.preseeded is False and b.use_polytopes is False and b.using_bounds is False and b.using_constraints is False
    assert b.bounds_list is None and b.constraint_func is None
    b.spanning_range = range(2, 4)
    assert list(b.get_spanning_range(np.eye(8))) == [2, 3]
    for k in (1, 2, 7, 15):
        b.build(k)
        assert b.n_params == 9 + 6 * k and b.cycles == k
    b.build(7)
    assert b.gate_sequence() == [0, 1, 0, 1, 0, 1, 0]
    # gate i sits on edge_params[i % 2][(i // 2) % len(that list)]
    assert b.edge_sequence() == [(0, 1), (0, 2), (1, 2), (0, 2), (2, 0), (0, 2), (0, 1)]
    assert b.edge_sequence(3) == [(0, 1), (0, 2), (1, 2)]
    b.build(2)  # the cycles restart at every build
    assert b.edge_sequence() == [(0, 1), (0, 2)] and b.gate_sequence() == [0, 1]
    assert b.target_invariant(np.eye(8)) == (-1, -1, -1, -1)


def test_to_gate_list_and_order_helpers():
    cx = CXGate()
    b = ThreeQubitCircuitTemplate([cx], [[(1, 2), (0, 2)]])
    b.build(2)
    x = np.arange(21, dtype=np.float64)
    gl = b.to_gate_list(x)
    assert gl[:3] == [("u", 0, (0.0, 1.0, 2.0)), ("u", 1, (3.0, 4.0, 5.0)), ("u", 2, (6.0, 7.0, 8.0))]
    assert gl[3] == ("gate", cx, (1, 2)) and gl[4] == ("u", 1, (9.0, 10.0, 11.0)) and gl[5] == ("u", 2, (12.0, 13.0, 14.0))
    assert gl[6] == ("gate", cx, (0, 2)) and gl[7] == ("u", 0, (15.0, 16.0, 17.0)) and gl[8] == ("u", 2, (18.0, 19.0, 20.0))
    assert len(gl) == 9
    with pytest.raises(ValueError):
        b.to_gate_list(x[:-1])
    q = b.to_qiskit_order(x)
    assert list(q[:4]) == [0.0, 1.0, 10.0, 11.0]  # P0, P1, P10, P11, ...
    assert np.array_equal(b.from_qiskit_order(q), x)
    assert np.array_equal(q, CircuitTemplate.to_qiskit_order(x))
    assert len(b.parameter_guess()) == 21


def test_constructor_errors_and_span_limit():
    for bad in ([[(0, 0)]], [[(0, 3)]], [[(0, 1, 2)]], [[]], []):
        with pytest.raises(ValueError):
            ThreeQubitCircuitTemplate([CXGate()], bad)
    with pytest.raises(ValueError):
        ThreeQubitCircuitTemplate([], [[(0, 1)]])
    b = ThreeQubitCircuitTemplate([CXGate()], [[(0, 1)]])
    b.build(MAX_SPAN)
    assert MAX_SPAN == 15 and b.n_params == 99
    with pytest.raises(ValueError, match="15"):
        b.build(16)
    with pytest.raises(ValueError):
        b.build(0)
    with pytest.raises(ValueError):
        b.eval(np.zeros(3))  # (wrong length: refused before the device is needed)


def test_two_qubit_template_still_refuses_three_qubits():
    with pytest.raises(NotImplementedError):
        CircuitTemplate(n_qubits=3)
    with pytest.raises(NotImplementedError):
        CircuitTemplate(n_qubits=2, edge_params=[[(1, 2)]])


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_model_cx_on_an_edge_is_the_explicit_permutation():
    for (a, b) in [(0, 2), (2, 0), (0, 1), (1, 0), (1, 2), (2, 1)]:
        w = q3_ref.unitary(np.zeros(15), [q3_cases.CX], [(a, b)])
        want = np.zeros((8, 8))
        for s in range(8):
            want[s ^ ((1 << b) if (s >> a) & 1 else 0), s] = 1.0  # control a, target b
        assert np.array_equal(w, want), (a, b)
    w02 = q3_ref.unitary(np.zeros(15), [q3_cases.CX], [(0, 2)])
    w20 = q3_ref.unitary(np.zeros(15), [q3_cases.CX], [(2, 0)])
    rev = [0, 4, 2, 6, 1, 5, 3, 7]  # q0 <-> q2
    assert np.array_equal(w20, w02[np.ix_(rev, rev)]) and not np.array_equal(w02, w20)


@pytest.mark.parametrize("k", [1, 4, 15])
@pytest.mark.parametrize("square", [False, True])
def test_model_gradient_against_central_differences(k, square):
    rng = np.random.default_rng(500 + k)
    gates = [[q3_cases.CX, q3_cases.SQISWAP, q3_cases.haar(rng, 4)][j % 3] for j in range(k)]
    edges = [q3_cases.ALL_EDGES[(j + k) % 6] for j in range(k)]
    t = q3_cases.haar(rng, 8)
    x = rng.uniform(0.0, 2.0 * np.pi, 9 + 6 * k)
    f, g, w = q3_ref.loss_grad(x, gates, edges, t, square)
    assert f == pytest.approx(q3_ref.loss(x, gates, edges, t, square), abs=1e-15)
    assert np.max(np.abs(w.conj().T @ w - np.eye(8))) < 1e-13
    h = 1e-6
    fd = np.array([(q3_ref.loss(x + h * e, gates, edges, t, square) - q3_ref.loss(x - h * e, gates, edges, t, square)) / (2 * h)
                   for e in np.eye(len(x))])
    assert np.max(np.abs(fd - g)) < 2e-9


def test_golden_angles_give_the_toffoli():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "q3_ccx_solution.json")))
    x = np.array(d["x"])
    assert len(x) == 45 and [tuple(e) for e in d["edges"]] == q3_cases.TOFFOLI_EDGES
    w = q3_ref.unitary(x, [q3_cases.CX] * 6, q3_cases.TOFFOLI_EDGES)
    assert q3_ref.basic_cost(w, q3_ref.CCX) < 1e-14
    assert q3_ref.equal_up_to_phase(w, q3_ref.CCX) < 1e-12
    ccx = np.eye(8)
    ccx[[3, 7]] = ccx[[7, 3]]
    assert np.array_equal(q3_ref.CCX, ccx)


# ---- optimizer ---------------------------------------------------------------------------------------------------------------
def _basis():
    return ThreeQubitCircuitTemplate([CXGate()], [q3_cases.TOFFOLI_EDGES], maximum_span_guess=6)


def test_optimizer_refusals_name_the_option():
    with pytest.raises(NotImplementedError, match="Weyl chamber only for 2Q gates"):
        TemplateOptimizer(_basis(), MakhlinFunctionalCost())
    with pytest.raises(NotImplementedError, match="use_callback"):
        TemplateOptimizer(_basis(), BasicCost(), use_callback=True)
    with pytest.raises(NotImplementedError, match="override_method"):
        TemplateOptimizer(_basis(), BasicCost(), override_method="Nelder-Mead")
    with pytest.raises(NotImplementedError, match="devices"):
        TemplateOptimizer(_basis(), BasicCost(), devices=[0, 1])
    with pytest.raises(NotImplementedError, match="deterministic"):
        TemplateOptimizer(_basis(), SquareCost(), deterministic=False)
    opt = TemplateOptimizer(_basis(), SquareCost(), override_method="BFGS", training_restarts=3, seed=1)
    assert opt._cost_kind == _ffi.COST_SQUARE and opt.training_restarts == 3


def test_optimizer_wants_eight_by_eight_targets():
    opt = TemplateOptimizer(_basis(), BasicCost(), seed=1)
    with pytest.raises(ValueError, match="8x8"):
        opt.approximate_target_U(np.eye(4))
    with pytest.raises(ValueError, match="8x8"):
        opt.approximate_from_distribution([np.eye(8), np.eye(4)])
    two = TemplateOptimizer(CircuitTemplate(maximum_span_guess=2), BasicCost(), seed=1)
    with pytest.raises(ValueError):
        two.approximate_target_U(np.eye(8))


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
needs_lib = pytest.mark.skipif(not os.path.exists(_ffi.LIB_PATH) and not os.path.exists("/opt/rocm/bin/hipcc"),
                               reason="no ROCm toolchain on this machine")


@needs_lib
def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "slam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _ffi.load_library()
    for name in ("slam_q3_eval", "slam_q3_minimize"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in _ffi.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert "#define SLAM_Q3_MAX_SPAN 15" in hdr
    assert lib.slam_abi_version() == 7


@needs_lib
def test_validation_errors_need_no_gpu():
    lib = _ffi.load_library()
    INVALID, UNSUPPORTED = -1, -3
    gates = np.zeros((1, 4, 4, 2))
    gi = np.zeros(2, np.int32)
    ed = np.array([[0, 1], [1, 2]], np.int32)
    t = np.zeros((1, 8, 8, 2))
    x = np.zeros((1, 21))
    tof = np.zeros(1, np.int32)
    loss = np.zeros(1)
    p = _ffi._ptr

    def ev(k=2, gates_=gates, gi_=gi, ed_=ed, t_=t, nt=1, x_=x, tof_=tof, M=1, cost=0, loss_=loss):
        rc = lib.slam_q3_eval(None, p(gates_), 1, k, p(gi_), p(ed_), p(t_), nt, p(x_), p(tof_), M, cost, p(loss_), None, None)
        return rc, lib.slam_last_error().decode()

    assert ev() == (INVALID, "ctx is NULL")  # everything else is in order: the context is looked at last
    rc, msg = ev(k=16)
    assert rc == UNSUPPORTED and "1..15" in msg
    assert ev(k=0)[0] == UNSUPPORTED
    rc, msg = ev(ed_=np.array([[0, 1], [1, 1]], np.int32))
    assert rc == INVALID and "edges[1]" in msg
    rc, msg = ev(ed_=np.array([[3, 1], [1, 2]], np.int32))
    assert rc == INVALID and "edges[0]" in msg
    rc, msg = ev(gi_=np.array([0, 1], np.int32))
    assert rc == INVALID and "gate_index[1]" in msg
    rc, msg = ev(cost=_ffi.COST_MAKHLIN)
    assert rc == UNSUPPORTED and "Weyl chamber only for 2Q gates" in msg
    rc, msg = ev(cost=9)
    assert rc == INVALID and "cost kind" in msg
    for kw in ({"gates_": None}, {"gi_": None}, {"ed_": None}, {"t_": None}, {"x_": None}, {"tof_": None}, {"loss_": None}, {"M": 0},
               {"nt": 0}, {"tof_": np.ones(1, np.int32)}):
        assert ev(**kw)[0] == INVALID, kw
    prm = _ffi.OptParams(restarts=2)

    def mn(k=2, ed_=ed, cost=0, prm_=prm, t_=t, nt=1, x0_=None):
        rc = lib.slam_q3_minimize(None, p(gates), 1, k, p(gi), p(ed_), p(t_), nt, cost, C.byref(prm_) if prm_ is not None else None, 1e-10,
                                  p(x0_), *([None] * 9))
        return rc, lib.slam_last_error().decode()

    assert mn() == (INVALID, "ctx is NULL")
    assert mn(k=16)[0] == UNSUPPORTED
    assert mn(ed_=np.array([[0, 0], [1, 2]], np.int32))[0] == INVALID
    assert mn(cost=_ffi.COST_MAKHLIN)[0] == UNSUPPORTED
    rc, msg = mn(prm_=None)
    assert rc == INVALID and "params is NULL" in msg
    assert mn(prm_=_ffi.OptParams(restarts=0))[0] == INVALID
    assert mn(t_=None)[0] == INVALID and mn(nt=0)[0] == INVALID
    # explicit start points [1, 2, 21]: finite with |x| < 1e8 (the optimizer's sincos table path), checked before the context
    for at in (0, 41):
        for bad in (np.nan, np.inf, -np.inf, 1e12, -1e12, 1e8):
            x0 = np.zeros((1, 2, 21))
            x0.flat[at] = bad
            rc, msg = mn(x0_=x0)
            assert rc == INVALID and f"x0[{at}]" in msg and "explicit seeds must be finite with |x| < 1e8" in msg, (at, bad, msg)
        x0 = np.zeros((1, 2, 21))
        x0.flat[at] = 9.9e7 if at else -9.9e7
        assert mn(x0_=x0) == (INVALID, "ctx is NULL")
