"""CPU: three-qubit basis gates (slam_decomposition_amd/gates.py: Gate3Q and its subclasses), mixed three-qubit templates
(basis3q.py), the NumPy model the GPU tests compare against (tests/q3m_ref.py), and the argument checks of slam_q3m_eval /
slam_q3m_minimize that need no GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import scipy.linalg
import scipy.optimize

import q3_cases
import q3_ref
import q3m_cases
import q3m_ref
from slam_decomposition_amd import _ffi, gates as G
from slam_decomposition_amd.basis import CircuitTemplate
from slam_decomposition_amd.basis3q import MAX_GATES3, ThreeQubitCircuitTemplate
from slam_decomposition_amd.cost_function import BasicCost, MakhlinFunctionalCost, SquareCost
from slam_decomposition_amd.optimizer import TemplateOptimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- gates -------------------------------------------------------------------------------------------------------------------
def _from_definition(perm=None, diag=None, blocks=()):
    """U|j> = |perm(j)> (a dict of the moved states), then diagonal entries, then 2x2 blocks i X on pairs."""
    m = np.zeros((8, 8), dtype=np.complex128)
    for j in range(8):
        m[(perm or {}).get(j, j), j] = 1.0
    for j, v in (diag or {}).items():
        m[j, j] = v
    for i, j in blocks:
        m[i, i] = m[j, j] = 0.0
        m[i, j] = m[j, i] = 1j
    return m


DEFINITIONS = {
    "CCZGate": _from_definition(diag={7: -1}),
    "CCXGate": _from_definition(perm={3: 7, 7: 3}),
    "CSwapGate": _from_definition(perm={3: 5, 5: 3}),
    "CCiXGate": _from_definition(blocks=[(6, 7)]),
    "CiSwap": _from_definition(blocks=[(5, 6)]),
    "Peres": _from_definition(perm={4: 7, 7: 4, 5: 6, 6: 5}),
    "Margolus": _from_definition(perm={6: 7, 7: 6}, diag={5: -1}),
    "CParitySwap": _from_definition(perm={1: 2, 2: 4, 4: 1, 3: 5, 5: 6, 6: 3}),
}


@pytest.mark.parametrize("name", sorted(DEFINITIONS))
def test_fixed_gate_matches_its_definition(name):
    g = getattr(G, name)()
    m = g.to_matrix()
    assert isinstance(g, G.Gate3Q) and g.num_qubits == 3 and m.shape == (8, 8) and m.dtype == np.complex128
    assert np.array_equal(m, DEFINITIONS[name])
    assert np.array_equal(m.conj().T @ m, np.eye(8))
    assert np.array_equal(G.gate_matrix(g), m) and np.array_equal(G.gate_matrix(m), m)


def test_fixed_gates_by_their_action():
    assert np.array_equal(G.CCXGate().to_matrix(), q3_ref.CCX)
    h2 = q3_ref.embed_1q(np.array([[1, 1], [1, -1]]) / math.sqrt(2.0), 2)
    assert np.max(np.abs(h2 @ G.CCZGate().to_matrix() @ h2 - q3_ref.CCX)) < 1e-15  # CCX = (H on q2) CCZ (H on q2)
    for s in range(8):  # bit by bit
        q0, q1, q2 = s & 1, (s >> 1) & 1, s >> 2
        e = np.zeros(8)
        e[s] = 1.0
        assert (G.CSwapGate().to_matrix() @ e)[(q0 | (q2 << 1) | (q1 << 2)) if q0 else s] == 1.0
        assert (G.Peres().to_matrix() @ e)[s ^ 3 if q2 else s] == 1.0
    sw01 = np.kron(np.eye(2), G.iSwapGate().to_matrix())  # iSWAP on (q0, q1)
    ci = G.CiSwap().to_matrix()
    assert np.max(np.abs(ci[4:, 4:] - sw01[4:, 4:])) < 1e-15 and np.array_equal(ci[:4, :4], np.eye(4))
    with pytest.raises(ValueError):
        G.gate_matrix(np.eye(3))
    with pytest.raises(ValueError):
        CircuitTemplate(base_gates=[G.CCZGate()])  # the two-qubit template keeps to 4x4 gates


def _circulator_reference(p_ab, p_ac, p_bc, g_ab, g_ac, g_bc, t):
    up = np.array([[0, 0], [1, 0]], dtype=np.complex128)  # qutip.create(2)
    one = np.eye(2)
    a, b, c = np.kron(np.kron(up, one), one), np.kron(np.kron(one, up), one), np.kron(np.kron(one, one), up)
    h = np.zeros((8, 8), dtype=np.complex128)
    for p, g, x, y in ((p_ab, g_ab, a, b), (p_ac, g_ac, a, c), (p_bc, g_bc, b, c)):
        h += g * (np.exp(1j * p) * x @ y.conj().T + np.exp(-1j * p) * y @ x.conj().T)
    return scipy.linalg.expm(-1j * t * h), h


def test_circulator_gate_against_expm():
    rng = np.random.default_rng(3700)
    sets = [tuple(rng.uniform(-math.pi, math.pi, 3)) + tuple(rng.uniform(-2.0, 2.0, 3)) + (float(rng.uniform(0.2, 1.5)),) for _ in range(3)]
    v, d = 4.0 / math.sqrt(2.0), 3.0 * math.sqrt(3.0) / 2.0
    named = [(G.VSwap(), (math.pi / 2, math.pi / 2, 0.0, math.pi / v, math.pi / v, 0.0, 1.0)),
             (G.VSwap(t_el=0.5), (math.pi / 2, math.pi / 2, 0.0, math.pi / v, math.pi / v, 0.0, 0.5)),
             (G.DeltaSwap(), (math.pi / 2, -math.pi / 2, math.pi / 2, math.pi / d, math.pi / d, math.pi / d, 1.0))]
    number = np.diag([bin(s).count("1") for s in range(8)]).astype(np.complex128)
    for gate, args in [(G.CirculatorSNAILGate(*s), s) for s in sets] + named:
        m = gate.to_matrix()
        want, h = _circulator_reference(*args)
        assert isinstance(gate, G.Gate3Q) and m.shape == (8, 8)
        assert np.max(np.abs(m - want)) < 1e-13, args
        assert np.max(np.abs(G.circulator_hamiltonian(*args[:6]) - h)) < 1e-15
        assert np.max(np.abs(m.conj().T @ m - np.eye(8))) < 1e-13
        assert np.max(np.abs(m @ number - number @ m)) < 1e-13  # excitation number is conserved
        cost = sum(abs(g) for g in args[3:6]) * args[6] / (math.pi / 2)
        assert gate.cost() == pytest.approx(cost, rel=1e-15) and gate.fidelity() == pytest.approx(max(1 - 0.001 * cost, 0.0), rel=1e-15)
    assert G.VSwap().cost() == pytest.approx(math.sqrt(2.0)) and G.DeltaSwap().cost() == pytest.approx(4.0 / math.sqrt(3.0))
    assert G.CirculatorSNAILGate(0, 0, 0, 1000.0, 1000.0, 1000.0).fidelity() == 0.0
    # VSwap moves an excitation of mode a (bit 2) to an equal superposition of b and c and back: at t = 1 it exchanges a with (b + c)
    assert abs(G.VSwap().to_matrix()[4, 4]) < 1e-12


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_embed_3q_agrees_with_embed_2q_and_the_bits():
    rng = np.random.default_rng(3701)
    g4 = q3_cases.haar(rng, 4)
    for a, b, c in q3m_cases.TRIPLES:
        assert np.max(np.abs(q3m_ref.embed_3q(np.kron(np.eye(2), g4), a, b, c) - q3_ref.embed_2q(g4, a, b))) < 1e-15
    # a permutation gate: |bit_a, bit_b, bit_c> -> by the gate's own table
    peres = G.Peres().to_matrix()
    for a, b, c in q3m_cases.TRIPLES:
        m = q3m_ref.embed_3q(peres, a, b, c)
        for s in range(8):
            want = s ^ ((1 << a) | (1 << b)) if (s >> c) & 1 else s
            assert m[want, s] == 1.0
    assert np.array_equal(q3m_ref.embed_3q(q3_ref.CCX, 0, 1, 2), q3_ref.CCX)


def test_model_reduces_to_the_two_qubit_model():
    gates, gate_index, edges, targets, x = q3_cases.parity_case(5)
    gl = [gates[i] for i in gate_index]
    f0, g0, w0 = q3_ref.loss_grad(x[0], gl, edges, targets[0], True)
    f1, g1, w1 = q3m_ref.loss_grad(x[0], gl, edges, targets[0], True)
    assert f0 == f1 and np.array_equal(g0, g1) and np.array_equal(w0, w1)


@pytest.mark.parametrize("square", [False, True])
def test_model_gradient_against_central_differences(square):
    """On the mixed template of the parity test (arities [3, 2, 3, 2, 2]): 1e-7 relative to the largest component."""
    case = q3m_cases.parity_template("mixed5")
    targets, xs = q3m_cases.parity_items("mixed5")
    x, t = xs[0], targets[0]
    f, g, w = q3m_ref.loss_grad(x, case.model_gates, case.edges, t, square)
    assert len(x) == 45 and f == pytest.approx(q3m_ref.loss(x, case.model_gates, case.edges, t, square), abs=1e-15)
    assert np.max(np.abs(w.conj().T @ w - np.eye(8))) < 1e-13
    h = 1e-6
    fd = np.array([(q3m_ref.loss(x + h * e, case.model_gates, case.edges, t, square) - q3m_ref.loss(x - h * e, case.model_gates, case.edges, t, square))
                   / (2 * h) for e in np.eye(len(x))])
    assert np.max(np.abs(fd - g)) < 1e-7 * np.max(np.abs(g))


def test_parity_items_stay_away_from_the_singular_point():
    for name in q3m_cases.PARITY_NAMES:
        case = q3m_cases.parity_template(name)
        targets, x = q3m_cases.parity_items(name)
        assert x.shape == (8, case.n)
        assert all(q3m_ref.overlap(q3m_ref.unitary(x[m], case.model_gates, case.edges), targets[m]) >= 0.05 for m in range(8)), name
    assert q3m_cases.parity_template("ten3").n == 99 and q3m_cases.parity_template("wide14").n == 99


def test_scipy_solves_the_chosen_targets():
    """What tests/test_gpu_q3m.py asks of the device: CCX from one CCZ, and the 8 targets of [CCZ, CX] within 32 starts each."""
    def solved_within(gates, edges, t, rng, starts):
        n = q3m_ref.n_params(edges)
        for s in range(starts):
            r = scipy.optimize.minimize(lambda v: q3m_ref.loss_grad(v, gates, edges, t)[:2], rng.uniform(0.0, 2.0 * math.pi, n), jac=True,
                                        method="BFGS", options={"gtol": 1e-9, "maxiter": 2500})
            if r.fun < 1e-8:
                return True
        return False

    rng = np.random.default_rng(3702)
    assert solved_within([G.CCZGate().to_matrix()], [(0, 1, 2)], q3_ref.CCX, rng, 16)
    case = q3m_cases.ccz_cx_case()
    for t in q3m_cases.ccz_cx_targets():
        assert solved_within(case.model_gates, case.edges, t, rng, 32)


# ---- the template ------------------------------------------------------------------------------------------------------------
def test_mixed_template_structure():
    ccz, cx, vs = G.CCZGate(), G.CXGate(), G.VSwap()
    b = ThreeQubitCircuitTemplate([ccz, cx], [[(0, 1, 2), (2, 1, 0)], [(0, 1), (1, 2)]], maximum_span_guess=4)
    assert b.arities == [3, 2] and b.gate_matrices.shape == (1, 4, 4) and b.gate_matrices3.shape == (1, 8, 8)
    b.build(4)
    assert b.gate_sequence() == [0, 1, 0, 1]
    assert b.edge_sequence() == [(0, 1, 2), (0, 1), (2, 1, 0), (1, 2)]
    assert b.n_params == 9 + 3 * (3 + 2 + 3 + 2) and b.has_three_qubit_position()
    assert b.mixed_description() == ([3, 2, 3, 2], [0, 0, 0, 0], [(0, 1, 2), (0, 1, 0), (2, 1, 0), (1, 2, 0)])
    b.build(1)
    assert b.n_params == 18 and b.edge_sequence() == [(0, 1, 2)]
    x = np.arange(18, dtype=np.float64)
    gl = b.to_gate_list(x)
    assert gl[3] == ("gate", ccz, (0, 1, 2))
    assert gl[4:] == [("u", 0, (9.0, 10.0, 11.0)), ("u", 1, (12.0, 13.0, 14.0)), ("u", 2, (15.0, 16.0, 17.0))]
    with pytest.raises(ValueError):
        b.to_gate_list(x[:-1])
    with pytest.raises(ValueError):
        b.eval(np.zeros(15))  # (wrong length: refused before the device is needed)
    assert len(b.parameter_guess()) == 18
    # a raw 8x8 array is a three-qubit gate too; second base gate of arity 3 gets the second table entry
    b2 = ThreeQubitCircuitTemplate([vs, cx, ccz.to_matrix()], [[(0, 1, 2)], [(0, 1)], [(1, 2, 0)]])
    b2.build(3)
    assert b2.mixed_description() == ([3, 2, 3], [0, 0, 1], [(0, 1, 2), (0, 1, 0), (1, 2, 0)]) and b2.table_sequence() == [0, 0, 1]
    # a template of two-qubit gates only is as before
    b3 = ThreeQubitCircuitTemplate([cx], [[(0, 1)], [(1, 2)]])
    b3.build(3)
    assert not b3.has_three_qubit_position() and b3.n_params == 27 and b3.table_sequence() == b3.gate_sequence()


def test_mixed_template_refusals():
    ccz, cx = G.CCZGate(), G.CXGate()
    # arity and edge length differ at position 1
    b = ThreeQubitCircuitTemplate([ccz, cx], [[(0, 1, 2)], [(0, 1, 2)]])
    b.build(1)
    with pytest.raises(ValueError, match="position 1"):
        b.build(2)
    assert b.cycles == 0
    b = ThreeQubitCircuitTemplate([ccz, cx], [[(0, 1)], [(0, 1)]])
    with pytest.raises(ValueError, match="position 0"):
        b.build(1)
    # n > 99: eleven three-qubit gates
    b = ThreeQubitCircuitTemplate([ccz], [[(0, 1, 2)]], maximum_span_guess=11)
    b.build(10)
    assert b.n_params == 99
    with pytest.raises(ValueError, match="99"):
        b.build(11)
    # k > 15 whatever the arities
    b = ThreeQubitCircuitTemplate([cx, cx, cx, cx, cx, cx, cx, ccz], [[(0, 1)]] * 7 + [[(0, 1, 2)]])
    b.build(8)
    assert b.n_params == 9 + 42 + 9
    with pytest.raises(ValueError, match="15"):
        b.build(16)
    # repeated or foreign qubits
    for bad in ([[(0, 0, 1)]], [[(0, 1, 3)]], [[(0, 1, 2, 0)]], [[(1, 1)]]):
        with pytest.raises(ValueError):
            ThreeQubitCircuitTemplate([ccz], bad)
    with pytest.raises(ValueError):
        ThreeQubitCircuitTemplate([cx], [[(0, 1, 2)]])  # no three-qubit gate: triples stay refused
    with pytest.raises(ValueError, match=str(MAX_GATES3)):
        ThreeQubitCircuitTemplate([ccz] * (MAX_GATES3 + 1), [[(0, 1, 2)]])


def test_optimizer_refusals_stay():
    def basis():
        return ThreeQubitCircuitTemplate([G.CCZGate()], [[(0, 1, 2)]], maximum_span_guess=1)

    with pytest.raises(NotImplementedError, match="Weyl chamber only for 2Q gates"):
        TemplateOptimizer(basis(), MakhlinFunctionalCost())
    with pytest.raises(NotImplementedError, match="use_callback"):
        TemplateOptimizer(basis(), BasicCost(), use_callback=True)
    with pytest.raises(NotImplementedError, match="devices"):
        TemplateOptimizer(basis(), BasicCost(), devices=[0, 1])
    with pytest.raises(NotImplementedError, match="deterministic"):
        TemplateOptimizer(basis(), SquareCost(), deterministic=False)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
needs_lib = pytest.mark.skipif(not os.path.exists(_ffi.LIB_PATH) and not os.path.exists("/opt/rocm/bin/hipcc"),
                               reason="no ROCm toolchain on this machine")


@needs_lib
def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "slam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _ffi.load_library()
    for name in ("slam_q3m_eval", "slam_q3m_minimize"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in _ffi.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert f"#define SLAM_Q3_MAX_GATES3 {MAX_GATES3}" in hdr and MAX_GATES3 >= 2
    assert lib.slam_abi_version() == 7


@needs_lib
def test_validation_errors_need_no_gpu():
    lib = _ffi.load_library()
    INVALID, UNSUPPORTED = -1, -3
    g2, g3 = np.zeros((1, 4, 4, 2)), np.zeros((2, 8, 8, 2))
    ar = np.array([3, 2], np.int32)
    gi = np.array([1, 0], np.int32)
    qb = np.array([[0, 1, 2], [1, 2, 9]], np.int32)  # (the third qubit of an arity-2 position is not looked at)
    t = np.zeros((1, 8, 8, 2))
    x = np.zeros((1, 24))
    tof = np.zeros(1, np.int32)
    loss = np.zeros(1)
    p = _ffi._ptr

    def ev(k=2, g2_=g2, n2=1, g3_=g3, n3=2, ar_=ar, gi_=gi, qb_=qb, t_=t, nt=1, x_=x, tof_=tof, M=1, cost=0, loss_=loss):
        rc = lib.slam_q3m_eval(None, p(g2_), n2, p(g3_), n3, k, p(ar_), p(gi_), p(qb_), p(t_), nt, p(x_), p(tof_), M, cost, p(loss_), None, None)
        return rc, lib.slam_last_error().decode()

    assert ev() == (INVALID, "ctx is NULL")  # everything else is in order: the context is looked at last
    rc, msg = ev(k=16)
    assert rc == UNSUPPORTED and "1..15" in msg
    assert ev(k=0)[0] == UNSUPPORTED
    rc, msg = ev(ar_=np.array([3, 4], np.int32))
    assert rc == INVALID and "arity[1]" in msg
    rc, msg = ev(qb_=np.array([[0, 1, 1], [1, 2, 0]], np.int32))
    assert rc == INVALID and "qubits[0]" in msg
    rc, msg = ev(qb_=np.array([[0, 1, 2], [1, 1, 0]], np.int32))
    assert rc == INVALID and "qubits[1]" in msg
    rc, msg = ev(qb_=np.array([[0, 1, 3], [1, 2, 0]], np.int32))
    assert rc == INVALID and "qubits[0]" in msg
    rc, msg = ev(gi_=np.array([2, 0], np.int32))
    assert rc == INVALID and "gate_index[0]" in msg
    rc, msg = ev(gi_=np.array([1, 1], np.int32))
    assert rc == INVALID and "gate_index[1]" in msg
    rc, msg = ev(n3=0)  # a three-qubit position with an empty table
    assert rc == INVALID and "gate_index[0]" in msg
    rc, msg = ev(n3=MAX_GATES3 + 1, g3_=np.zeros((MAX_GATES3 + 1, 8, 8, 2)))
    assert rc == UNSUPPORTED and "distinct three-qubit gates" in msg
    # n <= 99: eleven three-qubit positions have 108 parameters
    k11 = dict(k=11, ar_=np.full(11, 3, np.int32), gi_=np.zeros(11, np.int32), qb_=np.tile(np.array([0, 1, 2], np.int32), (11, 1)))
    rc, msg = ev(**k11)
    assert rc == UNSUPPORTED and "99" in msg and "108" in msg
    rc, msg = ev(cost=_ffi.COST_MAKHLIN)
    assert rc == UNSUPPORTED and "Weyl chamber only for 2Q gates" in msg
    assert ev(cost=9)[0] == INVALID
    bad = g3.copy()
    bad[1, 7, 7, 1] = np.nan
    rc, msg = ev(g3_=bad)
    assert rc == INVALID and "gates3" in msg
    for kw in ({"g2_": None}, {"g3_": None}, {"ar_": None}, {"gi_": None}, {"qb_": None}, {"t_": None}, {"x_": None}, {"tof_": None},
               {"loss_": None}, {"M": 0}, {"nt": 0}, {"tof_": np.ones(1, np.int32)}, {"n2": -1}, {"n3": -1}):
        assert ev(**kw)[0] == INVALID, kw
    # no two-qubit table at all is fine when no position asks for one
    only3 = dict(k=1, g2_=None, n2=0, ar_=np.array([3], np.int32), gi_=np.array([0], np.int32), qb_=np.array([[2, 0, 1]], np.int32))
    assert ev(**only3) == (INVALID, "ctx is NULL")
    prm = _ffi.OptParams(restarts=2)

    def mn(k=2, ar_=ar, qb_=qb, cost=0, prm_=prm, t_=t, nt=1, n3=2, x0_=None):
        rc = lib.slam_q3m_minimize(None, p(g2), 1, p(g3), n3, k, p(ar_), p(gi), p(qb_), p(t_), nt, cost,
                                   C.byref(prm_) if prm_ is not None else None, 1e-10, p(x0_), *([None] * 9))
        return rc, lib.slam_last_error().decode()

    assert mn() == (INVALID, "ctx is NULL")
    assert mn(k=16)[0] == UNSUPPORTED
    assert mn(ar_=np.array([1, 2], np.int32))[0] == INVALID
    assert mn(qb_=np.array([[0, 0, 2], [1, 2, 0]], np.int32))[0] == INVALID
    assert mn(n3=MAX_GATES3 + 1)[0] == UNSUPPORTED
    assert mn(cost=_ffi.COST_MAKHLIN)[0] == UNSUPPORTED
    rc, msg = mn(prm_=None)
    assert rc == INVALID and "params is NULL" in msg
    assert mn(prm_=_ffi.OptParams(restarts=0))[0] == INVALID
    assert mn(t_=None)[0] == INVALID and mn(nt=0)[0] == INVALID
    # explicit start points [1, 2, 24]: finite with |x| < 1e8 (the optimizer's sincos table path), checked before the context
    for at in (0, 47):
        for bad in (np.nan, np.inf, -np.inf, 1e12, -1e12, 1e8):
            x0 = np.zeros((1, 2, 24))
            x0.flat[at] = bad
            rc, msg = mn(x0_=x0)
            assert rc == INVALID and f"x0[{at}]" in msg and "explicit seeds must be finite with |x| < 1e8" in msg, (at, bad, msg)
        x0 = np.zeros((1, 2, 24))
        x0.flat[at] = 9.9e7 if at else -9.9e7
        assert mn(x0_=x0) == (INVALID, "ctx is NULL")
