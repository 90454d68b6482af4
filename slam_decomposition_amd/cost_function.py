"""Cost functions (reference: src/slam/cost_function.py:117-145).

``BasicCost``, ``SquareCost`` (the monotone map 0.8 (2 L - L^2) of BasicCost L, cost_function.py:169-173) and
``MakhlinFunctionalCost`` (cost_function.py:219-221) are the objectives the HIP optimizer implements (``slam_set_cost``); anything
else makes ``TemplateOptimizer`` raise the reference's "Unrecognized Cost Function".  ``EntanglementCostFunction`` (cost_function.py:44-99) is the
reference's second family: a W or a GHZ state goes through a three-qubit template and the objective is the entanglement left in it;
``MutualInformation`` and ``MutualInformationSquare`` run on the GPU (``slam_q3s_minimize``), the reference's empty stubs are refused.  The classes keep the reference's interface; ``unitary_fidelity`` on two single matrices is the reference's own
one-line NumPy expression (used for spot checks and logging, never inside the optimizer loop --
there the loss is fused into the HIP kernel).
"""
from __future__ import annotations

from abc import ABC

import numpy as np


class UnitaryCostFunction(ABC):
    def __init__(self):
        self.normalization = 1  # src/slam/cost_function.py:123

    def unitary_fidelity(self, current_u, target_u):
        raise NotImplementedError


class BasicCost(UnitaryCostFunction):
    """1 - |Tr(T^dagger U)| / d  (src/slam/cost_function.py:140-145)."""

    def unitary_fidelity(self, current_u, target_u):
        h = np.asarray(target_u).conj().T
        cur = np.asarray(current_u)
        return 1 - np.abs(np.trace(h @ cur)) / cur.shape[0]


class SquareCost(UnitaryCostFunction):
    """1 - (|Tr(T^dagger U)|^2 + d) / (d (d + 1))  (src/slam/cost_function.py:169-173): the objective most
    of the reference's notebooks use.  On the HIP path it is the same fused kernel with a different
    scalar map of |Tr| (and of the gradient scale)."""

    def unitary_fidelity(self, current_u, target_u):
        h = np.asarray(target_u).conj().T
        d = np.asarray(target_u).shape[0]
        return 1 - (np.abs(np.trace(h @ np.asarray(current_u))) ** 2 + d) / (d * (d + 1))


class MakhlinFunctionalCost(UnitaryCostFunction):
    """J = sum_i (g_i(U) - g_i(T))^2 over the Makhlin local invariants g = (Re G1, Im G1, Re G2) (src/slam/cost_function.py:219-221,
    weylchamber's ``J_T_LI``): the distance between the local-equivalence classes of U and T, zero whenever U = K1 T K2 with
    single-qubit K1, K2.  The reference's invariants come rounded to 8 digits, which leaves the functional piecewise constant
    below 1e-8; here -- on the host and in the HIP kernels -- it is the UNROUNDED functional."""

    def unitary_fidelity(self, current_u, target_u):
        from .weyl import g1g2g3

        d = np.asarray(g1g2g3(current_u)) - np.asarray(g1g2g3(target_u))
        return float(d @ d)


# ---- state objectives (src/slam/cost_function.py:44-99) ------------------------------------------------------------------------------
def _on_qubits(ops) -> np.ndarray:
    """kron(m2, m1, m0) with m_q = ops[q] (the identity elsewhere): basis index q0 + 2 q1 + 4 q2."""
    m = [np.asarray(ops.get(q, np.eye(2)), dtype=np.complex128) for q in range(3)]
    return np.kron(m[2], np.kron(m[1], m[0]))


def _controlled(u, control, target) -> np.ndarray:
    return _on_qubits({control: np.diag([1.0, 0.0])}) + _on_qubits({control: np.diag([0.0, 1.0]), target: u})


def _prepared_state(name: str) -> np.ndarray:
    """The reference's state preparation circuits (cost_function.py:47-59) applied to |000>."""
    x = np.array([[0.0, 1.0], [1.0, 0.0]])
    h = np.array([[1.0, 1.0], [1.0, -1.0]]) / np.sqrt(2.0)
    if name == "w":
        t = np.arccos(1.0 / np.sqrt(3.0))  # ry(2 t)
        ry = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
        circuit = [_on_qubits({0: ry}), _controlled(h, 0, 1), _controlled(x, 1, 2), _controlled(x, 0, 1), _on_qubits({0: x})]
    elif name == "ghz":
        circuit = [_on_qubits({0: h}), _controlled(x, 0, 1), _controlled(x, 0, 2)]
    else:
        raise NotImplementedError  # cost_function.py:58-59
    v = np.zeros(8, dtype=np.complex128)
    v[0] = 1.0
    for m in circuit:
        v = m @ v
    return v


def _entropy(rho) -> float:
    """-Tr rho log2 rho (qiskit's ``entropy``, base 2)."""
    ev = np.linalg.eigvalsh(rho)
    ev = ev[ev > 0.0]
    return float(-np.sum(ev * np.log2(ev)))


def pairwise_mutual_information(v) -> tuple:
    """(I(1:2), I(0:2), I(0:1)) of the three-qubit state v [8], in bits: for q = 0, 1, 2 the 4x4 state of the other two qubits
    (qiskit's ``partial_trace(sv, [q])``) and its ``mutual_information`` S(rho_a) + S(rho_b) - S(rho_ab)."""
    t = np.asarray(v, dtype=np.complex128).reshape(2, 2, 2)  # axes (q2, q1, q0)
    out = []
    for q in range(3):
        m = np.moveaxis(t, 2 - q, 2).reshape(4, 2)  # rows: the other two qubits (high, low), columns: qubit q
        rho = (m @ m.conj().T).reshape(2, 2, 2, 2)
        rho_hi, rho_lo = np.einsum("ajbj->ab", rho), np.einsum("jajb->ab", rho)
        out.append(_entropy(rho_hi) + _entropy(rho_lo) - _entropy(rho.reshape(4, 4)))
    return tuple(out)


class EntanglementCostFunction(ABC):
    """A start state -- "w", "ghz" (the reference's preparation circuits) or any length-8 vector of unit norm -- to which the template
    is appended; minimising the monotone of the final state undoes (equivalently: prepares) the entanglement.  ``state_vector`` is the
    start state, basis index q0 + 2 q1 + 4 q2."""

    def __init__(self, state="w"):
        if isinstance(state, str):
            self.state_vector = _prepared_state(state)
        else:
            v = np.array(state, dtype=np.complex128)
            if v.shape != (8,) or not np.all(np.isfinite(v)) or abs(float(np.vdot(v, v).real) - 1.0) > 1e-9:
                raise ValueError("state: \"w\", \"ghz\" or a vector of 8 amplitudes of unit norm")
            self.state_vector = v
        self.state = state

    def final_state(self, current_u) -> np.ndarray:
        u = np.asarray(current_u, dtype=np.complex128)
        if u.shape != (8, 8):
            raise ValueError("current_u must be the 8x8 unitary of a three-qubit template")
        return u @ self.state_vector

    def entanglement_monotone(self, current_u):
        """The objective at the 8x8 unitary of the bound template (the reference takes the circuit itself).  On the host; the
        optimizer's evaluations are fused into the HIP kernel."""
        raise NotImplementedError


class MutualInformation(EntanglementCostFunction):
    """I(1:2) + I(0:2) + I(0:1) of the final state (cost_function.py:68-84)."""

    def entanglement_monotone(self, current_u):
        return float(sum(pairwise_mutual_information(self.final_state(current_u))))


class MutualInformationSquare(EntanglementCostFunction):
    """The sum of the three squared mutual informations (cost_function.py:87-99)."""

    def entanglement_monotone(self, current_u):
        return float(sum(i * i for i in pairwise_mutual_information(self.final_state(current_u))))


class Negativity(EntanglementCostFunction):
    """Import parity only: the reference's body returns nothing (cost_function.py:102-104); ``TemplateOptimizer`` refuses it."""


class Formation(EntanglementCostFunction):
    """Import parity only (cost_function.py:107-109)."""


class EntropyofEntanglement(EntanglementCostFunction):
    """Import parity only (cost_function.py:112-114)."""
