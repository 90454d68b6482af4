"""``ThreeQubitCircuitTemplate``: the reference's ``CircuitTemplate(n_qubits=3, edge_params=...)`` (src/slam/basis.py:52-169) on the
HIP path -- 8x8 targets, two-qubit basis gates on the edges of a line or a triangle of three qubits.

The circuit, in time order: a ``U3`` on q0, q1, q2, then per two-qubit gate on its edge (a, b): the gate, a ``U3`` on a, a ``U3`` on b
(basis.py:152-169).  Gate i (0-based) is ``base_gates[i % len(base_gates)]`` on the edge
``edge_params[i % len(edge_params)][(i // len(edge_params)) % len(edge_params[i % len(edge_params)])]`` -- the reference's two nested
``cycle`` iterators, restarted at every ``build`` (this project's deviation C-2, see ``CircuitTemplate.build``).  Matrices are qiskit
little-endian: basis index q0 + 2 q1 + 4 q2, and a gate's 4x4 on the edge (a, b) has qubit a as its bit 0 (``circuit.append(gate,
[a, b])``), so (0, 2) and (2, 0) differ for CX.  ``eval`` and the optimizer run in the HIP library (csrc/slam_q3.hpp); this class
carries the structure.  ``CircuitTemplate`` itself keeps refusing ``n_qubits != 2``.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from . import runtime
from .basis import CircuitTemplate
from .basis_abc import VariationalTemplate
from .gates import gate_matrix

MAX_SPAN = 15  # SLAM_Q3_MAX_SPAN: n = 9 + 6 k <= 99 parameters


class ThreeQubitCircuitTemplate(VariationalTemplate):
    n_qubits = 3

    def __init__(self, base_gates, edge_params, maximum_span_guess=6, device=0):
        base_gates = list(base_gates)
        if not base_gates:
            raise ValueError("base_gates must not be empty")
        self.base_gates = base_gates
        self.gate_matrices = np.stack([gate_matrix(g) for g in base_gates])
        if len(edge_params) == 0:
            raise ValueError("edge_params must not be empty")
        edges = []
        for el in edge_params:
            el = [tuple(int(q) for q in e) for e in el]
            if not el:
                raise ValueError("every list of edge_params needs at least one edge")
            for e in el:
                if len(e) != 2 or e[0] == e[1] or not all(q in (0, 1, 2) for q in e):
                    raise ValueError(f"edge {e}: an edge is an ordered pair of distinct qubits from (0, 1, 2)")
            edges.append(el)
        self.edge_params = edges
        self.device = device
        self.filename = None
        self.no_exterior_1q = False
        self.using_bounds = False
        self.bounds_list = None
        self.using_constraints = False
        self.constraint_func = None
        self.maximum_span_guess = int(maximum_span_guess)
        self.spanning_range = range(1, self.maximum_span_guess + 1)
        self.coverage = None
        super().__init__(preseed=False, use_polytopes=False)
        self.cycles = 0
        self.trotter = False

    # ---- structure ---------------------------------------------------------------------------
    @staticmethod
    def _check_span(k: int) -> int:
        k = int(k)
        if k <= 0:
            raise ValueError()  # basis.py:127-128
        if k > MAX_SPAN:
            raise ValueError(f"three-qubit templates take at most {MAX_SPAN} two-qubit gates ({9 + 6 * MAX_SPAN} parameters), got {k}")
        return k

    def build(self, n_repetitions):
        """basis.py:124-134; the gate and edge cycles restart here (deviation C-2)."""
        self.cycles = 0  # (_reset: a refused size leaves an unbuilt template, as in the reference)
        self.cycles = self._check_span(n_repetitions)

    def get_spanning_range(self, target_u):
        return self.spanning_range

    def gate_sequence(self, k=None) -> List[int]:
        """Indices into ``base_gates`` of the k two-qubit gates, in circuit order."""
        k = self.cycles if k is None else int(k)
        return [i % len(self.base_gates) for i in range(k)]

    def edge_sequence(self, k=None) -> List[Tuple[int, int]]:
        """The edge (a, b) of each of the k two-qubit gates, in circuit order."""
        k = self.cycles if k is None else int(k)
        m = len(self.edge_params)
        return [self.edge_params[i % m][(i // m) % len(self.edge_params[i % m])] for i in range(k)]

    @property
    def n_params(self) -> int:
        return 9 + 6 * self.cycles

    # ---- numerics -----------------------------------------------------------------------------
    def eval(self, Xk):
        """8x8 unitary of the bound template (basis.py:102-104), computed by libslamhip."""
        if self.cycles <= 0:
            raise ValueError("build() the template first")
        Xk = np.asarray(Xk, dtype=np.float64).reshape(1, -1)
        if Xk.shape[1] != self.n_params:
            raise ValueError(f"expected {self.n_params} parameters, got {Xk.shape[1]}")
        ctx = runtime.get_context(self.device)
        _, _, w = ctx.q3_eval(self.gate_matrices, self.gate_sequence(), self.edge_sequence(), np.eye(8, dtype=np.complex128)[None], Xk,
                              want_grad=False, want_unitary=True)
        return w[0]

    def parameter_guess(self, t=0):
        """basis.py:106-111: uniform in [0, 2pi) from NumPy's global generator."""
        return np.random.random(self.n_params) * 2 * np.pi

    def to_gate_list(self, Xk) -> list:
        """The bound circuit in time order: ("u", qubit, (theta, phi, lam)) and ("gate", gate_object, (a, b))."""
        Xk = list(np.asarray(Xk, dtype=np.float64))
        if len(Xk) != self.n_params:
            raise ValueError(f"expected {self.n_params} parameters, got {len(Xk)}")
        out = [("u", q, tuple(Xk[3 * q : 3 * q + 3])) for q in range(3)]
        for j, (g, (a, b)) in enumerate(zip(self.gate_sequence(), self.edge_sequence())):
            out.append(("gate", self.base_gates[g], (a, b)))
            out.append(("u", a, tuple(Xk[9 + 6 * j : 12 + 6 * j])))
            out.append(("u", b, tuple(Xk[12 + 6 * j : 15 + 6 * j])))
        return out

    qiskit_parameter_order = staticmethod(CircuitTemplate.qiskit_parameter_order)
    from_qiskit_order = classmethod(CircuitTemplate.from_qiskit_order.__func__)
    to_qiskit_order = classmethod(CircuitTemplate.to_qiskit_order.__func__)
