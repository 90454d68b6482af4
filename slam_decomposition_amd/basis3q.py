"""``ThreeQubitCircuitTemplate``: the reference's ``CircuitTemplate(n_qubits=3, edge_params=...)`` (src/slam/basis.py:52-169) on the
HIP path -- 8x8 targets, two-qubit basis gates on the edges of a line or a triangle of three qubits, and three-qubit basis gates
(``gates.Gate3Q``: CCZ, Peres, VSwap, ...) on ordered triples of all three.

The circuit, in time order: a ``U3`` on q0, q1, q2, then per two-qubit gate on its edge (a, b): the gate, a ``U3`` on a, a ``U3`` on b
(basis.py:152-169).  Gate i (0-based) is ``base_gates[i % len(base_gates)]`` on the edge
``edge_params[i % len(edge_params)][(i // len(edge_params)) % len(edge_params[i % len(edge_params)])]`` -- the reference's two nested
``cycle`` iterators, restarted at every ``build`` (this project's deviation C-2, see ``CircuitTemplate.build``).  Matrices are qiskit
little-endian: basis index q0 + 2 q1 + 4 q2, and a gate's 4x4 on the edge (a, b) has qubit a as its bit 0 (``circuit.append(gate,
[a, b])``), so (0, 2) and (2, 0) differ for CX.  ``eval`` and the optimizer run in the HIP library (csrc/slam_q3.hpp); this class
carries the structure.  ``CircuitTemplate`` itself keeps refusing ``n_qubits != 2``.

A base gate whose matrix is 8x8 takes edges that are ordered triples (a, b, c) of the three distinct qubits -- gate-local bit 0 is
qubit a, bit 1 is b, bit 2 is c, like ``circuit.append(gate, [a, b, c])`` -- and is followed by a ``U3`` on a, on b, on c:
n = 9 + 3 * sum(arity).  The two cycles pair gates and edges as before; ``build`` refuses a size at which a gate meets an edge of the
wrong length, more than 99 parameters or more than 15 gates.  At most ``MAX_GATES3`` distinct three-qubit gates per template.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from . import runtime
from .basis import CircuitTemplate
from .basis_abc import VariationalTemplate
from .gates import gate_matrix

MAX_SPAN = 15  # SLAM_Q3_MAX_SPAN: n = 9 + 6 k <= 99 parameters
MAX_PARAMS = 99
MAX_GATES3 = 3  # SLAM_Q3_MAX_GATES3: distinct three-qubit gates of one template


class ThreeQubitCircuitTemplate(VariationalTemplate):
    n_qubits = 3

    def __init__(self, base_gates, edge_params, maximum_span_guess=6, device=0):
        base_gates = list(base_gates)
        if not base_gates:
            raise ValueError("base_gates must not be empty")
        self.base_gates = base_gates
        mats = [gate_matrix(g) for g in base_gates]
        self.arities = [3 if m.shape == (8, 8) else 2 for m in mats]
        # per base gate its entry in the table of its arity; gate_matrices: the 4x4 table (as before), gate_matrices3: the 8x8 one
        self._table_index = [self.arities[:i].count(a) for i, a in enumerate(self.arities)]
        two = [m for m in mats if m.shape == (4, 4)]
        three = [m for m in mats if m.shape == (8, 8)]
        if len(three) > MAX_GATES3:
            raise ValueError(f"a template takes at most {MAX_GATES3} three-qubit base gates, got {len(three)}")
        self.gate_matrices = np.stack(two) if two else np.zeros((0, 4, 4), dtype=np.complex128)
        self.gate_matrices3 = np.stack(three) if three else np.zeros((0, 8, 8), dtype=np.complex128)
        if len(edge_params) == 0:
            raise ValueError("edge_params must not be empty")
        edges = []
        for el in edge_params:
            el = [tuple(int(q) for q in e) for e in el]
            if not el:
                raise ValueError("every list of edge_params needs at least one edge")
            for e in el:
                if len(e) == 3 and three:
                    if sorted(e) != [0, 1, 2]:
                        raise ValueError(f"edge {e}: a three-qubit gate takes an ordered triple of the distinct qubits 0, 1, 2")
                elif len(e) != 2 or e[0] == e[1] or not all(q in (0, 1, 2) for q in e):
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

    def _check_size(self, k: int) -> int:
        """``_check_span``, then per position the gate's arity against its edge's length, then the parameter cap."""
        k = self._check_span(k)
        gs, es = self.gate_sequence(k), self.edge_sequence(k)
        for j, (g, e) in enumerate(zip(gs, es)):
            if self.arities[g] != len(e):
                raise ValueError(f"position {j}: base gate {g} acts on {self.arities[g]} qubits, its edge {e} has {len(e)}")
        n = 9 + 3 * sum(self.arities[g] for g in gs)
        if n > MAX_PARAMS:
            raise ValueError(f"three-qubit templates take at most {MAX_PARAMS} parameters, {k} gates of this template have {n}")
        return k

    def build(self, n_repetitions):
        """basis.py:124-134; the gate and edge cycles restart here (deviation C-2)."""
        self.cycles = 0  # (_reset: a refused size leaves an unbuilt template, as in the reference)
        self.cycles = self._check_size(n_repetitions)

    def get_spanning_range(self, target_u):
        return self.spanning_range

    def gate_sequence(self, k=None) -> List[int]:
        """Indices into ``base_gates`` of the k gates, in circuit order."""
        k = self.cycles if k is None else int(k)
        return [i % len(self.base_gates) for i in range(k)]

    def edge_sequence(self, k=None) -> List[Tuple[int, ...]]:
        """The edge of each of the k gates, in circuit order: (a, b) of a two-qubit gate, (a, b, c) of a three-qubit one."""
        k = self.cycles if k is None else int(k)
        m = len(self.edge_params)
        return [self.edge_params[i % m][(i // m) % len(self.edge_params[i % m])] for i in range(k)]

    def table_sequence(self, k=None) -> List[int]:
        """Per position the gate's entry in the table of its arity (``gate_matrices`` / ``gate_matrices3``); a template of two-qubit
        gates only: ``gate_sequence``."""
        return [self._table_index[g] for g in self.gate_sequence(k)]

    def has_three_qubit_position(self, k=None) -> bool:
        return any(self.arities[g] == 3 for g in self.gate_sequence(k))

    def mixed_description(self, k=None):
        """What ``slam_q3m_*`` take for k gates: (arity [k], index into the table of that arity [k], qubits [k, 3])."""
        gs, es = self.gate_sequence(k), self.edge_sequence(k)
        return [self.arities[g] for g in gs], self.table_sequence(k), [tuple(e) + (0,) * (3 - len(e)) for e in es]

    @property
    def n_params(self) -> int:
        return 9 + 3 * sum(self.arities[g] for g in self.gate_sequence())

    # ---- numerics -----------------------------------------------------------------------------
    def eval(self, Xk):
        """8x8 unitary of the bound template (basis.py:102-104), computed by libslamhip."""
        if self.cycles <= 0:
            raise ValueError("build() the template first")
        Xk = np.asarray(Xk, dtype=np.float64).reshape(1, -1)
        if Xk.shape[1] != self.n_params:
            raise ValueError(f"expected {self.n_params} parameters, got {Xk.shape[1]}")
        ctx = runtime.get_context(self.device)
        if self.has_three_qubit_position():
            _, _, w = ctx.q3m_eval(self.gate_matrices, self.gate_matrices3, *self.mixed_description(), np.eye(8, dtype=np.complex128)[None],
                                   Xk, want_grad=False, want_unitary=True)
        else:
            _, _, w = ctx.q3_eval(self.gate_matrices, self.table_sequence(), self.edge_sequence(), np.eye(8, dtype=np.complex128)[None], Xk,
                                  want_grad=False, want_unitary=True)
        return w[0]

    def parameter_guess(self, t=0):
        """basis.py:106-111: uniform in [0, 2pi) from NumPy's global generator."""
        return np.random.random(self.n_params) * 2 * np.pi

    def to_gate_list(self, Xk) -> list:
        """The bound circuit in time order: ("u", qubit, (theta, phi, lam)) and ("gate", gate_object, edge)."""
        Xk = list(np.asarray(Xk, dtype=np.float64))
        if len(Xk) != self.n_params:
            raise ValueError(f"expected {self.n_params} parameters, got {len(Xk)}")
        out = [("u", q, tuple(Xk[3 * q : 3 * q + 3])) for q in range(3)]
        base = 9
        for g, edge in zip(self.gate_sequence(), self.edge_sequence()):
            out.append(("gate", self.base_gates[g], edge))
            for q in edge:
                out.append(("u", q, tuple(Xk[base : base + 3])))
                base += 3
        return out

    qiskit_parameter_order = staticmethod(CircuitTemplate.qiskit_parameter_order)
    from_qiskit_order = classmethod(CircuitTemplate.from_qiskit_order.__func__)
    to_qiskit_order = classmethod(CircuitTemplate.to_qiskit_order.__func__)
