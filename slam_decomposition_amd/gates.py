"""Two-qubit basis gates: the 4x4 matrices the template optimizer consumes.

The reference wraps these in qiskit ``Gate`` subclasses
(src/slam/utils/gates/custom_gates.py); qiskit is not a dependency here, so a
gate is a small object exposing ``__array__`` / ``to_matrix()`` / ``params`` /
``name`` / ``num_qubits`` -- the members the hot path touches.  Any object with
``__array__`` or ``to_matrix()`` returning a 4x4 unitary (including a real
qiskit ``Gate``) is accepted by ``CircuitTemplate``.
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np

_SX = np.array([[0, 1], [1, 0]], dtype=np.complex128)
_SY = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
_SZ = np.array([[1, 0], [0, -1]], dtype=np.complex128)


class Gate2Q:
    """Minimal stand-in for ``qiskit.circuit.Gate`` (2 qubits)."""

    num_qubits = 2

    def __init__(self, name: str, params: Sequence[float], label: str | None = None):
        self.name = name
        self.params = list(params)
        self.label = label or name

    def __array__(self, dtype=None, copy=None):
        m = self._matrix()
        return m if dtype is None else m.astype(dtype)

    def to_matrix(self) -> np.ndarray:
        return np.asarray(self.__array__(), dtype=np.complex128)

    def _matrix(self) -> np.ndarray:  # pragma: no cover - abstract
        raise NotImplementedError

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(repr(p) for p in self.params)})"

    def __str__(self):
        return repr(self)


class UnitaryGate(Gate2Q):
    """A fixed 4x4 unitary given as an array."""

    def __init__(self, matrix, name: str = "unitary"):
        m = np.asarray(matrix, dtype=np.complex128)
        if m.shape != (4, 4):
            raise ValueError("UnitaryGate needs a 4x4 matrix")
        super().__init__(name, [])
        self._m = m

    def _matrix(self):
        return self._m


class CXGate(Gate2Q):
    """qiskit ``CXGate`` (control qubit 0, target qubit 1; little-endian matrix), star-imported by
    the reference at src/slam/basis.py:10."""

    def __init__(self):
        super().__init__("cx", [])

    def _matrix(self):
        return np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], dtype=np.complex128)


class CZGate(Gate2Q):
    def __init__(self):
        super().__init__("cz", [])

    def _matrix(self):
        return np.diag([1, 1, 1, -1]).astype(np.complex128)


class SwapGate(Gate2Q):
    def __init__(self):
        super().__init__("swap", [])

    def _matrix(self):
        return np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)


class RiSwapGate(Gate2Q):
    """``RiSwapGate(alpha)`` = iSWAP**alpha (src/slam/utils/gates/custom_gates.py:534-606)."""

    def __init__(self, alpha: float):
        super().__init__("riswap", [alpha], label="riswap")
        self.duration = self.cost()

    def cost(self) -> float:
        return float(self.params[0])  # custom_gates.py:564-568

    def _matrix(self):
        a = float(self.params[0]) / 2.0  # custom_gates.py:582-595
        c = math.cos(math.pi * a)
        isin = 1j * math.sin(math.pi * a)
        return np.array([[1, 0, 0, 0], [0, c, isin, 0], [0, isin, c, 0], [0, 0, 0, 1]], dtype=np.complex128)


class iSwapGate(RiSwapGate):
    def __init__(self):
        super().__init__(1.0)
        self.name = "iswap"


def canonical_matrix(c1: float, c2: float, c3: float) -> np.ndarray:
    """``weylchamber.canonical_gate(c1, c2, c3)`` = exp(i pi/2 (c1 XX + c2 YY + c3 ZZ)); the three
    terms commute, so the exponential factorises."""
    out = np.eye(4, dtype=np.complex128)
    for c, s in ((c1, _SX), (c2, _SY), (c3, _SZ)):
        ang = math.pi / 2.0 * c
        out = out @ (math.cos(ang) * np.eye(4) + 1j * math.sin(ang) * np.kron(s, s))
    return out


class CanonicalGate(Gate2Q):
    """``CanonicalGate(alpha, beta, gamma)`` (custom_gates.py:384-392): arguments in radians,
    rescaled by 2/pi before ``weylchamber.canonical_gate``."""

    def __init__(self, alpha, beta, gamma, name="can"):
        super().__init__(name, [alpha, beta, gamma])
        a, b, g = (2 * x / np.pi for x in (alpha, beta, gamma))
        self.data = canonical_matrix(a, b, g)

    def _matrix(self):
        return self.data


class BerkeleyGate(CanonicalGate):
    """custom_gates.py:395-400."""

    def __init__(self):
        super().__init__(np.pi / 4, np.pi / 8, 0, name="B")

    def __str__(self):
        return "B"


def conversion_gain_matrix(phi_c: float, phi_g: float, gc: float, gg: float, t: float = 1.0) -> np.ndarray:
    """Closed form of exp(-i t H), H = gc (e^{i phi_c} A B^+ + h.c.) + gg (e^{i phi_g} A B + h.c.)
    (src/slam/hamiltonian.py:84-111): two decoupled 2x2 rotations on {|01>,|10>} and {|00>,|11>}."""
    U = np.zeros((4, 4), dtype=np.complex128)
    cc, sc = math.cos(gc * t), math.sin(gc * t)
    cg, sg = math.cos(gg * t), math.sin(gg * t)
    U[1, 1] = U[2, 2] = cc
    U[2, 1] = -1j * np.exp(1j * phi_c) * sc
    U[1, 2] = -1j * np.exp(-1j * phi_c) * sc
    U[0, 0] = U[3, 3] = cg
    U[3, 0] = -1j * np.exp(1j * phi_g) * sg
    U[0, 3] = -1j * np.exp(-1j * phi_g) * sg
    return U


class ConversionGainGate(Gate2Q):
    """``ConversionGainGate(p1, p2, g1, g2, t_el)`` (custom_gates.py:163-212); effective argument
    meaning phi_c = p1, phi_g = p2, gc = g1, gg = g2."""

    def __init__(self, p1, p2, g1, g2, t_el=1):
        super().__init__("2QGate", [p1, p2, g1, g2, t_el])
        self.duration = self.cost()
        self.name = str(self)

    def cost(self):
        norm = np.pi / 2  # custom_gates.py:207-211
        return (sum(abs(np.array(self.params[2:4]))) * self.params[-1]) / norm

    def __str__(self):
        g1, g2, t = self.params[2], self.params[3], self.params[4]
        return f"2QGate({g1:.8f}, {g2:.8f}, {t:.8f})"

    def normalize_duration(self, new_duration):
        """custom_gates.py:192-205: rescale the drive strengths so that the gate lasts ``new_duration`` (same unitary, same cost)."""
        t = self.params[-1]
        self.params[2] = self.params[2] * t / new_duration
        self.params[3] = self.params[3] * t / new_duration
        self.params[-1] = new_duration
        self.duration = self.cost()
        self.name = str(self)

    def _matrix(self):
        p1, p2, g1, g2, t = (float(v) for v in self.params)
        return conversion_gain_matrix(p1, p2, g1, g2, t)


_A = np.kron(np.array([[0, 0], [1, 0]], dtype=np.complex128), np.eye(2))  # a (x) I, a = qutip.create(2)
_B = np.kron(np.eye(2), np.array([[0, 0], [1, 0]], dtype=np.complex128))  # I (x) a


def smush_hamiltonian(phi_c: float, phi_g: float, gc: float, gg: float, gx: float, gy: float) -> np.ndarray:
    """H = gx (A + A^+) + gy (B + B^+) + gc (e^{i phi_c} A B^+ + h.c.) + gg (e^{i phi_g} A B + h.c.)  (hamiltonian.py:114-144)."""
    Ad, Bd = _A.conj().T, _B.conj().T
    conv = np.exp(1j * phi_c) * (_A @ Bd)
    gain = np.exp(1j * phi_g) * (_A @ _B)
    return gx * (_A + Ad) + gy * (_B + Bd) + gc * (conv + conv.conj().T) + gg * (gain + gain.conj().T)


def smush_matrix(phi_c, phi_g, gc, gg, gx: Sequence[float], gy: Sequence[float], t: float = 1.0) -> np.ndarray:
    """U = U_{N-1} ... U_0,  U_s = exp(-i (t / N) H_s): the conversion-gain pulse with the single-qubit drives (gx[s], gy[s]) of
    slice s (ConversionGainSmushGate, hamiltonian.py:114-144).  Each slice exponential through the eigen-decomposition of the
    Hermitian H_s, for any phases."""
    gx = np.atleast_1d(np.asarray(gx, dtype=np.float64))
    gy = np.atleast_1d(np.asarray(gy, dtype=np.float64))
    if gx.shape != gy.shape or gx.ndim != 1 or gx.size == 0:
        raise ValueError("gx and gy must be sequences of the same, non-zero length")
    tau = float(t) / gx.size
    U = np.eye(4, dtype=np.complex128)
    for s in range(gx.size):
        w, V = np.linalg.eigh(smush_hamiltonian(float(phi_c), float(phi_g), float(gc), float(gg), gx[s], gy[s]))
        U = (V * np.exp(-1j * tau * w)) @ V.conj().T @ U
    return U


class ConversionGainSmushGate(Gate2Q):
    """``ConversionGainSmushGate(pc, pg, gc, gg, gx, gy, t_el)`` (custom_gates.py:215-257): a conversion-gain pulse with
    single-qubit drives applied during it, cut into N = len(gx) time slices with their own drive amplitudes.  Params are
    ``[pc, pg, gc, gg, *gx, *gy, t]``; ``xy_len`` = N."""

    def __init__(self, pc, pg, gc, gg, gx, gy, t_el=1):
        gx = [float(v) for v in np.atleast_1d(np.asarray(gx, dtype=np.float64))]
        gy = [float(v) for v in np.atleast_1d(np.asarray(gy, dtype=np.float64))]
        if len(gx) != len(gy) or not gx:
            raise ValueError("gx and gy must have the same, non-zero length")
        self.xy_len = len(gx)
        super().__init__("2QSmushGate", [pc, pg, gc, gg, *gx, *gy, t_el])
        self.duration = self.cost()

    @property
    def gx(self):
        return self.params[4 : 4 + self.xy_len]

    @property
    def gy(self):
        return self.params[4 + self.xy_len : 4 + 2 * self.xy_len]

    def cost(self):
        norm = np.pi / 2  # as ConversionGainGate: (|gc| + |gg|) t / (pi / 2)
        return (abs(float(self.params[2])) + abs(float(self.params[3]))) * float(self.params[-1]) / norm

    def _matrix(self):
        pc, pg, gc, gg = (float(v) for v in self.params[:4])
        return smush_matrix(pc, pg, gc, gg, self.gx, self.gy, float(self.params[-1]))


# ---- three-qubit gates (basis3q.ThreeQubitCircuitTemplate only) ----------------------------------------------------------------
class Gate3Q(Gate2Q):
    """Sibling of ``Gate2Q`` for three qubits: ``to_matrix()`` is 8x8 complex128, qiskit little-endian -- basis index
    q0 + 2 q1 + 4 q2 of the gate's own three qubits.  ``U|j> = |pi(j)>`` below means the permutation matrix with U[pi(j), j] = 1."""

    num_qubits = 3


def _permutation8(pi: Sequence[int]) -> np.ndarray:
    m = np.zeros((8, 8), dtype=np.complex128)
    for j, pj in enumerate(pi):
        m[pj, j] = 1.0
    return m


def _swapped(*pairs) -> list:
    pi = list(range(8))
    for i, j in pairs:
        pi[i], pi[j] = j, i
    return pi


class _FixedGate3Q(Gate3Q):
    NAME = ""

    def __init__(self):
        super().__init__(self.NAME, [])


class CCZGate(_FixedGate3Q):
    """-1 on |7>."""

    NAME = "ccz"

    def _matrix(self):
        m = np.eye(8, dtype=np.complex128)
        m[7, 7] = -1.0
        return m


class CCXGate(_FixedGate3Q):
    """Toffoli, controls q0 and q1, target q2: |3> <-> |7>."""

    NAME = "ccx"

    def _matrix(self):
        return _permutation8(_swapped((3, 7)))


class CSwapGate(_FixedGate3Q):
    """Fredkin, control q0, swaps q1 and q2: |3> <-> |5>."""

    NAME = "cswap"

    def _matrix(self):
        return _permutation8(_swapped((3, 5)))


def _ix_on_pair(i: int, j: int) -> np.ndarray:
    m = np.eye(8, dtype=np.complex128)
    m[i, i] = m[j, j] = 0.0
    m[i, j] = m[j, i] = 1j
    return m


class CCiXGate(_FixedGate3Q):
    """i X on the pair {|6>, |7>} (custom_gates.py:316-486 holds the reference's fixed three-qubit gates)."""

    NAME = "ccix"

    def _matrix(self):
        return _ix_on_pair(6, 7)


class CiSwap(_FixedGate3Q):
    """i X on the pair {|5>, |6>}: the iSWAP of q0 and q1 while q2 = 1."""

    NAME = "ciswap"

    def _matrix(self):
        return _ix_on_pair(5, 6)


class Peres(_FixedGate3Q):
    """As the reference has it: for q2 = 1, X on q0 and on q1 -- |4> <-> |7>, |5> <-> |6>."""

    NAME = "peres"

    def _matrix(self):
        return _permutation8(_swapped((4, 7), (5, 6)))


class Margolus(_FixedGate3Q):
    """-1 on |5>, |6> <-> |7>."""

    NAME = "margolus"

    def _matrix(self):
        m = _permutation8(_swapped((6, 7)))
        m[5, 5] = -1.0
        return m


class CParitySwap(_FixedGate3Q):
    """Two 3-cycles of basis states: 1 -> 2 -> 4 -> 1 and 3 -> 5 -> 6 -> 3."""

    NAME = "cpswap"

    def _matrix(self):
        pi = list(range(8))
        for cyc in ((1, 2, 4), (3, 5, 6)):
            for i in range(3):
                pi[cyc[i]] = cyc[(i + 1) % 3]
        return _permutation8(pi)


def circulator_hamiltonian(p_ab: float, p_ac: float, p_bc: float, g_ab: float, g_ac: float, g_bc: float) -> np.ndarray:
    """H = g_ab (e^{i p_ab} A B^+ + h.c.) + g_ac (e^{i p_ac} A C^+ + h.c.) + g_bc (e^{i p_bc} B C^+ + h.c.) with A, B, C the 2x2 raising
    operator [[0, 0], [1, 0]] on the left, middle and right Kronecker factor: mode a is bit 2, mode c is bit 0 (the reference's
    CirculatorHamiltonian, hamiltonian.py:244-272)."""
    up = np.array([[0, 0], [1, 0]], dtype=np.complex128)
    one = np.eye(2, dtype=np.complex128)
    A = np.kron(up, np.kron(one, one))
    B = np.kron(one, np.kron(up, one))
    Cm = np.kron(one, np.kron(one, up))
    h = np.zeros((8, 8), dtype=np.complex128)
    for p, g, x, y in ((p_ab, g_ab, A, B), (p_ac, g_ac, A, Cm), (p_bc, g_bc, B, Cm)):
        term = g * np.exp(1j * p) * (x @ y.conj().T)
        h += term + term.conj().T
    return h


class CirculatorSNAILGate(Gate3Q):
    """``CirculatorSNAILGate(p1, p2, p3, g1, g2, g3, t_el=1)`` = exp(-i t H), H = ``circulator_hamiltonian`` of the phases
    (p_ab, p_ac, p_bc) and strengths (g_ab, g_ac, g_bc) (custom_gates.py:95-160).  Computed from ``numpy.linalg.eigh`` of the 8x8
    Hermitian H."""

    def __init__(self, p1, p2, p3, g1, g2, g3, t_el=1.0, name: str = "3QGate"):
        super().__init__(name, [p1, p2, p3, g1, g2, g3, t_el])
        self.duration = self.cost()

    def cost(self) -> float:
        """sum |g| * t / (pi / 2)"""
        return sum(abs(float(g)) for g in self.params[3:6]) * float(self.params[6]) / (math.pi / 2)

    def fidelity(self) -> float:
        return max(1.0 - 0.001 * self.cost(), 0.0)

    def _matrix(self):
        w, v = np.linalg.eigh(circulator_hamiltonian(*(float(p) for p in self.params[:6])))
        return (v * np.exp(-1j * float(self.params[6]) * w)) @ v.conj().T


class VSwap(CirculatorSNAILGate):
    def __init__(self, t_el=1.0):
        v = 4.0 / math.sqrt(2.0)
        super().__init__(math.pi / 2, math.pi / 2, 0.0, math.pi / v, math.pi / v, 0.0, t_el, name="vswap")


class DeltaSwap(CirculatorSNAILGate):
    def __init__(self, t_el=1.0):
        v = 3.0 * math.sqrt(3.0) / 2.0
        super().__init__(math.pi / 2, -math.pi / 2, math.pi / 2, math.pi / v, math.pi / v, math.pi / v, t_el, name="deltaswap")


def gate_matrix(gate) -> np.ndarray:
    """4x4 (two-qubit gate) or 8x8 (three-qubit gate) complex128 matrix of a gate object / array."""
    if hasattr(gate, "to_matrix"):
        m = gate.to_matrix()
    else:
        m = np.asarray(gate)
    m = np.asarray(m, dtype=np.complex128)
    if m.shape == (8, 8):
        return m
    if m.shape != (4, 4):
        raise ValueError(f"2Q basis gate must be a 4x4 matrix, got shape {m.shape}")
    return m
