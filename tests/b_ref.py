"""Test-side restatement of the closed-form decomposition into one or two gates of the B class (``slam_b_decompose``,
csrc/slam_b.hpp), in NumPy.  Nothing is shared with csrc/; matrices are rebuilt with ``kak_ref`` (``can``, ``kron2``, ``random_su2``) and
the alignments decompose with ``slam_decomposition_amd.weyl.kak``, the host route, as tests/cx_ref.py does (``kak_ref.lapack_kak`` has
no chamber order to align two decompositions by).

Conventions: kron(a, b) puts a on the high bit (qubit 1); CAN(c) = exp(i pi/2 (c1 XX + c2 YY + c3 ZZ)), c in units of pi;
B = CAN(1/2, 1/4, 0); RP(t) = exp(+i t P / 2) -- the sign matters: exp(-i t P / 2) on the first qubit gives the mirror class.  A template
row holds six angles per layer: U3(theta, phi, lam) of qubit 0 (the low bit), then of qubit 1.

Two B gates reach every class (Zhang, Vala, Sastry, Whaley, PRL 93, 020502).  For the folded chamber point 1/2 >= c1 >= c2 >= |c3|

    B (RY(pi c3) (x) RZ(bz) RY(by) RZ(bz)) B   ~   CAN(c1, c2, c3),
    sin(by / 2) = sqrt(2) sin(pi c1 / 2) cos(pi c2 / 2),
    bz = atan2(sqrt(max(cos(pi c1) cos(pi c2), 0)), sqrt(2) sin(pi c2 / 2) cos(pi c1 / 2)),

the paper's arccos / arcsin forms rewritten without cancellation (``interior``); a point with c1 > 1/2 is folded to
(1 - c1, c2, -c3) first.  cos(pi c1) is formed as sin(pi (1/2 - c1)): bz has a square-root singularity on the face c1 = 1/2, which is a
property of the map (the circuit's coordinates depend on bz^2), and the subtraction 1/2 - c1 is exact there.

Any gate G of the class: G ~ L B R by aligning B with G once, so B K B ~ L^+ G (R^+ K L^+) G R^+ and the interior layer of the G-circuit
is R^+ K L^+.  The exterior layers come from aligning the interior circuit with the target (``align``).
"""
from __future__ import annotations

import numpy as np

import kak_ref as kr
from closed_form_ref import SIZE_TOL, _I, _X, _Y, _Z, dress, template, u3, u3_angles, up_to_phase  # noqa: F401 (re-exported)
from closed_form_ref import fold_chamber as fold, loss as loss_of  # noqa: F401 (this module's names for them)
from slam_decomposition_amd import weyl

POINT = (0.5, 0.25, 0.0)


def can(c) -> np.ndarray:
    return kr.can(np.asarray(c, dtype=np.float64))


B = can(POINT)
CX = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], dtype=np.complex128)
ISWAP = np.array([[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)
SWAP = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)
SQISWAP = can((0.25, 0.25, 0.0))


def rp(p, t) -> np.ndarray:
    """exp(+i t P / 2)."""
    return np.cos(0.5 * t) * _I + 1j * np.sin(0.5 * t) * p


def angles(c):
    """(by, bz) for a FOLDED point c (units of pi)."""
    c1, c2 = np.pi * c[0], np.pi * c[1]
    cos_c1 = np.sin(np.pi * (0.5 - c[0]))
    by = 2.0 * np.arcsin(min(np.sqrt(2.0) * np.sin(0.5 * c1) * np.cos(0.5 * c2), 1.0))
    bz = np.arctan2(np.sqrt(max(cos_c1 * np.cos(c2), 0.0)), np.sqrt(2.0) * np.sin(0.5 * c2) * np.cos(0.5 * c1))
    return by, bz


def interior(c):
    """(q1, q0): the interior layer kron(q1, q0) of B K B ~ CAN(c) for a FOLDED point c."""
    by, bz = angles(c)
    return rp(_Y, np.pi * c[2]), rp(_Z, bz) @ rp(_Y, by) @ rp(_Z, bz)


def expected_size(T) -> np.ndarray:
    """Per matrix of T[N, 4, 4]: span_rules.minimal_span for family ``b`` on the 8-digit coordinates, local targets at two gates."""
    from slam_decomposition_amd import span_rules

    k = span_rules.minimal_span(weyl.c1c2c3_batch(np.asarray(T)), POINT)
    return np.where(k == 0, 2, k)


def align(W, T):
    """((L1, L0), (R1, R0), gap): 2x2 local gates with T ~ (L1 (x) L0) W (R1 (x) R0) up to a phase for W, T of (nearly) one class: KAK of
    both, W's mirrored where that brings its chamber point closer to T's."""
    kw, kt = weyl.kak(W), weyl.kak(T)
    cw, ct = np.asarray(kw[3]), np.asarray(kt[3])
    d0 = np.max(np.abs(cw - ct))
    d1 = np.max(np.abs(np.array([1 - cw[0], cw[1], -cw[2]]) - ct))
    if d1 < d0:
        kw = weyl.mirror_kak(*kw)
    L = (kt[1] @ kw[1].conj().T, kt[2] @ kw[2].conj().T)
    R = (kw[4].conj().T @ kt[4], kw[5].conj().T @ kt[5])
    return L, R, float(min(d0, d1))


_GATE_CACHE = {}


def gate_factors(G):
    """(L, R) with G ~ kron(*L) B kron(*R); ``ValueError`` for a gate outside the class."""
    key = np.asarray(G, dtype=np.complex128).tobytes()
    if key not in _GATE_CACHE:
        f = np.abs(fold(np.array(weyl.c1c2c3(G))))
        if not np.max(np.abs(f - np.array(POINT))) < SIZE_TOL:
            raise ValueError("the gate is not of the B class")
        L, R, gap = align(B, G)
        assert gap < 4 * SIZE_TOL
        _GATE_CACHE[key] = (L, R)
    return _GATE_CACHE[key]


def decompose(T, G):
    """(x, cycles, loss, gap) for the 4x4 unitary T and a gate G of the B class: the 6 (cycles + 1) angles of a circuit of G-gates, the
    BasicCost loss of ``template(x, G, cycles)`` against T and the chamber distance left by the alignment of the interior circuit."""
    T = np.asarray(T, dtype=np.complex128)
    G = np.asarray(G, dtype=np.complex128)
    (L1, L0), (R1, R0) = gate_factors(G)
    c = np.asarray(weyl.kak(T)[3])
    f8 = fold(np.round(c, 8))
    k = 1 if np.max(np.abs(np.abs(f8) - np.array(POINT))) < SIZE_TOL else 2
    layers = []
    V = G
    if k == 2:
        q1, q0 = interior(fold(c))
        q1, q0 = R1.conj().T @ q1 @ L1.conj().T, R0.conj().T @ q0 @ L0.conj().T
        layers.append((q1, q0))
        V = G @ np.kron(q1, q0) @ G
    Lw, Rw, gap = align(V, T)
    layers = [Rw] + layers + [Lw]
    x = np.array([a for q1, q0 in layers for a in list(u3_angles(q0)) + list(u3_angles(q1))])
    return x, k, loss_of(T, template(x, G, k)), gap


def _named():
    out = [("identity", np.eye(4, dtype=np.complex128)), ("B", B), ("CX", CX), ("iSWAP", ISWAP), ("SWAP", SWAP), ("sqrt(iSWAP)", SQISWAP)]
    for c in ((0.5, 0.25, 1e-9), (0.5, 0.25, 2e-8), (0.5 - 1e-9, 1e-9, 0.0), (0.5, 0.3, 0.1), (0.5 - 1e-12, 0.3, 0.1), (0.7, 0.2, 0.1),
              (0.3, 0.2, -0.1), (1e-9, 1e-9, 1e-9), (0.25, 0.25, 0.25)):
        out.append(("CAN(%.13g, %g, %g)" % c, can(c)))
    return out


# the named and hard inputs: (name, gate).  "CAN(0.5, 0.25, 2e-08)" lies on the size rule's tolerance, where either size is right
NAMED = _named()
ON_BOUNDARY = ("CAN(0.5, 0.25, 2e-08)",)
ONE_GATE = ("B", "CAN(0.5, 0.25, 1e-09)")


def basis_gates(rng):
    """(name, matrix) of the basis gates the tests run: B as ``BerkeleyGate`` gives it, CAN at the point and two randomly dressed
    members of the class."""
    from slam_decomposition_amd.gates import BerkeleyGate, CanonicalGate, gate_matrix

    return [("B", gate_matrix(BerkeleyGate())), ("CAN", gate_matrix(CanonicalGate(np.pi / 4, np.pi / 8, 0.0))),
            ("dressed B 1", dress(rng, B)), ("dressed B 2", dress(rng, B))]
