"""Test-side restatement of the closed-form decomposition into gates of any supercontrolled class CAN(1/2, beta, 0), 0 <= beta <= 1/2
(``slam_sc_decompose``, ``slam_sc_counts``; csrc/slam_sc.hpp), in NumPy.  Nothing is shared with csrc/.

Conventions (tests/closed_form_ref.py): kron(a, b) puts a on the high bit (qubit 1); CAN(c) = exp(i pi/2 (c1 XX + c2 YY + c3 ZZ)), c in
units of pi, so Ud(a, b, c) = exp(i (a XX + b YY + c ZZ)) = CAN(2 a / pi, 2 b / pi, 2 c / pi); rz(t) = diag(e^{-i t / 2}, e^{i t / 2}).
S = CAN(1/2, beta, 0), beta' = pi beta / 2.  A target T = (K1l (x) K1r) Ud(a, b, c) (K2l (x) K2r) with pi/4 >= a >= b >= |c| -- the folded
coordinates of tests/approx_ref.py times pi/2 -- is the product (leftmost factor applied last; every matrix of ``matrices`` depends on beta
alone)

    three gates, every target:
        (K1l K31l (x) K1r K31r) S (K3221l (x) K32r rz(-2c) K21r) S (K22l rz(-2a) K11l (x) K22r rz(2b) K11r) S (K12l K2l (x) K12r K2r)
    two gates, exact where c = 0, the best two-gate circuit elsewhere (|Tr(T^+ W)| = 4 |cos c|):
        (K1l K12l^+ (x) K1r K12r^+ ipz) S (K11l^+ rz(-2a) K11l (x) ipz K11r^+ rz(2b) K11r) S (K12l K2l (x) K12r K2r)
    one gate:  (K1l (x) K1r) S (K2l (x) K2r)            no gate:  K1l K2l (x) K1r K2r

up to a phase: the construction of qiskit's TwoQubitBasisDecomposer, which is exact for every supercontrolled gate.  The formulas are
symmetric under exchanging both qubits of every pair.  The best circuit of k gates reaches |Tr(T^+ W)| = 4 t_k with the t_k of
tests/approx_ref.py at a free beta (``traces``); the size is chosen as there (``select``).

For 0 < beta < 1/2 the exact two-gate set is a polytope larger than the plane c3 = 0; this formula is exact on the plane only.
"""
from __future__ import annotations

import numpy as np

import approx_ref as ar
from approx_ref import fold, gate_fidelity, row_loss, row_matrix, rows_losses  # noqa: F401 (re-exported)
from closed_form_ref import can, dress, loss as loss_of, template, u3_angles, up_to_phase  # noqa: F401 (re-exported)

NAMES = ("K11l", "K11r", "K12l", "K12r", "K3221l", "K21r", "K22l", "K22r", "K31l", "K31r", "K32r")
IPZ = np.array([[1j, 0], [0, -1j]])


def rz(t) -> np.ndarray:
    return np.array([[np.exp(-0.5j * t), 0], [0, np.exp(0.5j * t)]])


def ud(a, b, c) -> np.ndarray:
    return can(np.array([a, b, c]) / (0.5 * np.pi))


def matrices(beta: float) -> dict:
    """The eleven fixed 2x2 matrices of the gate class (1/2, beta, 0)."""
    bp = 0.5 * np.pi * beta
    em, ep = np.exp(-1j * bp), np.exp(1j * bp)
    Em, Ep = np.exp(-2j * bp), np.exp(2j * bp)
    c2, s2 = np.cos(2 * bp), np.sin(2 * bp)
    r = 1 / np.sqrt(2)
    return {
        "K11l": 1 / (1 + 1j) * np.array([[-1j * em, em], [-1j * ep, -ep]]),
        "K11r": r * np.array([[1j * em, -em], [ep, -1j * ep]]),
        "K12l": 1 / (1 + 1j) * np.array([[1j, 1j], [-1, 1]]),
        "K12r": r * np.array([[1j, 1], [-1, -1j]]),
        "K3221l": r * np.array([[1 + 1j * c2, 1j * s2], [1j * s2, 1 - 1j * c2]]),
        "K21r": 1 / (1 - 1j) * np.array([[-1j * Em, Em], [1j * Ep, Ep]]),
        "K22l": r * np.array([[1, -1], [1, 1]], dtype=np.complex128),
        "K22r": np.array([[0, 1], [-1, 0]], dtype=np.complex128),
        "K31l": r * np.array([[em, em], [-ep, ep]]),
        "K31r": 1j * np.array([[ep, 0], [0, -em]]),
        "K32r": 1 / (1 - 1j) * np.array([[ep, -em], [-1j * ep, -1j * em]]),
    }


def _h(m):
    return np.conj(m).T


def interior(k: int, abc, beta: float):
    """The k - 1 interior layers [(q1, q0), ...] of the k-gate circuit of S-gates, first applied first."""
    a, b, c = abc
    m = matrices(beta)
    if k == 2:
        return [(_h(m["K11l"]) @ rz(-2 * a) @ m["K11l"], IPZ @ _h(m["K11r"]) @ rz(2 * b) @ m["K11r"])]
    if k == 3:
        return [(m["K22l"] @ rz(-2 * a) @ m["K11l"], m["K22r"] @ rz(2 * b) @ m["K11r"]),
                (m["K3221l"], m["K32r"] @ rz(-2 * c) @ m["K21r"])]
    return []


def circuit(k: int, abc, beta: float, K1=None, K2=None) -> np.ndarray:
    """The k-gate circuit for the target kron(*K1) Ud(a, b, c) kron(*K2) multiplied out (K1 = K2 = 1 by default)."""
    I2 = np.eye(2, dtype=np.complex128)
    K1l, K1r = (I2, I2) if K1 is None else K1
    K2l, K2r = (I2, I2) if K2 is None else K2
    m = matrices(beta)
    S = can((0.5, beta, 0.0))
    if k == 0:
        return np.kron(K1l @ K2l, K1r @ K2r)
    if k == 1:
        return np.kron(K1l, K1r) @ S @ np.kron(K2l, K2r)
    bottom = np.kron(m["K12l"] @ K2l, m["K12r"] @ K2r)
    W = S @ bottom
    for q1, q0 in interior(k, abc, beta):
        W = S @ np.kron(q1, q0) @ W
    if k == 2:
        return np.kron(K1l @ _h(m["K12l"]), K1r @ _h(m["K12r"]) @ IPZ) @ W
    return np.kron(K1l @ m["K31l"], K1r @ m["K31r"]) @ W


def traces(c, beta: float) -> np.ndarray:
    """t_k [N, 4] for the (unfolded) coordinates c [N, 3] and the gate class (1/2, beta, 0)."""
    f = fold(c)
    a, b, cc = (0.5 * np.pi * f[:, j] for j in range(3))
    bp = 0.5 * np.pi * beta
    q = 0.25 * np.pi
    t0 = np.abs(np.cos(a) * np.cos(b) * np.cos(cc) + 1j * np.sin(a) * np.sin(b) * np.sin(cc))
    t1 = np.abs(np.cos(q - a) * np.cos(bp - b) * np.cos(cc) + 1j * np.sin(q - a) * np.sin(bp - b) * np.sin(cc))
    return np.stack([t0, t1, np.abs(np.cos(cc)), np.ones(len(f))], axis=1)


def expected(c, beta: float, f: float) -> np.ndarray:
    """E_k [N, 4] = F_k f^k."""
    return gate_fidelity(traces(c, beta)) * float(f) ** np.arange(4)[None, :]


def select(c, beta: float, f: float) -> np.ndarray:
    """The chosen k [N]: the first largest E_k (strict > in the order 0, 1, 2, 3)."""
    return np.argmax(expected(c, beta, f), axis=1)


def tie_margin(c, beta: float, f: float) -> np.ndarray:
    """The difference of the two largest E_k per target [N]."""
    e = np.sort(expected(c, beta, f), axis=1)
    return e[:, -1] - e[:, -2]


def predicted_loss(c, beta: float, k) -> np.ndarray:
    """L_k [N] for the sizes k [N] (or one size)."""
    t = traces(c, beta)
    k = np.broadcast_to(np.asarray(k), (len(t),))
    return 1.0 - t[np.arange(len(t)), k]


coordinates = ar.coordinates


def _overlap(d) -> float:
    """|Tr CAN(d)|^2 / 16."""
    h = 0.5 * np.pi * np.asarray(d)
    return float(np.prod(np.cos(h)) ** 2 + np.prod(np.sin(h)) ** 2)


def decompose(T, G, f: float = 1.0, force=None):
    """(x, k, loss, predicted, gap) for the 4x4 unitary T and a supercontrolled gate G, dressed or not, the way the kernel goes: the
    interior layers of ``interior`` at the target's own (unfolded) KAK coordinates, r^+ . l^+ of G = (l1 (x) l0) CAN(c) (r1 (x) r0)
    around them, and the exterior layers from aligning the interior circuit with the target -- W's chamber point or its mirror image,
    whichever the trace formula prefers."""
    from slam_decomposition_amd import weyl

    T, G = np.asarray(T, dtype=np.complex128), np.asarray(G, dtype=np.complex128)
    _, l1, l0, cg, r1, r0 = weyl.kak(G)
    beta = float(fold(cg)[0, 1])
    kt = weyl.kak(T)
    ct = np.asarray(kt[3])
    k = int(select(ct[None], beta, f)[0]) if force is None else int(force)
    layers = [(_h(r1) @ q1 @ _h(l1), _h(r0) @ q0 @ _h(l0)) for q1, q0 in interior(k, 0.5 * np.pi * ct, beta)]
    W = np.eye(4, dtype=np.complex128)
    for j in range(k):
        W = G @ W
        if j < len(layers):
            W = np.kron(*layers[j]) @ W
    kw = weyl.kak(W)
    cw = np.asarray(kw[3])
    if _overlap(np.array([1 - cw[0], cw[1], -cw[2]]) - ct) > _overlap(cw - ct):
        kw = weyl.mirror_kak(*kw)
    gap = float(np.max(np.abs(np.asarray(kw[3]) - ct)))
    L = (kt[1] @ _h(kw[1]), kt[2] @ _h(kw[2]))
    R = (_h(kw[4]) @ kt[4], _h(kw[5]) @ kt[5])
    layers = [(L[0] @ R[0], L[1] @ R[1])] if k == 0 else [R] + layers + [L]
    x = np.array([a for q1, q0 in layers for a in list(u3_angles(q0)) + list(u3_angles(q1))])
    return x, k, loss_of(T, template(x, G, k)), float(predicted_loss(ct[None], beta, k)[0]), gap
