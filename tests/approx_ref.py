"""Test-side model of the fidelity-aware approximate decomposition (``slam_approx_decompose``, ``slam_approx_counts``;
csrc/slam_approx.hpp), in NumPy.  Nothing is shared with csrc/.

Coordinates are ``c1c2c3`` in units of pi, rounded to 8 digits and folded as ``span_rules._fold`` folds them:
(x, y, z) = (c1, c2, c3), or (1 - c1, c2, -c3) where c1 > 1/2; a = pi x / 2, b = pi y / 2, c = pi z / 2.  The basis gate has the class
(1/2, beta, 0): beta = 0 (family 0, the CNOT class), 1/2 (family 1, the iSWAP class), 1/4 (family 2, the B class); beta' = pi beta / 2.
The best circuit of k gates reaches |Tr(T^+ W)| = 4 t_k:

    t_0 = |cos a cos b cos c + i sin a sin b sin c|
    t_1 = |cos(pi/4 - a) cos(beta' - b) cos c + i sin(pi/4 - a) sin(beta' - b) sin c|
    t_2 = |cos c| (families 0, 1: two gates reach the plane c3 = 0 exactly), 1 (family 2)
    t_3 = 1 (families 0, 1; family 2 has no k = 3)

L_k = 1 - t_k (BasicCost), F_k = (4 + 16 t_k^2) / 20 (the average gate fidelity, 1 - SquareCost), E_k = F_k f^k for the fidelity f of
one basis gate.  The k with the largest E_k is chosen, compared in the order k = 0, 1, 2, 3 with strict >: ties go to fewer gates.
"""
from __future__ import annotations

import numpy as np

from oracle import slam_oracle as o

BETA = (0.0, 0.5, 0.25)  # by family
N_SIZES = (4, 4, 3)      # sizes 0 .. N_SIZES[family] - 1


def fold(c) -> np.ndarray:
    """[N, 3] (or [3]) coordinates with c3 >= 0 -> c1 <= 1/2, c3 of either sign."""
    c = np.array(c, dtype=np.float64, copy=True).reshape(-1, 3)
    m = c[:, 0] > 0.5
    c[m, 0] = 1.0 - c[m, 0]
    c[m, 2] = -c[m, 2]
    return c


def traces(c, family: int) -> np.ndarray:
    """t_k [N, N_SIZES[family]] for the (unfolded) coordinates c [N, 3]."""
    f = fold(c)
    a, b, cc = (0.5 * np.pi * f[:, j] for j in range(3))
    bp = 0.5 * np.pi * BETA[family]
    q = 0.25 * np.pi
    t0 = np.abs(np.cos(a) * np.cos(b) * np.cos(cc) + 1j * np.sin(a) * np.sin(b) * np.sin(cc))
    t1 = np.abs(np.cos(q - a) * np.cos(bp - b) * np.cos(cc) + 1j * np.sin(q - a) * np.sin(bp - b) * np.sin(cc))
    one = np.ones(len(f))
    cols = [t0, t1, one] if family == 2 else [t0, t1, np.abs(np.cos(cc)), one]
    return np.stack(cols, axis=1)


def gate_fidelity(t) -> np.ndarray:
    """F = (4 + 16 t^2) / 20."""
    return (4.0 + 16.0 * np.asarray(t) ** 2) / 20.0


def expected(c, family: int, f: float) -> np.ndarray:
    """E_k [N, sizes]."""
    t = traces(c, family)
    return gate_fidelity(t) * float(f) ** np.arange(t.shape[1])[None, :]


def select(c, family: int, f: float) -> np.ndarray:
    """The chosen k [N]: the first largest E_k."""
    return np.argmax(expected(c, family, f), axis=1)  # argmax returns the first of equals: strict > in the order 0, 1, 2, 3


def tie_margin(c, family: int, f: float) -> np.ndarray:
    """The difference of the two largest E_k per target [N]."""
    e = np.sort(expected(c, family, f), axis=1)
    return e[:, -1] - e[:, -2]


def predicted_loss(c, family: int, k) -> np.ndarray:
    """L_k [N] for the sizes k [N] (or one size)."""
    t = traces(c, family)
    k = np.broadcast_to(np.asarray(k), (len(t),))
    return 1.0 - t[np.arange(len(t)), k]


def coordinates(T) -> np.ndarray:
    """The 8-digit c1c2c3 of T [N, 4, 4] from the oracle."""
    return np.array([o.c1c2c3(t, 8) for t in np.asarray(T)])


def row_matrix(x, G, k: int) -> np.ndarray:
    """A returned row multiplied out on the CPU: the 6 (k + 1) angles in the front of x through the oracle."""
    x = np.asarray(x, dtype=np.float64)
    if k == 0:
        return o.layer_matrix(x[:6])
    return o.template_eval(x[: 6 * (k + 1)], [np.asarray(G)] * k)


def row_loss(x, G, k: int, T) -> float:
    return o.basic_cost(row_matrix(x, G, k), T)


def _u3_batch(t, p, l) -> np.ndarray:
    c, s = np.cos(0.5 * t), np.sin(0.5 * t)
    m = np.empty((len(t), 2, 2), dtype=np.complex128)
    m[:, 0, 0] = c
    m[:, 0, 1] = -np.exp(1j * l) * s
    m[:, 1, 0] = np.exp(1j * p) * s
    m[:, 1, 1] = np.exp(1j * (p + l)) * c
    return m


def _layer_batch(x6) -> np.ndarray:
    q0, q1 = _u3_batch(x6[:, 0], x6[:, 1], x6[:, 2]), _u3_batch(x6[:, 3], x6[:, 4], x6[:, 5])
    return np.einsum("nij,nkl->nikjl", q1, q0).reshape(len(x6), 4, 4)


def rows_losses(x, G, k: int, T) -> np.ndarray:
    """``row_loss`` for many rows of one size at once (the same products in batched NumPy; tests/test_approx_analytic_host.py holds
    it to ``row_matrix``): BasicCost of rows x [N, 24] against T [N, 4, 4]."""
    x = np.asarray(x, dtype=np.float64)
    W = _layer_batch(x[:, :6])
    for j in range(1, k + 1):
        W = _layer_batch(x[:, 6 * j: 6 * j + 6]) @ (np.asarray(G) @ W)
    return 1.0 - np.abs(np.einsum("nij,nij->n", np.conj(np.asarray(T)), W)) / 4.0


CX = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], dtype=np.complex128)
CZ = np.diag([1, 1, 1, -1]).astype(np.complex128)
ISWAP = np.array([[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)
SWAP = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)


def named_targets(rng):
    """(name, matrix): identity, a random local gate, CX, CZ, iSWAP, SWAP, B, sqrt(iSWAP), CAN(0.3, 0.1, 0), CAN(0.7, 0.2, 0.05)."""
    import kak_ref as kr

    local = kr.kron2(kr.random_su2(rng, 1), kr.random_su2(rng, 1))[0]
    return [("identity", np.eye(4, dtype=np.complex128)), ("local", local), ("CX", CX), ("CZ", CZ), ("iSWAP", ISWAP), ("SWAP", SWAP),
            ("B", o.canonical_matrix(0.5, 0.25, 0.0)), ("sqrt(iSWAP)", o.canonical_matrix(0.25, 0.25, 0.0)),
            ("CAN(0.3, 0.1, 0)", o.canonical_matrix(0.3, 0.1, 0.0)), ("CAN(0.7, 0.2, 0.05)", o.canonical_matrix(0.7, 0.2, 0.05))]


def basis_gates(rng):
    """(name, family, matrix): CX, iSWAP and B, bare and dressed with fixed random local gates."""
    from closed_form_ref import dress

    out = []
    for name, family, g in (("CX", 0, CX), ("iSWAP", 1, ISWAP), ("B", 2, o.canonical_matrix(0.5, 0.25, 0.0))):
        out.append((name, family, g))
        out.append(("dressed " + name, family, dress(rng, g)))
    return out
